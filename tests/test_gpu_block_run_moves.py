"""The whole README loop per block in one launch: gpf_run_blocks_rejuvenate / pf_run_blocks_rejuvenate (gpf_k_block_run_move.hpp) against the loop it
stands for,

    for t in range(T):
        pf_resample_blocks(state, bs, method, ess_frac=f, sort_particles=s, check=False)
        pf_rejuvenate_blocks(state, None, (), n_iters, method=kind, only_resampled=True, count=True)
        pf_update_blocks(state, (t,), (None,), ys[:, t], bs)

on the device (keep_prev twins) and on the CPU oracle (tests/block_run_moves_spec.py).  Every comparison is np.array_equal: the contract is bit identity."""
import numpy as np
import pytest

import block_run_moves_spec as ms
from test_gpu_block_conditional import model_of
from test_gpu_block_run import data, same_state

pytestmark = pytest.mark.gpu

T, N_ITERS = 5, 2
# both sides of each team-shape boundary (128 | 129, 512 | 513), ragged last blocks, idle waves, the largest block, a tiny one
SHAPES = [(5 * 128, 128), (4 * 129 + 40, 129), (2 * 512, 512), (2 * 513 + 100, 513), (2048 + 300, 2048), (300, 7)]


def device_loop(g, st, bs, ys, method, kind, ess_frac=0.5, sort_particles=True, n_iters=N_ITERS):
    """the loop of calls; what pf_run_blocks_rejuvenate returns, with the loop's count per step in place of the per-block counts"""
    B, steps = ys.shape[0], ys.shape[1]
    lml, ess, res, acc = np.empty((B, steps)), np.empty((B, steps)), np.zeros((B, steps), bool), np.zeros(steps, np.int64)
    for t in range(steps):
        g.pf_resample_blocks(st, bs, method, ess_frac=ess_frac, sort_particles=sort_particles, check=False)
        res[:, t] = g.block_resampled(st)
        acc[t] = g.pf_rejuvenate_blocks(st, None, (), n_iters, method=kind, only_resampled=True, count=True)
        g.pf_update_blocks(st, (t + 2,), (None,), ys[:, t], bs)
        ess[:, t], lml[:, t] = g.block_stats(st, bs)
    return ms.BlockRunMoves(lml, ess, res, acc)


def same_run(got, want):
    """got: the call's; want: a loop's, whose accept counts are per step"""
    return (np.array_equal(got.lml, want.lml) and np.array_equal(got.ess, want.ess) and np.array_equal(got.resampled, want.resampled)
            and np.array_equal(got.accepted.sum(axis=0), want.accepted) and not got.accepted[~got.resampled].any())


def twins(g, m, ys, n, bs, seed=23, **kw):
    return [g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=seed, keep_prev=True, **kw) for _ in range(2)]


def lockstep(g, n, bs, method, kind, ess_frac=0.5, sort_particles=True):
    m = g.models.lgssm2()
    ys = data(g, m, n, bs)
    a, b = twins(g, m, ys, n, bs)
    want = device_loop(g, a, bs, ys[:, 1:T + 1], method, kind, ess_frac, sort_particles)
    got = g.pf_run_blocks_rejuvenate(b, ys[:, 1:T + 1], bs, method, rejuvenate=kind, n_iters=N_ITERS, ess_frac=ess_frac, sort_particles=sort_particles)
    assert same_run(got, want) and got.accepted.shape == (ys.shape[0], T) and got.accepted.dtype == np.int64
    assert a.traces.shape[1] == 4 and same_state(g, a, b, bs)
    more = [device_loop(g, st, bs, ys[:, T + 1:T + 2], method, kind, ess_frac, sort_particles) for st in (a, b)]
    assert all(np.array_equal(x, y) for x, y in zip(*more)) and same_state(g, a, b, bs)
    a.close(); b.close()
    return want


# ----------------------------------------------------------------------------- 1. lockstep with the device loop
@pytest.mark.parametrize("kind", ["move", "reweight"])
@pytest.mark.parametrize("method", ["multinomial", "residual", "stratified"])
@pytest.mark.parametrize("n,bs", SHAPES)
def test_lockstep_with_the_device_loop(g, n, bs, method, kind):
    want = lockstep(g, n, bs, method, kind)
    assert want.resampled.any() and not want.resampled.all(), "the case must have a (block, step) that resampled and one that did not"


@pytest.mark.parametrize("n,bs,method,kind,ess_frac,sort_particles", [(4 * 129 + 40, 129, "stratified", "move", 0.5, False), (300, 7, "multinomial", "reweight", None, True)])
def test_lockstep_unsorted_and_ungated(g, n, bs, method, kind, ess_frac, sort_particles):
    assert lockstep(g, n, bs, method, kind, ess_frac, sort_particles).resampled.all() == (ess_frac is None)   # (None: every block moves at every step)


# ----------------------------------------------------------------------------- 2. models and row widths (W = 2, 4, 8), the first step after the initialisation
@pytest.mark.parametrize("kind", ["move", "reweight"])
@pytest.mark.parametrize("name", ["lgssm2", "bearings4", "object_motion", "sv1"])
def test_models_against_the_oracle_loop(g, o, name, kind):
    n, bs = 1030, 100
    m = model_of(g, name)
    ys = data(g, m, n, bs, steps=T + 1)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=31, keep_prev=True)
    f = o.initialize_blocks(o.OracleFilter(m.model_id, m.params, n, 31, keep_prev=True), bs, ys[:, 0])
    want = ms.run_blocks_rejuvenate(o, f, bs, ys[:, 1:], ys[:, 0], "multinomial", kind, N_ITERS)
    got = g.pf_run_blocks_rejuvenate(st, ys[:, 1:], bs, "multinomial", rejuvenate=kind, n_iters=N_ITERS)
    assert want.resampled.any() and not want.resampled.all() and np.isfinite(f.lw).all() and same_run(got, want)
    assert np.array_equal(st.traces, f.rows) and np.array_equal(st.log_weights, f.lw) and np.array_equal(st.parents, f.parents)
    st.close()


# ----------------------------------------------------------------------------- 3. composition, per-block parameters with the shared series
@pytest.mark.parametrize("kind", ["move", "reweight"])
def test_runs_compose(g, kind):
    n, bs = 2 * 513 + 100, 513
    m = g.models.lgssm2()
    ys = data(g, m, n, bs)
    a, b = twins(g, m, ys, n, bs, seed=41)
    whole = g.pf_run_blocks_rejuvenate(a, ys[:, 1:6], bs, "residual", rejuvenate=kind, n_iters=N_ITERS)
    parts = [g.pf_run_blocks_rejuvenate(b, ys[:, lo:hi], bs, "residual", rejuvenate=kind, n_iters=N_ITERS) for lo, hi in ((1, 3), (3, 6))]
    assert all(np.array_equal(w, np.concatenate([p, q], axis=1)) for w, p, q in zip(whole, *parts)) and same_state(g, a, b, bs)
    more = [device_loop(g, st, bs, ys[:, 6:7], "residual", kind) for st in (a, b)]
    assert all(np.array_equal(x, y) for x, y in zip(*more)) and same_state(g, a, b, bs)
    a.close(); b.close()


def test_per_block_parameters_and_the_shared_series(g):
    n, bs = 600, 100
    models = [g.models.lgssm2(rho=r, sr=s) for r, s in ((0.9, 0.3), (0.95, 0.5), (0.99, 0.8), (0.9, 0.8), (0.99, 0.3), (0.95, 0.4))]
    y = np.ascontiguousarray(g.models.simulate(models[1], T + 1))               # ONE series for all blocks
    tiled = np.ascontiguousarray(np.broadcast_to(y, (len(models),) + y.shape))
    a, b = twins(g, models[0], tiled, n, bs, seed=5, params=models)
    want = device_loop(g, a, bs, tiled[:, 1:], "residual", "move")
    got = g.pf_run_blocks_rejuvenate(b, y[1:], bs, "residual", rejuvenate="move", n_iters=N_ITERS)
    assert same_run(got, want) and same_state(g, a, b, bs)
    assert len(set(got.lml[:, -1])) == len(models)                            # the parameters matter
    a.close(); b.close()


# ----------------------------------------------------------------------------- 3b. weights at entry
# one block size per team shape (64 x 2, 64 x 8, 256 x 8), each with its own resampler
@pytest.mark.parametrize("ess_frac", [None, 0.5])
@pytest.mark.parametrize("kind", ["move", "reweight"])
@pytest.mark.parametrize("bs,method", [(100, "multinomial"), (129, "residual"), (600, "stratified")])
def test_invalid_weights_at_entry(g, bs, method, kind, ess_frac):
    """block 0 with a NaN, block 1 with a +Inf (both skipped by every resample, never moved, propagated anyway), block 2 all -Inf (the uniform fallback
    where the gate lets it resample), block 3 healthy: the loop with every resample's exception caught, against one call through the C ABI -- status,
    message, the resample words, outputs, accept counts and state, bit for bit"""
    import ctypes as C
    from test_gpu_block_run import pd
    n, steps = 4 * bs, 3
    m = g.models.lgssm2()
    ys = data(g, m, n, bs, steps=steps + 1)
    a, b = twins(g, m, ys, n, bs, seed=13)
    lw = a.log_weights.copy()
    lw[3] = np.nan; lw[bs + 5] = np.inf; lw[2 * bs:3 * bs] = -np.inf
    a.log_weights = lw; b.log_weights = lw
    w_lml, w_ess, w_res, w_acc, errs = np.empty((4, steps)), np.empty((4, steps)), np.zeros((4, steps), bool), np.zeros(steps, np.int64), []
    for t in range(steps):
        try:
            g.pf_resample_blocks(a, bs, method, ess_frac=ess_frac, sort_particles=True, check=False)
        except g.ErrorException as e:
            errs.append(str(e))
        w_res[:, t] = g.block_resampled(a)
        w_acc[t] = g.pf_rejuvenate_blocks(a, None, (), N_ITERS, method=kind, only_resampled=True, count=True)
        g.pf_update_blocks(a, (t + 2,), (None,), ys[:, t + 1], bs)
        w_ess[:, t], w_lml[:, t] = g.block_stats(a, bs)
    obs = np.ascontiguousarray(ys[:, 1:])
    ess, lml, res, acc, inv = np.empty((steps, 4)), np.empty((steps, 4)), np.zeros((steps, 4), np.int32), np.zeros((steps, 4), np.int64), C.c_int32(-1)
    st = b._L.gpf_run_blocks_rejuvenate(b._h, pd(obs), obs.shape[2], steps, 0, bs, {"multinomial": 0, "residual": 1, "stratified": 2}[method], 1,
                                        float("nan") if ess_frac is None else ess_frac, {"move": 0, "reweight": 1}[kind], N_ITERS, pd(ess), pd(lml),
                                        res.ctypes.data_as(C.POINTER(C.c_int32)), acc.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(inv))
    if ess_frac is None:
        assert len(errs) == steps and st != 0 and b._L.gpf_last_error(b._h).decode() in errs and inv.value != 0
        assert (res[:, :2] & 1 == 0).all() and (res[:, :2] >> 8 != 0).all() and (res[:, 2] == (4 << 8 | 1)).all() and (res[:, 3] == 1).all()
    else:
        assert errs == [] and st == 0 and inv.value == 0 and (res[:, :3] == 0).all()
    got_res = (res & 1).astype(bool).T
    assert np.array_equal(got_res, w_res) and np.array_equal(lml.T, w_lml, equal_nan=True) and np.array_equal(ess.T, w_ess, equal_nan=True)
    assert np.array_equal(acc.sum(axis=1), w_acc) and not acc.T[~got_res].any()
    assert np.isnan(lml[:, :2]).all() and np.isnan(ess[:, :3]).all() and np.isfinite(lml[:, 3]).all() and np.isfinite(ess[:, 3]).all()
    assert same_state(g, a, b, bs)
    a.close(); b.close()


# ----------------------------------------------------------------------------- 4. refusals: nothing changed, the epoch included
def test_refusals_leave_the_state_alone(g):
    n, bs = 300, 100
    m = g.models.lgssm2()
    ys = data(g, m, n, bs)
    run = ys[:, 1:T + 1]
    keep, twin = twins(g, m, ys, n, bs, seed=3)
    plain = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3)
    whole = g.pf_initialize(m, (1,), ys[0, 0], n, seed=3, keep_prev=True)
    g.pf_update(whole, (2,), (None,), ys[0, 1])                               # (its last step is the whole filter's: no per-block observations)
    store = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, keep_prev=True, history=8)
    cases = [(plain, {}, "gpf_rejuvenate needs keep_prev = 1"), (whole, {}, "per-block observations of this block size"),
             (keep, {"rejuvenate": "gibbs"}, "Method gibbs not recognized."), (keep, {"n_iters": -1}, "n_iters < 0"), (store, {}, "trajectory store")]
    for st, kw, text in cases:
        before = st.traces, st.log_weights, st.parents
        with pytest.raises(g.ErrorException, match=text):
            g.pf_run_blocks_rejuvenate(st, run, bs, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(before, (st.traces, st.log_weights, st.parents)))
    # the refused state and its twin run on alike: the epoch did not move
    r1, r2 = (g.pf_run_blocks_rejuvenate(st, run, bs, n_iters=N_ITERS) for st in (keep, twin))
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2)) and same_state(g, keep, twin, bs)
    for st in (keep, twin, plain, whole, store):
        st.close()
