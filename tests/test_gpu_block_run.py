"""A whole series per block in one launch: gpf_run_blocks / pf_run_blocks (gpf_k_block_run.hpp) against the loop it stands for,

    for t in range(T):
        pf_resample_blocks(state, bs, method, ess_frac=f, sort_particles=s, check=False)
        pf_update_blocks(state, (t,), (None,), ys[:, t], bs)

run on the device (two states from the same pf_initialize_blocks) and on the CPU oracle (tests/block_run_spec.py).  Every comparison is
np.array_equal: rows, log-weights, parents, block_stats, the three outputs, and the same again after both states continue with the same calls --
which holds only if epoch, row buffer and per-block bookkeeping were left as the loop leaves them.

Two readings of the issue, both forced by the library as it stands:
  * the continuation "pf_resample_blocks + pf_update_blocks + pf_rejuvenate_blocks": gpf_rejuvenate_blocks needs keep_prev = 1 and gpf_run_blocks
    refuses keep_prev states, so no state can take both.  The rejuvenation is still called on both states; it must refuse on both with the same text
    (the keep_prev one: its earlier checks -- per-block observations present, their block size -- passed on both) and change nothing.
  * "for ess_frac = 0.5 every case has a (block, step) that resampled and one that did not": a block of ONE particle has ESS = 1 > 0.5, so at
    block size 1 no block can ever resample; there the condition asserted is that none did."""
import ctypes as C

import numpy as np
import pytest

import block_run_spec as rs
from test_gpu_block_conditional import block_obs, model_of

pytestmark = pytest.mark.gpu

T = 5
OK, INVALID_ARGUMENT, INVALID_WEIGHTS, UNKNOWN_METHOD, STATE = 0, 1, 2, 3, 6   # gpf_status
NAN = float("nan")
# both sides of each team-shape boundary (128 | 129: 2 | 8 particles per lane; 512 | 513: a wave | the workgroup), a ragged last block, five wave
# teams (the second workgroup has idle waves), the largest block, degenerate sizes
SHAPES = [(500, 100), (5 * 128, 128), (4 * 129 + 40, 129), (2 * 512, 512), (2 * 513 + 100, 513), (2048 + 300, 2048), (37, 1), (300, 7)]
VARIANTS = [("multinomial", True), ("residual", True), ("stratified", True), ("stratified", False)]
# data seeds under which the oracle's loop (rs.run_blocks, on the CPU) has both a block that resamples and one that does not at ess_frac = 0.5
DATA_SEED = 7


def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def data(g, m, n, bs, steps=T + 2, seed=DATA_SEED):
    """[B, steps, n_obs]: step 0 initialises, 1 .. T are the run's, T + 1 is the continuation's"""
    return np.ascontiguousarray(block_obs(g, m, (n + bs - 1) // bs, steps, seed))


def device_loop(g, st, bs, ys, method, ess_frac, sort_particles):
    """the loop of calls, errors of invalid weights caught as the issue says; what pf_run_blocks returns, and the errors' texts"""
    B, steps = ys.shape[0], ys.shape[1]
    lml, ess, res, errs = np.empty((B, steps)), np.empty((B, steps)), np.zeros((B, steps), bool), []
    for t in range(steps):
        try:
            g.pf_resample_blocks(st, bs, method, ess_frac=ess_frac, sort_particles=sort_particles, check=False)
        except g.ErrorException as e:
            errs.append(str(e))
        res[:, t] = g.block_resampled(st)
        g.pf_update_blocks(st, (t + 2,), (None,), ys[:, t], bs)
        ess[:, t], lml[:, t] = g.block_stats(st, bs)
    return rs.BlockRun(lml, ess, res), errs


def same_state(g, a, b, bs):
    ea, la = g.block_stats(a, bs); eb, lb = g.block_stats(b, bs)
    parts = {"rows": np.array_equal(a.traces, b.traces), "log-weights": np.array_equal(a.log_weights, b.log_weights, equal_nan=True),
             "parents": np.array_equal(a.parents, b.parents), "block ESS": np.array_equal(ea, eb, equal_nan=True),
             "block log-ML": np.array_equal(la, lb, equal_nan=True),
             "log_ml_est": np.array_equal([g.get_lml_est(a)], [g.get_lml_est(b)], equal_nan=True)}   # (NaN beside a NaN weight)
    assert all(parts.values()), [k for k, v in parts.items() if not v]
    return True


def same_run(x, y):
    return np.array_equal(x.lml, y.lml, equal_nan=True) and np.array_equal(x.ess, y.ess, equal_nan=True) and np.array_equal(x.resampled, y.resampled)


def continue_both(g, a, b, bs, y_next, method):
    """one more iteration of the loop on both states, then the rejuvenation both must refuse alike (the module's docstring)"""
    texts = []
    for st in (a, b):
        g.pf_resample_blocks(st, bs, method, check=False)
        g.pf_update_blocks(st, (T + 2,), (None,), y_next, bs)
        with pytest.raises(g.ErrorException) as e:
            g.pf_rejuvenate_blocks(st)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "keep_prev" in texts[0]
    assert same_state(g, a, b, bs)


# ----------------------------------------------------------------------------- 1. lockstep with the device loop
@pytest.mark.parametrize("ess_frac", [None, 0.5])
@pytest.mark.parametrize("method,sort_particles", VARIANTS)
@pytest.mark.parametrize("n,bs", SHAPES)
def test_lockstep_with_the_device_loop(g, n, bs, method, sort_particles, ess_frac):
    m = g.models.lgssm2()
    ys = data(g, m, n, bs)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=23) for _ in range(2))
    want, errs = device_loop(g, a, bs, ys[:, 1:T + 1], method, ess_frac, sort_particles)
    got = g.pf_run_blocks(b, ys[:, 1:T + 1], bs, method, ess_frac=ess_frac, sort_particles=sort_particles)
    assert not errs
    if ess_frac is None:
        assert want.resampled.all()
    elif bs == 1:
        assert not want.resampled.any()                                       # (ESS of one particle is 1 > 0.5)
    else:
        assert want.resampled.any() and not want.resampled.all(), "the case must have a (block, step) that resampled and one that did not"
    assert same_run(got, want)
    assert got.lml.shape == (ys.shape[0], T) and got.resampled.dtype == bool
    assert same_state(g, a, b, bs)
    continue_both(g, a, b, bs, ys[:, T + 1], method)
    a.close(); b.close()


# ----------------------------------------------------------------------------- 2. models and widths, against the oracle's loop
@pytest.mark.parametrize("method", ["multinomial", "residual", "stratified"])
@pytest.mark.parametrize("name", ["lgssm2", "bearings4", "object_motion", "sv1"])
def test_models_against_the_oracle_loop(g, o, name, method):
    n, bs = 1030, 100
    m = model_of(g, name)
    ys = data(g, m, n, bs, steps=T + 1)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=31)
    f = o.initialize_blocks(o.OracleFilter(m.model_id, m.params, n, 31), bs, ys[:, 0])
    want = rs.run_blocks(o, f, bs, ys[:, 1:], method, ess_frac=0.5)
    got = g.pf_run_blocks(st, ys[:, 1:], bs, method, ess_frac=0.5)
    assert want.resampled.any() and not want.resampled.all()
    assert same_run(got, want)
    assert np.array_equal(st.traces, f.rows) and np.array_equal(st.log_weights, f.lw) and np.array_equal(st.parents, f.parents)
    ess, lml = g.block_stats(st, bs)
    assert np.array_equal(ess, want.ess[:, -1]) and np.array_equal(lml, want.lml[:, -1])
    st.close()


# ----------------------------------------------------------------------------- 3. per-block parameters, the shared series
def test_per_block_parameters_and_the_shared_series(g):
    n, bs = 600, 100
    ms = [g.models.lgssm2(rho=r, sr=s) for r, s in ((0.9, 0.3), (0.95, 0.5), (0.99, 0.8), (0.9, 0.8), (0.99, 0.3), (0.95, 0.4))]
    B = len(ms)
    y = np.ascontiguousarray(g.models.simulate(ms[1], T + 1))                  # ONE series for all blocks
    tiled = np.ascontiguousarray(np.broadcast_to(y, (B,) + y.shape))
    shared, per_block, loop = (g.pf_initialize_blocks(ms[0], (1,), tiled[:, 0], n, bs, seed=5, params=ms) for _ in range(3))
    r_shared = g.pf_run_blocks(shared, y[1:], bs, "residual", ess_frac=0.5)
    r_tiled = g.pf_run_blocks(per_block, tiled[:, 1:], bs, "residual", ess_frac=0.5)
    r_loop, errs = device_loop(g, loop, bs, tiled[:, 1:], "residual", 0.5, True)
    assert not errs and same_run(r_shared, r_loop) and same_run(r_tiled, r_loop)
    assert same_state(g, shared, loop, bs) and same_state(g, per_block, loop, bs)
    assert len({x for x in r_shared.lml[:, -1]}) == B                          # the parameters matter
    # block b equals block b of a filter created with block b's parameters (the claim of test_gpu_block_params.py, through the run)
    for k, mk in enumerate(ms):
        one = g.pf_initialize_blocks(mk, (1,), tiled[:, 0], n, bs, seed=5)
        r_one = g.pf_run_blocks(one, y[1:], bs, "residual", ess_frac=0.5)
        _, lml = g.block_stats(one, bs)
        assert r_shared.lml[k, -1] == lml[k] == r_one.lml[k, -1]
        assert np.array_equal(r_shared.lml[k], r_one.lml[k]) and np.array_equal(r_shared.resampled[k], r_one.resampled[k])
        assert np.array_equal(shared.traces[k * bs:(k + 1) * bs], one.traces[k * bs:(k + 1) * bs])
        one.close()
    continue_both(g, shared, loop, bs, tiled[:, 0], "residual")
    for st in (shared, per_block, loop):
        st.close()


# ----------------------------------------------------------------------------- 4. composition
@pytest.mark.parametrize("n,bs", [(500, 100), (2 * 513 + 100, 513)])
def test_runs_compose(g, n, bs):
    m = g.models.lgssm2()
    ys = data(g, m, n, bs)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=41) for _ in range(2))
    whole = g.pf_run_blocks(a, ys[:, 1:6], bs, "stratified", ess_frac=0.5)
    first = g.pf_run_blocks(b, ys[:, 1:3], bs, "stratified", ess_frac=0.5)
    second = g.pf_run_blocks(b, ys[:, 3:6], bs, "stratified", ess_frac=0.5)
    assert same_run(whole, rs.BlockRun(*(np.concatenate([p, q], axis=1) for p, q in zip(first, second))))
    assert same_state(g, a, b, bs)
    continue_both(g, a, b, bs, ys[:, 6], "stratified")
    a.close(); b.close()


# ----------------------------------------------------------------------------- 5. weights at entry
@pytest.mark.parametrize("ess_frac", [None, 0.5])
@pytest.mark.parametrize("n,bs", [(500, 100), (4 * 600, 600)])
def test_invalid_weights_at_entry(g, n, bs, ess_frac):
    """block 1 all -Inf (safe_softmax's uniform fallback where its gate lets it resample), block 2 with a NaN (skipped by every resample, propagated
    anyway): the loop with every iteration's exception caught, against one call through the C ABI -- status, message, `invalid`, outputs, state"""
    m = g.models.lgssm2()
    ys = data(g, m, n, bs)
    B = ys.shape[0]
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=13) for _ in range(2))
    lw = a.log_weights.copy()
    lw[bs:2 * bs] = -np.inf
    lw[2 * bs + 3] = np.nan
    a.log_weights = lw; b.log_weights = lw
    want, errs = device_loop(g, a, bs, ys[:, 1:T + 1], "multinomial", ess_frac, True)
    obs = np.ascontiguousarray(ys[:, 1:T + 1])
    ess, lml, res, inv = np.empty((T, B)), np.empty((T, B)), np.zeros((T, B), np.int32), C.c_int32(-1)
    st = b._L.gpf_run_blocks(b._h, pd(obs), obs.shape[2], T, 0, bs, 0, 1, NAN if ess_frac is None else ess_frac, pd(ess), pd(lml),
                             res.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(inv))
    if ess_frac is None:
        # every block resamples: the NaN block is reported (flag 1) and left alone at every step, the all -Inf block resamples uniformly (flag 4) and
        # stays all -Inf (its new weight is logsumexp = -Inf)
        assert errs == ["Invalid weights (NaN)."] * T
        assert (st, b._L.gpf_last_error(b._h).decode()) == (INVALID_WEIGHTS, "Invalid weights (NaN).") and inv.value == 1
        assert (res[:, 2] == 1 << 8).all() and (res[:, 1] == (4 << 8 | 1)).all()
    else:
        # behind an ESS gate invalid weights have a NaN ESS: the comparison is false, the block keeps its particles and nothing is reported
        assert errs == [] and st == OK and inv.value == 0
        assert (res[:, 1:3] == 0).all()
    assert same_run(rs.BlockRun(lml.T, ess.T, (res & 1).astype(bool).T), want)
    assert np.isnan(lml[:, 2]).all() and np.isnan(ess[:, 2]).all() and (lml[:, 1] == -np.inf).all() and np.isnan(ess[:, 1]).all()
    assert np.isfinite(lml[:, [0, 3]]).all() and np.isfinite(ess[:, [0, 3]]).all()
    assert same_state(g, a, b, bs)
    a.close(); b.close()


# ----------------------------------------------------------------------------- 6. refusals: status, text, nothing changed
def test_refusals_leave_the_state_alone(g):
    m = g.models.lgssm2()
    n, bs = 300, 100
    ys = data(g, m, n, bs)
    obs = np.ascontiguousarray(ys[:, 1:T + 1])
    big = np.ascontiguousarray(np.tile(obs[0], (42, 1, 1)))
    L = g._lib.load()
    who = "gpf_run_blocks"

    def call(st, obs=obs, n_obs=2, n_steps=T, shared=0, block_size=bs, method=0):
        return L.gpf_run_blocks(st._h, pd(obs) if obs is not None else None, n_obs, n_steps, shared, block_size, method, 1, 0.5, None, None, None, None)

    def snapshot(st):
        return st.traces.copy(), st.log_weights.copy(), st.parents.copy()

    def refused(st, status, text, **kw):
        before = snapshot(st) if kw.pop("look", True) else None
        assert (call(st, **kw), L.gpf_last_error(st._h).decode()) == (status, text)
        if before is not None:
            assert all(np.array_equal(x, y) for x, y in zip(before, snapshot(st)))

    plain = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3)
    twin = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3)
    assert L.gpf_run_blocks(None, pd(obs), 2, T, 0, bs, 0, 1, 0.5, None, None, None, None) == INVALID_ARGUMENT
    # the gate: view, shard, block_size < 1, the per-block parameters' block size, the forward smoother's
    view = plain[0:100]
    refused(view, STATE, who + " on a sub-state view: call it on the filter", look=False)
    shard = g.DeviceParticleFilterState(m, 100, seed=1, n_global=200, gid0=0)
    assert L.gpf_initialize(shard._h, pd(np.ascontiguousarray(ys[0, 0])), 2) == 0
    refused(shard, STATE, who + " on a shard of a sharded filter")
    refused(plain, INVALID_ARGUMENT, "block_size < 1", block_size=0)
    bp = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, params=[m] * 3)
    refused(bp, INVALID_ARGUMENT, who + ": block_size 50 differs from the 100 of the per-block parameters (gpf_set_block_params)", block_size=50)
    # a store of either kind, forward mode, keep_prev
    store = g.pf_initialize(m, (1,), ys[0, 0], n, seed=3, history=8)
    bstore = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, history=8)
    for st in (store, bstore):
        refused(st, STATE, who + " on a filter with a trajectory store: recording a step is host bookkeeping per step (run the loop of gpf_resample_blocks / gpf_update_blocks)")
    fwd = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, forward=True)
    refused(fwd, STATE, who + ": forward smoothing per block is on (gpf_forward_enable_blocks): its statistics are closed by a call per step")
    refused(fwd, INVALID_ARGUMENT, who + ": block_size 50 differs from the 100 forward smoothing per block was initialised with (gpf_forward_enable_blocks)",
            block_size=50)
    keep = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, keep_prev=True)
    refused(keep, STATE, who + " on a keep_prev filter: x_{t-1} serves only the rejuvenation moves, and the run has none")
    # blocks of more than 2048 particles; strata
    wide = g.pf_initialize_blocks(m, (1,), ys[:2, 0], 4200, 2100, seed=3)
    refused(wide, INVALID_ARGUMENT, who + ": blocks of more than 2048 particles are not the work of one team", obs=big, block_size=2100)
    om = g.models.object_motion()
    yo = data(g, om, n, bs)
    strata = g.pf_initialize_blocks(om, (1,), yo[:, 0], n, bs, seed=3, strata=[0.0, 1.0])
    refused(strata, STATE, who + ": strata are set on this filter; the run extends every block with the default proposal only",
            obs=np.ascontiguousarray(yo[:, 1:T + 1]))
    # the call's own arguments
    for k in (0, -1, 4097):
        refused(plain, INVALID_ARGUMENT, who + ": need 1 <= n_steps <= 4096 (longer series: call it in chunks, they compose)", n_steps=k)
    huge = g.pf_initialize_blocks(m, (1,), np.zeros((300000, 2)), 300000, 1, seed=3)     # (4096 x 300000 x 2 words > 2^31)
    refused(huge, INVALID_ARGUMENT, who + ": the observations of the call exceed 2^31 words on the device: fewer steps per call", n_steps=4096, block_size=1,
            look=False)                                                       # (refused before the observations are looked at)
    refused(plain, UNKNOWN_METHOD, "Resampling method not recognized.", method=7)
    refused(plain, INVALID_ARGUMENT, "this model takes 2 observation values per step and block", n_obs=3)
    refused(plain, INVALID_ARGUMENT, "this model takes 2 observation values per step and block", obs=None)
    bad = obs.copy(); bad[2, 3, 1] = np.inf
    refused(plain, INVALID_ARGUMENT, who + ": the observation of step 4, block 2 is not finite", obs=bad)
    bad_shared = obs[0].copy(); bad_shared[1, 0] = np.nan
    refused(plain, INVALID_ARGUMENT, who + ": the observation of step 2 is not finite", obs=bad_shared, shared=1)
    # nothing moved, the epoch included: the refused state and its twin run on alike
    r1 = g.pf_run_blocks(plain, obs, bs, "multinomial", ess_frac=0.5)
    r2 = g.pf_run_blocks(twin, obs, bs, "multinomial", ess_frac=0.5)
    assert same_run(r1, r2) and same_state(g, plain, twin, bs)
    for st in (view, plain, twin, shard, bp, store, bstore, fwd, keep, wide, strata, huge):
        st.close()
