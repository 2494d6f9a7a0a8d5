"""The whole series per block in one launch on a filter with the block-wise trajectory store: gpf_run_blocks_history / pf_run_blocks_history
(k_block_series<.., RunHist>, gpf_k_block_run.hpp) against the loop it stands for -- pf_resample_blocks(check=False); pf_update_blocks -- on a twin from the same seed.  The state,
the three outputs and every query of the store must be the loop's, bit for bit: every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import block_history_spec as hs
from test_gpu_block_conditional import model_of
from test_gpu_block_run import STATE, VARIANTS, data, device_loop, pd, same_run, same_state

pytestmark = pytest.mark.gpu

T = 4
# both sides of every team_dispatch edge (128 | 129, 512 | 513), the degenerate and the largest block; every case has a short last block
SHAPES = [(5, 1), (3 * 7 + 3, 7), (3 * 128 + 40, 128), (3 * 129 + 40, 129), (2 * 512 + 100, 512), (2 * 513 + 100, 513), (3 * 2048 + 300, 2048)]
# (model, n, block size, method): d = 4, 1 and 2 at a size inside the wave team's first shape
MODELS = [("bearings4", 3 * 65 + 20, 65, "residual"), ("sv1", 3 * 65 + 20, 65, "stratified"), ("object_motion", 3 * 65 + 20, 65, "multinomial")]


def eq(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def history_steps(st):
    k = C.c_int32(0)
    st._check(st._L.gpf_history_steps(st._h, C.byref(k)))
    return int(k.value)


def queries(g, st, bs, weights):
    """every answer of the store, as a flat list of arrays (the sampling queries advance the epoch: equal draws on twins mean equal epochs too)"""
    out = []
    for t in range(1, history_steps(st) + 1):
        out += [st.history_column(t, c) for c in range(st.model.dim)] + list(g.block_moments(st, bs, step=t))
    out += list(g.block_sample_trajectories(st, bs, 2, return_indices=True))
    if weights:
        out += list(g.block_backward_trajectories(st, bs, 2, return_indices=True))
        out += list(g.block_smoothed_moments(st, bs, return_weights=True))
        out += list(g.block_smoothed_pair_moments(st, bs))
        out += list(g.block_map_trajectories(st, bs, return_indices=True, return_log_density=True))
    return out


def same_store(g, a, b, bs, weights):
    return history_steps(a) == history_steps(b) and all(eq(x, y) for x, y in zip(queries(g, a, bs, weights), queries(g, b, bs, weights), strict=True))


LOCKSTEP = [("lgssm2", n, bs, me, so, ef, w, 23) for n, bs in SHAPES for me, so in VARIANTS for ef in (0.5, None) for w in (False, True)]
LOCKSTEP += [(name, n, bs, me, True, 0.5, True, 31) for name, n, bs, me in MODELS]


@pytest.mark.parametrize("name,n,bs,method,sort_particles,ess_frac,weights,seed", LOCKSTEP)
def test_lockstep_with_the_loop(g, name, n, bs, method, sort_particles, ess_frac, weights, seed):
    m = model_of(g, name)
    ys = data(g, m, n, bs, steps=T + 2)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=seed, history=T + 2, history_weights=weights) for _ in range(2))
    want, errs = device_loop(g, a, bs, ys[:, 1:T + 1], method, ess_frac, sort_particles)
    got = g.pf_run_blocks_history(b, ys[:, 1:T + 1], bs, method, ess_frac=ess_frac, sort_particles=sort_particles)
    # the gate: a (block, step) that resampled and one that did not; all without it; none at block size 1 (the ESS of one particle is 1 > 0.5)
    assert not errs and (want.resampled.any(), want.resampled.all()) == ((True, True) if ess_frac is None else (False, False) if bs == 1 else (True, False))
    assert same_run(got, want) and same_state(g, a, b, bs) and same_store(g, a, b, bs, weights)
    for st in (a, b):                                                         # later block-wise calls continue identically, the store with them
        g.pf_resample_blocks(st, bs, method, check=False)
        g.pf_update_blocks(st, (T + 2,), (None,), ys[:, T + 1], bs)
    assert same_state(g, a, b, bs) and same_store(g, a, b, bs, weights)
    a.close(); b.close()


def answers(g, st, bs):
    """the store's answers with a refusal's text in place of an answer that is refused (invalid weights): twins must answer or refuse alike"""
    out = []
    for t in range(1, history_steps(st) + 1):
        out += [st.history_column(t, c) for c in range(st.model.dim)]
    for q in (lambda: g.block_sample_trajectories(st, bs, 2, return_indices=True), lambda: g.block_backward_trajectories(st, bs, 2, return_indices=True),
              lambda: g.block_smoothed_moments(st, bs, return_weights=True), lambda: g.block_map_trajectories(st, bs, return_indices=True, return_log_density=True)):
        try:
            out += list(q())
        except g.ErrorException as e:
            out.append(np.frombuffer(str(e).encode(), np.uint8))
    return out


# one block size per team shape (64 x 2, 64 x 8, 256 x 8), each with its own resampler
@pytest.mark.parametrize("ess_frac", [None, 0.5])
@pytest.mark.parametrize("bs,method", [(100, "multinomial"), (129, "residual"), (600, "stratified")])
def test_invalid_weights_at_entry(g, bs, method, ess_frac):
    """block 0 with a NaN, block 1 with a +Inf (both skipped by every resample, propagated anyway), block 2 all -Inf (the uniform fallback where the gate
    lets it resample), block 3 healthy: the loop with every iteration's exception caught, against one call through the C ABI -- status, message, the
    resample words, outputs, state and the store's answers, bit for bit"""
    n, steps = 4 * bs, 3
    m = g.models.lgssm2()
    ys = data(g, m, n, bs, steps=steps + 1)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=13, history=steps + 1, history_weights=True) for _ in range(2))
    lw = a.log_weights.copy()
    lw[3] = np.nan; lw[bs + 5] = np.inf; lw[2 * bs:3 * bs] = -np.inf
    a.log_weights = lw; b.log_weights = lw
    want, errs = device_loop(g, a, bs, ys[:, 1:], method, ess_frac, True)
    obs = np.ascontiguousarray(ys[:, 1:])
    ess, lml, res, inv = np.empty((steps, 4)), np.empty((steps, 4)), np.zeros((steps, 4), np.int32), C.c_int32(-1)
    st = b._L.gpf_run_blocks_history(b._h, pd(obs), obs.shape[2], steps, 0, bs, {"multinomial": 0, "residual": 1, "stratified": 2}[method], 1,
                                     float("nan") if ess_frac is None else ess_frac, pd(ess), pd(lml), res.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(inv))
    if ess_frac is None:
        # every block resamples: the NaN and +Inf blocks are reported and left alone at every step, the all -Inf block resamples uniformly (flag 4)
        assert len(errs) == steps and st != 0 and b._L.gpf_last_error(b._h).decode() in errs and inv.value != 0
        assert (res[:, :2] & 1 == 0).all() and (res[:, :2] >> 8 != 0).all() and (res[:, 2] == (4 << 8 | 1)).all() and (res[:, 3] == 1).all()
    else:
        # behind an ESS gate invalid weights have a NaN ESS: the comparison is false, the block keeps its particles and nothing is reported
        assert errs == [] and st == 0 and inv.value == 0 and (res[:, :3] == 0).all()
    assert same_run(type(want)(lml.T, ess.T, (res & 1).astype(bool).T), want)
    assert np.isnan(lml[:, :2]).all() and np.isnan(ess[:, :3]).all() and (lml[:, 2] == -np.inf).all() and np.isfinite(lml[:, 3]).all() and np.isfinite(ess[:, 3]).all()
    assert same_state(g, a, b, bs)
    assert history_steps(a) == history_steps(b) == steps + 1 and all(eq(x, y) for x, y in zip(answers(g, a, bs), answers(g, b, bs), strict=True))
    a.close(); b.close()


def test_composition_and_a_composed_map_on_entry(g):
    """two updates, a resample across blocks (step 3 HAS a map), run(2), a loop iteration, run(3): against the loop and block_history_spec fed by the twin"""
    n, bs, steps = 4 * 100, 100, 9                                           # (blocks are copied whole across blocks: no short last block here)
    m = g.models.lgssm2()
    ys = data(g, m, n, bs, steps=steps)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=5, history=steps, history_weights=True) for _ in range(2))
    gen = hs.Genealogy(n)

    def update(st, t):                                                        # (the twin a's step ends here: its final rows into the restatement)
        if st is a:
            gen.set_rows(np.stack([a.history_column(gen.steps, c) for c in range(m.dim)], axis=1))
            gen.begin_step(np.zeros((n, m.dim)))
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs)

    def iteration(st, t):
        g.pf_resample_blocks(st, bs, "residual", ess_frac=0.5, check=False)
        if st is a:
            gen.resample("blocks", a.parents, g.block_resampled(a), bs)
        update(st, t)

    gen.begin_step(np.zeros((n, m.dim)))
    for st in (a, b):
        update(st, 1); update(st, 2)
        assert g.pf_resample_across_blocks(st, bs, "multinomial", ess_frac=None, check=False) is not None
    gen.resample("global", a.parents)
    for t in range(3, 9):
        iteration(a, t)
    r1 = g.pf_run_blocks_history(b, ys[:, 3:5], bs, "residual", ess_frac=0.5)
    assert history_steps(b) == 5
    b.history_column(5, 0)                                                    # (a query in between: step 5 has its snapshot before the loop goes on)
    iteration(b, 5)
    r2 = g.pf_run_blocks_history(b, ys[:, 6:9], bs, "residual", ess_frac=0.5)
    assert r1.resampled.any() and r2.resampled.any() and not (r1.resampled.all() and r2.resampled.all())
    assert same_state(g, a, b, bs)
    gen.set_rows(np.stack([a.history_column(steps, c) for c in range(m.dim)], axis=1))
    for t in range(1, steps + 1):
        for c in range(m.dim):
            assert eq(b.history_column(t, c), gen.trace(t, c)), (t, c)
    assert same_store(g, a, b, bs, True)
    a.close(); b.close()


WHO = "gpf_run_blocks_history"
NO_STORE = WHO + " needs the block-wise trajectory store (gpf_history_enable_blocks before gpf_initialize_blocks); without a store: gpf_run_blocks"
REFUSALS = {
    "no store": (dict(), T, STATE, NO_STORE),
    "plain store": (dict(plain=True), T, STATE, NO_STORE),
    "one step too many": (dict(history=T), T, STATE, "trajectory store full: raise max_steps of gpf_history_enable"),
    "forward": (dict(history=T + 1, forward=True), T, STATE, WHO + ": forward smoothing per block is on (gpf_forward_enable_blocks): its statistics are closed by a call per step"),
    "keep_prev": (dict(history=T + 1, keep_prev=True), T, STATE, WHO + " on a keep_prev filter: x_{t-1} serves only the rejuvenation moves, and the run has none"),
    "block size 2049": (dict(history=T + 1, n=2 * 2049, bs=2049), T, STATE, WHO + ": blocks of more than 2048 particles on a filter with a trajectory store (they would need sub-state views)"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_state_store_and_epoch_alone(g, case):
    kw, steps, status, text = dict(REFUSALS[case][0]), *REFUSALS[case][1:]
    n, bs, plain = kw.pop("n", 230), kw.pop("bs", 100), kw.pop("plain", False)
    m = g.models.lgssm2()
    ys = data(g, m, n, bs, steps=T + 1)
    obs = np.ascontiguousarray(ys[:, 1:])
    make = (lambda: g.pf_initialize(m, (1,), ys[0, 0], n, seed=3, history=8)) if plain else (lambda: g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, **kw))
    st, twin = make(), make()
    before = st.traces.copy(), st.log_weights.copy(), st.parents.copy(), history_steps(st)
    got = st._L.gpf_run_blocks_history(st._h, pd(obs), 2, steps, 0, bs, 0, 1, 0.5, None, None, None, None)
    assert (got, st._L.gpf_last_error(st._h).decode()) == (status, text)
    assert all(eq(x, y) for x, y in zip(before, (st.traces, st.log_weights, st.parents, history_steps(st))))
    if case == "one step too many":                                           # one step shorter fills the store exactly; pf_run_blocks still refuses a store
        for s in (st, twin):
            g.pf_run_blocks_history(s, obs[:, :T - 1], bs, "multinomial")
        assert history_steps(st) == T and same_store(g, st, twin, bs, False)
        with pytest.raises(g.ErrorException, match="gpf_run_blocks on a filter with a trajectory store: recording a step is host bookkeeping per step"):
            g.pf_run_blocks(st, obs, bs)
    else:                                                                     # the epoch too: the refused state and its twin propagate alike
        for s in (st, twin):
            g.pf_update(s, (2,), (None,), ys[0, 1]) if plain else g.pf_update_blocks(s, (2,), (None,), ys[:, 1], bs)
    assert eq(st.traces, twin.traces) and eq(st.parents, twin.parents) and eq(st.log_weights, twin.log_weights)
    st.close(); twin.close()
