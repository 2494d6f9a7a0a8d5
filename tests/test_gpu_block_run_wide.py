"""A whole series per block in one launch for blocks of up to 8192 particles: gpf_run_blocks_wide / pf_run_blocks_wide (gpf_k_block_run_wide.hpp)
against the loop it stands for -- pf_resample_blocks(check=False); pf_update_blocks, through sub-state views above 2048 particles per block -- on the
device and on the CPU oracle (tests/block_run_spec.py).  Helpers and conventions are tests/test_gpu_block_run.py's; every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import block_run_spec as rs
from test_gpu_block_conditional import model_of
from test_gpu_block_run import INVALID_ARGUMENT, INVALID_WEIGHTS, NAN, OK, STATE, T, VARIANTS, data, device_loop, pd, same_run, same_state

pytestmark = pytest.mark.gpu

# the first size past the old team with a tiny ragged block; no multiple of 512 or 64 with the network padded to 8192; the cap and the full LDS plan;
# the dispatch to k_block_run
SHAPES = [(2 * 2049 + 100, 2049), (2 * 5000, 5000), (8192 + 3000, 8192), (600, 300)]
# data seed under which the oracle's loop (rs.run_blocks, on the CPU) has a block-step that resampled and one that did not, in every ess_frac = 0.5 case
DATA_SEED = 7


def same_as_oracle(g, st, f, bs, run):
    ess, lml = g.block_stats(st, bs)
    return (np.array_equal(st.traces, f.rows) and np.array_equal(st.log_weights, f.lw) and np.array_equal(st.parents, f.parents)
            and np.array_equal(ess, run.ess[:, -1]) and np.array_equal(lml, run.lml[:, -1]))


def model_data(g, m, n, bs):
    """data() for every model: block_obs has no noise scale for line_model, whose series gets lgssm2's (0.3 x 8^U(-1, 1) per block and step)"""
    if m.name != "line_model":
        return data(g, m, n, bs, steps=T + 1, seed=DATA_SEED)
    base, rng, B = np.asarray(g.models.simulate(m, T + 1)), np.random.default_rng(DATA_SEED), (n + bs - 1) // bs
    return np.ascontiguousarray(base[None] + 0.3 * 8.0 ** rng.uniform(-1, 1, (B, T + 1, 1)) * rng.standard_normal((B,) + base.shape))


@pytest.mark.parametrize("method,sort_particles", VARIANTS)
@pytest.mark.parametrize("n,bs,ess_frac", [s + (0.5,) for s in SHAPES] + [(2 * 5000, 5000, None)])
def test_lockstep_with_the_loop_and_the_oracle(g, o, n, bs, ess_frac, method, sort_particles):
    m = g.models.lgssm2()
    ys = data(g, m, n, bs, seed=DATA_SEED)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=23) for _ in range(2))
    f = o.initialize_blocks(o.OracleFilter(m.model_id, m.params, n, 23), bs, ys[:, 0])
    spec = rs.run_blocks(o, f, bs, ys[:, 1:T + 1], method, ess_frac=ess_frac, sort_particles=sort_particles)
    want, errs = device_loop(g, a, bs, ys[:, 1:T + 1], method, ess_frac, sort_particles)
    got = g.pf_run_blocks_wide(b, ys[:, 1:T + 1], bs, method, ess_frac=ess_frac, sort_particles=sort_particles)
    assert not errs
    if ess_frac is None:
        assert got.resampled.all()
    else:
        assert got.resampled.any() and not got.resampled.all(), "the case must have a (block, step) that resampled and one that did not"
    assert same_run(got, want) and same_run(got, spec)
    assert got.lml.shape == (ys.shape[0], T) and same_state(g, a, b, bs) and same_as_oracle(g, b, f, bs, spec)
    for st in (a, b):                                                          # epoch, row buffer and bookkeeping are the loop's: both go on alike
        g.pf_resample_blocks(st, bs, method, check=False)
        g.pf_update_blocks(st, (T + 2,), (None,), ys[:, T + 1], bs)
    assert same_state(g, a, b, bs)
    a.close(); b.close()


@pytest.mark.parametrize("name,method", [("bearings4", "residual"), ("sv1", "stratified"), ("object_motion", "multinomial"), ("line_model", "residual")])
def test_models_against_the_oracle_loop(g, o, name, method):
    n, bs = 2 * 2500, 2500
    m = model_of(g, name)
    ys = model_data(g, m, n, bs)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=31)
    f = o.initialize_blocks(o.OracleFilter(m.model_id, m.params, n, 31), bs, ys[:, 0])
    want = rs.run_blocks(o, f, bs, ys[:, 1:], method, ess_frac=0.5)
    got = g.pf_run_blocks_wide(st, ys[:, 1:], bs, method, ess_frac=0.5)
    assert want.resampled.any() and not want.resampled.all()
    assert same_run(got, want) and same_as_oracle(g, st, f, bs, want)
    st.close()


def test_per_block_parameters_shared_series_and_composition(g):
    n, bs = 3 * 2500, 2500
    ms = [g.models.lgssm2(rho=r, sr=s) for r, s in ((0.9, 0.3), (0.95, 0.5), (0.99, 0.8))]
    y = np.ascontiguousarray(g.models.simulate(ms[1], T + 1))                  # ONE series for all blocks
    tiled = np.ascontiguousarray(np.broadcast_to(y, (len(ms),) + y.shape))
    whole, parts, loop = (g.pf_initialize_blocks(ms[0], (1,), tiled[:, 0], n, bs, seed=5, params=ms) for _ in range(3))
    r_whole = g.pf_run_blocks_wide(whole, y[1:], bs, "residual", ess_frac=0.5)
    r_first = g.pf_run_blocks_wide(parts, y[1:3], bs, "residual", ess_frac=0.5)
    r_second = g.pf_run_blocks_wide(parts, tiled[:, 3:], bs, "residual", ess_frac=0.5)
    r_loop, errs = device_loop(g, loop, bs, tiled[:, 1:], "residual", 0.5, True)
    assert not errs and same_run(r_whole, r_loop)
    assert same_run(r_whole, rs.BlockRun(*(np.concatenate([p, q], axis=1) for p, q in zip(r_first, r_second))))
    assert same_state(g, whole, loop, bs) and same_state(g, parts, loop, bs)
    assert len(set(r_whole.lml[:, -1])) == len(ms)                             # the parameters matter
    for st in (whole, parts, loop):
        st.close()


@pytest.mark.parametrize("ess_frac", [None, 0.5])
def test_invalid_weights_at_entry(g, ess_frac):
    """block 1 all -Inf, block 2 with a NaN at 4096 particles per block: the loop with every error caught against one call through the C ABI"""
    n, bs = 4 * 4096, 4096
    m = g.models.lgssm2()
    ys = data(g, m, n, bs)
    B = ys.shape[0]
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=13) for _ in range(2))
    lw = a.log_weights.copy()
    lw[bs:2 * bs], lw[2 * bs + 3] = -np.inf, np.nan
    a.log_weights = b.log_weights = lw
    want, errs = device_loop(g, a, bs, ys[:, 1:T + 1], "multinomial", ess_frac, True)
    obs = np.ascontiguousarray(ys[:, 1:T + 1])
    ess, lml, res, inv = np.empty((T, B)), np.empty((T, B)), np.zeros((T, B), np.int32), C.c_int32(-1)
    st = b._L.gpf_run_blocks_wide(b._h, pd(obs), obs.shape[2], T, 0, bs, 0, 1, NAN if ess_frac is None else ess_frac, pd(ess), pd(lml),
                                  res.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(inv))
    if ess_frac is None:
        assert errs == ["Invalid weights (NaN)."] * T
        assert (st, b._L.gpf_last_error(b._h).decode()) == (INVALID_WEIGHTS, "Invalid weights (NaN).") and inv.value == 1
        assert (res[:, 2] == 1 << 8).all() and (res[:, 1] == (4 << 8 | 1)).all()
    else:
        assert errs == [] and st == OK and inv.value == 0
        assert (res[:, 1:3] == 0).all()
    assert same_run(rs.BlockRun(lml.T, ess.T, (res & 1).astype(bool).T), want)
    assert np.isnan(lml[:, 2]).all() and (lml[:, 1] == -np.inf).all() and np.isfinite(lml[:, [0, 3]]).all()
    assert same_state(g, a, b, bs)
    a.close(); b.close()


WHO = "gpf_run_blocks_wide"
REFUSALS = {
    "block size 8193": (dict(n=2 * 8193, bs=8193), INVALID_ARGUMENT,
                        WHO + ": blocks of more than 8192 particles are not the work of one team, the wide one included (run the loop of gpf_resample_blocks / gpf_update_blocks)"),
    "store": (dict(history=8, bs=2048, n=2 * 2048), STATE,
              WHO + " on a filter with a trajectory store: recording a step is host bookkeeping per step (run the loop of gpf_resample_blocks / gpf_update_blocks)"),
    "keep_prev": (dict(keep_prev=True), STATE, WHO + " on a keep_prev filter: x_{t-1} serves only the rejuvenation moves, and the run has none"),
    "forward": (dict(forward=True, bs=2048, n=2 * 2048), STATE,
                WHO + ": forward smoothing per block is on (gpf_forward_enable_blocks): its statistics are closed by a call per step"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_the_state_alone(g, case):
    kw, status, text = dict(REFUSALS[case][0]), *REFUSALS[case][1:]
    n, bs = kw.pop("n", 2 * 2500), kw.pop("bs", 2500)
    m = g.models.lgssm2()
    ys = data(g, m, n, bs)
    obs = np.ascontiguousarray(ys[:, 1:T + 1])
    st, twin = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, **kw), g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, **kw)
    before = st.traces.copy(), st.log_weights.copy(), st.parents.copy()
    got = st._L.gpf_run_blocks_wide(st._h, pd(obs), 2, T, 0, bs, 0, 1, 0.5, None, None, None, None)
    assert (got, st._L.gpf_last_error(st._h).decode()) == (status, text)
    assert all(np.array_equal(x, y) for x, y in zip(before, (st.traces, st.log_weights, st.parents)))
    for s in (st, twin):                                                       # the epoch too: the refused state and its twin go on alike
        g.pf_resample_blocks(s, bs, "multinomial", check=False)
    assert np.array_equal(st.traces, twin.traces) and np.array_equal(st.parents, twin.parents) and np.array_equal(st.log_weights, twin.log_weights)
    st.close(); twin.close()
