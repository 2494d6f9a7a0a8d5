"""One conditional SMC sweep per block in one launch (gpf.h gpf_sweep_blocks, pf_sweep_blocks) against the loop of calls it stands for -- T x
(pf_resample_blocks(conditional=True[, reference=, observations=], check=False), pf_update_blocks(reference=)), then block_sample_trajectories(twin, bs,
1) -- on a twin with a block-wise trajectory store, bit for bit: every comparison is np.array_equal with NaN positions compared as such.  The loop's
pieces are pinned to the mpmath restatements elsewhere.  The RNG epoch has no getter: it is compared through the iteration both states run after the
sweep, which agrees only where the epochs do.  The statistical case is the invariance experiment of tests/test_gpu_block_ancestor.py, one call a sweep."""
import ctypes as C
import warnings

import numpy as np
import pytest

import block_ancestor_spec as asp
import block_conditional_spec as cs
from test_gpu_block_ancestor import line_data
from test_gpu_block_conditional import block_obs, eq, model_of, n_of, references

pytestmark = pytest.mark.gpu
T = 5
OK, INVALID_ARGUMENT, INVALID_WEIGHTS, STATE = 0, 1, 2, 6                     # gpf_status
SEED = 17


pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def inputs(g, name, n, bs, steps):
    """(model, data [B, steps, n_obs], retained paths [B, steps, d]); step 0 initialises"""
    B = (n + bs - 1) // bs
    if name == "line_model":                                                 # slopes of the model's support and outlier flags: some particles hold them
        rng = np.random.default_rng(11)
        ref = np.stack([rng.integers(-2, 3, (B, steps)), rng.integers(0, 2, (B, steps))], axis=2).astype(np.float64)
        return g.models.line_model(), np.ascontiguousarray(line_data(g, B, steps)), ref
    m = model_of(g, name)
    return m, np.ascontiguousarray(block_obs(g, m, B, steps)), np.ascontiguousarray(references(g, m, B, steps))


def pair(g, m, ys, ref, n, bs, steps, **kw):
    """(the state the sweep runs on: no store; its twin for the loop: a store of `steps` steps)"""
    return (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, reference=ref[:, 0], **kw),
            g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, reference=ref[:, 0], history=steps, **kw))


def iterate(g, st, bs, y, r, anc, ess_frac):
    """one iteration of the loop; the texts of the errors of invalid weights"""
    errs = []
    kw = dict(reference=r, observations=y) if anc else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            g.pf_resample_blocks(st, bs, "multinomial", conditional=True, ess_frac=ess_frac, check=False, **kw)
        except g.ErrorException as e:
            errs.append(str(e))
    res = g.block_resampled(st)
    g.pf_update_blocks(st, (), (), y, bs, reference=r)
    return res, errs


def loop(g, st, bs, ys, ref, anc, ess_frac, steps=None):
    """the loop of calls on the twin -> what pf_sweep_blocks returns (the path over the last T + 1 steps of the store), and the errors"""
    B, n_steps = ref.shape[0], ref.shape[1]
    ys = np.broadcast_to(ys, (B,) + ys.shape[-2:])
    lml, ess, res, errs = np.empty((B, n_steps)), np.empty((B, n_steps)), np.zeros((B, n_steps), bool), []
    for t in range(n_steps):
        res[:, t], e = iterate(g, st, bs, ys[:, t], ref[:, t], anc, ess_frac)
        errs += e
        ess[:, t], lml[:, t] = g.block_stats(st, bs)
    path, idx = g.block_sample_trajectories(st, bs, 1, steps=steps, return_indices=True)
    return g.BlockSweep(path[:, 0], idx[:, 0], lml, ess, res), errs


def same(g, got, want, a, b, bs, where):
    for k in got._fields:
        assert eq(getattr(got, k), getattr(want, k)), (where, k)
    for k in ("traces", "log_weights", "parents"):
        assert eq(getattr(a, k), getattr(b, k)), (where, k)
    assert all(eq(x, y) for x, y in zip(g.block_stats(a, bs), g.block_stats(b, bs))), (where, "block_stats")


def c_sweep(g, st, obs, ref, bs, ess_frac=0.5, outs=False, n_obs=2, n_steps=T, shared=0, n_ref=2):
    """the C call, which returns its outputs beside an error -> (status, error text, BlockSweep with the resample words | None, *invalid)"""
    r, o, inv = None, (None,) * 6, C.c_int32(-1)
    if outs:
        B = st.n_particles // bs
        r = g.BlockSweep(np.empty((B, n_steps + 1, st.dim)), np.full(B, -1, np.int64), np.empty((n_steps, B)), np.empty((n_steps, B)), np.zeros((n_steps, B), np.int32))
        o = (pd(r.path), r.index.ctypes.data_as(C.POINTER(C.c_int64)), pd(r.ess), pd(r.lml), r.resampled.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(inv))
    rc = st._L.gpf_sweep_blocks(st._h, pd(obs), n_obs, n_steps, shared, pd(ref), n_ref, bs, 1, ess_frac, *o)
    return rc, st._L.gpf_last_error(st._h).decode(), r and r._replace(lml=r.lml.T, ess=r.ess.T, resampled=r.resampled.T), inv.value


def lockstep(g, name, bs, anc, ess_frac):
    n = n_of(bs)
    m, ys, ref = inputs(g, name, n, bs, T + 2)
    a, b = pair(g, m, ys, ref, n, bs, T + 2)
    got = g.pf_sweep_blocks(a, ys[:, 1:T + 1], ref[:, 1:T + 1], bs, ancestor_sampling=anc, ess_frac=ess_frac)
    want, errs = loop(g, b, bs, ys[:, 1:T + 1], ref[:, 1:T + 1], anc, ess_frac)
    assert errs == []
    same(g, got, want, a, b, bs, "sweep")
    for st in (a, b):                                                        # the epoch, and everything a later call reads
        res, _ = iterate(g, st, bs, ys[:, T + 1], ref[:, T + 1], anc, None)
        assert res.all()
    same(g, got, want, a, b, bs, "continued")
    a.close(); b.close()
    return got


# both sides of every team boundary (128 | 129: 2 | 8 particles per lane; 512 | 513: a wave | the workgroup); n_of: three blocks and a short fourth;
# then d = 1, 2 (a discrete latent), 4 and line_model
CASES = [("lgssm2", bs, anc, f) for bs in (1, 7, 128, 129, 512, 513, 2048) for anc in (True, False) for f in (None, 0.5)]
CASES += [("sv1", 129, True, 0.5), ("object_motion", 100, True, 0.5), ("bearings4", 513, True, 0.5), ("line_model", 64, True, 0.5)]


@pytest.mark.parametrize("name,bs,anc,ess_frac", CASES)
def test_lockstep_with_the_loop(g, name, bs, anc, ess_frac):
    r = lockstep(g, name, bs, anc, ess_frac)
    assert r.resampled.all() if ess_frac is None else (bs > 1 or not r.resampled.any())   # (ESS = 1 is never below 0.5)
    assert (r.index >= 1).all() and (r.index <= bs).all() and np.isfinite(r.path).all()


def test_block_params_with_the_shared_series(g):
    sets = [g.models.lgssm2(), g.models.lgssm2(theta=0.3, sq=0.2), g.models.lgssm2(rho=0.9, sr=0.3)]
    bs, B = 100, 7
    n = bs * B - 30
    m, ys, ref = inputs(g, "lgssm2", n, bs, T + 1)
    a, b = pair(g, m, ys, ref, n, bs, T + 1, params=[sets[k % 3] for k in range(B)])
    shared = np.ascontiguousarray(ys[0, 1:])
    got = g.pf_sweep_blocks(a, shared, ref[:, 1:], bs, ess_frac=0.5)
    want, _ = loop(g, b, bs, shared, ref[:, 1:], True, 0.5)
    same(g, got, want, a, b, bs, "per-block parameters")
    assert not eq(got.lml[0], got.lml[1]) and got.resampled.any() and not got.resampled.all()
    a.close(); b.close()


def test_two_sweeps_compose(g):
    bs, n, T1 = 129, n_of(129), 2
    m, ys, ref = inputs(g, "lgssm2", n, bs, T + 1)
    a, b = pair(g, m, ys, ref, n, bs, T + 1)
    for lo, hi in ((1, T1 + 1), (T1 + 1, T + 1)):
        got = g.pf_sweep_blocks(a, ys[:, lo:hi], ref[:, lo:hi], bs, ess_frac=0.5)
        want, _ = loop(g, b, bs, ys[:, lo:hi], ref[:, lo:hi], True, 0.5, steps=(lo, hi))
        same(g, got, want, a, b, bs, (lo, hi))
    a.close(); b.close()


@pytest.mark.parametrize("ess_frac", [None, 0.5])
def test_invalid_blocks(g, ess_frac):
    """block 1 all -Inf, block 2 with a NaN at entry"""
    bs, B = 100, 4
    m, ys, ref = inputs(g, "lgssm2", bs * B, bs, T + 1)
    a, b = pair(g, m, ys, ref, bs * B, bs, T + 1)
    lw = a.log_weights.copy()
    lw[bs:2 * bs] = -np.inf
    lw[2 * bs + 3] = np.nan
    a.log_weights = lw; b.log_weights = lw
    want, errs = loop(g, b, bs, ys[:, 1:], ref[:, 1:], True, ess_frac)
    rc, text, r, inv = c_sweep(g, a, np.ascontiguousarray(ys[:, 1:]), np.ascontiguousarray(ref[:, 1:]), bs, float("nan") if ess_frac is None else ess_frac, outs=True)
    if ess_frac is None:                                                     # the NaN block is reported at every step and left alone, the -Inf block resamples uniformly
        assert errs == ["Invalid weights (NaN)."] * T and (rc, text, inv) == (INVALID_WEIGHTS, "Invalid weights (NaN).", 1)
        assert (r.resampled[2] == 1 << 8).all() and (r.resampled[1] == (4 << 8 | 1)).all()
    else:                                                                    # behind an ESS gate invalid weights have a NaN ESS: nothing resamples, nothing is reported
        assert errs == [] and (rc, inv) == (OK, 0) and (r.resampled[1:3] == 0).all()
    same(g, r._replace(resampled=(r.resampled & 1).astype(bool)), want, a, b, bs, "invalid blocks")
    assert r.index[2] == 0 and np.isnan(r.path[2]).all() and np.isfinite(r.path[[0, 1, 3]]).all() and (r.index[[0, 1, 3]] >= 1).all()
    assert (r.lml[1] == -np.inf).all() and np.isnan(r.lml[2]).all() and np.isfinite(r.lml[[0, 3]]).all()
    a.close(); b.close()


def test_a_reference_no_particle_leads_to_keeps_ancestor_0(g):
    bs, B = 129, 4
    m, ys, ref = inputs(g, "line_model", bs * B, bs, T + 1)
    ref[[0, 2, 3], :, 0] = 7.0                                               # a slope outside uniform_discrete(-2, 2), except in block 1
    a, b = pair(g, m, ys, ref, bs * B, bs, T + 1)
    got = g.pf_sweep_blocks(a, ys[:, 1:], ref[:, 1:], bs, ess_frac=None)
    want, _ = loop(g, b, bs, ys[:, 1:], ref[:, 1:], True, None)
    same(g, got, want, a, b, bs, "fallback")
    assert (a.parents[cs.slot0(bs * B, bs)][[0, 2, 3]] == 1).all() and got.resampled.all()
    a.close(); b.close()


def test_refusals_change_nothing(g):
    """(state, status, a piece of the text that names the refusal, the arguments that differ); the full texts are those of gpf_run_blocks' refusals"""
    m, om = g.models.lgssm2(), g.models.object_motion()
    n, bs = 300, 100
    _, ys, ref = inputs(g, "lgssm2", n, bs, T + 1)
    obs, rf = np.ascontiguousarray(ys[:, 1:]), np.ascontiguousarray(ref[:, 1:])
    init = lambda **kw: g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=3, reference=ref[:, 0], **kw)
    plain, twin = init(), init()
    shard = g.DeviceParticleFilterState(m, 100, seed=1, n_global=200, gid0=0)
    assert shard._L.gpf_initialize(shard._h, pd(np.ascontiguousarray(ys[0, 0])), 2) == 0
    bad_obs, bad_ref = obs.copy(), rf.copy()
    bad_obs[2, 3, 1], bad_ref[1, 2, 0] = np.inf, np.nan
    cases = [(plain[0:100], STATE, "on a sub-state view", {}), (shard, STATE, "on a shard of a sharded filter", {}),
             (plain, INVALID_ARGUMENT, "block_size < 1", dict(bs=0)),
             (init(params=[m] * 3), INVALID_ARGUMENT, "block_size 50 differs from the 100 of the per-block parameters", dict(bs=50)),
             (g.pf_initialize(m, (1,), ys[0, 0], n, seed=3, history=8), STATE, "on a filter with a trajectory store", {}),
             (init(history=8), STATE, "on a filter with a trajectory store", {}),
             (init(forward=True), STATE, "forward smoothing per block is on", {}), (init(keep_prev=True), STATE, "on a keep_prev filter", {}),
             (g.pf_initialize_blocks(m, (1,), ys[:2, 0], 4200, 2100, seed=3), INVALID_ARGUMENT, "blocks of more than 2048 particles", dict(bs=2100)),
             (g.pf_initialize_blocks(om, (1,), block_obs(g, om, 3, 1)[:, 0], n, bs, seed=3, strata=[0.0, 1.0]), STATE, "strata are set on this filter", {}),
             (plain, INVALID_ARGUMENT, "need 1 <= n_steps <= 4096", dict(n_steps=0)), (plain, INVALID_ARGUMENT, "need 1 <= n_steps <= 4096", dict(n_steps=4097)),
             # (4096 x 300000 x 2 reference words: refused before the inputs are looked at)
             (g.pf_initialize_blocks(m, (1,), np.zeros((300000, 2)), 300000, 1, seed=3), INVALID_ARGUMENT, "exceed 2^31 words on the device",
              dict(n_steps=4096, bs=1, shared=1)),
             (plain, INVALID_ARGUMENT, "this model takes 2 observation values", dict(n_obs=3)), (plain, INVALID_ARGUMENT, "this model takes 2 observation values", dict(obs=None)),
             (plain, INVALID_ARGUMENT, "the reference has 2 values per block", dict(ref=None)), (plain, INVALID_ARGUMENT, "the reference has 2 values per block", dict(n_ref=3)),
             (plain, INVALID_ARGUMENT, "the observation of step 4, block 2 is not finite", dict(obs=bad_obs)),
             (plain, INVALID_ARGUMENT, "the reference of block 1 is not finite (step 3)", dict(ref=bad_ref))]
    assert plain._L.gpf_sweep_blocks(None, pd(obs), 2, T, 0, pd(rf), 2, bs, 1, 0.5, *(None,) * 6) == INVALID_ARGUMENT
    for st, status, piece, kw in cases:
        look = st.n_particles == n                                           # (the filters of the common size: rows, weights and parents before and after)
        before = (st.traces, st.log_weights, st.parents) if look else ()
        kw = dict(dict(obs=obs, ref=rf, bs=bs), **kw)
        rc, text, _, _ = c_sweep(g, st, kw.pop("obs"), kw.pop("ref"), kw.pop("bs"), **kw)
        assert rc == status and piece in text, (piece, rc, text)
        assert all(np.array_equal(x, y) for x, y in zip(before, (st.traces, st.log_weights, st.parents)))
    # nothing moved, the epoch included: the refused state and its twin sweep alike
    r1, r2 = (g.pf_sweep_blocks(st, obs, rf, bs) for st in (plain, twin))
    same(g, r1, r2, plain, twin, bs, "after the refusals")
    for st in {id(c[0]): c[0] for c in cases if c[0] is not plain}.values():     # (the view goes before its filter)
        st.close()
    plain.close(); twin.close()


def test_invariance_against_the_exact_smoother(g):
    """retained paths drawn from the exact smoothing law: the sweep's paths have that law too (tests/block_ancestor_spec.py, T = 8, 4096 blocks of 8)"""
    m, ys, ref, mu, Sigma = asp.invariance_setup(g.models)
    n, bs = cs.INV_B * cs.INV_N, cs.INV_N
    st = g.pf_initialize_blocks(m, (1,), np.tile(ys[0], (cs.INV_B, 1)), n, bs, seed=cs.INV_SEED, reference=ref[:, 0])
    r = g.pf_sweep_blocks(st, np.ascontiguousarray(ys[1:]), np.ascontiguousarray(ref[:, 1:]), bs, ess_frac=None)
    zm, zv = cs.invariance_bounds(r.path, mu, Sigma, cs.INV_B)
    assert np.all(zm <= cs.INV_SIGMAS) and np.all(zv <= cs.INV_SIGMAS), (zm, zv)
    st.close()
