"""Particle Gibbs with backward simulation per block in one launch (gpf.h gpf_sweep_blocks_backward, pf_sweep_blocks_backward) against the loop it stands
for -- T x (conditional resample, pinned update), then block_backward_trajectories(twin, bs, 1) -- on a twin whose store records weights, bit for bit
(np.array_equal, NaN positions compared as such); against the mpmath definition of the backward draw (hp_checks.check_backward); and the invariance
experiment of tests/block_ancestor_spec.py.  The epoch is compared through the iteration both states run after the call."""
import ctypes as C

import numpy as np
import pytest

import block_ancestor_spec as asp
import block_backward_spec as bsp
import block_conditional_spec as cs
import hp_checks as hc
import hp_reference as hp
from test_gpu_block_conditional import eq, references
from test_gpu_block_sweep import INVALID_ARGUMENT, INVALID_WEIGHTS, SEED, T, inputs, iterate, pd, same
from test_hp_block_smoothing import case_obs

pytestmark = pytest.mark.gpu
n_of = lambda bs: 2 * bs + (bs + 1) // 2                                     # three blocks, the last one short (bs > 1)


def pair(g, m, ys, ref, n, bs, steps, **kw):
    """(the state the call runs on: no store; its twin for the loop: a store of `steps` steps that records weights)"""
    init = lambda **k: g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, reference=ref[:, 0], **kw, **k)
    return init(), init(history=steps, history_weights=True)


def loop(g, st, bs, ys, ref, anc, ess_frac, steps=None):
    """the loop of calls on the twin -> what pf_sweep_blocks_backward returns"""
    B, n_steps = ref.shape[:2]
    ys = np.broadcast_to(ys, (B,) + ys.shape[-2:])
    lml, ess, res = np.empty((B, n_steps)), np.empty((B, n_steps)), np.zeros((B, n_steps), bool)
    for t in range(n_steps):
        res[:, t], _ = iterate(g, st, bs, ys[:, t], ref[:, t], anc, ess_frac)
        ess[:, t], lml[:, t] = g.block_stats(st, bs)
    path, idx = g.block_backward_trajectories(st, bs, 1, steps=steps, return_indices=True)
    return g.BlockSweepBackward(path[:, 0], idx[:, 0], lml, ess, res)


def c_call(g, st, obs, ref, bs, ess_frac=0.5, n_ref=2, path=True, idx=True):
    """the C call, which returns its outputs beside an error -> (status, error text, BlockSweepBackward)"""
    B, n_steps = ref.shape[:2]
    r = g.BlockSweepBackward(np.empty((B, n_steps + 1, st.dim)), np.full((B, n_steps + 1), -1, np.int64), np.empty((n_steps, B)), np.empty((n_steps, B)),
                             np.zeros((n_steps, B), np.int32))
    rc = st._L.gpf_sweep_blocks_backward(st._h, pd(obs), obs.shape[-1], n_steps, 0, pd(ref), n_ref, bs, 1, ess_frac, pd(r.path) if path else None,
                                         r.indices.ctypes.data_as(C.POINTER(C.c_int64)) if idx else None, pd(r.ess), pd(r.lml),
                                         r.resampled.ctypes.data_as(C.POINTER(C.c_int32)), None)
    return rc, st._L.gpf_last_error(st._h).decode(), r._replace(lml=r.lml.T, ess=r.ess.T,resampled=(r.resampled.T & 1).astype(bool))


def lockstep(g, name, bs, anc, ess_frac, ref_edit=None, **kw):
    n = n_of(bs)
    m, ys, ref = inputs(g, name, n, bs, T + 2)
    if ref_edit is not None:
        ref_edit(ref)
    a, b = pair(g, m, ys, ref, n, bs, T + 2, **kw)
    obs = np.ascontiguousarray(ys[0, 1:T + 1]) if kw else ys[:, 1:T + 1]      # (per-block parameters: with the shared series)
    got = g.pf_sweep_blocks_backward(a, obs, ref[:, 1:T + 1], bs, ancestor_sampling=anc, ess_frac=ess_frac)
    same(g, got, loop(g, b, bs, obs, ref[:, 1:T + 1], anc, ess_frac), a, b, bs, "call")
    assert (got.indices >= 1).all() and (got.indices <= n).all() and np.isfinite(got.path).all()
    for st in (a, b):                                                        # the epoch, and everything a later call reads
        iterate(g, st, bs, ys[:, T + 1], ref[:, T + 1], anc, None)
    same(g, got, got, a, b, bs, "continued")
    a.close(); b.close()
    return got


# both sides of every team boundary (128 | 129: 2 | 8 particles per lane; 512 | 513: a wave | the workgroup); then d = 4, 1, a discrete latent whose
# logtrans reads the observation row, and line_model
CASES = [("lgssm2", bs, anc, f) for bs in (1, 7, 128, 129, 512, 513, 2048) for anc in (True, False) for f in (None, 0.5)]
CASES += [(name, 129, True, 0.5) for name in ("bearings4", "sv1", "object_motion", "line_model")]


@pytest.mark.parametrize("name,bs,anc,ess_frac", CASES)
def test_lockstep_with_the_twin(g, name, bs, anc, ess_frac):
    lockstep(g, name, bs, anc, ess_frac)


def test_block_params_with_the_shared_series(g):
    sets = [g.models.lgssm2(), g.models.lgssm2(theta=0.3, sq=0.2), g.models.lgssm2(rho=0.9, sr=0.3)]
    lockstep(g, "lgssm2", 129, True, 0.5, params=sets)


def test_a_held_particle_no_candidate_leads_to_takes_its_recorded_parent(g):
    """line_model, blocks of 2: the retained slope changes at every step between two values outside the support, so no particle leads to slot 0"""
    def foreign(ref):
        ref[:, :, 0] = 7.0 + 2.0 * (np.arange(ref.shape[1]) % 2)
    held = lockstep(g, "line_model", 2, True, None, ref_edit=foreign).path[:, :, 0] >= 7.0      # the path holds the retained particle there
    assert held[:, 1:].any() and held[:, :-1][held[:, 1:]].all()             # ... whose recorded parent is the retained particle of the step below


def test_invalid_blocks(g):
    """block 1 with a +Inf, block 2 with a NaN weight at entry: index 0 and NaN paths there, the error after the whole call"""
    bs, B = 100, 4
    m, ys, ref = inputs(g, "lgssm2", bs * B, bs, T + 1)
    a, b = pair(g, m, ys, ref, bs * B, bs, T + 1)
    lw = a.log_weights.copy()
    lw[bs + 7], lw[2 * bs + 3] = np.inf, np.nan
    a.log_weights = lw; b.log_weights = lw
    want = loop(g, b, bs, ys[:, 1:], ref[:, 1:], True, None)
    rc, text, r = c_call(g, a, np.ascontiguousarray(ys[:, 1:]), np.ascontiguousarray(ref[:, 1:]), bs, float("nan"))
    assert (rc, text) == (INVALID_WEIGHTS, "Invalid weights (NaN).")
    same(g, r, want, a, b, bs, "invalid blocks")
    assert (r.indices[1:3] == 0).all() and np.isnan(r.path[1:3]).all() and np.isfinite(r.path[[0, 3]]).all() and (r.indices[[0, 3]] >= 1).all()
    a.close(); b.close()


@pytest.mark.parametrize("name,bs", [("lgssm2", 129), ("object_motion", 129), ("lgssm2", 513), ("object_motion", 513)])
def test_the_draws_follow_the_definition(g, name, bs):
    """the loop on a plain filter fills the Store of tests/block_backward_spec.py from what a caller sees; the call's indices go through the mpmath check"""
    m, n = hc.case_model(g, name), n_of(bs)
    ys, ref = case_obs(g, m, 3, T), references(g, m, 3, T)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, reference=ref[:, 0]) for _ in range(2))
    S = bsp.Store(n, bs, m.dim)
    for t in range(1, T):
        S.begin_step(ys[:, t - 1])
        g.pf_resample_blocks(b, bs, "multinomial", conditional=True, ess_frac=0.5, check=False, reference=ref[:, t], observations=ys[:, t])
        S.resample_blocks(b.parents, g.block_resampled(b))
        S.end_step(b.traces[:, :m.dim], b.log_weights)
        g.pf_update_blocks(b, (), (), ys[:, t], bs, reference=ref[:, t])
    S.begin_step(ys[:, T - 1])
    S.end_step(b.traces[:, :m.dim], b.log_weights)
    got = g.pf_sweep_blocks_backward(a, ys[:, 1:], ref[:, 1:], bs, ess_frac=0.5)
    assert got.resampled.any() and not got.resampled.all()
    v = hc.Violations()
    hc.check_backward(v, [hp.Ref(m)] * 3, S, [0, 2], SEED, 1 + 2 * (T - 1), got.indices[:, None, :], f"sweep backward {name} {bs}")
    v.finish(f"sweep backward {name} {bs}")
    assert all(np.array_equal(got.path[:, s], S.x(s + 1)[got.indices[:, s] - 1]) for s in range(T))
    a.close(); b.close()


@pytest.mark.parametrize("anc", [True, False])
def test_invariance_against_the_exact_smoother(g, anc):
    """retained paths drawn from the exact smoothing law: the call's paths have that law too (tests/block_ancestor_spec.py, T = 8, 4096 blocks of 8)"""
    m, ys, ref, mu, Sigma = asp.invariance_setup(g.models)
    n, bs = cs.INV_B * cs.INV_N, cs.INV_N
    st = g.pf_initialize_blocks(m, (1,), np.tile(ys[0], (cs.INV_B, 1)), n, bs, seed=cs.INV_SEED, reference=ref[:, 0])
    r = g.pf_sweep_blocks_backward(st, np.ascontiguousarray(ys[1:]), np.ascontiguousarray(ref[:, 1:]), bs, ancestor_sampling=anc, ess_frac=None)
    zm, zv = cs.invariance_bounds(r.path, mu, Sigma, cs.INV_B)
    assert np.all(zm <= cs.INV_SIGMAS) and np.all(zv <= cs.INV_SIGMAS), (zm, zv)
    st.close()


def test_two_calls_compose_and_the_new_refusals_change_nothing(g):
    bs, n, T1 = 129, n_of(129), 2
    m, ys, ref = inputs(g, "lgssm2", n, bs, T + 1)
    a, b = pair(g, m, ys, ref, n, bs, T + 1)
    for lo, hi in ((1, T1 + 1), (T1 + 1, T + 1)):
        obs, rf = np.ascontiguousarray(ys[:, lo:hi]), np.ascontiguousarray(ref[:, lo:hi])
        before = (a.traces, a.log_weights, a.parents)                        # (the epoch: the call below agrees with the twin only where it stood)
        for kw in (dict(path=False), dict(idx=False), dict(n_ref=3)):
            assert c_call(g, a, obs, rf, bs, **kw)[0] == INVALID_ARGUMENT and all(eq(x, y) for x, y in zip(before, (a.traces, a.log_weights, a.parents))), kw
        got = g.pf_sweep_blocks_backward(a, obs, rf, bs, ess_frac=0.5)
        same(g, got, loop(g, b, bs, obs, rf, True, 0.5, steps=(lo, hi)), a, b, bs, (lo, hi))
    a.close(); b.close()
