"""The particle Gibbs chain per block in one launch: gpf_gibbs_blocks / pf_gibbs_blocks (gpf_k_block_gibbs.hpp) against the loop of existing calls it
stands for -- per sweep a fresh handle made by pf_initialize_blocks(seed=seeds[k], reference=path[:, 0]), pf_sweep_blocks[_backward] on it, its path the
next reference.  Every comparison is np.array_equal on paths and lml."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_block_conditional import block_obs, model_of, references

pytestmark = pytest.mark.gpu

SEED, SEEDS, B = 23, [1009, 2**63 + 5, 77, 31337], 4


def the_loop(g, m, n, bs, ys, ref, seeds, params=None, ancestor_sampling=True, backward=False, ess_frac=0.5, thin=1):
    """(paths, lml) of the issue's loop, written out; ys [B, T, n_obs]"""
    sweep = g.pf_sweep_blocks_backward if backward else g.pf_sweep_blocks
    kept, lml = [], []
    for k, s in enumerate(seeds):
        tw = g.pf_initialize_blocks(m, (), ys[:, 0], n, bs, seed=s, params=params, reference=ref[:, 0])
        sw = sweep(tw, ys[:, 1:], ref[:, 1:], bs, ancestor_sampling=ancestor_sampling, ess_frac=ess_frac)
        lml.append(sw.lml[:, -1])
        ref = sw.path
        if (k + 1) % thin == 0:
            kept.append(sw.path)
        tw.close()
    return np.stack(kept, axis=1), np.stack(lml, axis=1)


def ckpt(st):
    """the checkpoint's bytes; its parents are padded to 8 bytes and the library leaves the pad of an odd particle count unwritten"""
    b = st.checkpoint()
    return b[:b.size - 4 * (st.n_particles % 2)].tobytes()


def setup(g, m, bs, T, params=None):
    """a carrier state of B blocks with a short last one, its series and an initial retained path"""
    n = 3 * bs + 7
    if m.name == "line_model":
        ys = np.stack([[g.models.line_obs(t + 1, float(s)) for t in range(T)] for s in (-2, 0, 1, 2)])
    else:
        ys = np.ascontiguousarray(block_obs(g, m, B, T))
    ref = np.ascontiguousarray(references(g, m, B, T))
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, params=params)
    return st, n, ys, ref


# the three team shapes of team_dispatch and the 128 | 129 boundary; K = 3 sweeps over T = 4 steps: the slabs are reused twice, the path handed over twice
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("ancestor_sampling", [True, False])
@pytest.mark.parametrize("bs", [7, 128, 129, 513])
def test_lockstep_with_the_loop(g, bs, ancestor_sampling, backward):
    m = g.models.lgssm2()
    st, n, ys, ref = setup(g, m, bs, 4)
    kw = dict(ancestor_sampling=ancestor_sampling, backward=backward, ess_frac=0.5)
    before = ckpt(st)
    r = g.pf_gibbs_blocks(st, ys, ref, bs, SEEDS[:3], **kw)
    paths, lml = the_loop(g, m, n, bs, ys, ref, SEEDS[:3], **kw)
    assert r.paths.shape == (B, 3, 4, m.dim) and r.lml.shape == (B, 3) and np.isfinite(r.lml).all()
    assert np.array_equal(r.paths, paths) and np.array_equal(r.lml, lml)
    assert ckpt(st) == before                                                 # the state is the carrier only
    assert not np.array_equal(r.paths[:, 0], r.paths[:, 1])                   # (the sweeps differ: fresh seeds, a new retained path)


@pytest.mark.parametrize("case", ["bearings4", "sv1", "object_motion", "line_model", "block_params", "shared_series", "ess_frac_none"])
def test_further_cases(g, case):
    bs, lg = 100, g.models.lgssm2
    m = g.models.line_model() if case == "line_model" else model_of(g, case) if case in ("bearings4", "sv1", "object_motion") else lg()
    params = [lg(rho=(0.9, 0.95, 0.99)[b % 3], sr=(0.3, 0.5, 0.8, 0.4)[b]) for b in range(B)] if case == "block_params" else None
    st, n, ys, ref = setup(g, m, bs, 4, params)
    kw = dict(ess_frac=None) if case == "ess_frac_none" else {}
    if case == "shared_series":
        ys = np.ascontiguousarray(np.broadcast_to(ys[0], ys.shape))           # the per-block copy of one series
        r = g.pf_gibbs_blocks(st, ys[0], ref, bs, SEEDS[:2])
    else:
        r = g.pf_gibbs_blocks(st, ys, ref, bs, SEEDS[:2], **kw)
    paths, lml = the_loop(g, m, n, bs, ys, ref, SEEDS[:2], params=params, **kw)
    assert np.array_equal(r.paths, paths) and np.array_equal(r.lml, lml) and np.isfinite(r.lml).all()


@pytest.mark.parametrize("backward", [False, True])
def test_thinning_and_composition(g, backward):
    bs, m = 100, g.models.lgssm2()
    st, n, ys, ref = setup(g, m, bs, 4)
    full = g.pf_gibbs_blocks(st, ys, ref, bs, SEEDS, backward=backward)
    thinned = g.pf_gibbs_blocks(st, ys, ref, bs, SEEDS, backward=backward, thin=2)
    assert thinned.paths.shape[1] == 2 and np.array_equal(thinned.paths, full.paths[:, 1::2]) and np.array_equal(thinned.lml, full.lml)
    first = g.pf_gibbs_blocks(st, ys, ref, bs, SEEDS[:2], backward=backward)
    second = g.pf_gibbs_blocks(st, ys, first.paths[:, -1], bs, SEEDS[2:], backward=backward)
    assert np.array_equal(np.concatenate([first.paths, second.paths], axis=1), full.paths)
    assert np.array_equal(np.concatenate([first.lml, second.lml], axis=1), full.lml)
    assert g.pf_gibbs_blocks(st, ys, ref, bs, SEEDS[:1], thin=2).paths.shape == (B, 0, 4, 2)      # K < thin: no path kept, lml only


@pytest.mark.parametrize("case", ["view", "keep_prev", "store", "T_1", "ref_nan", "ref_shape", "no_seeds", "thin_0"])
def test_refusals_leave_the_state_alone(g, case):
    n, bs, m = 307, 100, g.models.lgssm2()
    ys = np.ascontiguousarray(block_obs(g, m, B, 3))
    ref = np.ascontiguousarray(references(g, m, B, 3))
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=case == "keep_prev", history=4 if case == "store" else 0)
    seeds, thin = SEEDS[:2], 1
    if case == "T_1": ys, ref = ys[:, :1], ref[:, :1]
    if case == "ref_nan": ref[2, 1, 0] = np.nan
    if case == "ref_shape": ref = ref[:, :2]
    if case == "no_seeds": seeds = []
    if case == "thin_0": thin = 0
    before = ckpt(st)
    with pytest.raises(g.ErrorException):
        g.pf_gibbs_blocks(st[0:100] if case == "view" else st, ys, ref, bs, seeds, thin=thin)
    assert ckpt(st) == before
    # the library's own refusals of what the package stops first
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    sd = np.asarray(SEEDS[:2], np.uint64)
    out, lml = np.zeros((B, 2, 3, 2)), np.zeros((B, 2))
    n_steps, K = (1, 2) if case == "T_1" else (3, 0) if case == "no_seeds" else (3, 2)
    if case in ("T_1", "no_seeds", "thin_0"):
        got = st._L.gpf_gibbs_blocks(st._h, pd(ys), 2, n_steps, 0, pd(ref), 2, bs, 1, 0, 0.5, sd.ctypes.data_as(C.POINTER(C.c_uint64)), K, thin, pd(out), pd(lml))
        assert got == 1 and st._L.gpf_last_error(st._h) and ckpt(st) == before
