"""Marginal smoothing per block on the device (gpf.h gpf_block_smooth):

  1. means, variances, weights and lineage blocks bit for bit against the NumPy restatement of tests/block_smooth_spec.py, which is fed only with what a
     caller sees: four models, keep_prev on and off, the edges of the three team shapes, a short last block, a sub-range of steps; state, store and epoch
     unchanged; step T is block_moments;
  2. line_model: the weights sit on the slopes alive at T; the ESS gate's unequal stored weights; per-block parameters;
  3. the nested filter: block resample, then resampling across blocks, every step -- blocks_out is the lineage;
  4. a whole-filter pf_resample inside a block-wise step: NaN and 0 from that step down for the blocks it scattered, the restatement for the others;
  5. edge weights: a -Inf particle of a past step has W = 0 exactly, a target no candidate leads to hands its mass to its recorded parent, a NaN block;
  6. refused calls change nothing; a state without history_weights is refused;
  7. two kernels, one law: backward simulation's step-s indices have W_s as their marginal; the law against the exact smoother; what the feature is for
     (the CPU rehearsals: tests/test_block_smooth_host.py)."""
import ctypes as C

import numpy as np
import pytest

import block_backward_spec as bsp
import block_smooth_spec as ssp
from test_gpu_block_backward import MODELS, SEED, SIZES, T, Dev
from test_gpu_block_conditional import block_obs, eq, n_of, refused, snapshot, unchanged

pytestmark = pytest.mark.gpu


def state_of(st):
    """snapshot without the checkpoint's trailing padding (the parents are n 4-byte words in a blob of whole 8-byte words: for odd n the last four bytes
    are never written)"""
    s = snapshot(st)
    return (s[0][:len(s[0]) - (-4 * st.n_particles) % 8],) + s[1:]


def got(d, steps=None):
    return d.g.block_smoothed_moments(d.st, d.bs, steps=steps, return_weights=True, return_blocks=True)


def want(d, o, lo=1, hi=None, P=None):
    return ssp.smooth(o, d.m.name, d.m.params if P is None else P, d.S, lo, hi)


def check(a, b, where):
    for k, what in enumerate(("mean", "var", "weights")):
        assert eq(a[k], b[k]), (where, what, np.argwhere(~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))))[:5])
    assert np.array_equal(a[3], b[3]), (where, "blocks")


# ----------------------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_moments_weights_and_blocks_are_the_restatement(g, o, name, bs, keep_prev):
    d = Dev(g, name, bs, keep_prev=keep_prev)
    before = state_of(d.st)
    a = got(d)
    check(a, want(d, o), (name, bs, keep_prev))
    assert a[0].shape == a[1].shape == (d.B, T, d.m.dim) and a[2].shape == (d.B, T, bs) and a[3].shape == (d.B, T)
    assert np.array_equal(a[3], np.repeat(np.arange(1, d.B + 1)[:, None], T, axis=1))        # (no resample across blocks: the lineage stays)
    assert np.all(a[2][-1, :, d.n - (d.B - 1) * bs:] == 0.0)                                 # 0 beyond the short last block
    assert np.all(np.abs(a[2].sum(axis=2) - 1.0) < 1e-12)                                    # not renormalised, and 1 up to rounding
    check(got(d, steps=(2, 3)), want(d, o, 2, 3), (name, bs, keep_prev, "sub-range"))         # walked from T, written for steps 2 and 3
    mu, s2 = g.block_moments(d.st, bs)                                                       # step T is the block's own estimate
    assert eq(a[0][:, -1], mu[:, :d.m.dim]) and eq(a[1][:, -1], s2[:, :d.m.dim])
    assert eq(g.block_smoothed_weights(d.st, bs), a[2]) and len(g.block_smoothed_moments(d.st, bs, steps=T)) == 2
    assert unchanged(before, state_of(d.st))                                                 # rows, weights, parents, the store and (checkpoint) the epoch
    d.close()


def test_smoothing_moves_the_weights_of_past_steps(g):
    """somewhere below T the smoothing weights are not the step's recorded ones (otherwise the tests above compare filtering weights)"""
    d = Dev(g, "lgssm2", 129)
    W = g.block_smoothed_weights(d.st, 129)
    own = np.exp(d.S.lw[0][:129] - np.logaddexp.reduce(d.S.lw[0][:129]))
    assert np.max(np.abs(W[0, 0, :129] - own)) > 1e-4
    d.close()


# ----------------------------------------------------------------------------- 2. single properties
def test_line_model_weights_sit_on_the_slopes_alive_at_T(g, o):
    bs = 129
    d = Dev(g, "line_model", bs, n=8 * bs)
    a = got(d)
    check(a, want(d, o), "line_model")
    W, zero = a[2], 0
    for b in range(d.B):
        alive = np.unique(d.S.x(T)[b * bs:(b + 1) * bs][W[b, T - 1] > 0, 0])
        for s in range(1, T):
            slopes = d.S.x(s)[b * bs:(b + 1) * bs, 0]
            assert np.all(np.isin(slopes[W[b, s - 1] > 0], alive)), (b, s)
            zero += int(((W[b, s - 1] == 0) & np.isfinite(d.S.lw[s - 1][b * bs:(b + 1) * bs])).sum())
    assert zero > 0                                                          # (the -Inf transition took weight away from particles that had some)
    d.close()


def test_the_ess_gate_leaves_unequal_weights_in_the_store(g, o):
    d = Dev(g, "lgssm2", 7, n=40 * 7 + 5, ess_frac=0.5)
    assert d.n_res > 0 and d.n_not > 0, (d.n_res, d.n_not)
    check(got(d), want(d, o), "ess gate")
    d.close()


def test_per_block_parameters_are_the_final_blocks(g, o):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    bs = 129
    assign = np.arange((n_of(bs) + bs - 1) // bs) % 3
    d = Dev(g, "object_motion", bs, keep_prev=True, params=[sets[k] for k in assign])
    a = got(d)
    P = np.stack([sets[k].params for k in assign])
    check(a, want(d, o, P=P), "block params")
    assert not eq(a[2], want(d, o, P=sets[0].params)[2])                     # (the rows matter)
    d.close()


# ----------------------------------------------------------------------------- 3. the nested filter
@pytest.mark.parametrize("bs", [8, 300])
def test_nested_filter_follows_the_lineages_blocks(g, o, bs):
    d = Dev(g, "object_motion", bs, n=24 * bs, keep_prev=True, ess_frac=0.8, across=True)
    assert d.fired > 0
    a = got(d)
    check(a, want(d, o), ("nested", bs))
    blocks = a[3]
    assert np.array_equal(blocks[:, -1], np.arange(1, d.B + 1)) and np.all((blocks >= 1) & (blocks <= d.B))
    for s in range(T, 1, -1):                                                # c_{s-1} is the block of the recorded parents of block c_s
        born = d.S.step_map(s)[(blocks[:, s - 1] - 1) * bs] // bs
        assert np.array_equal(blocks[:, s - 2] - 1, born), s
    assert np.any(blocks != blocks[:, -1:])                                  # (some lineage changed its block)
    d.close()


# ----------------------------------------------------------------------------- 4. a whole-filter resample inside a block-wise step
def test_a_whole_filter_resample_leaves_the_scattered_blocks_undefined(g, o):
    """step 2 ends with pf_resample on the whole filter from weights that sit on two particles of different blocks: a block of two particles has both
    parents in one block (its lineage goes on there) or one in each (undefined: NaN and 0 from step 1 down); steps 2 .. T are unaffected"""
    bs, B = 2, 64
    n = bs * B

    def scatter(d, t):
        if t == 2:
            lw = np.full(n, -40.0)
            lw[5] = lw[40] = 0.0
            d.st.log_weights = lw
            g.pf_resample(d.st, "multinomial", check=False)
            d.epoch += 1
            d.S.resample_global(d.st.parents)

    d = Dev(g, "lgssm2", bs, n=n, resample=False, after_update=scatter)
    a = got(d)
    check(a, want(d, o), "whole-filter resample")
    born = d.S.step_map(2).reshape(B, bs) // bs
    mixed = born[:, 0] != born[:, 1]
    assert mixed.any() and (~mixed).any()
    assert np.all(a[3][mixed, 0] == 0) and np.all(np.isnan(a[0][mixed, 0])) and np.all(np.isnan(a[1][mixed, 0])) and np.all(np.isnan(a[2][mixed, 0]))
    assert np.array_equal(a[3][~mixed, 0], born[~mixed, 0] + 1) and np.all(np.isfinite(a[0][~mixed, 0]))
    assert np.all(np.isfinite(a[0][:, 1:])) and np.all(a[3][:, 1:] == np.arange(1, B + 1)[:, None])
    d.close()


# ----------------------------------------------------------------------------- 5. edge weights
@pytest.mark.parametrize("bs,B", [(7, 64), (513, 3)])                        # a wave team; the workgroup team with a ragged lane and wave
def test_a_particle_of_weight_zero_at_a_past_step_has_smoothing_weight_zero(g, o, bs, B):
    dead = np.arange(bs * B) % bs % 2 == 1                                   # local 1, 3, 5 of every block

    def kill(d, t):
        if t == 2:                                                           # step 2, which no resample follows: the -Inf weights stay in its record
            lw = d.st.log_weights
            lw[dead] = -np.inf
            d.st.log_weights = lw

    d = Dev(g, "lgssm2", bs, n=bs * B, resample=False, after_update=kill)
    assert np.all(np.isneginf(d.S.lw[1][dead])) and np.all(np.isfinite(d.S.lw[1][~dead]))
    a = got(d)
    check(a, want(d, o), "dead particles")
    W2 = a[2][:, 1].reshape(-1)
    assert np.all(W2[dead] == 0.0) and np.all(np.abs(a[2][:, 1].sum(axis=1) - 1.0) < 1e-12)          # exactly zero; the others carry all the mass
    d.close()


@pytest.mark.parametrize("bs,B", [(129, 4), (513, 4)])                       # a wave team; the workgroup team with a ragged lane and wave
def test_a_target_no_candidate_leads_to_hands_its_mass_to_its_recorded_parent(g, o, bs, B):
    odd = np.arange(bs * B) % 3 == 0

    def foreign_slope(d, t):
        if t == T:                                                           # the last step: a slope outside uniform_discrete(-2, 2), which no particle of step
            rows = d.st.traces                                               # T - 1 holds, and equal weights, so that the step's resample keeps such particles
            rows[odd, 0] = 7.0
            d.st.traces = rows
            d.st.log_weights = np.zeros(bs * B)

    d = Dev(g, "line_model", bs, n=bs * B, after_update=foreign_slope, final_resample=True)
    a = got(d)
    check(a, want(d, o), "fallback")
    W = a[2]
    xT = d.S.x(T).reshape(B, bs, -1)
    held = xT[:, :, 0] == 7.0
    assert held.any() and (~held).any()
    parent = d.S.step_map(T).reshape(B, bs) - np.arange(B)[:, None] * bs     # local: every block resampled inside itself
    for b in range(B):                                                       # the mass of the foreign targets alone, parent by parent, in ascending j
        acc = np.zeros(bs)
        for j in np.flatnonzero(held[b]):
            acc[parent[b, j]] = acc[parent[b, j]] + W[b, T - 1, j]
        assert np.all(W[b, T - 2] >= acc) and acc.sum() > 0
    assert np.all(np.abs(W[:, T - 2].sum(axis=1) - 1.0) < 1e-12)             # no mass is lost
    d.close()


@pytest.mark.parametrize("bs", [7, 513])                                      # (n_of: three full blocks and a short fourth)
def test_a_nan_block_reads_nan(g, bs):
    a, b = Dev(g, "lgssm2", bs), Dev(g, "lgssm2", bs)
    lw = b.st.log_weights
    lw[bs + 3] = np.nan
    b.st.log_weights = lw
    ra, rb = got(a), got(b)
    assert all(np.all(np.isnan(x[1])) for x in rb[:3]) and np.all(rb[3][1] == 0)
    keep = np.arange(a.B) != 1
    assert all(eq(x[keep], y[keep]) for x, y in zip(ra, rb))
    a.close(); b.close()


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_change_nothing(g):
    m = g.models.object_motion()
    bs, n, B = 7, 26, 4
    ys = block_obs(g, m, B, 3)
    E = g.ErrorException
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def raw(st, size=bs, lo=1, hi=2, out=True):
        return st._L.gpf_block_smooth(st._h, size, lo, hi, P(np.empty(B * 3 * 2)) if out else None, None, None, None)

    def raw_refused(st, code, store=True, **kw):
        before = snapshot(st, store)
        assert raw(st, **kw) == code and unchanged(before, snapshot(st, store)), kw

    # no store; a store without the weights mode (a state without history_weights is what it was: the call is refused, nothing else differs)
    plain = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED)
    refused(g, plain, lambda: g.block_smoothed_moments(plain, bs), E, store=False)
    raw_refused(plain, g._lib.ERR_STATE, store=False)
    plain.close()
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, history=3)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    with pytest.raises(E, match="history_weights=True"):
        g.block_smoothed_weights(st, bs)
    raw_refused(st, g._lib.ERR_STATE)
    st.close()
    # the weights mode: bad steps, all outputs NULL, a bad block size
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, history=3, history_weights=True)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    for steps in ((0, 2), (2, 1), (1, 3), 3):
        refused(g, st, lambda: g.block_smoothed_moments(st, bs, steps=steps), E)
    for kw in (dict(lo=0), dict(lo=2, hi=1), dict(hi=3), dict(out=False), dict(size=0)):
        raw_refused(st, g._lib.ERR_INVALID_ARGUMENT, **kw)
    raw_refused(st, g._lib.ERR_INVALID_ARGUMENT, size=13)                    # (not the size the walked step was entered with)
    assert g.block_smoothed_moments(st, bs)[0].shape == (B, 2, 2)            # (the state is alive and well)
    # a whole-filter update in the walked range: step 3 has no per-block observation rows
    g.pf_update(st, (3,), (None,), ys[0, 2])
    refused(g, st, lambda: g.block_smoothed_moments(st, bs), E)
    raw_refused(st, g._lib.ERR_STATE, hi=3)
    assert g.block_smoothed_weights(st, bs, steps=3).shape == (B, 1, bs)     # (step 3 alone walks nothing)
    st.close()
    # blocks of 4096 particles
    big = g.pf_initialize_blocks(m, (1,), np.tile(ys[0, 0], (2, 1)), 2 * 4096, 4096, seed=SEED, history=2, history_weights=True)
    refused(g, big, lambda: g.block_smoothed_moments(big, 4096), E)
    before = snapshot(big)
    assert big._L.gpf_block_smooth(big._h, 4096, 1, 1, P(np.empty(4)), None, None, None) == g._lib.ERR_STATE and unchanged(before, snapshot(big))
    big.close()
    # a block size that differs from the per-block parameters'
    sets = [g.models.object_motion(), g.models.object_motion(sy=0.2)]
    bp = g.pf_initialize_blocks(m, (1,), ys[:2, 0], 28, 14, seed=SEED, history=2, history_weights=True, params=sets)
    refused(g, bp, lambda: g.block_smoothed_moments(bp, 7), E)
    bp.close()


# ----------------------------------------------------------------------------- 7. laws, and what the feature is for
def test_backward_draws_have_the_smoothing_weights_as_their_marginal(g):
    """two kernels, one law: 16 blocks of 16 lgssm2 particles, T = 6, 4096 backward draws per block; count / k of every (block, step, particle) against
    W_s in units of sqrt(W (1 - W) / k), over the cells with k W >= 5: within 5 units (the two CPU restatements with the same seeds:
    block_smooth_spec.PAIR_REHEARSED)"""
    d = Dev(g, "lgssm2", ssp.PAIR_N, n=ssp.PAIR_B * ssp.PAIR_N, steps=ssp.PAIR_T, seed=ssp.PAIR_SEED)
    W = g.block_smoothed_weights(d.st, ssp.PAIR_N)
    _, idx = g.block_backward_trajectories(d.st, ssp.PAIR_N, ssp.PAIR_K, return_indices=True)
    d.close()
    worst, cells = ssp.pair_units(idx, W, ssp.PAIR_N)
    print("backward simulation against the smoothing weights:", cells, "cells, worst", round(worst, 2))
    assert cells > 200 and worst <= ssp.PAIR_SIGMAS, (worst, cells)


def test_smoothed_means_follow_the_exact_smoother(g):
    """lgssm2 defaults, T = 8, LAW_B blocks of LAW_N particles on the same data, multinomial every step: the across-block average of the smoothed mean of
    every step and column within 5 across-block standard errors of the exact smoother's.  FFBSm is consistent, not unbiased: block_smooth_spec.LAW_N is
    the smallest of 64, 128, 256 at which the CPU restatement of this seeded experiment stays inside the bound (block_smooth_spec.LAW_REHEARSED) --
    fixed from the restatement, not from the device."""
    m, ys, mu, _ = bsp.law_setup(g.models)
    N = ssp.LAW_N
    d = Dev(g, "lgssm2", N, n=ssp.LAW_B * N, steps=ssp.LAW_T, seed=ssp.LAW_SEED, ys=np.tile(ys[None], (ssp.LAW_B, 1, 1)))
    mean, _ = g.block_smoothed_moments(d.st, N)
    d.close()
    z = ssp.law_units(mean, mu)
    print("marginal smoothing: mean z", np.round(z, 2).tolist())
    assert np.all(z <= ssp.LAW_SIGMAS), z


def test_smoothed_means_of_step_1_spread_less_than_the_ancestral_ones(g):
    """what it is for: lgssm2, T = 32, 256 blocks of 16 particles on the same data, multinomial every step.  Every block's genealogy has coalesced, so
    the ancestral block_mean(state, bs, (1, c)) is one particle's x_1; the smoothed mean averages over the block's step-1 particles"""
    Tl, B, N = 32, 256, 16
    m = g.models.lgssm2()
    ys = np.asarray(g.models.simulate(m, Tl))
    d = Dev(g, "lgssm2", N, n=B * N, steps=Tl, ys=np.tile(ys[None], (B, 1, 1)))
    mean, _ = g.block_smoothed_moments(d.st, N, steps=1)
    for c in range(m.dim):
        anc = g.block_mean(d.st, N, (1, c))
        print("column", c, ": spread over", B, "blocks of the step-1 mean: ancestral", float(anc.std()), "smoothed", float(mean[:, 0, c].std()))
        assert mean[:, 0, c].std() < anc.std()
    d.close()
