"""Pairwise smoothing per block on the device (gpf.h gpf_block_smooth_pairs):

  1. mean, second moments, lag-one cross moments and lineage blocks bit for bit against the NumPy restatement of tests/block_pairs_spec.py, which is fed
     only with what a caller sees: four models, the edges of the three team shapes, a short last block, keep_prev, a sub-range with one pair, a single
     step with none; the mean is block_smoothed_moments'; second is exactly symmetric; state, store and epoch unchanged;
  2. line_model: no pair links two slopes, so cross[slope][slope] is second[slope][slope]; the ESS gate's unequal stored weights; per-block parameters;
  3. the nested filter: block resample, then resampling across blocks, every step;
  4. a whole-filter pf_resample inside a block-wise step: NaN for the scattered blocks' lower steps and the pairs touching them; a -Inf particle; a
     target on its fallback; a NaN block;
  5. refused calls change nothing;
  6. the law against the exact smoother (the CPU rehearsal and its three rejected controls: tests/test_block_pairs_host.py)."""
import ctypes as C

import numpy as np
import pytest

import block_backward_spec as bsp
import block_pairs_spec as psp
from test_block_smooth_host import gamma
from test_gpu_block_backward import MODELS, SEED, SIZES, T, Dev
from test_gpu_block_conditional import block_obs, eq, n_of, refused, snapshot, unchanged

pytestmark = pytest.mark.gpu
LEVELS = 11                                                                   # additions on a term's way up the tree of DESIGN.md 3.5


def state_of(st):
    """snapshot without the checkpoint's trailing padding (the parents are n 4-byte words in a blob of whole 8-byte words: for odd n the last four bytes
    are never written)"""
    s = snapshot(st)
    return (s[0][:len(s[0]) - (-4 * st.n_particles) % 8],) + s[1:]


def got(d, steps=None):
    return d.g.block_smoothed_pair_moments(d.st, d.bs, steps=steps, return_blocks=True)


def want(d, o, lo=1, hi=None, P=None):
    return psp.pairs(o, d.m.name, d.m.params if P is None else P, d.S, lo, hi)


def check(a, b, where):
    for k, what in enumerate(("mean", "second", "cross")):
        assert a[k].shape == b[k].shape, (where, what, a[k].shape, b[k].shape)
        assert eq(a[k], b[k]), (where, what, np.argwhere(~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))))[:5])
    assert np.array_equal(a[3], b[3]), (where, "blocks")


# ----------------------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("keep_prev,bs", [(False, bs) for bs in SIZES] + [(True, 7), (True, 513)])
@pytest.mark.parametrize("name", MODELS)
def test_moments_pairs_and_blocks_are_the_restatement(g, o, name, bs, keep_prev):
    d = Dev(g, name, bs, keep_prev=keep_prev)
    before = state_of(d.st)
    a, w = got(d), want(d, o)
    dim = d.m.dim
    check(a, w, (name, bs, keep_prev))
    assert a[0].shape == (d.B, T, dim) and a[1].shape == (d.B, T, dim, dim) and a[2].shape == (d.B, T - 1, dim, dim) and a[3].shape == (d.B, T)
    assert np.array_equal(a[3], np.repeat(np.arange(1, d.B + 1)[:, None], T, axis=1))        # (no resample across blocks: the lineage stays)
    assert np.array_equal(a[1], a[1].transpose(0, 1, 3, 2)) and np.all(np.isfinite(a[1])) and np.all(np.isfinite(a[2]))
    # walked from T, written for steps 2 and 3 and their one pair: what the restatement returns for that range (tests/test_block_pairs_host.py)
    check(got(d, steps=(2, 3)), (w[0][:, 1:3], w[1][:, 1:3], w[2][:, 1:2], w[3][:, 1:3]), (name, bs, keep_prev, "sub-range"))
    one = got(d, steps=T)                                                                    # a single step: no pair
    check(one, (w[0][:, T - 1:], w[1][:, T - 1:], w[2][:, :0], w[3][:, T - 1:]), (name, bs, keep_prev, "one step"))
    assert one[2].shape == (d.B, 0, dim, dim)
    assert eq(a[0], g.block_smoothed_moments(d.st, bs)[0])                                   # the marginal smoother's mean
    assert len(g.block_smoothed_pair_moments(d.st, bs)) == 3
    assert unchanged(before, state_of(d.st))                                                 # rows, weights, parents, the store and (checkpoint) the epoch
    d.close()


def test_the_cross_moment_is_not_the_product_of_the_means(g):
    """somewhere the pairs carry dependence (otherwise the tests above could pass on mean_s (x) mean_{s+1})"""
    d = Dev(g, "lgssm2", 129)
    mean, _, cross = g.block_smoothed_pair_moments(d.st, 129)
    assert np.max(np.abs(cross - mean[:, :-1, :, None] * mean[:, 1:, None, :])) > 1e-4
    d.close()


# ----------------------------------------------------------------------------- 2. single properties
def test_line_model_no_pair_links_two_slopes(g, o):
    """logtrans is -Inf between different slopes and a recorded parent has its child's slope, so every pair (i, j) of positive weight has x_s^i[0] =
    x_{s+1}^j[0] and in exact arithmetic cross_s[0][0] = sum_i x_s^i[0]^2 sum_j t_ij = second_s[0][0].  Roundings per term (i, j), all terms positive:
    cross -- r (1), t (1), t x (1), at most bs additions into A, x A (1), LEVELS additions; second -- r (1), t (1), at most bs additions into W, two
    products, LEVELS additions.  sum |terms| is second_s[0][0] itself up to its own gamma"""
    bs = 129
    d = Dev(g, "line_model", bs, n=8 * bs)
    a = got(d)
    check(a, want(d, o), "line_model")
    k = 4 + bs + LEVELS
    second, cross = a[1][:, :-1, 0, 0], a[2][:, :, 0, 0]
    bound = 2 * gamma(k) * second / (1 - gamma(k))
    err = np.abs(cross - second)
    live = second > 0                                                        # (a block whose whole weight sits on slope 0 has 0 = 0)
    print("line_model, cross[slope][slope] against second[slope][slope]: worst error / bound", float((err[live] / bound[live]).max()))
    assert live.any() and np.all(second >= 0) and np.all(err <= bound), (err.max(), bound.min())
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


# ----------------------------------------------------------------------------- 4. special cases
def test_a_whole_filter_resample_leaves_the_scattered_blocks_and_their_pairs_undefined(g, o):
    """step 2 ends with pf_resample on the whole filter from weights that sit on two particles of different blocks: a block of two particles has both
    parents in one block (its lineage goes on there) or one in each (undefined: step 1 and the pair (1, 2) read NaN); the rest is unaffected"""
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
    assert np.array_equal(a[3][~mixed, 0], born[~mixed, 0] + 1) and np.all(np.isfinite(a[1][~mixed, 0])) and np.all(np.isfinite(a[2][~mixed, 0]))
    assert np.all(np.isfinite(a[1][:, 1:])) and np.all(np.isfinite(a[2][:, 1:])) and np.all(a[3][:, 1:] == np.arange(1, B + 1)[:, None])
    sub = got(d, steps=(2, 4))                                               # a range above the undefined step: nothing of it is NaN
    check(sub, tuple(x[:, 1:] for x in a), "whole-filter resample, steps 2 .. 4")
    d.close()


@pytest.mark.parametrize("bs,B", [(7, 64), (513, 3)])                        # a wave team; the workgroup team with a ragged lane and wave
def test_a_particle_of_weight_zero_at_a_past_step(g, o, bs, B):
    dead = np.arange(bs * B) % bs % 2 == 1                                   # local 1, 3, 5 of every block

    def kill(d, t):
        if t == 2:                                                           # step 2, which no resample follows: the -Inf weights stay in its record
            lw = d.st.log_weights
            lw[dead] = -np.inf
            d.st.log_weights = lw

    d = Dev(g, "lgssm2", bs, n=bs * B, resample=False, after_update=kill)
    assert np.all(np.isneginf(d.S.lw[1][dead])) and np.all(np.isfinite(d.S.lw[1][~dead]))
    a = got(d)
    check(a, want(d, o), "dead particles")                                   # (the dead particles are targets of weight 0 in the walk from 2 to 1: skipped)
    assert np.all(np.isfinite(a[2]))
    d.close()


@pytest.mark.parametrize("bs,B", [(129, 4), (513, 4)])                       # a wave team; the workgroup team with a ragged lane and wave
def test_a_target_on_its_fallback(g, o, bs, B):
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
    assert np.any(d.S.x(T)[:, 0] == 7.0) and np.any(d.S.x(T)[:, 0] != 7.0)
    # the foreign targets pair slope 7 with their parents' slopes: the last pair's cross[0][0] is no longer second[0][0]
    assert np.any(a[2][:, T - 2, 0, 0] != a[1][:, T - 2, 0, 0])
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


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_change_nothing(g):
    m = g.models.object_motion()
    bs, n, B = 7, 26, 4
    ys = block_obs(g, m, B, 3)
    E = g.ErrorException
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def raw(st, size=bs, lo=1, hi=2, out=True, cross=False):
        return st._L.gpf_block_smooth_pairs(st._h, size, lo, hi, P(np.empty(B * 3 * 2)) if out else None, None, P(np.empty(B * 3 * 4)) if cross else None, None)

    def raw_refused(st, code, store=True, **kw):
        before = snapshot(st, store)
        assert raw(st, **kw) == code and unchanged(before, snapshot(st, store)), kw

    # no store; a store without the weights mode
    plain = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED)
    refused(g, plain, lambda: g.block_smoothed_pair_moments(plain, bs), E, store=False)
    raw_refused(plain, g._lib.ERR_STATE, store=False)
    plain.close()
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, history=3)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    with pytest.raises(E, match="history_weights=True"):
        g.block_smoothed_pair_moments(st, bs)
    raw_refused(st, g._lib.ERR_STATE)
    st.close()
    # the weights mode: bad steps, all outputs NULL, cross_out with one step, a bad block size
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, history=3, history_weights=True)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    for steps in ((0, 2), (2, 1), (1, 3), 3):
        refused(g, st, lambda: g.block_smoothed_pair_moments(st, bs, steps=steps), E)
    for kw in (dict(lo=0), dict(lo=2, hi=1), dict(hi=3), dict(out=False), dict(size=0), dict(lo=2, hi=2, cross=True), dict(lo=1, hi=1, out=False, cross=True)):
        raw_refused(st, g._lib.ERR_INVALID_ARGUMENT, **kw)
    raw_refused(st, g._lib.ERR_INVALID_ARGUMENT, size=13)                    # (not the size the walked step was entered with)
    assert raw(st, cross=True) == 0 and raw(st, out=False, cross=True) == 0  # (a pair in the range: cross_out alone is a call)
    assert [x.shape for x in g.block_smoothed_pair_moments(st, bs)] == [(B, 2, 2), (B, 2, 2, 2), (B, 1, 2, 2)]       # (the state is alive and well)
    # a whole-filter update in the walked range: step 3 has no per-block observation rows
    g.pf_update(st, (3,), (None,), ys[0, 2])
    refused(g, st, lambda: g.block_smoothed_pair_moments(st, bs), E)
    raw_refused(st, g._lib.ERR_STATE, hi=3)
    assert g.block_smoothed_pair_moments(st, bs, steps=3)[1].shape == (B, 1, 2, 2)           # (step 3 alone walks nothing)
    st.close()
    # blocks of 4096 particles
    big = g.pf_initialize_blocks(m, (1,), np.tile(ys[0, 0], (2, 1)), 2 * 4096, 4096, seed=SEED, history=2, history_weights=True)
    refused(g, big, lambda: g.block_smoothed_pair_moments(big, 4096), E)
    before = snapshot(big)
    assert big._L.gpf_block_smooth_pairs(big._h, 4096, 1, 1, P(np.empty(4)), None, None, None) == g._lib.ERR_STATE and unchanged(before, snapshot(big))
    big.close()
    # a block size that differs from the per-block parameters'
    sets = [g.models.object_motion(), g.models.object_motion(sy=0.2)]
    bp = g.pf_initialize_blocks(m, (1,), ys[:2, 0], 28, 14, seed=SEED, history=2, history_weights=True, params=sets)
    refused(g, bp, lambda: g.block_smoothed_pair_moments(bp, 7), E)
    bp.close()


# ----------------------------------------------------------------------------- 6. the law
def test_pair_moments_follow_the_exact_smoother(g):
    """lgssm2 defaults, T = 8, LAW_B blocks of LAW_N particles on the same data, multinomial every step: the across-block average of every entry of
    cross_s and second_s within 5 across-block standard errors of the exact smoother's Sigma[s, s+1] + mu_s mu_{s+1}' and Sigma[s, s] + mu_s mu_s'.
    block_pairs_spec.LAW_N is the smallest of 64, 128, 256 at which the CPU restatement of this seeded experiment stays inside the bound
    (block_pairs_spec.LAW_REHEARSED) -- fixed from the restatement, not from the device; the same run rejects three wrong answers there"""
    m, ys, mu, Sigma = bsp.law_setup(g.models)
    N = psp.LAW_N
    d = Dev(g, "lgssm2", N, n=psp.LAW_B * N, steps=psp.LAW_T, seed=psp.LAW_SEED, ys=np.tile(ys[None], (psp.LAW_B, 1, 1)))
    mean, second, cross = g.block_smoothed_pair_moments(d.st, N)
    d.close()
    exact_second, exact_cross = psp.law_exact(mu, Sigma)
    zs, zc = psp.law_units(second, exact_second), psp.law_units(cross, exact_cross)
    print("pairwise smoothing: second worst", round(float(zs.max()), 2), "cross worst", round(float(zc.max()), 2),
          "controls", {k: round(v, 2) for k, v in psp.law_controls(cross, mean, exact_cross).items()})
    assert np.all(zs <= psp.LAW_SIGMAS) and np.all(zc <= psp.LAW_SIGMAS), (zs, zc)
