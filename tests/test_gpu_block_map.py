"""The most probable path per block on the device (gpf.h gpf_block_map_path):

  1. paths, indices and logp bit for bit against the NumPy restatement of tests/block_map_spec.py, which is fed only with what a caller sees: five models,
     the edges of the wave, the two wave-team shapes and the workgroup team, a short last block, a step and a sub-range of steps; the query twice gives
     the same bits and changes nothing -- state, store, epoch, and what block_smoothed_moments returns afterwards;
  2. the nested filter; per-block parameters; a rejuvenation behind a resample; ESS-gated steps with identity maps;
  3. the -Inf and NaN rules: no sequence of positive density (line_model, a slope no child holds), NaN totals, an undefined lineage (NaN at EVERY step);
  4. refused calls change nothing;
  5. what it is for: object_motion's MAP `moving` sequence against the per-step smoothed majority where that majority is clear.

(The restatement against the enumeration of all sequences: tests/test_block_map_host.py.)"""
import ctypes as C

import numpy as np
import pytest

import block_map_spec as msp
from test_gpu_block_backward import SEED, Dev, quiet
from test_gpu_block_conditional import block_obs, eq, n_of, refused, snapshot, unchanged
from test_gpu_block_smooth import state_of

pytestmark = pytest.mark.gpu
MODELS = ["lgssm2", "sv1", "object_motion", "line_model", "bearings4"]
SIZES = [1, 2, 7, 64, 65, 128, 129, 256, 257, 512, 513, 2048]               # a wave 2 / 8 per lane, the workgroup, and the edges of a wave and of each shape


def got(d, steps=None):
    return d.g.block_map_trajectories(d.st, d.bs, steps=steps, return_indices=True, return_log_density=True)


def want(d, o, lo=1, hi=None, P=None):
    return msp.map_paths(o, d.m.name, d.m.params if P is None else P, d.S, lo, hi)


def check(a, b, where):
    assert eq(a[2], b[2]), (where, "logp", a[2], b[2])
    assert np.array_equal(a[1], b[1]), (where, "indices", np.argwhere(a[1] != b[1])[:5])
    assert eq(a[0], b[0]), (where, "paths")


# ----------------------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_paths_indices_and_logp_are_the_restatement(g, o, name, bs):
    T = 4 if bs <= 7 else 3
    d = Dev(g, name, bs, steps=T)
    before = state_of(d.st)
    mom = g.block_smoothed_moments(d.st, bs)
    a = got(d)
    w = want(d, o)
    check(a, w, (name, bs))
    assert a[0].shape == (d.B, T, d.m.dim) and a[1].shape == (d.B, T) and a[2].shape == (d.B,)
    assert np.all(np.isfinite(a[2])) and np.all((a[1] - 1) // bs == np.arange(d.B)[:, None])   # (no resample across blocks: the lineage stays)
    for s in range(1, T + 1):                                                # the path is the rows its indices name
        assert eq(a[0][:, s - 1], d.S.x(s)[a[1][:, s - 1] - 1])
    check(got(d, steps=(2, 3)), (w[0][:, 1:3], w[1][:, 1:3], w[2]), (name, bs, "sub-range"))   # maximised over all steps, written for steps 2 and 3
    check(got(d, steps=1), (w[0][:, :1], w[1][:, :1], w[2]), (name, bs, "one step"))
    assert eq(g.block_map_trajectories(d.st, bs), a[0]) and len(g.block_map_trajectories(d.st, bs, return_log_density=True)) == 2
    b = got(d)                                                               # twice: the same bits
    assert all(eq(x, y) for x, y in zip(a, b))
    assert unchanged(before, state_of(d.st))                                 # rows, weights, parents, the store and (checkpoint) the epoch
    assert all(eq(x, y) for x, y in zip(mom, g.block_smoothed_moments(d.st, bs)))
    d.close()


def test_the_map_path_is_not_the_ancestral_line_of_a_particle(g):
    """somewhere the path leaves the recorded genealogy (otherwise the tests above compare ancestral paths)"""
    d = Dev(g, "lgssm2", 129, steps=4)
    _, idx, _ = got(d)
    off = sum(int(np.sum(d.S.step_map(s)[idx[:, s - 1] - 1] != idx[:, s - 2] - 1)) for s in range(2, 5))
    assert off > 0
    d.close()


# ----------------------------------------------------------------------------- 2. the filters the store serves
@pytest.mark.parametrize("bs", [8, 300])
def test_nested_filter_follows_the_lineages_blocks(g, o, bs):
    d = Dev(g, "object_motion", bs, n=24 * bs, keep_prev=True, ess_frac=0.8, across=True)
    assert d.fired > 0
    a = got(d)
    check(a, want(d, o), ("nested", bs))
    blocks = (a[1] - 1) // bs
    assert np.array_equal(blocks[:, -1], np.arange(d.B)) and np.any(blocks != blocks[:, -1:])            # (some lineage changed its block)
    assert len({tuple(r) for r in blocks[:, :1].tolist()}) < d.B                                         # (final blocks share a lineage block at step 1)
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


@pytest.mark.parametrize("bs", [7, 300])
def test_a_rejuvenation_behind_a_resample(g, o, bs):
    """the store's snapshot of a step is what the step ended with: the moved rows"""
    moved = []

    def resample_and_move(d, t):
        if t < 4:
            quiet(lambda: g.pf_resample_blocks(d.st, bs, "multinomial", check=False))
            d.S.resample_blocks(d.st.parents, g.block_resampled(d.st))
            rows = d.st.traces
            g.pf_rejuvenate_blocks(d.st, None, (), 1, method="move")
            moved.append(not eq(rows, d.st.traces))

    d = Dev(g, "lgssm2", bs, steps=4, keep_prev=True, resample=False, after_update=resample_and_move)
    assert any(moved)
    check(got(d), want(d, o), ("rejuvenated", bs))
    d.close()


def test_ess_gated_steps_have_identity_maps(g, o):
    d = Dev(g, "lgssm2", 7, n=40 * 7 + 5, ess_frac=0.5)
    assert d.n_res > 0 and d.n_not > 0, (d.n_res, d.n_not)
    check(got(d), want(d, o), "ess gate")
    d.close()


# ----------------------------------------------------------------------------- 3. the -Inf and NaN rules
@pytest.mark.parametrize("bs,B", [(7, 8), (513, 3)])
def test_no_sequence_of_positive_density_reads_minus_inf_and_nan(g, o, bs, B):
    T = 4

    def foreign_slope(d, t):
        if t == T:                                                           # every particle of block 1 on a slope outside uniform_discrete(-2, 2) at the last step
            rows = d.st.traces
            rows[bs:2 * bs, 0] = 7.0
            d.st.traces = rows

    d = Dev(g, "line_model", bs, n=bs * B, after_update=foreign_slope)
    a = got(d)
    check(a, want(d, o), ("dead block", bs))
    assert np.isneginf(a[2][1]) and np.all(np.isnan(a[0][1])) and np.all(a[1][1] == 0)
    keep = np.arange(B) != 1
    assert np.all(np.isfinite(a[2][keep])) and np.all(a[1][keep] >= 1)
    for b in np.flatnonzero(keep):                                           # one slope along the whole path
        assert np.all(a[0][b, :, 0] == a[0][b, 0, 0])
    d.close()


@pytest.mark.parametrize("bs", [7, 513])
def test_nan_totals_read_nan(g, o, bs):
    def poison(d, t):
        if t == 1:                                                           # block 1's step-1 rows: every later row and every score of the block is NaN
            rows = d.st.traces
            rows[bs:2 * bs] = np.nan
            d.st.traces = rows

    d = Dev(g, "lgssm2", bs, resample=False, after_update=poison)
    a = got(d)
    check(a, want(d, o), ("nan", bs))
    assert np.isnan(a[2][1]) and np.all(np.isnan(a[0][1])) and np.all(a[1][1] == 0)
    keep = np.arange(d.B) != 1
    assert np.all(np.isfinite(a[2][keep])) and np.all(a[1][keep] >= 1)
    d.close()


def test_a_whole_filter_resample_leaves_the_scattered_blocks_without_a_path(g, o):
    """step 2 ends with pf_resample on the whole filter from weights that sit on two particles of different blocks: a block of two particles has both
    parents in one block (its lineage goes on there) or one in each -- then the block has no path at ANY step (the smoothers still answer steps 2 .. T)"""
    bs, B = 2, 64
    n = bs * B

    def scatter(d, t):
        if t == 2:
            lw = np.full(n, -40.0)
            lw[5] = lw[40] = 0.0
            d.st.log_weights = lw
            g.pf_resample(d.st, "multinomial", check=False)
            d.S.resample_global(d.st.parents)

    d = Dev(g, "lgssm2", bs, n=n, resample=False, after_update=scatter)
    a = got(d)
    check(a, want(d, o), "whole-filter resample")
    born = d.S.step_map(2).reshape(B, bs) // bs
    mixed = born[:, 0] != born[:, 1]
    assert mixed.any() and (~mixed).any()
    assert np.all(a[1][mixed] == 0) and np.all(np.isnan(a[0][mixed])) and np.all(np.isnan(a[2][mixed]))
    assert np.all(a[1][~mixed] >= 1) and np.all(np.isfinite(a[0][~mixed])) and np.all(np.isfinite(a[2][~mixed]))
    assert np.array_equal((a[1][~mixed, 0] - 1) // bs, born[~mixed, 0])
    d.close()


# ----------------------------------------------------------------------------- 4. refusals
def test_refusals_change_nothing(g):
    m = g.models.object_motion()
    bs, n, B = 7, 26, 4
    ys = block_obs(g, m, B, 3)
    E = g.ErrorException
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def raw(st, size=bs, lo=1, hi=2, out=True):
        return st._L.gpf_block_map_path(st._h, size, lo, hi, P(np.empty(B * 3 * 2)) if out else None, None, None)

    def raw_refused(st, code, store=True, **kw):
        before = snapshot(st, store)
        assert raw(st, **kw) == code and unchanged(before, snapshot(st, store)), kw

    # no store; a store without the weights mode
    plain = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED)
    refused(g, plain, lambda: g.block_map_trajectories(plain, bs), E, store=False)
    raw_refused(plain, g._lib.ERR_STATE, store=False)
    plain.close()
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, history=3)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    with pytest.raises(E, match="history_weights=True"):
        g.block_map_trajectories(st, bs)
    raw_refused(st, g._lib.ERR_STATE)
    st.close()
    # the weights mode: bad steps, all outputs NULL, a bad block size
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, history=3, history_weights=True)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    for steps in ((0, 2), (2, 1), (1, 3), 3):
        refused(g, st, lambda: g.block_map_trajectories(st, bs, steps=steps), E)
    for kw in (dict(lo=0), dict(lo=2, hi=1), dict(hi=3), dict(out=False), dict(size=0)):
        raw_refused(st, g._lib.ERR_INVALID_ARGUMENT, **kw)
    raw_refused(st, g._lib.ERR_INVALID_ARGUMENT, size=13)                    # (not the size the steps were entered with)
    before = snapshot(st)
    lp = np.empty(B)
    assert st._L.gpf_block_map_path(st._h, bs, 1, 2, None, None, P(lp)) == 0 and np.all(np.isfinite(lp))      # (logp alone is a query)
    assert g.block_map_trajectories(st, bs).shape == (B, 2, 2) and unchanged(before, snapshot(st))
    # a whole-filter update: step 3 has no per-block observation rows, and the recursion walks EVERY step whatever the range
    g.pf_update(st, (3,), (None,), ys[0, 2])
    refused(g, st, lambda: g.block_map_trajectories(st, bs), E)
    refused(g, st, lambda: g.block_map_trajectories(st, bs, steps=1), E)
    raw_refused(st, g._lib.ERR_STATE, hi=3)
    st.close()
    # blocks of 4096 particles
    big = g.pf_initialize_blocks(m, (1,), np.tile(ys[0, 0], (2, 1)), 2 * 4096, 4096, seed=SEED, history=2, history_weights=True)
    refused(g, big, lambda: g.block_map_trajectories(big, 4096), E)
    before = snapshot(big)
    assert big._L.gpf_block_map_path(big._h, 4096, 1, 1, P(np.empty(4)), None, None) == g._lib.ERR_STATE and unchanged(before, snapshot(big))
    big.close()
    # a block size that differs from the per-block parameters'
    sets = [g.models.object_motion(), g.models.object_motion(sy=0.2)]
    bp = g.pf_initialize_blocks(m, (1,), ys[:2, 0], 28, 14, seed=SEED, history=2, history_weights=True, params=sets)
    refused(g, bp, lambda: g.block_map_trajectories(bp, 7), E)
    bp.close()


# ----------------------------------------------------------------------------- 5. what it is for
SENSE_B, SENSE_N, SENSE_T, SENSE_SEED = 64, 256, 10, 17
SENSE_CLEAR = (0.2, 0.8)                                                     # a smoothed proportion outside this interval is a clear majority


def sense_data(g):
    """the README example: the object stays still for 5 steps, then oscillates for 5; every block its own noisy observations"""
    m = g.models.object_motion()
    rng = np.random.default_rng(SENSE_SEED)
    y, ys = 0.0, np.zeros((SENSE_B, SENSE_T, 2))
    for t in range(1, SENSE_T + 1):
        y += np.sin(t) if t > 5 else 0.0
        ys[:, t - 1, 0] = y + m.info["sobs"] * rng.standard_normal(SENSE_B)
        ys[:, t - 1, 1] = np.sin(t)
    return m, ys


def sense_agreement(moving, W, x_moving):
    """moving [B, T] the MAP sequence, W [B, T, N] smoothing weights, x_moving [B, T, N] the particles' flags -> (share of clear steps, agreement on them)"""
    prop = (W * (x_moving != 0)).sum(axis=2)
    clear = (prop < SENSE_CLEAR[0]) | (prop > SENSE_CLEAR[1])
    return float(clear.mean()), float(((moving != 0) == (prop > 0.5))[clear].mean())


def test_the_map_moving_sequence_agrees_with_the_clear_smoothed_majorities(g):
    """object_motion, 64 blocks of 256, T = 10 on the README's data (still for 5 steps, moving for 5).  Where the smoothed proportion of `moving` is outside
    [0.2, 0.8] -- at least half of all (block, step) cells for this seed -- the MAP sequence says what the majority says, in every such cell.  The two
    estimators answer different questions (the joint mode against the marginal ones), so this is no identity; it was rehearsed with the CPU restatements
    of both (tests/block_map_spec.py, tests/block_smooth_spec.py) on the oracle's filter for this seed and data: 0.892 of the 640 cells clear, no
    disagreement among them (the MAP sequences have the object moving in 0 - 2 % of the blocks at steps 1 - 5 and in 77 - 100 % at steps 6 - 10)."""
    m, ys = sense_data(g)
    d = Dev(g, "object_motion", SENSE_N, n=SENSE_B * SENSE_N, steps=SENSE_T, seed=SENSE_SEED, ys=ys, model=m, ess_frac=0.5)
    path, idx, _ = got(d)
    W = g.block_smoothed_weights(d.st, SENSE_N)
    assert np.all((idx - 1) // SENSE_N == np.arange(SENSE_B)[:, None])
    x_moving = np.stack([d.S.x(s)[:, 0].reshape(SENSE_B, SENSE_N) for s in range(1, SENSE_T + 1)], axis=1)
    d.close()
    share, agree = sense_agreement(path[:, :, 0], W, x_moving)
    print("MAP against the smoothed majority: clear cells", round(share, 3), "agreement on them", round(agree, 4))
    assert share >= 0.5, share
    assert agree == 1.0, agree
