"""Pairwise smoothing per block on the device against its DEFINITION: hp_checks.check_pairs over the mpmath reference of tests/hp_weights.py
(smooth_step's pair sums, second, cross), fed with what a caller sees -- the Store of tests/block_backward_spec.py filled by the Dev helper and the
outputs of block_smoothed_pair_moments(..., return_blocks=True).  tests/test_hp_block_pairs.py is the CPU rehearsal: the same check on the NumPy
restatement, the negative controls, the guard's condition and the evidence for shapes and thinning; its cases, constants and helpers are used here.
tests/test_gpu_block_pairs.py compares the kernel bit for bit with a twin written beside it and cannot see a mistake the two share; this can.  Every
tolerance is a derived E bound.  The reference is the cost (about 0.2 ms per (target, candidate) pair): the thinning is the rehearsal's."""
import numpy as np
import pytest

import hp_checks as hc
import test_hp_block_pairs as cpu
import test_hp_block_smoothing as cpu_s
from test_gpu_hp_block_smoothing import dev, thin

pytestmark = pytest.mark.gpu
T, SIZES = cpu.T, cpu.SIZES


def got(d, steps=None):
    return d.g.block_smoothed_pair_moments(d.st, d.bs, steps=steps, return_blocks=True)


def pairs_case(g, name, bs, label, lo=None, sets=None, blocks=None, steps=None, **kw):
    """(Dev, fallbacks, outputs) of one checked case"""
    d, refs = dev(g, name, bs, T, sets=sets, **kw)
    blocks = cpu_s.blocks_of(bs) if blocks is None else blocks
    if name == "object_motion":
        hc.moving_inputs(d.S, blocks, label=label)
    out, v = got(d, steps), hc.Violations()
    fell = hc.check_pairs(v, refs, d.S, blocks, *out, label, lo=lo, steps=steps)
    v.finish(label)
    return d, fell, out


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", ["object_motion", "lgssm2"])
def test_pairs_follow_the_definition(g, name, bs):
    d, _, out = pairs_case(g, name, bs, f"pairs {name} {bs}", lo=cpu_s.smooth_lo(bs), after_update=thin if bs == 513 else None)
    if bs == 513:
        assert np.isneginf(d.S.lw[-1]).sum() == d.n - cpu_s.thin_mask(d.n, bs).sum()
    assert np.all(np.isfinite(out[2]))
    d.close()


@pytest.mark.parametrize("name", ["sv1", "bearings4"])
def test_pairs_of_the_other_models(g, name):
    pairs_case(g, name, 7, f"pairs {name} 7", ess_frac=0.5)[0].close()


def test_pairs_of_four_columns_on_the_workgroup_team(g):
    """bearings4 at 513: the last step thinned to KEEP survivors, one block, the top transition only"""
    pairs_case(g, "bearings4", 513, "pairs bearings4 513", after_update=thin, **cpu.BEARINGS_WIDE)[0].close()


@pytest.mark.parametrize("name,bs", cpu_s.DEAD)
def test_pairs_with_dead_and_flushed_past_particles(g, name, bs):
    """the case of the CPU rehearsal: no resample; after step 2 some weights become -Inf and one per block -800 (kill)"""
    def kill(d, t):
        if t == 2:                                                           # step 2, which no resample follows: the weights stay in its record
            dead, flushed = cpu_s.kill(d.n, bs)
            lw = d.st.log_weights
            lw[dead], lw[flushed] = -np.inf, -800.0
            d.st.log_weights = lw

    blocks = cpu_s.dead_blocks(bs)
    d, _, out = pairs_case(g, name, bs, f"pairs {name} {bs} with dead particles", blocks=blocks, resample=False, after_update=kill)
    dead, flushed = cpu_s.kill(d.n, bs)
    assert np.isneginf(d.S.lw[1][dead]).all() and np.all(d.S.lw[1][flushed] == -800.0) and np.all(np.isfinite(out[2][blocks]))
    d.close()


def test_pairs_fallback_hands_the_pair_to_the_recorded_parent(g):
    """line_model with a foreign slope on every third particle of step T (the case of tests/test_gpu_hp_block_smoothing.py)"""
    bs, B = 129, 4

    def foreign_slope(d, t):
        if t == T:
            rows = d.st.traces
            rows[np.arange(bs * B) % 3 == 0, 0] = 7.0
            d.st.traces = rows
            d.st.log_weights = np.zeros(bs * B)

    d, fell, _ = pairs_case(g, "line_model", bs, "pairs fallback", n=bs * B, after_update=foreign_slope, final_resample=True)
    assert fell > 0
    d.close()


def test_pairs_with_block_parameters(g):
    pairs_case(g, "object_motion", 7, "pairs block parameters", sets=cpu_s.param_sets(g), keep_prev=True)[0].close()


def test_a_nan_block_reads_nan_and_lineage_0(g):
    d, refs = dev(g, "lgssm2", 7, T)
    lw = d.st.log_weights
    lw[7 + 3] = np.nan
    d.st.log_weights = lw
    d.S.lw[-1] = lw.copy()
    out, v = got(d), hc.Violations()
    hc.check_pairs(v, refs, d.S, cpu_s.blocks_of(7), *out, "pairs, a NaN block")
    assert all(np.isnan(x[1]).all() for x in out[:3]) and np.all(out[3][1] == 0) and np.isfinite(out[2][0]).all()
    v.finish("pairs, a NaN block")
    d.close()


def test_a_windowed_call_is_walked_from_the_last_step(g):
    d, _, out = pairs_case(g, "lgssm2", 7, "pairs, steps (1, 2)", steps=cpu.WINDOW)
    assert out[0].shape[1] == 2 and out[2].shape[1] == 1
    d.close()


def test_both_smoothers_in_the_nested_filter(g):
    """block resample, then resampling across blocks, every step: the targets' block, the candidates' block and the observation row differ only here.
    Every block, both smoothers, one reference walk"""
    bs, B = cpu.NESTED_BS, cpu.NESTED_B
    m = hc.case_model(g, "object_motion")
    d, refs = dev(g, "object_motion", bs, T, n=B * bs, keep_prev=True, ess_frac=0.8, across=True, ys=cpu.nested_obs(g, m))
    blocks = list(range(B))
    assert d.fired > 0
    hc.moving_inputs(d.S, blocks, travelling=True, label="nested")
    walk = hc.reference_walk(refs, d.S, blocks, pairs=True)
    out, v = got(d), hc.Violations()
    hc.check_pairs(v, refs, d.S, blocks, *out, "pairs nested", walk=walk)
    v.finish("pairs nested")
    print("nested: (block, step) where the lineage changed its block:", cpu.check_nested(out[3], d.S))
    sm, v = g.block_smoothed_moments(d.st, bs, return_weights=True, return_blocks=True), hc.Violations()
    hc.check_smooth(v, refs, d.S, blocks, *sm, "smooth nested", walk=walk)
    v.finish("smooth nested")
    d.close()


def test_a_target_of_weight_zero_with_an_infinite_row_is_skipped(g):
    """the rehearsal's case: a particle of the last step with current weight -Inf and +Inf in one column of its row, in a block that stays valid.  The
    pair below it and every lower step are finite and within bound; its own step reads NaN in that column only"""
    def poison(d, t):
        if t == T:
            dead, inf = cpu.skip_mask(d.n, 7)
            lw, rows = d.st.log_weights, d.st.traces
            lw[dead] = -np.inf
            rows[:, :2][inf] = np.inf
            d.st.log_weights, d.st.traces = lw, rows

    d, _, out = pairs_case(g, "lgssm2", 7, "pairs, a skipped target with an infinite row", after_update=poison)
    dead, inf = cpu.skip_mask(d.n, 7)
    assert np.isinf(d.S.x(T)[inf]).all() and np.isneginf(d.S.lw[-1][dead]).all()
    cpu.check_skip(out, cpu_s.blocks_of(7))
    d.close()
