"""Forward-only smoothing per block on the device against its DEFINITION: hp_forward.check_forward -- the mpmath values of the pairwise reference walked
backwards over the whole store, the Float64 bound of every entry derived by E propagation through the forward statements --, fed with what a caller sees:
the Store of tests/block_backward_spec.py filled by the Dev helper and the outputs of block_forward_moments.  tests/test_hp_block_forward.py is the CPU
rehearsal: the same check on the NumPy restatement and the negative controls; its cases and helpers are used here.  tests/test_gpu_block_forward.py
compares the kernel bit for bit with a twin written beside it and cannot see a mistake the two share; this can.  No value is skipped."""
import numpy as np
import pytest

import hp_checks as hc
import hp_forward as hf
import hp_reference as hp
import test_hp_block_forward as cpu
import test_hp_block_smoothing as cpu_s
from test_gpu_block_forward import Forward
from test_gpu_hp_block_smoothing import dev
from test_hp_block_pairs import NESTED_B, NESTED_BS, nested_obs

pytestmark = pytest.mark.gpu
T = cpu.T


def forward_case(g, name, bs, label, sets=None, store=True, **kw):
    """(Dev, outputs) of one checked case: every block, every entry"""
    d, refs = dev(Forward(g, store), name, bs, T, sets=sets, **kw)
    blocks = cpu.all_blocks(d.S)
    if name == "object_motion":
        hc.moving_inputs(d.S, blocks, label=label)
    out, v = g.block_forward_moments(d.st, bs), hc.Violations()
    hf.check_forward(v, refs, d.S, blocks, out, label)
    v.finish(label)
    return d, out


@pytest.mark.parametrize("name", ["lgssm2", "object_motion", "sv1", "bearings4"])
@pytest.mark.parametrize("ess", [None, 0.5])
def test_forward_moments_follow_the_definition(g, name, ess):
    d, out = forward_case(g, name, 7, f"forward {name} 7 ess {ess}", ess_frac=ess)
    assert all(np.all(np.isfinite(x)) for x in out[:6])
    d.close()


def test_forward_with_dead_and_flushed_past_particles(g):
    def kill(d, t):
        if t == 2:                                                           # step 2, which no resample follows: the weights stay in its record
            dead, flushed = cpu_s.kill(d.n, 7)
            lw = d.st.log_weights
            lw[dead], lw[flushed] = -np.inf, -800.0
            d.st.log_weights = lw

    d, _ = forward_case(g, "lgssm2", 7, "forward lgssm2 7 with dead particles", resample=False, after_update=kill)
    dead, flushed = cpu_s.kill(d.n, 7)
    assert np.isneginf(d.S.lw[1][dead]).all() and np.all(d.S.lw[1][flushed] == -800.0)
    d.close()


def test_forward_fallback_takes_the_recorded_parent(g):
    """line_model with a foreign slope on every third particle of steps 2 and 3 and equal weights, so that the step's resample keeps such particles"""
    bs, B = 7, 4

    def foreign_slope(d, t):
        if t >= 2:
            rows = d.st.traces
            rows[np.arange(bs * B) % 3 == 0, 0] = 5.0 + t
            d.st.traces = rows
            d.st.log_weights = np.zeros(bs * B)

    d, _ = forward_case(g, "line_model", bs, "forward fallback", n=bs * B, after_update=foreign_slope, final_resample=True)
    assert np.any(d.S.x(2)[:, 0] == 7.0) and np.any(d.S.x(3)[:, 0] == 8.0)
    d.close()


def test_forward_with_block_parameters(g):
    forward_case(g, "object_motion", 7, "forward block parameters", sets=cpu_s.param_sets(g), keep_prev=True)[0].close()


def test_forward_without_a_store(g):
    """the same check where no store exists: the Store of the reference is filled from the state's rows"""
    m = hc.case_model(g, "lgssm2")
    n, bs = cpu_s.n_of(7), 7
    B = (n + bs - 1) // bs
    ys = cpu_s.case_obs(g, m, B, T)
    import block_backward_spec as bsp
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=cpu_s.SEED, forward=True)
    S = bsp.Store(n, bs, m.dim)
    S.begin_step(ys[:, 0])
    for t in range(1, T):
        g.pf_resample_blocks(st, bs, "multinomial", ess_frac=0.5, check=False)
        S.resample_blocks(st.parents, g.block_resampled(st))
        S.end_step(st.traces[:, :m.dim], st.log_weights)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs)
        S.begin_step(ys[:, t])
    S.end_step(st.traces[:, :m.dim], st.log_weights)
    v = hc.Violations()
    hf.check_forward(v, [hp.Ref(m)] * B, S, list(range(B)), g.block_forward_moments(st, bs), "forward without a store")
    v.finish("forward without a store")
    st.close()


def test_a_nan_block_reads_nan(g):
    d, refs = dev(Forward(g), "lgssm2", 7, T)
    lw = d.st.log_weights
    lw[7 + 3] = np.nan
    d.st.log_weights = lw
    d.S.lw[-1] = lw.copy()
    out, v = g.block_forward_moments(d.st, 7), hc.Violations()
    hf.check_forward(v, refs, d.S, cpu.all_blocks(d.S), out, "forward, a NaN block")
    assert all(np.isnan(x[1]).all() for x in out[:6]) and all(np.isfinite(x[0]).all() for x in out[:6])
    v.finish("forward, a NaN block")
    d.close()


def test_forward_in_the_nested_filter(g):
    """block resample, then resampling across blocks, every step: the targets' block, the candidates' block and the observation row differ only here"""
    bs, B = NESTED_BS, NESTED_B
    m = hc.case_model(g, "object_motion")
    d, refs = dev(Forward(g), "object_motion", bs, T, n=B * bs, keep_prev=True, ess_frac=0.8, across=True, ys=nested_obs(g, m))
    blocks = list(range(B))
    assert d.fired > 0
    hc.moving_inputs(d.S, blocks, travelling=True, label="nested")
    v = hc.Violations()
    hf.check_forward(v, refs, d.S, blocks, g.block_forward_moments(d.st, bs), "forward nested")
    v.finish("forward nested")
    d.close()
