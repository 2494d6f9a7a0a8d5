"""Marginal smoothing and one backward draw over a store RECORDED BY gpf_run_blocks_history against their mpmath definitions (tests/hp_checks.py, with the
bounds those checks derive).  The answers come from the filter the new call ran on; the definitions' inputs are what a caller of the loop sees on a twin."""
import numpy as np
import pytest

import hp_checks as hc
import hp_reference as hp
import test_hp_block_smoothing as cpu
from test_gpu_block_backward import Dev

pytestmark = pytest.mark.gpu
BS, B, STEPS = 8, 2, 4                                                        # 2 blocks of 8; the initialisation and T = 3 steps of the run


@pytest.mark.parametrize("name", ["lgssm2", "object_motion"])
def test_smoothing_and_a_backward_draw_follow_the_definitions(g, name):
    m = hc.case_model(g, name)
    ys = cpu.case_obs(g, m, B, STEPS)
    d = Dev(g, name, BS, n=B * BS, steps=STEPS, seed=cpu.SEED, model=m, ys=ys)           # the twin: multinomial, every block resamples at every step
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], B * BS, BS, seed=cpu.SEED, history=STEPS, history_weights=True)
    g.pf_run_blocks_history(st, ys[:, 1:], BS, "multinomial", ess_frac=None)
    refs, blocks, v, label = [hp.Ref(m) for _ in range(B)], list(range(B)), hc.Violations(), f"run history {name}"
    hc.check_smooth(v, refs, d.S, blocks, *g.block_smoothed_moments(st, BS, return_weights=True, return_blocks=True), label)
    _, idx = g.block_backward_trajectories(st, BS, 1, return_indices=True)
    hc.check_backward(v, refs, d.S, blocks, cpu.SEED, d.epoch, idx, label)    # (the run left the twin's epoch: 1 + 2 T)
    v.finish(label)
    assert np.array_equal(st.log_weights, d.S.lw[-1])
    d.close(); st.close()
