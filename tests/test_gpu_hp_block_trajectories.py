"""The draws of gpf_block_sample_trajectories against the DEFINITION, not the integer spec: tests/hp_weights.py restates safe_softmax and the
categorical draw in mpmath on the exact uniforms u = U / 2^64 of the draws' resample slots b n_samples + j.  A slot whose uniform lies within the
reference's own quantisation bound of a CDF boundary is undecidable and not compared; at most hp_checks.MAX_UNDECIDABLE per block.  The weights and
the seed were chosen so that the reference alone stays within that (reference_of(...).undecidable, evaluated on the CPU).  Every block holds one
pair of log-weights more than 708 apart (exp_ flushes the lower one: `dead`, never drawn) and one -Inf."""
import numpy as np
import pytest

import hp_checks as hc
import hp_weights as hw

pytestmark = pytest.mark.gpu
N, SEED, EPOCH, K_DRAWS = 1000, 77, 1, 70
# block size -> the blocks that are checked: the first, the second and the last (7: 6 particles; 300: 100; 999: ONE particle)
BLOCKS = {7: [0, 1, 142], 300: [0, 1, 3], 999: [0, 1]}


def hand_weights(bs):
    """log-weights of spread 3 around 0; in every checked block the maximum 12.5, a weight 721 below it and a -Inf"""
    lw = 3.0 * np.random.default_rng(bs).standard_normal(N)
    for b in BLOCKS[bs]:
        i0, cnt = b * bs, min(bs, N - b * bs)
        if cnt >= 3:
            lw[i0 + cnt // 2] = 12.5
            lw[i0] = -708.5
            lw[i0 + cnt - 1] = -np.inf
    return lw


def reference_of(lw, bs, b):
    i0 = b * bs
    sm = hw.Softmax(lw[i0:min(i0 + bs, N)])
    return sm, hw.multinomial(sm, SEED, EPOCH, K_DRAWS, slot0=b * K_DRAWS)


@pytest.mark.parametrize("bs", sorted(BLOCKS))
def test_draws_follow_the_definition(g, bs):
    lw = hand_weights(bs)
    refs = {b: reference_of(lw, bs, b) for b in BLOCKS[bs]}
    for b, (sm, ref) in refs.items():                                          # the reference alone, before anything runs on the device
        assert len(ref.undecidable) <= hc.MAX_UNDECIDABLE, (bs, b, ref.undecidable)
        assert sm.n < 3 or sm.dead.sum() == 2
    m = g.models.object_motion()
    B = (N + bs - 1) // bs
    st = g.pf_initialize_blocks(m, (1,), np.tile(np.asarray(g.models.simulate(m, 1))[0], (B, 1)), N, bs, seed=SEED, history=1)
    st.log_weights = lw
    _, idx = g.block_sample_trajectories(st, bs, K_DRAWS, return_indices=True)   # the second epoch-advancing call: epoch 1
    for b, (sm, ref) in refs.items():
        left_out = hw.check_ancestors(ref, idx[b] - 1, sm, f"block {b} of size {bs}")
        print(f"block size {bs}, block {b}: {left_out} undecidable slots, eps {ref.eps:.3g}")
        assert left_out <= hc.MAX_UNDECIDABLE
    st.close()
