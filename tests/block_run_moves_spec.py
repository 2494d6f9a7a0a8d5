"""Expected results of the whole README loop per block in one launch (gpf.h gpf_run_blocks_rejuvenate), from the CPU oracle only: per step
block_run_spec.resample_step, oracle.rejuvenate_blocks on the blocks that resampled -- under each block's PREVIOUS observation --, oracle.update_blocks,
block_run_spec.block_stats, on a keep_prev OracleFilter.

Imported by tests/test_gpu_block_run_moves.py (device vs this) and tests/test_block_run_moves_host.py (this vs the three oracle calls written out)."""
from collections import namedtuple

import numpy as np

import block_run_spec as rs

BlockRunMoves = namedtuple("BlockRunMoves", ["lml", "ess", "resampled", "accepted"])


def run_blocks_rejuvenate(o, f, nb, observations, prev_obs, method="multinomial", kind="move", n_iters=1, ess_frac=0.5, sort_particles=True):
    """the loop on the oracle filter f; prev_obs: (n_blocks, n_obs), the observations of the step f is in.  accepted: the loop's count per step, (T,)"""
    B = len(o.blocks_of(f, nb))
    ys = rs.series(observations, B)
    T = ys.shape[1]
    lml, ess, res, acc = np.empty((B, T)), np.empty((B, T)), np.zeros((B, T), bool), np.zeros(T, np.int64)
    for t in range(T):
        res[:, t] = rs.resample_step(o, f, nb, method, ess_frac, sort_particles)
        acc[t] = o.rejuvenate_blocks(f, nb, prev_obs if t == 0 else ys[:, t - 1], kind, mask=res[:, t], n_iters=n_iters)
        o.update_blocks(f, nb, ys[:, t])
        ess[:, t], lml[:, t] = rs.block_stats(o, f, nb)
    return BlockRunMoves(lml, ess, res, acc)
