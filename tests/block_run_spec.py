"""Expected results of a whole series per block in one launch (gpf.h gpf_run_blocks), built from the CPU oracle only: the loop the call stands for,

    for t in 1:T
        for b in blocks; if ess_frac === nothing || effective_sample_size(state[b]) < ess_frac * length(b); pf_resample!(state[b], method); end; end
        for b in blocks; pf_update!(state[b], new_args, argdiffs, observations[b][t]); end
    end

(README.md:60-79 per block; test/resample.jl:130-162, test/update.jl:179-189), restated over oracle.oracle: `resample_blocks`, `update_blocks`, and the
sub-states' effective_sample_size / log_ml_estimate after every update.  One difference from `resample_blocks` with check = False, which is the device's
rule (k_block_resample): a block whose weights hold a NaN or +Inf is left as it stands instead of raising, and the loop goes on.

Imported by tests/test_gpu_block_run.py (device vs this) and tests/test_block_run_host.py (this vs the oracle's own loop)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

BlockRun = namedtuple("BlockRun", ["lml", "ess", "resampled"])


def series(obs, n_blocks: int) -> np.ndarray:
    """(n_blocks, T, n_obs) from either form of the call's observations: per block, or one (T, n_obs) series shared by all blocks"""
    obs = np.asarray(obs, np.float64)
    if obs.ndim == 2:
        obs = np.broadcast_to(obs, (n_blocks,) + obs.shape)
    assert obs.ndim == 3 and obs.shape[0] == n_blocks, obs.shape
    return obs


def resample_step(o, f, nb: int, method: str, ess_frac, sort_particles: bool) -> np.ndarray:
    """oracle.resample_blocks(check = False) with the device's rule for NaN / +Inf blocks; the mask of the blocks that resampled"""
    e, mask = f.epoch, []
    for a, b in o.blocks_of(f, nb):
        v = f[a:b]
        f.epoch = e
        go = (ess_frac is None or v.effective_sample_size() < ess_frac * v.n) and not v.summary().bad
        if go:
            v.resample(method, sort_particles=sort_particles, check=False)
        mask.append(bool(go))
    f.epoch = e + 1
    return np.array(mask)


def block_stats(o, f, nb: int):
    """(ess, lml) of every sub-state (src/utils.jl:163-178): what gpf_block_stats returns"""
    vs = [f[a:b] for a, b in o.blocks_of(f, nb)]
    return np.array([v.effective_sample_size() for v in vs]), np.array([v.log_ml_estimate() for v in vs])


def run_blocks(o, f, nb: int, observations, method: str = "multinomial", ess_frac=0.5, sort_particles: bool = True) -> BlockRun:
    """the loop on the oracle filter f (initialised, block-wise); observations as pf_run_blocks takes them.  Returns what the call returns"""
    B = len(o.blocks_of(f, nb))
    ys = series(observations, B)
    T = ys.shape[1]
    lml, ess, res = np.empty((B, T)), np.empty((B, T)), np.zeros((B, T), bool)
    for t in range(T):
        res[:, t] = resample_step(o, f, nb, method, ess_frac, sort_particles)
        o.update_blocks(f, nb, ys[:, t])
        ess[:, t], lml[:, t] = block_stats(o, f, nb)
    return BlockRun(lml, ess, res)
