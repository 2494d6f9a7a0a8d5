"""What gpf_block_sample_trajectories (gpf.h) returns, restated from what a caller sees: the log-weights, the seed, the epoch the call ran under,
n, block_size and n_samples give the indices; the genealogy of tests/block_history_spec.py gives the paths.

  indices  block b holds the particles [b bs, min((b + 1) bs, n)), bs = min(block_size, n).  Its weights are summarised as a sub-state's are
           (oracle.WeightSummary with the block's particle count: K, maximum, flags, fixed-point weights, inclusive CDF, S); draw j reads resample
           slot b n_samples + j of the epoch (oracle.targets_multinomial from that slot on) and takes the first cell whose CDF exceeds the target
           (oracle.upper_bound).  1-based inside the block; 0 for a block whose log-weights hold a NaN or +Inf.
  paths    traj[b, j, s - lo, c] = Genealogy.trace(s, c)[b bs + idx[b, j] - 1]; NaN where the index is 0.
  epoch    the number of epoch-advancing calls made on the state before the call; the tests count them.

The oracle's pieces are test infrastructure only.  Helper module, no tests."""
import numpy as np


def block_ranges(n, block_size):
    bs = min(int(block_size), int(n))
    return bs, [(b0, min(b0 + bs, n)) for b0 in range(0, n, bs)]


def draw_indices(o, lw, seed, epoch, block_size, n_samples):
    """[n_blocks, n_samples] int64"""
    lw = np.ascontiguousarray(lw, np.float64)
    bs, ranges = block_ranges(lw.size, block_size)
    out = np.zeros((len(ranges), n_samples), np.int64)
    for b, (i0, i1) in enumerate(ranges):
        s = o.WeightSummary(np.ascontiguousarray(lw[i0:i1]), i1 - i0)
        if s.bad:
            continue
        T = o.targets_multinomial(int(seed), int(epoch), b * n_samples, n_samples, s.S)
        out[b] = o.upper_bound(s.cdf, T) + 1
    return out


def paths(gen, idx, block_size, lo, hi, dim):
    """[n_blocks, n_samples, hi - lo + 1, dim] from a block_history_spec.Genealogy whose current rows are set"""
    bs, ranges = block_ranges(gen.n, block_size)
    idx = np.asarray(idx, np.int64)
    assert idx.shape[0] == len(ranges)
    out = np.full(idx.shape + (hi - lo + 1, dim), np.nan)
    ok = idx > 0
    part = (np.arange(len(ranges), dtype=np.int64)[:, None] * bs + idx - 1)[ok]
    for s in range(lo, hi + 1):
        for c in range(dim):
            out[..., s - lo, c][ok] = gen.trace(s, c)[part]
    return out
