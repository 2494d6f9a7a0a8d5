"""The genealogy of a block-wise filter with a trajectory store, restated in NumPy (gpf.h gpf_history_enable_blocks): what trace[t => c] of every
current particle is, given the rows recorded at the end of every step and the resamples that happened during it.

A resample of step s (1-based; it happens between the update that began step s and the one that begins step s + 1) maps every particle j of the
new order to the particle g[j] of the old order it is a copy of:

  - ("blocks", parents, block_resampled, nb) -- pf_resample_blocks: `parents` is state.parents right after the call, 1-based and LOCAL to the
    block for the blocks that resampled; for a block that did not resample the entries are whatever an earlier call left there and mean nothing:
    its particles stayed where they were.  g[j] = (j // nb) * nb + parents[j] - 1 if block_resampled[j // nb] else j.
  - ("global", parents) -- pf_resample on the whole filter, or pf_resample_across_blocks when it fired: 1-based indices into the whole
    state, g[j] = parents[j] - 1.

The resamples of one step apply in call order, so following a current particle back one walks them last to first.  Nothing here is read from
the device's ancestor maps."""
import numpy as np


def resample_map(event, n):
    """g[0..n): the old-order index every new-order particle was copied from (0-based)"""
    if event[0] == "blocks":
        _, parents, block_resampled, nb = event
        parents, block_resampled = np.asarray(parents, np.int64), np.asarray(block_resampled, bool)
        assert parents.shape == (n,) and block_resampled.shape == ((n + nb - 1) // nb,)
        j = np.arange(n, dtype=np.int64)
        blk = j // nb
        local = np.where(block_resampled[blk], parents - 1, 0)                 # (stale entries are never looked at)
        g = np.where(block_resampled[blk], blk * nb + local, j)
        cnt = np.minimum(nb, n - blk * nb)
        assert np.all((local >= 0) & (local < cnt)), "a resampled block's parents must be local to the block"
        return g
    if event[0] == "global":
        g = np.asarray(event[1], np.int64) - 1
        assert g.shape == (n,) and g.min() >= 0 and g.max() < n
        return g
    raise ValueError(event[0])


class Genealogy:
    """rows[s - 1]: the [n, d] latent columns at the END of step s (final particle order of that step); events[s - 1]: the resamples of step s in
    call order"""

    def __init__(self, n):
        self.n, self.rows, self.events = int(n), [], []

    def begin_step(self, rows):
        """pf_initialize_blocks / pf_update_blocks returned: a new step, with these rows so far"""
        self.rows.append(np.array(rows, np.float64)); self.events.append([])

    def set_rows(self, rows):
        """the current step's rows changed (rejuvenation, a resample's gather): the step's record is its final rows"""
        self.rows[-1] = np.array(rows, np.float64)

    def resample(self, *event):
        self.events[-1].append(event)

    @property
    def steps(self):
        return len(self.rows)

    def index(self, t):
        """for every current particle: its ancestor's index in the final order of step t"""
        idx = np.arange(self.n, dtype=np.int64)
        for s in range(self.steps, t, -1):                                     # the resamples of steps T, T-1, ..., t+1 -- those of step t
            for ev in reversed(self.events[s - 1]):                            # itself happened before its final order
                idx = resample_map(ev, self.n)[idx]
        return idx

    def trace(self, t, c):
        """trace[t => c] of every current particle"""
        assert 1 <= t <= self.steps
        return self.rows[t - 1][self.index(t), c]
