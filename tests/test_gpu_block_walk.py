"""Random walks over the block-wise calls on the device (tests/block_walk_spec.py): the state machine behind gpf_update_blocks, gpf_resample_blocks and its
conditional and ancestor forms, gpf_resample_across_blocks, gpf_rejuvenate_blocks, the block-wise trajectory store and its draws, walked in orders no
per-feature test chose.

  test_walk                   device and model in lockstep over the plan of a seed: rows, log-weights, parents, block_resampled, block_stats, every
                              history column, the per-block parameters and every getter, bit for bit (np.array_equal, NaN == NaN; no tolerance anywhere);
                              refused calls change nothing; a third of the seeds issue their state-changing ops in bursts with no read-back in between,
                              which is how a production loop calls the library (the staging ring's ticket wait).
  test_burst_equals_checked   the device against itself: one plan read back after every op and once not at all give the same final state, store columns
                              and path draws -- the staging ring and the deferred work pinned without the oracle.

GPF_BLOCKWALK_SEEDS / GPF_BLOCKWALK_OFFSET select other plans for a longer hunt.  tests/test_block_walk_host.py holds the rehearsal on the model alone
and the coverage the committed seeds must have."""
import numpy as np
import pytest

import block_walk_spec as ws

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", ws.SEEDS)
def test_walk(g, o, seed):
    w = ws.walk(g, o, seed)
    assert len(w.log) == len(w.ops)


@pytest.mark.parametrize("seed", [ws.OFFSET + 1, ws.OFFSET + 8, ws.OFFSET + 13])
def test_burst_equals_checked(g, seed):
    refused_a, a = ws.device_only(g, seed, readback=True)
    refused_b, b = ws.device_only(g, seed, readback=False)
    assert refused_a == refused_b, (seed, refused_a, refused_b)
    assert len(a) == len(b) >= 3
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y, equal_nan=True), (seed, ws.plan(seed)[0], "output", k)
