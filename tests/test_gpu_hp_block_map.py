"""The most probable path per block on the device against its DEFINITION: the checks of tests/hp_map.py (the same dynamic programme in mpmath from the
models of tests/hp_reference.py; every tolerance a derived E bound) fed with what a caller sees -- the Store of tests/block_backward_spec.py filled by
the Dev helper, and the device's paths, indices and logp.  tests/test_hp_block_map.py is the CPU rehearsal: the same checks on the NumPy restatement and
the negative controls.  The bit-for-bit tests (tests/test_gpu_block_map.py) cannot see a mistake the kernel shares with its twin; these can."""
import numpy as np
import pytest

import hp_map as hm
import hp_reference as hp
import test_hp_block_map as cpu
from test_gpu_block_backward import Dev

pytestmark = pytest.mark.gpu


def got(d):
    return d.g.block_map_trajectories(d.st, d.bs, return_indices=True, return_log_density=True)


@pytest.mark.parametrize("bs,T", cpu.SHAPES)
@pytest.mark.parametrize("name", cpu.MODELS)
def test_the_device_returns_a_maximiser_and_its_total(g, name, bs, T):
    d = Dev(g, name, bs, n=2 * bs + 5, steps=T)
    worst = hm.check_map([hp.Ref(d.m)] * d.B, d.S, cpu.checked_blocks(bs, d.B), *got(d), f"device map {name} {bs}")
    print(f"device map {name} {bs} x {T}: worst |logp - S| / bound", round(worst, 3))
    d.close()


def test_the_nested_filter(g):
    bs, B = 7, 12
    d = Dev(g, "object_motion", bs, n=B * bs, keep_prev=True, ess_frac=0.8, across=True)
    assert d.fired > 0
    out = got(d)
    assert np.any((out[1] - 1) // bs != np.arange(B)[:, None])              # (some lineage changed its block)
    hm.check_map([hp.Ref(d.m)] * B, d.S, list(range(B)), *out, "device map nested")
    d.close()


def test_per_block_parameters(g):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    bs = 7
    assign = np.arange(3) % 3
    d = Dev(g, "object_motion", bs, n=2 * bs + 5, keep_prev=True, params=[sets[k] for k in assign])
    hm.check_map([hp.Ref(sets[k]) for k in assign], d.S, list(range(d.B)), *got(d), "device map block parameters")
    d.close()
