"""gpf_run_blocks_wide without a GPU: the symbol in every layer, and the package's own argument checks (they come before the library is called)."""
import os
import types

import numpy as np
import pytest

import gpf_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_in_every_layer():
    header = open(os.path.join(ROOT, "include", "gpf.h")).read()
    julia = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert "gpf_status gpf_run_blocks_wide(gpf_handle h," in header
    assert "gpf_run_blocks_wide" in [p[0] for p in g._lib.SYMBOLS]
    assert callable(g.pf_run_blocks_wide) and g.pf_run_blocks_wide is g.api.pf_run_blocks_wide
    assert "ccall((:gpf_run_blocks_wide, libgpf)" in julia and "function pf_run_blocks_wide!(" in julia


@pytest.mark.parametrize("kw,text", [
    (dict(method="systematic"), "Resampling method systematic not recognized."),
    (dict(state=object.__new__(g.api.DeviceParticleFilterSubState)), "pf_run_blocks_wide works on the whole filter"),   # (the check is on the type alone)
    (dict(block_size=0), "block_size < 1"),
    (dict(observations=np.zeros((3, 5, 2))), "observations of shape (2, T, n_obs), or (T, n_obs) for one series shared by all blocks, expected: got (3, 5, 2)"),
    (dict(observations=np.zeros(5)), "observations of shape (2, T, n_obs), or (T, n_obs) for one series shared by all blocks, expected: got (5,)"),
])
def test_argument_checks_of_the_package(kw, text):
    args = dict(state=types.SimpleNamespace(n_particles=10000), observations=np.zeros((2, 5, 2)), block_size=5000, method="multinomial")
    args.update(kw)                                                            # (every one is refused before the handle is touched)
    with pytest.raises(g.ErrorException) as e:
        g.pf_run_blocks_wide(args["state"], args["observations"], args["block_size"], args["method"])
    assert str(e.value) == text
