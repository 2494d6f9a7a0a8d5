"""gpf_run_blocks_history without a GPU: the symbol in every layer, and the package's own argument checks (they come before the library is called)."""
import os
import types

import numpy as np
import pytest

import gpf_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_in_every_layer():
    header = open(os.path.join(ROOT, "include", "gpf.h")).read()
    julia = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    blocks = open(os.path.join(ROOT, "genparticlefilters.jl_amd", "csrc", "libgpf_blocks.hip")).read()
    proto = "gpf_status gpf_run_blocks_history(gpf_handle h, const double* obs, int32_t n_obs, int32_t n_steps, int32_t shared_obs,\n"
    assert proto in header and "gpf_status gpf_run_blocks_history(gpf_handle h," in blocks
    assert dict((p[0], p[2]) for p in g._lib.SYMBOLS)["gpf_run_blocks_history"] == dict((p[0], p[2]) for p in g._lib.SYMBOLS)["gpf_run_blocks"]
    assert callable(g.pf_run_blocks_history) and g.pf_run_blocks_history is g.api.pf_run_blocks_history
    assert "ccall((:gpf_run_blocks_history, libgpf)" in julia and "function pf_run_blocks_history!(" in julia


@pytest.mark.parametrize("kw,text", [
    (dict(method="systematic"), "Resampling method systematic not recognized."),
    (dict(state=object.__new__(g.api.DeviceParticleFilterSubState)), "pf_run_blocks_history works on the whole filter"),   # (the check is on the type alone)
    (dict(block_size=0), "block_size < 1"),
    (dict(observations=np.zeros((3, 5, 2))), "observations of shape (2, T, n_obs), or (T, n_obs) for one series shared by all blocks, expected: got (3, 5, 2)"),
])
def test_argument_checks_of_the_package(kw, text):
    args = dict(state=types.SimpleNamespace(n_particles=200), observations=np.zeros((2, 5, 2)), block_size=100, method="multinomial")
    args.update(kw)                                                            # (every one is refused before the handle is touched)
    with pytest.raises(g.ErrorException) as e:
        g.pf_run_blocks_history(args["state"], args["observations"], args["block_size"], args["method"])
    assert str(e.value) == text
