"""Particle Gibbs with backward simulation per block in one launch (gpf.h gpf_sweep_blocks_backward), the parts that need no GPU: the entry point in
every layer (header, library, ctypes table, Julia glue, the build's list of units) and the argument checks of pf_sweep_blocks_backward."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_block_sweep_host import PROTO, ROOT

NAME = "gpf_sweep_blocks_backward"


def test_the_entry_point_in_every_layer(g):
    import __graft_entry__ as ge
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpf.h")).read(), flags=re.S)
    m = re.search(r"gpf_status\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr)
    assert m, NAME + " is not declared in include/gpf.h"
    assert [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", re.sub(r"\bconst\b", "", a).strip()).replace(" ", "") for a in m.group(1).split(",")] == PROTO
    assert hasattr(C.CDLL(g._lib.LIB_PATH), NAME), NAME + " is not exported by the built library"
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table[NAME][1:] == table["gpf_sweep_blocks"][1:]
    assert "libgpf_sweep_back.hip" in ge.HIP_UNITS and os.path.exists(os.path.join(ge.CSRC, "libgpf_sweep_back.hip"))
    assert '#include "gpf_k_block_sweep.hpp"' in open(os.path.join(ge.CSRC, "gpf_kernels.hpp")).read()
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert "ccall((:" + NAME + ", libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}, Cint, Int64, Cint, Cdouble, " \
           "Ptr{Cdouble}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint})" in jl and "\nfunction pf_sweep_blocks_backward!(s::DeviceParticleFilterState, " in jl


def test_package_exports_and_argument_checks(g):
    sig = inspect.signature(g.pf_sweep_blocks_backward).parameters
    assert list(sig) == ["state", "observations", "reference", "block_size", "ancestor_sampling", "ess_frac"]
    assert (sig["ancestor_sampling"].default, sig["ess_frac"].default) == (True, 0.5)
    assert sig["ancestor_sampling"].kind is sig["ess_frac"].kind is inspect.Parameter.KEYWORD_ONLY
    assert g.BlockSweepBackward._fields == ("path", "indices", "lml", "ess", "resampled")

    class Stub:                                                               # (no handle: every check below comes before the library is called)
        n_particles = 300
    y, r = np.zeros((3, 5, 2)), np.zeros((3, 5, 2))
    # observations that are neither per block nor shared; a reference that is not per block and step; a T that differs between the two
    for args, text in (((y, r, 0), "block_size < 1"), ((np.zeros((4, 5, 2)), r, 100), r"observations of shape \(3, T, n_obs\), or \(T, n_obs\)"),
                       ((y, np.zeros((5, 2)), 100), r"a reference of shape \(3, 5, dim\) expected"), ((y, np.zeros((3, 4, 2)), 100), r"a reference of shape \(3, 5, dim\)"),
                       ((y[0], np.zeros((3, 6, 2)), 100), r"a reference of shape \(3, 5, dim\) expected")):
        with pytest.raises(g.ErrorException, match=text):
            g.pf_sweep_blocks_backward(Stub(), *args)
