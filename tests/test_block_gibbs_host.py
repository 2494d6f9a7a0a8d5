"""The particle Gibbs chain per block in one launch (gpf.h gpf_gibbs_blocks), the parts that need no GPU: the entry point in every layer and the
argument checks of pf_gibbs_blocks that come before the library."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_in_every_layer(g):
    import __graft_entry__ as ge
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpf.h")).read(), flags=re.S)
    m = re.search(r"gpf_status\s+gpf_gibbs_blocks\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "gpf_gibbs_blocks is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", re.sub(r"\bconst\b", "", a).strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == ["gpf_handle", "double*", "int32_t", "int32_t", "int32_t", "double*", "int32_t", "int64_t", "int32_t", "int32_t", "double",
                      "uint64_t*", "int32_t", "int32_t", "double*", "double*"]
    pd = C.POINTER(C.c_double)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_gibbs_blocks"][1:] == (C.c_int, [C.c_void_p, pd, C.c_int32, C.c_int32, C.c_int32, pd, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                                        C.c_double, C.POINTER(C.c_uint64), C.c_int32, C.c_int32, pd, pd])
    assert hasattr(C.CDLL(g._lib.LIB_PATH), "gpf_gibbs_blocks")
    assert "libgpf_gibbs.hip" in ge.HIP_UNITS and os.path.exists(os.path.join(ge.CSRC, "libgpf_gibbs.hip"))
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert ("ccall((:gpf_gibbs_blocks, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}, Cint, Int64, Cint, Cint, Cdouble, "
            "Ptr{UInt64}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble})") in jl
    assert "pf_gibbs_blocks" in open(os.path.join(ROOT, "README.md")).read()
    assert g.BlockGibbs._fields == ("paths", "lml")


def test_package_argument_checks(g):
    sig = inspect.signature(g.pf_gibbs_blocks).parameters
    assert list(sig) == ["state", "observations", "reference", "block_size", "seeds", "ancestor_sampling", "backward", "ess_frac", "thin"]
    assert sig["seeds"].default is inspect.Parameter.empty and sig["ancestor_sampling"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [sig[k].default for k in ("ancestor_sampling", "backward", "ess_frac", "thin")] == [True, False, 0.5, 1]

    class Stub:                                                               # (no handle: every check below comes before the library is called)
        n_particles, model = 300, g.models.lgssm2()
    ok = {"observations": np.zeros((3, 5, 2)), "reference": np.zeros((3, 5, 2)), "block_size": 100, "seeds": [9, 10]}
    for kw, text in (({"block_size": 0}, "block_size < 1"),
                     ({"observations": np.zeros((4, 5, 2))}, r"observations of shape \(3, T, n_obs\), or \(T, n_obs\)"),
                     ({"observations": np.zeros((3, 1, 2)), "reference": np.zeros((3, 1, 2))}, "the whole series expected"),
                     ({"observations": np.zeros((1, 2))}, "the whole series expected"),
                     ({"reference": np.zeros((3, 4, 2))}, r"a reference of shape \(3, 5, dim\) expected"),
                     ({"reference": np.zeros((5, 2))}, r"a reference of shape \(3, 5, dim\) expected"),
                     ({"seeds": []}, "one fresh seed per sweep expected"), ({"thin": 0}, "thin < 1")):
        with pytest.raises(g.ErrorException, match=text):
            g.pf_gibbs_blocks(Stub(), **{**ok, **kw})
    with pytest.raises(TypeError, match="seeds"):
        g.pf_gibbs_blocks(Stub(), **{k: v for k, v in ok.items() if k != "seeds"})
    view = object.__new__(g.DeviceParticleFilterSubState)                     # (a view: refused by its type alone)
    with pytest.raises(g.ErrorException, match="works on the whole filter"):
        g.pf_gibbs_blocks(view, **ok)
