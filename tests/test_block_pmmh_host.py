"""The particle-marginal MH move per block in one launch (gpf.h gpf_pmmh_blocks), the parts that need no GPU: the entry point in every layer and the
argument checks of pf_pmmh_blocks that come before the library."""
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
    m = re.search(r"gpf_status\s+gpf_pmmh_blocks\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "gpf_pmmh_blocks is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", re.sub(r"\bconst\b", "", a).strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == ["gpf_handle", "double*", "int32_t", "int32_t", "int32_t", "int64_t", "double*", "int32_t", "double*", "int64_t", "uint64_t",
                      "int32_t", "int32_t", "double", "int32_t", "int32_t*", "double*"]
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_pmmh_blocks"][1:] == (C.c_int, [C.c_void_p, pd, C.c_int32, C.c_int32, C.c_int32, C.c_int64, pd, C.c_int32, pd, C.c_int64, C.c_uint64,
                                                       C.c_int32, C.c_int32, C.c_double, C.c_int32, pi, pd])
    assert hasattr(C.CDLL(g._lib.LIB_PATH), "gpf_pmmh_blocks")
    assert "libgpf_pmmh.hip" in ge.HIP_UNITS and os.path.exists(os.path.join(ge.CSRC, "libgpf_pmmh.hip"))
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert ("ccall((:gpf_pmmh_blocks, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cint, Int64, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Int64, UInt64, "
            "Cint, Cint, Cdouble, Cint, Ptr{Cint}, Ptr{Cdouble})") in jl
    assert "pf_pmmh_blocks" in open(os.path.join(ROOT, "README.md")).read()
    assert g.BlockPmmh._fields == ("accepted", "lml")


def test_package_argument_checks(g):
    sig = inspect.signature(g.pf_pmmh_blocks).parameters
    assert list(sig) == ["state", "observations", "params", "log_threshold", "block_size", "method", "seed", "ess_frac", "sort_particles", "keep_mass"]
    assert sig["seed"].kind is inspect.Parameter.KEYWORD_ONLY and sig["seed"].default is inspect.Parameter.empty
    assert [sig[k].default for k in ("method", "ess_frac", "sort_particles", "keep_mass")] == ["multinomial", 0.5, True, True]
    assert "fresh" in g.pf_pmmh_blocks.__doc__.lower() and "different from the state's" in g.pf_pmmh_blocks.__doc__

    class Stub:                                                               # (no handle: every check below comes before the library is called)
        n_particles, model = 300, g.models.lgssm2()
    ok = {"observations": np.zeros((3, 5, 2)), "params": [Stub.model] * 3, "log_threshold": np.zeros(3), "block_size": 100, "seed": 9}
    for kw, text in (({"method": "systematic"}, "Resampling method systematic not recognized"), ({"block_size": 0}, "block_size < 1"),
                     ({"observations": np.zeros((4, 5, 2))}, r"observations of shape \(3, T, n_obs\), or \(T, n_obs\)"),
                     ({"observations": np.zeros((0, 2))}, r"observations of shape \(3, T, n_obs\)"),
                     ({"log_threshold": np.zeros(4)}, r"one log-threshold per block expected: shape \(3,\)"),
                     ({"params": [Stub.model] * 2}, "one parameter vector per block expected: 3 rows")):
        with pytest.raises(g.ErrorException, match=text):
            g.pf_pmmh_blocks(Stub(), **{**ok, **kw})
    with pytest.raises(TypeError, match="seed"):
        g.pf_pmmh_blocks(Stub(), **{k: v for k, v in ok.items() if k != "seed"})
    view = object.__new__(g.DeviceParticleFilterSubState)                     # (a view: refused by its type alone)
    with pytest.raises(g.ErrorException, match="works on the whole filter"):
        g.pf_pmmh_blocks(view, **ok)
