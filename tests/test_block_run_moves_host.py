"""The whole README loop per block in one launch (gpf.h gpf_run_blocks_rejuvenate), the parts that need no GPU: the entry point in every layer, the
argument checks of pf_run_blocks_rejuvenate that come before the library, and tests/block_run_moves_spec.py against the three oracle calls written out."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import block_run_moves_spec as ms
from test_gpu_block_conditional import block_obs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_in_every_layer(g):
    import __graft_entry__ as ge
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpf.h")).read(), flags=re.S)
    m = re.search(r"gpf_status\s+gpf_run_blocks_rejuvenate\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "gpf_run_blocks_rejuvenate is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", re.sub(r"\bconst\b", "", a).strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == ["gpf_handle", "double*", "int32_t", "int32_t", "int32_t", "int64_t", "int32_t", "int32_t", "double", "int32_t", "int32_t",
                      "double*", "double*", "int32_t*", "int64_t*", "int32_t*"]
    pd, pi, pl = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_run_blocks_rejuvenate"][1:] == (C.c_int, [C.c_void_p, pd, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                                                 C.c_int32, C.c_int32, pd, pd, pi, pl, pi])
    assert hasattr(C.CDLL(g._lib.LIB_PATH), "gpf_run_blocks_rejuvenate")
    assert "libgpf_run_move.hip" in ge.HIP_UNITS and os.path.exists(os.path.join(ge.CSRC, "libgpf_run_move.hip"))
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert ("ccall((:gpf_run_blocks_rejuvenate, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cint, Int64, Cint, Cint, Cdouble, Cint, Cint, "
            "Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Int64}, Ptr{Cint})") in jl


def test_package_argument_checks(g):
    sig = inspect.signature(g.pf_run_blocks_rejuvenate).parameters
    assert list(sig) == ["state", "observations", "block_size", "method", "rejuvenate", "n_iters", "ess_frac", "sort_particles"]
    assert [sig[k].default for k in list(sig)[3:]] == ["multinomial", "move", 1, 0.5, True] and sig["rejuvenate"].kind is inspect.Parameter.KEYWORD_ONLY
    assert g.BlockRunMoves._fields == ("lml", "ess", "resampled", "accepted") and g.BlockRun._fields == ("lml", "ess", "resampled")

    class Stub:                                                               # (no handle: every check below comes before the library is called)
        n_particles = 300
    y = np.zeros((3, 5, 2))
    for kw, text in (({"method": "systematic"}, "Resampling method systematic not recognized"), ({"rejuvenate": "gibbs"}, "Method gibbs not recognized"),
                     ({"block_size": 0}, "block_size < 1"), ({"observations": np.zeros((4, 5, 2))}, r"observations of shape \(3, T, n_obs\), or \(T, n_obs\)"),
                     ({"observations": np.zeros((0, 2))}, r"observations of shape \(3, T, n_obs\)"), ({"block_size": 5000}, r"observations of shape \(1, T, n_obs\)")):
        with pytest.raises(g.ErrorException, match=text):
            g.pf_run_blocks_rejuvenate(Stub(), **{"observations": y, "block_size": 100, **kw})


@pytest.mark.parametrize("kind", ["move", "reweight"])
def test_spec_is_the_three_oracle_calls(g, o, kind):
    n, bs, m = 330, 100, g.models.lgssm2()                                    # (a short last block)
    ys = block_obs(g, m, 4, 5)
    f, h = (o.initialize_blocks(o.OracleFilter(m.model_id, m.params, n, 19, keep_prev=True), bs, ys[:, 0]) for _ in range(2))
    got = ms.run_blocks_rejuvenate(o, f, bs, ys[:, 1:], ys[:, 0], "residual", kind, n_iters=2)
    e0 = h.epoch
    for t in range(1, ys.shape[1]):
        mask = o.resample_blocks(h, bs, "residual", ess_frac=0.5, check=False)
        acc = o.rejuvenate_blocks(h, bs, ys[:, t - 1], kind, mask=mask, n_iters=2)
        o.update_blocks(h, bs, ys[:, t])
        assert np.array_equal(got.resampled[:, t - 1], mask) and got.accepted[t - 1] == acc
    assert np.array_equal(f.rows, h.rows) and np.array_equal(f.lw, h.lw) and np.array_equal(f.parents, h.parents)
    assert f.epoch == h.epoch == e0 + 3 * (ys.shape[1] - 1) and f.rows.shape[1] == 4 and got.resampled.any() and not got.resampled.all()
