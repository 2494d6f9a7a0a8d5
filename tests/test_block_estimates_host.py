"""Per-block estimates (gpf.h gpf_block_moments / gpf_block_proportion), the parts that need no GPU: the entry points exist in every layer
(header, library, ctypes table, package, Julia glue), and the reference the GPU tests compare against -- the oracle's o_wsum over one block's
rows with the block's own WeightSummary -- is pinned to a plain-NumPy restatement of the summation tree of DESIGN.md §3.5."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "gpf_block_moments": ["gpf_handle", "int64_t", "double*", "double*"],
    "gpf_block_proportion": ["gpf_handle", "int64_t", "int32_t", "double*", "int32_t", "double*"],
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpf.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_header_declares_the_entry_point(name):
    m = re.search(r"gpf_status\s+%s\s*\(([^;]*?)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", re.sub(r"\bconst\b", "", a).strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == ENTRY_POINTS[name]


def test_header_cites_the_reference_and_documents_the_deviation():
    txt = open(os.path.join(ROOT, "include", "gpf.h")).read()
    doc = txt[txt.index("gpf_block_stats(gpf_handle"):txt.index("gpf_block_proportion(gpf_handle")]
    assert "src/statistics.jl:13-14, 48-50" in doc and "src/statistics.jl:91-101" in doc
    assert "DEVIATION" in doc and "NaN" in doc


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_library_exports_the_entry_point(g, name):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, name), f"{name} is not exported by the built library"


def test_ctypes_table(g):
    C = ctypes
    pd = C.POINTER(C.c_double)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_block_moments"][1:] == (C.c_int, [C.c_void_p, C.c_int64, pd, pd])
    assert table["gpf_block_proportion"][1:] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, pd, C.c_int32, pd])


def test_package_exports(g):
    for name in ("block_mean", "block_var", "block_moments", "block_proportionmap"):
        assert callable(getattr(g, name, None)), name


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_julia_glue_calls_the_entry_point(name):
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:%s, libgpf\), Cint, \(" % name, jl), f"no ccall of {name}"
    for fn in ("block_mean", "block_var", "block_moments", "block_proportionmap"):
        assert re.search(r"^function %s\(" % fn, jl, re.M), fn


# ----------------------------------------------------------------------------- the reference of the GPU tests, rehearsed on the CPU
CHUNK = 2048


def tree_sum(t):
    """DESIGN.md §3.5 for one chunk: the perfect binary tree over the term index, neighbours first, missing terms +0.0"""
    assert 1 <= t.size <= CHUNK
    buf = np.zeros(CHUNK)
    buf[:t.size] = t
    w = 1
    while w < CHUNK:
        buf[0::2 * w] = buf[0::2 * w] + buf[w::2 * w]
        w *= 2
    return buf[0]


def numpy_block_value(q, S, rows, col, pw, c):
    w = q.astype(np.float64) / np.float64(S)
    v = rows[:, col].copy()
    if pw == 2:
        v = v - c
        v = v * v
    if pw == 3:
        v = np.where(v == c, 1.0, 0.0)
    return tree_sum(w * v)


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("model_name,keep_prev,N,nb", [("lgssm2", False, 1000, 100), ("lgssm2", False, 5000, 2048), ("lgssm2", False, 300, 7), ("lgssm2", False, 37, 1),
                                                        ("bearings4", True, 1539, 513), ("object_motion", False, 1000, 129)])
def test_oracle_block_reference_is_the_spec_tree(g, o, model_name, keep_prev, N, nb):
    m = g.models.by_name(model_name)
    ys = g.models.simulate(m, 4)
    f = o.OracleFilter(m.model_id, m.params, N, 11, keep_prev=keep_prev).initialize(ys[0])
    for t in range(1, 3):
        f.update(ys[t])
    n_checked = 0
    for b0 in range(0, N, nb):
        b1 = min(b0 + nb, N)
        cnt = b1 - b0
        lw_b, rows_b = np.ascontiguousarray(f.lw[b0:b1]), np.ascontiguousarray(f.rows[b0:b1])
        s = o.WeightSummary(lw_b, cnt)
        sub = f[b0:b1].summary()
        assert np.array_equal(s.q, sub.q) and s.S == sub.S and s.K == sub.K          # OracleSubState.summary() is this summary
        for col in range(f.W):
            mu = o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, cnt, 1, 0.0)
            assert same(mu, numpy_block_value(s.q, s.S, rows_b, col, 1, 0.0)), (b0, col, "mean")
            assert same(o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, cnt, 2, mu), numpy_block_value(s.q, s.S, rows_b, col, 2, mu)), (b0, col, "var")
            for c in np.unique(rows_b[:, col])[:3]:
                assert same(o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, cnt, 3, float(c)), numpy_block_value(s.q, s.S, rows_b, col, 3, float(c))), (b0, col, "proportion")
            n_checked += 1
    assert n_checked == ((N + nb - 1) // nb) * f.W
