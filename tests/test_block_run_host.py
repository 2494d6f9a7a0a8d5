"""A whole series per block in one launch (gpf.h gpf_run_blocks), the parts that need no GPU: the entry point exists in every layer (header, library,
ctypes table, package, Julia glue, the build's list of units); the argument checks of pf_run_blocks that come before the library; and the restatement
tests/block_run_spec.py reduces to the oracle's own loop -- oracle.resample_blocks, oracle.update_blocks, the sub-states' statistics -- where that
loop is defined, and leaves a block with NaN weights alone where it is not."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import block_run_spec as rs
from test_gpu_block_conditional import block_obs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = ["gpf_handle", "double*", "int32_t", "int32_t", "int32_t", "int64_t", "int32_t", "int32_t", "double", "double*", "double*", "int32_t*", "int32_t*"]


def header():
    return open(os.path.join(ROOT, "include", "gpf.h")).read()


# ----------------------------------------------------------------------------- the entry point in every layer
def test_header_declares_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"gpf_status\s+gpf_run_blocks\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "gpf_run_blocks is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", re.sub(r"\bconst\b", "", a).strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == PROTO


def test_header_states_the_contract():
    txt = header()
    end = txt.index("gpf_status gpf_run_blocks(gpf_handle")
    doc = txt[txt.rindex("/*", 0, end):end]
    for piece in ("README.md:60-79", "test/resample.jl:130-162", "gpf_resample_blocks(h, method, block_size, NaN, sort_particles, ess_frac, GPF_CHECK_FALSE, NULL, NULL)",
                  "gpf_update_blocks(h, obs[:, t], n_obs, block_size)", "E + 2 n_steps", "bit for bit", "[n_blocks][n_steps][n_obs]", "[n_steps][n_obs]",
                  "[n_steps][n_blocks]", "Invalid weights (NaN).", "GPF_K_STEP", "T1 + T2"):
        assert piece in doc, piece
    for refusal in ("GPF_ERR_STATE", "GPF_ERR_INVALID_ARGUMENT", "GPF_ERR_UNKNOWN_METHOD", "sub-state view", "shard", "trajectory store of either kind",
                    "forward smoothing", "keep_prev", "strata", "2048", "4096", "2^31", "non-finite", "rejuvenation, proposals, a reference path, tempering"):
        assert refusal in doc, refusal


def test_library_exports_the_entry_point(g):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, "gpf_run_blocks"), "gpf_run_blocks is not exported by the built library"
    assert L.gpf_abi_version() == 1                                          # additive: the ABI version stays


def test_ctypes_table(g):
    C = ctypes
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_run_blocks"][1:] == (C.c_int, [C.c_void_p, pd, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double, pd, pd, pi, pi])


def test_the_build_compiles_the_unit():
    import __graft_entry__ as ge
    assert "libgpf_run.hip" in ge.HIP_UNITS and os.path.exists(os.path.join(ge.CSRC, "libgpf_run.hip"))
    host = open(os.path.join(ge.CSRC, "gpf_host.hpp")).read()
    assert "void launch_block_run(gpf_filter* h, const RunArgs& a, int method);" in host
    assert '#include "gpf_k_block_run.hpp"' in open(os.path.join(ge.CSRC, "gpf_kernels.hpp")).read()


def test_julia_glue_calls_the_entry_point():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:gpf_run_blocks, libgpf\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}, Cint, Cint, Cint, Int64, Cint, Cint, Cdouble, Ptr\{Cdouble\}, "
                     r"Ptr\{Cdouble\}, Ptr\{Cint\}, Ptr\{Cint\}\)", jl)
    assert re.search(r"^function pf_run_blocks!\(s::DeviceParticleFilterState, observations::Union\{Array\{Float64,3\},Matrix\{Float64\}\}, block_size::Int", jl, re.M)


# ----------------------------------------------------------------------------- the package: what pf_run_blocks checks before the library
def test_package_exports_and_argument_checks(g):
    assert list(inspect.signature(g.pf_run_blocks).parameters) == ["state", "observations", "block_size", "method", "ess_frac", "sort_particles"]
    sig = inspect.signature(g.pf_run_blocks).parameters
    assert (sig["method"].default, sig["ess_frac"].default, sig["sort_particles"].default) == ("multinomial", 0.5, True)
    assert sig["ess_frac"].kind is inspect.Parameter.KEYWORD_ONLY and g.BlockRun._fields == ("lml", "ess", "resampled")

    class Stub:                                                               # (no handle: every check below comes before the library is called)
        n_particles = 300
    y = np.zeros((3, 5, 2))
    with pytest.raises(g.ErrorException, match="Resampling method systematic not recognized"):
        g.pf_run_blocks(Stub(), y, 100, "systematic")
    with pytest.raises(g.ErrorException, match="Resampling method multinomial_sorted not recognized"):
        g.pf_run_blocks(Stub(), y, 100, "multinomial_sorted")
    with pytest.raises(g.ErrorException, match="block_size < 1"):
        g.pf_run_blocks(Stub(), y, 0)
    for bad in (np.zeros((4, 5, 2)), np.zeros((3, 0, 2)), np.zeros(10), np.zeros((0, 2)), np.zeros((3, 5, 2, 1))):
        with pytest.raises(g.ErrorException, match=r"observations of shape \(3, T, n_obs\), or \(T, n_obs\)"):
            g.pf_run_blocks(Stub(), bad, 100)
    with pytest.raises(g.ErrorException, match=r"observations of shape \(1, T, n_obs\)"):     # (the block size is clamped to the particle count)
        g.pf_run_blocks(Stub(), y, 5000)


# ----------------------------------------------------------------------------- the restatement against the oracle's own loop
def oracle_pair(g, o, n, bs, seed=19, steps=6):
    m = g.models.lgssm2()
    ys = block_obs(g, m, (n + bs - 1) // bs, steps)
    return m, ys, [o.initialize_blocks(o.OracleFilter(m.model_id, m.params, n, seed), bs, ys[:, 0]) for _ in range(2)]


@pytest.mark.parametrize("method,ess_frac,sort_particles", [("multinomial", None, True), ("residual", 0.5, True), ("stratified", 0.5, False)])
def test_spec_reduces_to_the_oracle_loop(g, o, method, ess_frac, sort_particles):
    n, bs = 330, 100                                                          # (a short last block)
    m, ys, (f, h) = oracle_pair(g, o, n, bs)
    got = rs.run_blocks(o, f, bs, ys[:, 1:], method, ess_frac=ess_frac, sort_particles=sort_particles)
    e0 = h.epoch
    for t in range(1, ys.shape[1]):
        mask = o.resample_blocks(h, bs, method, ess_frac=ess_frac, sort_particles=sort_particles, check=False)
        o.update_blocks(h, bs, ys[:, t])
        assert np.array_equal(got.resampled[:, t - 1], mask)
        for k, (a, b) in enumerate(o.blocks_of(h, bs)):
            assert got.ess[k, t - 1] == h[a:b].effective_sample_size() and got.lml[k, t - 1] == h[a:b].log_ml_estimate()
    assert np.array_equal(f.rows, h.rows) and np.array_equal(f.lw, h.lw) and np.array_equal(f.parents, h.parents)
    assert f.epoch == h.epoch == e0 + 2 * (ys.shape[1] - 1) and f.lml_est == h.lml_est == 0.0
    if ess_frac is not None:
        assert got.resampled.any() and not got.resampled.all()


def test_spec_shared_series_and_invalid_blocks(g, o):
    n, bs = 300, 100
    m, ys, (f, h) = oracle_pair(g, o, n, bs)
    one = ys[0, 1:]
    a = rs.run_blocks(o, f, bs, one, "multinomial", ess_frac=None)
    b = rs.run_blocks(o, h, bs, np.tile(one, (3, 1, 1)), "multinomial", ess_frac=None)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(f.rows, h.rows) and np.array_equal(f.lw, h.lw)
    # a NaN in block 1: oracle.resample_blocks raises there; the restatement leaves the block as it stands, propagates it, and goes on
    f.lw[150] = np.nan; h.lw[150] = np.nan
    with pytest.raises(o.OracleError, match="Invalid weights"):
        o.resample_blocks(h, bs, "multinomial", check=False)
    rows1, par1 = f.rows[bs:2 * bs].copy(), f.parents.copy()
    r = rs.run_blocks(o, f, bs, one[:1], "multinomial", ess_frac=None)
    assert list(r.resampled[:, 0]) == [True, False, True] and np.isnan(r.lml[1, 0]) and np.isnan(r.ess[1, 0]) and np.isfinite(r.lml[[0, 2], 0]).all()
    assert np.array_equal(f.parents[bs:2 * bs], par1[bs:2 * bs]) and not np.array_equal(f.rows[bs:2 * bs], rows1)   # kept its parents, was propagated
    assert np.isnan(f.lw[150]) and np.isfinite(np.delete(f.lw, 150)).all()
