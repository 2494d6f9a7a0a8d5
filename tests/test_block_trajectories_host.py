"""Whole trajectories per block (gpf.h gpf_block_sample_trajectories), the parts that need no GPU: the entry point exists in every layer (header,
library, ctypes table, package, Julia glue), and the reference the GPU tests compare the draws against -- tests/block_trajectories_spec.py -- gives the
hand-computed answer on weights whose CDF cells are known exactly."""
import ctypes
import inspect
import os
import re

import numpy as np

import hp_weights as hw
from block_history_spec import Genealogy
from block_trajectories_spec import draw_indices, paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gpf_block_sample_trajectories"
PARAMS = ["gpf_handle", "int64_t", "int32_t", "int32_t", "int32_t", "double*", "int64_t*"]


def test_header_declares_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpf.h")).read(), flags=re.S)
    m = re.search(r"gpf_status\s+%s\s*\(([^;]*?)\)\s*;" % NAME, hdr)
    assert m, f"{NAME} is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", a.strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == PARAMS                                                   # (no const: both arrays are outputs)


def test_header_cites_the_reference_and_documents_the_deviation():
    txt = open(os.path.join(ROOT, "include", "gpf.h")).read()
    doc = txt[txt.index("gpf_block_history_proportion(gpf_handle"):txt.index(NAME + "(gpf_handle")]
    assert "src/utils.jl:7,189-194" in doc and "src/view.jl:35-48" in doc
    assert "DEVIATION" in doc and "NaN" in doc and "2048" in doc
    assert "b * n_samples + j" in doc and "resample_u64" in doc and "mulhi64" in doc and "fix_K" in doc      # the numerical spec of the draw
    assert "freed before it returns" in doc                                   # who owns the scratch


def test_library_exports_the_entry_point(g):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, NAME), f"{NAME} is not exported by the built library"


def test_ctypes_table(g):
    C = ctypes
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table[NAME][1:] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)])


def test_package_exports(g):
    assert callable(getattr(g, "block_sample_trajectories", None))
    sig = inspect.signature(g.block_sample_trajectories).parameters
    assert list(sig)[:3] == ["state", "block_size", "n_samples"] and sig["n_samples"].default == 1
    assert sig["steps"].default is None and sig["return_indices"].default is False


def test_julia_glue_calls_the_entry_point():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:%s, libgpf\), Cint, \(Ptr\{Cvoid\}, Int64, Cint, Cint, Cint, Ptr\{Cdouble\}, Ptr\{Int64\}\)" % NAME, jl), f"no ccall of {NAME}"
    assert re.search(r"^function block_sample_trajectories\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)


# ----------------------------------------------------------------------------- the reference of the GPU tests on a hand-computed example
# 2 blocks of 3 particles, K = fix_K(3) = 52.  Block 0 has the weights (1, 0, 1): q = (2^52, 0, 2^52), cdf = (2^52, 2^52, 2^53), S = 2^53, the target is
# floor(U 2^53 / 2^64) = U >> 11, so the draw is particle 1 if U < 2^63 and particle 3 otherwise -- particle 2 never.  Block 1 has (1, 1, 0):
# cdf = (2^52, 2^53, 2^53): particle 1 if U < 2^63, else particle 2.  U is the 64-bit word of the draw's resample slot, from the Python Philox of
# tests/hp_reference.py.
SEED, EPOCH, K_DRAWS = 12345, 3, 40
NEG = -np.inf
LW_HAND = np.array([0.0, NEG, 0.0, 0.0, 0.0, NEG])


def by_hand(slot0, hi_particle):
    U = [hw.resample_u64(SEED, slot0 + j, EPOCH) for j in range(K_DRAWS)]
    return np.array([1 if u < 2 ** 63 else hi_particle for u in U], np.int64)


def test_spec_on_exact_cdf_cells(o):
    assert o.fix_K(3) == 52
    s = o.WeightSummary(LW_HAND[:3].copy(), 3)
    assert list(s.cdf) == [2 ** 52, 2 ** 52, 2 ** 53] and s.S == 2 ** 53
    idx = draw_indices(o, LW_HAND, SEED, EPOCH, 3, K_DRAWS)
    assert idx.shape == (2, K_DRAWS) and idx.dtype == np.int64
    assert np.array_equal(idx[0], by_hand(0, 3))                              # block 0: slot j
    assert np.array_equal(idx[1], by_hand(K_DRAWS, 2))                        # block 1: slot n_samples + j
    assert set(idx[0]) == {1, 3} and set(idx[1]) == {1, 2}                    # both cells of either block were drawn
    assert not np.array_equal(by_hand(0, 2), by_hand(K_DRAWS, 2))             # ... from different uniforms
    # another epoch, other draws
    assert not np.array_equal(draw_indices(o, LW_HAND, SEED, EPOCH + 1, 3, K_DRAWS), idx)
    # a short last block: n = 5 in blocks of 3 -> the last block has 2 particles and K = fix_K(2)
    idx5 = draw_indices(o, LW_HAND[:5], SEED, EPOCH, 3, K_DRAWS)
    assert idx5.shape == (2, K_DRAWS) and np.array_equal(idx5[1], by_hand(K_DRAWS, 2))


def test_spec_one_block_is_sample_unweighted(g, o):
    """block_size >= n: draw j reads slot j, the numbering of OracleFilter.sample_unweighted at the same seed and epoch"""
    m = g.models.lgssm2()
    rng = np.random.default_rng(3)
    n = 37
    lw = rng.standard_normal(n) * 3.0
    f = o.OracleFilter(m.model_id, m.params, n, SEED)
    f.lw, f.epoch = lw.copy(), EPOCH
    _, want = f.sample_unweighted(K_DRAWS)
    for bs in (n, n + 5, 2 ** 40):
        got = draw_indices(o, lw, SEED, EPOCH, bs, K_DRAWS)
        assert got.shape == (1, K_DRAWS) and np.array_equal(got[0], want)
    assert not np.array_equal(draw_indices(o, lw, SEED, EPOCH, 19, K_DRAWS)[0], want)     # (two blocks: other weights, another K)


def test_spec_all_neginf_block_is_uniform(o):
    """q = (1, 1, 1), S = 3: the target floor(3 U / 2^64) IS the drawn cell"""
    lw = np.array([NEG, NEG, NEG, 0.0, NEG, 0.0])
    idx = draw_indices(o, lw, SEED, EPOCH, 3, K_DRAWS)
    assert np.array_equal(idx[0], [3 * hw.resample_u64(SEED, j, EPOCH) // 2 ** 64 + 1 for j in range(K_DRAWS)])
    assert set(idx[0]) == {1, 2, 3}
    assert np.array_equal(idx[1], by_hand(K_DRAWS, 3))


def test_spec_nan_block_reads_zero_and_nan_paths(o):
    lw = LW_HAND.copy()
    lw[4] = np.nan
    idx = draw_indices(o, lw, SEED, EPOCH, 3, 5)
    assert np.all(idx[1] == 0) and np.array_equal(idx[0], by_hand(0, 3)[:5])
    lw[4] = np.inf
    assert np.all(draw_indices(o, lw, SEED, EPOCH, 3, 5)[1] == 0)
    # the paths: the hand example of tests/test_block_history_host.py has 2 blocks of 2 particles and 3 steps
    gen = Genealogy(4)
    gen.begin_step([[10.0], [11.0], [12.0], [13.0]])
    gen.begin_step([[20.0], [21.0], [22.0], [23.0]])
    gen.resample("blocks", [2, 2, 99, -5], [True, False], 2)
    gen.set_rows([[21.0], [21.0], [22.0], [23.0]])
    gen.begin_step([[30.0], [31.0], [32.0], [33.0]])
    gen.resample("global", [3, 4, 1, 2])
    gen.set_rows([[32.0], [33.0], [30.0], [31.0]])
    tr = paths(gen, np.array([[2, 1], [0, 0]]), 2, 1, 3, 1)
    assert tr.shape == (2, 2, 3, 1)
    # current particle 1 (block 0, index 2) is a copy of old particle 3, whose step-2 value is 23 and step-1 value 13; particle 0 <- 2: 22, 12
    assert tr[0, :, :, 0].tolist() == [[13.0, 23.0, 33.0], [12.0, 22.0, 32.0]]
    assert np.all(np.isnan(tr[1]))
    assert paths(gen, np.array([[1], [2]]), 2, 2, 2, 1)[:, 0, 0, 0].tolist() == [22.0, 21.0]   # block 1's particle 3 <- old 1: its step-2 value is 21
