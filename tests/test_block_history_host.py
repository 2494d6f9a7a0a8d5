"""The block-wise trajectory store (gpf.h gpf_history_enable_blocks, gpf_block_history_moments, gpf_block_history_proportion), the parts that need
no GPU: the entry points exist in every layer (header, library, ctypes table, package, Julia glue), and the reference the GPU tests compare the
recorded genealogy against -- tests/block_history_spec.py -- gives the hand-computed answer on a small example with a stale parents array."""
import ctypes
import os
import re

import numpy as np
import pytest

from block_history_spec import Genealogy, resample_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "gpf_history_enable_blocks": ["gpf_handle", "int32_t"],
    "gpf_block_history_moments": ["gpf_handle", "int32_t", "int64_t", "double*", "double*"],
    "gpf_block_history_proportion": ["gpf_handle", "int32_t", "int64_t", "int32_t", "double*", "int32_t", "double*"],
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
    doc = txt[txt.index("the block-wise trajectory store"):txt.index("gpf_block_history_proportion(gpf_handle")]
    assert "src/statistics.jl:13-14, 48-50, 91-101" in doc and "src/view.jl:35-48" in doc
    assert "DEVIATION" in doc and "NaN" in doc and "2048" in doc


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_library_exports_the_entry_point(g, name):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, name), f"{name} is not exported by the built library"


def test_ctypes_table(g):
    C = ctypes
    pd = C.POINTER(C.c_double)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_history_enable_blocks"][1:] == (C.c_int, [C.c_void_p, C.c_int32])
    assert table["gpf_block_history_moments"][1:] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, pd, pd])
    assert table["gpf_block_history_proportion"][1:] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, pd, C.c_int32, pd])


def test_package_exports(g):
    import inspect
    for name in ("block_mean", "block_var", "block_moments", "block_proportionmap", "pf_initialize_blocks"):
        assert callable(getattr(g, name, None)), name
    assert "step" in inspect.signature(g.block_moments).parameters
    assert "history" in inspect.signature(g.pf_initialize_blocks).parameters
    assert "history_blocks" in inspect.signature(g.DeviceParticleFilterState.__init__).parameters


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_julia_glue_calls_the_entry_point(name):
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:%s, libgpf\), Cint, \(" % name, jl), f"no ccall of {name}"
    for sig in (r"block_mean\(s::DeviceParticleFilterState, block_size::Int, addr::Pair", r"block_var\(s::DeviceParticleFilterState, block_size::Int, addr::Pair",
                r"block_proportionmap\(s::DeviceParticleFilterState, block_size::Int, addr::Pair", r"block_moments\(s::DeviceParticleFilterState, block_size::Int, step::Integer"):
        assert re.search(r"^function %s" % sig, jl, re.M), sig


# ----------------------------------------------------------------------------- the reference of the GPU tests on a hand-written example
def hand_example(stale_a=(99, -5), stale_b=(7, 0)):
    """2 blocks of 2 particles, 3 steps.  Step 2: block 0 resamples (both slots from its particle 1), block 1 does not -- its parents entries
    are stale_a.  Step 3: block 1 resamples (swaps its particles), block 0 does not (stale_b); then the blocks are swapped whole (global parents)."""
    gen = Genealogy(4)
    gen.begin_step([[10.0], [11.0], [12.0], [13.0]])
    gen.begin_step([[20.0], [21.0], [22.0], [23.0]])
    gen.resample("blocks", [2, 2, stale_a[0], stale_a[1]], [True, False], 2)
    gen.set_rows([[21.0], [21.0], [22.0], [23.0]])
    gen.begin_step([[30.0], [31.0], [32.0], [33.0]])
    gen.resample("blocks", [stale_b[0], stale_b[1], 2, 1], [False, True], 2)
    gen.resample("global", [3, 4, 1, 2])
    gen.set_rows([[33.0], [32.0], [30.0], [31.0]])
    return gen


def test_genealogy_hand_example():
    gen = hand_example()
    assert gen.steps == 3
    assert list(gen.trace(3, 0)) == [33.0, 32.0, 30.0, 31.0]
    # step 3, back through the block swap, then block 1's own swap: current 0 <- 2 <- 3, 1 <- 3 <- 2, 2 <- 0, 3 <- 1
    assert list(gen.index(2)) == [3, 2, 0, 1]
    assert list(gen.trace(2, 0)) == [23.0, 22.0, 21.0, 21.0]
    # ... and step 2's resample is not part of the way from step 2 to step 2, but it is on the way to step 1
    assert list(gen.index(1)) == [3, 2, 1, 1]
    assert list(gen.trace(1, 0)) == [13.0, 12.0, 11.0, 11.0]


def test_genealogy_ignores_stale_parents():
    ref = hand_example()
    for stale_a, stale_b in [((1, 1), (2, 2)), ((2, 1), (1, 2)), ((-7, 10 ** 9), (0, 0)), ((4, 3), (3, 4))]:
        gen = hand_example(stale_a, stale_b)
        for t in (1, 2, 3):
            assert np.array_equal(gen.trace(t, 0), ref.trace(t, 0)), (stale_a, stale_b, t)
    # reading the stale entries as block-local parents WOULD change the answer: the example can tell the two apart
    naive = resample_map(("blocks", [2, 2, 1, 1], [True, True], 2), 4)
    assert list(naive) != list(resample_map(("blocks", [2, 2, 1, 1], [True, False], 2), 4))
    # and reading a resampled block's parents as GLOBAL indices would, too
    assert list(resample_map(("blocks", [7, 0, 2, 1], [False, True], 2), 4)) == [0, 1, 3, 2]


def test_genealogy_equals_carrying_the_trajectories_along():
    """the same answer by brute force: every particle carries its whole past through every gather"""
    rng = np.random.default_rng(5)
    n, nb, T, d = 23, 5, 6, 2
    B = (n + nb - 1) // nb
    gen, carried = Genealogy(n), []                                         # carried[s]: [n, d] values of step s + 1 of the CURRENT particles
    for s in range(T):
        rows = rng.standard_normal((n, d))
        gen.begin_step(rows); carried.append(rows.copy())
        for _ in range(int(rng.integers(0, 3))):
            if rng.random() < 0.6:
                mask = rng.random(B) < 0.5
                cnt = np.minimum(nb, n - (np.arange(n) // nb) * nb)
                parents = np.where(mask[np.arange(n) // nb], rng.integers(0, 10 ** 6, n) % cnt + 1, rng.integers(-50, 50, n))
                ev = ("blocks", parents, mask, nb)
            else:
                ev = ("global", rng.integers(1, n + 1, n))
            gen.resample(*ev)
            g_map = resample_map(ev, n)
            carried = [c[g_map] for c in carried]
        if rng.random() < 0.5:                                              # rejuvenation: the current step's values change in place
            carried[-1] = carried[-1] + 1.0
        gen.set_rows(carried[-1])
        for t in range(1, s + 2):
            for c in range(d):
                assert np.array_equal(gen.trace(t, c), carried[t - 1][:, c]), (s, t, c)
