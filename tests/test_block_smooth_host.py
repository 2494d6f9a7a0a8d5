"""Marginal smoothing per block (gpf.h gpf_block_smooth), the parts that need no GPU: the entry point exists in every layer (header, library, ctypes
table, package, Julia glue); the NumPy restatement -- tests/block_smooth_spec.py -- reduces to what it must where its answer is known (T = 1: the
oracle's block mean and variance; no transition density: every step's own normalised weights; every target on its fallback: the ancestral weights);
backward simulation's restatement has the smoothing weights as the marginal law of its step-s indices; and the law experiment of
tests/test_gpu_block_smooth.py passes on the CPU oracle's filter."""
import ctypes
import inspect
import os
import re
import time

import numpy as np
import pytest

import block_backward_spec as bsp
import block_smooth_spec as ssp
from test_block_backward_host import small_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = ["gpf_handle", "int64_t", "int32_t", "int32_t", "double*", "double*", "double*", "int64_t*"]


def header():
    return open(os.path.join(ROOT, "include", "gpf.h")).read()


def test_header_declares_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"gpf_status\s+gpf_block_smooth\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "gpf_block_smooth is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", a.strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == PROTO


def test_header_states_the_definition():
    txt = header()
    end = txt.index("gpf_status gpf_block_smooth(gpf_handle")
    doc = txt[txt.rindex("/*", 0, end):end]
    assert "Hürzeler & Künsch 1998" in doc and "Doucet, Godsill & Andrieu 2000" in doc
    for piece in ("c_T = b", "g_{s+1}[c_{s+1} bs] / bs", "lineage is undefined", "(double)q_j / (double)S", "exp_fix(lwa_ij - m_j, K)", "r_ij = (double)q_ij / (double)D_j",
                  "recorded parent", "ASCENDING j", "not renormalised", "gpf_block_moments' values bit for bit", "the epoch does not advance"):
        assert piece in doc, piece
    for refusal in ("GPF_ERR_STATE", "GPF_ERR_INVALID_ARGUMENT", "whole-filter call", "2048", "all outputs NULL", "per-block parameters", "2^31"):
        assert refusal in doc, refusal


def test_library_exports_the_entry_point(g):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, "gpf_block_smooth"), "gpf_block_smooth is not exported by the built library"
    assert L.gpf_abi_version() == 1                                                          # additive: the ABI version stays


def test_ctypes_table(g):
    C = ctypes
    pd = C.POINTER(C.c_double)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_block_smooth"][1:] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, pd, pd, pd, C.POINTER(C.c_int64)])


def test_package_exports_and_argument_checks(g):
    assert list(inspect.signature(g.block_smoothed_moments).parameters) == ["state", "block_size", "steps", "return_weights", "return_blocks"]
    assert list(inspect.signature(g.block_smoothed_weights).parameters) == ["state", "block_size", "steps"]

    class NoStore:
        history_blocks = True
    for call in (g.block_smoothed_moments, g.block_smoothed_weights):
        with pytest.raises(g.ErrorException, match="history_weights=True"):                  # the message names the keyword
            call(NoStore(), 4)


def test_julia_glue_calls_the_entry_point():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:gpf_block_smooth, libgpf\), Cint, \(Ptr\{Cvoid\}, Int64, Cint, Cint, Ptr\{Cdouble\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}, Ptr\{Int64\}\)", jl)
    assert re.search(r"^function block_smoothed_moments\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)
    assert re.search(r"^function block_smoothed_weights\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)


# ----------------------------------------------------------------------------- the restatement where its answer is known
def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def gamma(k):
    """Higham's gamma_k: the relative error bound of k roundings"""
    u = 2.0 ** -53
    return k * u / (1 - k * u)


@pytest.mark.parametrize("name,n,bs", [("lgssm2", 26, 7), ("bearings4", 1031, 513), ("sv1", 300, 129)])
def test_at_one_step_it_is_the_oracles_block_mean_and_var(g, o, name, n, bs):
    m, L = small_loop(g, o, name, n, bs, 1)
    S = L.store
    mean, var, W, blocks = ssp.smooth(o, name, m.params, S)
    f = L.L.f[0]
    for b in range(S.B):
        b0, b1 = b * bs, min((b + 1) * bs, n)
        s = o.WeightSummary(np.ascontiguousarray(f.lw[b0:b1]), b1 - b0)
        rows_b = np.ascontiguousarray(f.rows[b0:b1])
        assert np.array_equal(W[b, 0, :b1 - b0], s.q.astype(np.float64) / np.float64(s.S)) and np.all(W[b, 0, b1 - b0:] == 0.0) and blocks[b, 0] == b + 1
        for col in range(m.dim):
            mu = o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, b1 - b0, 1, 0.0)
            assert same(mean[b, 0, col], mu), (b, col)
            assert same(var[b, 0, col], o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, b1 - b0, 2, mu)), (b, col)


def test_without_a_transition_density_every_step_has_its_own_weights(g, o):
    """logtrans = 0: r_ij = w_s^i whatever j, so W_s^i = w_s^i sum_j W_{s+1}^j.  The sum is 1 up to its rounding: step T's weights are cnt quotients
    (one rounding each), every step below adds one product and cnt - 1 additions per particle -- (T - s)(cnt + 2) roundings at most, all terms positive"""
    n, bs, T = 3 * 7 + 5, 7, 4
    m, L = small_loop(g, o, "lgssm2", n, bs, T, ess_frac=0.5)              # (the ESS gate leaves unequal stored weights in some blocks)
    S = L.store
    _, _, W, blocks = ssp.smooth(o, "lgssm2", m.params, S, trans=False)
    unequal = 0
    for b in range(S.B):
        b0, b1 = b * bs, min((b + 1) * bs, n)
        for s in range(1, T + 1):
            ws = o.WeightSummary(np.ascontiguousarray(S.lw[s - 1][b0:b1]), b1 - b0)
            own = ws.q.astype(np.float64) / np.float64(ws.S)
            unequal += int(own.max() != own.min())
            assert np.all(np.abs(W[b, s - 1, :b1 - b0] - own) <= gamma((T - s) * (b1 - b0 + 2)) * own), (b, s)
            assert blocks[b, s - 1] == b + 1
    assert unequal > 0
    full = ssp.smooth(o, "lgssm2", m.params, S)[2]
    assert np.array_equal(full[:, -1], W[:, -1]) and not np.array_equal(full[:, :-1], W[:, :-1])    # (the density matters; step T is the same)


def test_with_every_target_on_its_fallback_the_weights_are_the_ancestral_ones(g, o):
    """r_ij = [i is j's recorded parent]: W_s^i is the total current weight of particle i's descendants, so the smoothed mean is the ancestral
    block mean of the past choice (history_mean per block) up to the order of the additions: at most cnt + 1 roundings of positive terms per step"""
    n, bs, T = 3 * 7 + 5, 7, 4
    m, L = small_loop(g, o, "lgssm2", n, bs, T)
    S = L.store
    mean, _, W, _ = ssp.smooth(o, "lgssm2", m.params, S, fallback=True)
    for b in range(S.B):
        b0, b1 = b * bs, min((b + 1) * bs, n)
        ws = o.WeightSummary(np.ascontiguousarray(S.lw[T - 1][b0:b1]), b1 - b0)
        wT = ws.q.astype(np.float64) / np.float64(ws.S)
        for s in range(1, T + 1):
            anc = S.gen.index(s)[b0:b1]                                        # the step-s ancestor of every current particle of the block
            assert np.all(anc // bs == b)
            want = np.bincount(anc - b0, weights=wT, minlength=b1 - b0)
            tol = gamma((T - s + 1) * (b1 - b0 + 2))
            assert np.all(np.abs(W[b, s - 1, :b1 - b0] - want) <= tol * want), (b, s)
            x = S.x(s)[b0:b1]
            ancestral = (wT[:, None] * S.x(s)[anc]).sum(axis=0)                # mean(state[b], s => c)
            assert np.all(np.abs(mean[b, s - 1] - ancestral) <= 2 * tol * (want[:, None] * np.abs(x)).sum(axis=0) + 1e-300), (b, s)


def test_a_target_no_candidate_leads_to_hands_its_mass_to_its_recorded_parent(g, o):
    """line_model (logtrans 0 where the slope persists, -Inf elsewhere), the hand-built store of tests/test_block_backward_host.py: the two step-2
    particles of slope 7 give their weight to their recorded parents, the two of slope 1 share theirs among the step-1 particles of slope 1"""
    m = g.models.line_model()
    S = bsp.Store(4, 4, 2)
    x1 = np.array([[1.0, 0.0], [1.0, 1.0], [2.0, 0.0], [-1.0, 0.0]])
    x2 = np.array([[7.0, 0.0], [1.0, 0.0], [7.0, 1.0], [1.0, 1.0]])
    S.begin_step(np.zeros((1, 2))); S.end_step(x1, np.zeros(4))
    S.begin_step(np.zeros((1, 2))); S.resample_blocks(np.array([3, 4, 1, 2]), np.array([True])); S.end_step(x2, np.log([0.1, 0.2, 0.3, 0.4]))
    _, _, W, blocks = ssp.smooth(o, "line_model", m.params, S)
    # targets 0 and 2 (slope 7): recorded parents 2 and 0; targets 1 and 3 (slope 1): half each to candidates 0 and 1; ascending j
    w2 = W[0, 1]
    assert np.array_equal(W[0, 0], np.array([w2[1] * 0.5 + w2[2] + w2[3] * 0.5, w2[1] * 0.5 + w2[3] * 0.5, w2[0], 0.0]))
    assert np.array_equal(blocks, [[1, 1]])


# ----------------------------------------------------------------------------- two kernels, one law (the CPU rehearsal)
def test_backward_simulations_indices_have_the_smoothing_weights_as_their_law(g, o):
    """the experiment of tests/test_gpu_block_smooth.py::test_backward_draws_have_the_smoothing_weights_as_their_marginal with the two restatements on
    the oracle's filter, the same seeds: the worst cell stays within the bound, and is the value written beside the constant"""
    n = ssp.PAIR_B * ssp.PAIR_N
    m, L = small_loop(g, o, "lgssm2", n, ssp.PAIR_N, ssp.PAIR_T, seed=ssp.PAIR_SEED)
    _, idx = bsp.backward(o, "lgssm2", m.params, L.store, L.seed, L.epoch, ssp.PAIR_K)
    W = ssp.smooth(o, "lgssm2", m.params, L.store)[2]
    worst, cells = ssp.pair_units(idx, W, ssp.PAIR_N)
    print("backward simulation against the smoothing weights, restatements:", cells, "cells, worst", round(worst, 2))
    assert cells > 200
    assert worst <= ssp.PAIR_SIGMAS, worst
    assert round(worst, 2) == ssp.PAIR_REHEARSED


# ----------------------------------------------------------------------------- the law experiment on the CPU
def law_run(g, o, N):
    m, ys, mu, _ = bsp.law_setup(g.models)
    L = bsp.StoreLoop(o, m, ssp.LAW_B * N, N, ssp.LAW_SEED)
    obs = lambda t: np.tile(ys[t], (ssp.LAW_B, 1))
    L.initialize(obs(0))
    for t in range(1, ssp.LAW_T):
        L.resample()
        L.update(obs(t))
    mean = ssp.smooth(o, "lgssm2", m.params, L.store)[0]
    return ssp.law_units(mean, mu)


def test_law_experiment_on_the_restatement(g, o):
    """the experiment of tests/test_gpu_block_smooth.py::test_smoothed_means_follow_the_exact_smoother on the oracle's filter, at the block size that
    test fixes: the across-block average of every smoothed mean within 5 across-block standard errors of the exact one"""
    t0 = time.time()
    z = law_run(g, o, ssp.LAW_N)
    print("marginal smoothing, restatement, N =", ssp.LAW_N, ": mean z", np.round(z, 2).tolist(), "worst", round(float(z.max()), 2), "in", round(time.time() - t0, 1), "s")
    assert np.all(z <= ssp.LAW_SIGMAS), z
    assert round(float(z.max()), 2) == ssp.LAW_REHEARSED[ssp.LAW_N]
