"""Backward simulation per block (gpf.h gpf_history_enable_blocks_weights, gpf_block_backward_sample), the parts that need no GPU: the two entry points
exist in every layer (header, library, ctypes table, package, Julia glue); the NumPy restatement -- tests/block_backward_spec.py -- reduces to
independent categorical draws per step where it must, draws a hand-built two-step store with the exact probabilities, takes the recorded parent where
no candidate can lead to the held particle, and passes the law experiment of tests/test_gpu_block_backward.py on the CPU oracle's filter."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import block_backward_spec as bsp
import block_conditional_spec as cs
from block_ancestor_spec import logtrans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "gpf_history_enable_blocks_weights": ["gpf_handle", "int32_t"],
    "gpf_block_backward_sample": ["gpf_handle", "int64_t", "int32_t", "int32_t", "int32_t", "double*", "int64_t*"],
}


def header():
    return open(os.path.join(ROOT, "include", "gpf.h")).read()


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_header_declares_the_entry_point(name):
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"gpf_status\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
    assert m, f"{name} is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", a.strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == PROTOS[name]


def test_header_documents_the_backward_pass():
    txt = header()
    end = txt.index("gpf_status gpf_history_enable_blocks_weights(gpf_handle")
    doc = txt[txt.rindex("/*", 0, end):end]
    assert "Godsill, Doucet & West 2004" in doc and "Whiteley 2010" in doc and "Lindsten & Schoen 2013" in doc
    assert "8 bytes more per particle and step" in doc and "FINAL order" in doc                # the price and the moment of the records
    assert "E + (T - s)" in doc and "logtrans" in doc and "recorded parent" in doc             # the uniforms, the density, the fallback
    assert "CURRENT parameter row" in doc and "T - step_lo + 1" in doc
    assert "only a valid smoother when every resample was block-wise or across blocks" in doc
    for refusal in ("GPF_ERR_STATE", "GPF_ERR_INVALID_ARGUMENT", "whole-filter call", "2048", "traj_out NULL", "per-block parameters"):
        assert refusal in doc, refusal
    assert "no backward simulation" not in txt                                                # (what gpf_block_sample_trajectories' text used to say)


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_library_exports_the_entry_point(g, name):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, name), f"{name} is not exported by the built library"
    assert L.gpf_abi_version() == 1                                                          # additive: the ABI version stays


def test_ctypes_table(g):
    C = ctypes
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_history_enable_blocks_weights"][1:] == (C.c_int, [C.c_void_p, C.c_int32])
    assert table["gpf_block_backward_sample"][1:] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)])


def test_package_exports_and_argument_checks(g):
    p = inspect.signature(g.pf_initialize_blocks).parameters["history_weights"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(g.block_backward_trajectories).parameters) == ["state", "block_size", "n_samples", "steps", "return_indices"]
    with pytest.raises(ValueError, match="history=T"):                                       # refused before anything is created
        g.pf_initialize_blocks(g.models.lgssm2(), (1,), np.zeros((2, 2)), 8, 4, history_weights=True)

    class NoStore:
        history_blocks = True
    with pytest.raises(g.ErrorException, match="history_weights=True"):                      # the message names the keyword
        g.block_backward_trajectories(NoStore(), 4)


def test_julia_glue_calls_the_entry_points():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:gpf_history_enable_blocks_weights, libgpf\), Cint, \(Ptr\{Cvoid\}, Cint\)", jl)
    assert re.search(r"ccall\(\(:gpf_block_backward_sample, libgpf\), Cint, \(Ptr\{Cvoid\}, Int64, Cint, Cint, Cint, Ptr\{Cdouble\}, Ptr\{Int64\}\)", jl)
    assert re.search(r"^function block_backward_trajectories\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)
    assert "history_weights::Bool=false" in jl


# ----------------------------------------------------------------------------- the restatement where its answer is known
def small_loop(g, o, name, n, bs, T, seed=17, ess_frac=None):
    from test_gpu_block_conditional import block_obs, model_of
    m = model_of(g, name)
    B = (n + bs - 1) // bs
    ys = block_obs(g, m, B, T)
    L = bsp.StoreLoop(o, m, n, bs, seed)
    L.initialize(ys[:, 0])
    for t in range(1, T):
        L.resample(ess_frac)
        L.update(ys[:, t])
    return m, L


def test_without_a_transition_density_the_steps_are_independent_categorical_draws(g, o):
    """logtrans = 0 and every block resampling every step: the candidates are the held particle's own block with equal weights, so step s of draw j is
    the categorical draw of slot b n_samples + j at epoch E + (T - s) from that block's recorded weights -- whatever the later steps held"""
    n, bs, T, ns = 3 * 7 + 5, 7, 4, 3
    m, L = small_loop(g, o, "lgssm2", n, bs, T)
    S = L.store
    traj, idx = bsp.backward(o, "lgssm2", m.params, S, L.seed, L.epoch, ns, trans=False)
    for b in range(S.B):
        b0, b1 = b * bs, min((b + 1) * bs, n)
        for s in range(1, T + 1):
            ws = o.WeightSummary(np.ascontiguousarray(S.lw[s - 1][b0:b1]), b1 - b0)
            want = b0 + o.upper_bound(ws.cdf, o.targets_multinomial(L.seed, L.epoch + (T - s), b * ns, ns, ws.S)) + 1
            assert np.array_equal(idx[b, :, s - 1], want), (b, s)
            assert np.array_equal(traj[b, :, s - 1], S.x(s)[want - 1])
    full, _ = bsp.backward(o, "lgssm2", m.params, S, L.seed, L.epoch, ns)
    assert not np.array_equal(full[:, :, :-1], traj[:, :, :-1]) and np.array_equal(full[:, :, -1], traj[:, :, -1])   # (the density matters; step T is the same draw)


def test_draw_frequencies_of_a_hand_built_store_match_the_exact_kernel(g, o):
    """one block of four sv1 particles, two steps, unequal weights at both, no resample: P(i2, i1) = w2[i2] w1[i1] f(x2[i2] | x1[i1]) / sum_k w1[k]
    f(x2[i2] | x1[k]).  2^16 draws of the restatement against these sixteen probabilities: Pearson's chi-square has 15 degrees of freedom, mean 15 and
    standard deviation sqrt(30); the bound is 5 of these units above the mean (the fixed-point weights differ from the real ones by < 2^-50)."""
    m = g.models.by_name("sv1")
    S = bsp.Store(4, 4, 1)
    x1, x2 = np.array([[-0.6], [-0.1], [0.3], [0.9]]), np.array([[-0.4], [0.0], [0.2], [0.7]])
    lw1, lw2 = np.log([0.1, 0.2, 0.3, 0.4]), np.log([0.4, 0.3, 0.2, 0.1])
    S.begin_step(np.zeros((1, 1))); S.end_step(x1, lw1)
    S.begin_step(np.zeros((1, 1))); S.end_step(x2, lw2)
    ns = 1 << 16
    traj, idx = bsp.backward(o, "sv1", m.params, S, seed=11, epoch=3, n_samples=ns)
    f = np.exp(np.stack([logtrans("sv1", m.params, x1, x2[i], np.zeros(1)) for i in range(4)]))     # [i2, i1]
    back = np.exp(lw1)[None, :] * f
    prob = np.exp(lw2)[:, None] * back / back.sum(axis=1, keepdims=True)
    assert abs(prob.sum() - 1.0) < 1e-12
    got = np.zeros((4, 4))
    np.add.at(got, (idx[0, :, 1] - 1, idx[0, :, 0] - 1), 1)
    chi2 = float(((got - ns * prob) ** 2 / (ns * prob)).sum())
    print("chi-square of 2^16 draws over 16 cells:", round(chi2, 2))
    assert chi2 <= 15 + 5 * np.sqrt(30), chi2
    assert np.array_equal(traj[0, :, 0, 0], x1[idx[0, :, 0] - 1, 0]) and np.array_equal(traj[0, :, 1, 0], x2[idx[0, :, 1] - 1, 0])


def test_a_held_particle_no_candidate_leads_to_takes_its_recorded_parent(g, o):
    """line_model: logtrans is 0 where the slope persists and -Inf elsewhere.  A step-2 particle whose slope no step-1 candidate holds has all -Inf
    ancestor weights and keeps its recorded parent; one whose slope some candidates hold is drawn among exactly those."""
    m = g.models.line_model()
    S = bsp.Store(4, 4, 2)
    x1 = np.array([[1.0, 0.0], [1.0, 1.0], [2.0, 0.0], [-1.0, 0.0]])
    x2 = np.array([[7.0, 0.0], [1.0, 0.0], [7.0, 1.0], [1.0, 1.0]])          # slope 7: nobody's; slope 1: particles 0 and 1
    S.begin_step(np.zeros((1, 2))); S.end_step(x1, np.zeros(4))
    S.begin_step(np.zeros((1, 2))); S.resample_blocks(np.array([3, 4, 1, 2]), np.array([True])); S.end_step(x2, np.zeros(4))
    traj, idx = bsp.backward(o, "line_model", m.params, S, seed=5, epoch=0, n_samples=256)
    i2, i1 = idx[0, :, 1] - 1, idx[0, :, 0] - 1
    parent = np.array([2, 3, 0, 1])
    odd = x2[i2, 0] == 7.0
    assert odd.any() and (~odd).any()
    assert np.array_equal(i1[odd], parent[i2[odd]])
    assert set(i1[~odd]) == {0, 1}


# ----------------------------------------------------------------------------- the law experiment on the CPU
def law_run(g, o, N):
    m, ys, mu, Sigma = bsp.law_setup(g.models)
    L = bsp.StoreLoop(o, m, bsp.LAW_B * N, N, bsp.LAW_SEED)
    obs = lambda t: np.tile(ys[t], (bsp.LAW_B, 1))
    L.initialize(obs(0))
    for t in range(1, bsp.LAW_T):
        L.resample()
        L.update(obs(t))
    traj, _ = bsp.backward(o, "lgssm2", m.params, L.store, L.seed, L.epoch, 1)
    return bsp.law_units(traj[:, 0], mu, Sigma)


def test_law_experiment_on_the_restatement(g, o):
    """the experiment of tests/test_gpu_block_backward.py::test_backward_draws_follow_the_exact_smoother on the oracle's filter, at the block size that
    test fixes: every smoothed mean within 5 standard errors, every variance within 5 sqrt(2 / B)"""
    zm, zv = law_run(g, o, bsp.LAW_N)
    print("backward simulation, restatement, N =", bsp.LAW_N, ": mean z", np.round(zm, 2).tolist(), "variance z", np.round(zv, 2).tolist())
    assert np.all(zm <= cs.INV_SIGMAS) and np.all(zv <= cs.INV_SIGMAS), (zm, zv)
