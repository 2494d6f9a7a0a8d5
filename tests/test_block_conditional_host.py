"""Conditional SMC for block-wise filters (gpf.h gpf_initialize_blocks_ref, gpf_update_blocks_ref, gpf_resample_blocks_conditional), the parts that
need no GPU: the three entry points exist in every layer (header with citation and refusals, library, ctypes table, package, Julia glue); the
restatement the GPU tests compare against -- tests/block_conditional_spec.py -- reduces to the plain oracle where it must; and the invariance
experiment of tests/test_gpu_block_conditional.py run once on the CPU through that restatement: the evidence that its fixed seed, shapes and bounds
hold for a correct implementation, and that the plain filter at the same shape fails them."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import block_conditional_spec as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_PARAMS = ["gpf_handle", "constdouble*", "int32_t", "int64_t", "constdouble*", "int32_t"]
PROTOS = {
    "gpf_initialize_blocks_ref": STEP_PARAMS,
    "gpf_update_blocks_ref": STEP_PARAMS,
    "gpf_resample_blocks_conditional": ["gpf_handle", "int32_t", "int64_t", "double", "int32_t", "int32_t*", "int64_t*"],
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


def doc_before(name):
    """the comment block in front of the declaration"""
    txt = header()
    end = txt.index(name + "(gpf_handle")
    return txt[txt.rindex("/*", 0, end):end]


def test_header_documents_the_pinned_step():
    doc = doc_before("gpf_initialize_blocks_ref")
    assert "Andrieu, Doucet & Holenstein (2010)" in doc and "test/update.jl:179-189" in doc and "src/update.jl:12-25" in doc
    assert "b * block_size" in doc and "bootstrap weight" in doc and "bit-identical" in doc
    assert "finite" in doc and "GPF_ERR_INVALID_ARGUMENT" in doc and "n_ref" in doc          # the refusals
    assert "default proposal only" in doc and "strata" in doc
    assert "DISCRETE" in doc and "caller's business" in doc                                  # discrete latents are not validated
    assert "Rejuvenation" in doc and "retained value" in doc
    assert "no copy of the reference between calls" in doc


def test_header_documents_the_conditional_resample():
    doc = doc_before("gpf_resample_blocks_conditional")
    assert "Andrieu, Doucet & Holenstein (2010)" in doc and "no counterpart" in doc and "src/resample.jl:19-175" in doc
    assert "local index 0" in doc and "same counters" in doc and "logsumexp(block weights) - log(block size)" in doc
    for refusal in ("GPF_RESAMPLE_RESIDUAL", "_STRATIFIED", "not a valid conditional scheme", "priority", "2048", "epoch included"):
        assert refusal in doc, refusal


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_library_exports_the_entry_point(g, name):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, name), f"{name} is not exported by the built library"
    assert L.gpf_abi_version() == 1                                                          # additive: the ABI version stays


def test_ctypes_table(g):
    C = ctypes
    table = {s[0]: s for s in g._lib.SYMBOLS}
    pd = C.POINTER(C.c_double)
    for name in ("gpf_initialize_blocks_ref", "gpf_update_blocks_ref"):
        assert table[name][1:] == (C.c_int, [C.c_void_p, pd, C.c_int32, C.c_int64, pd, C.c_int32])
    assert table["gpf_resample_blocks_conditional"][1:] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_int32, C.POINTER(C.c_int32),
                                                                      C.POINTER(C.c_int64)])


def test_package_exports_and_argument_checks(g):
    for fn, kw in ((g.pf_initialize_blocks, "reference"), (g.pf_update_blocks, "reference")):
        p = inspect.signature(fn).parameters[kw]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(g.pf_resample_blocks).parameters["conditional"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    # the combinations that are refused before anything is touched (no state needed: the checks come first)
    ref = np.zeros((2, 2))
    with pytest.raises(ValueError, match="default proposal"):
        g.pf_update_blocks(None, (), (), np.zeros((2, 2)), 4, [None, None], reference=ref)
    with pytest.raises(ValueError, match="default proposal"):
        g.pf_update_blocks(None, (), (), np.zeros((2, 2)), 4, strata=[0.0, 1.0], reference=ref)
    with pytest.raises(ValueError, match="default proposal"):
        g.pf_initialize_blocks(g.models.object_motion(), (), np.zeros((2, 2)), 8, 4, strata=[0.0, 1.0], reference=ref)
    for method in ("residual", "stratified"):
        with pytest.raises(ValueError, match="not a valid conditional scheme"):
            g.pf_resample_blocks(None, 4, method, conditional=True)
    with pytest.raises(ValueError, match="priority_fn"):
        g.pf_resample_blocks(None, 4, "multinomial", priority_fn=g.Tempering(0.5), conditional=True)


def test_julia_glue_calls_the_entry_points():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    step = r"\(Ptr\{Cvoid\}, Ptr\{Cdouble\}, Cint, Int64, Ptr\{Cdouble\}, Cint\)"
    for name in ("gpf_initialize_blocks_ref", "gpf_update_blocks_ref"):
        assert re.search(r"ccall\(\(:%s, libgpf\), Cint, %s" % (name, step), jl), f"no ccall of {name}"
    assert re.search(r"ccall\(\(:gpf_resample_blocks_conditional, libgpf\), Cint, \(Ptr\{Cvoid\}, Cint, Int64, Cdouble, Cint, Ptr\{Cint\}, Ptr\{Int64\}\)", jl)
    assert re.search(r"^function pf_resample_blocks_conditional!\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)
    assert re.search(r"^function pf_update_blocks_ref!\(s::DeviceParticleFilterState", jl, re.M)


# ----------------------------------------------------------------------------- the restatement, on the CPU alone
N, NB, SEED = 3 * 7 + 5, 7, 31                                                              # three full blocks and a short one


def obs_rows(g, m, B, t, seed=3):
    base = np.asarray(g.models.simulate(m, t + 1))[t]
    return base[None, :] + 0.3 * np.random.default_rng(seed + t).standard_normal((B, base.size))


@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("name", ["sv1", "object_motion", "lgssm2", "bearings4"])
def test_spec_with_the_plain_slot_as_reference_is_the_plain_step(g, o, name, keep_prev):
    """reference = what the plain oracle step put into slot 0: rows and log-weights come back bit for bit (the pinned weight IS the bootstrap weight)"""
    m = g.models.bearings4(sb=0.5) if name == "bearings4" else g.models.by_name(name)
    B = (N + NB - 1) // NB
    b0 = cs.slot0(N, NB)
    plain = o.OracleFilter(m.model_id, m.params, N, SEED, keep_prev=keep_prev)
    pinned = o.OracleFilter(m.model_id, m.params, N, SEED, keep_prev=keep_prev)
    o.initialize_blocks(plain, NB, obs_rows(g, m, B, 0))
    cs.pinned_initialize(o, pinned, NB, obs_rows(g, m, B, 0), plain.rows[b0, :m.dim])
    assert np.array_equal(plain.rows, pinned.rows) and np.array_equal(plain.lw, pinned.lw)
    for t in (1, 2):
        o.update_blocks(plain, NB, obs_rows(g, m, B, t))
        cs.pinned_update(o, pinned, NB, obs_rows(g, m, B, t), plain.rows[b0, :m.dim])
        assert np.array_equal(plain.rows, pinned.rows) and np.array_equal(plain.lw, pinned.lw), t
        assert plain.epoch == pinned.epoch
    # another reference: slot 0 differs (row and weight), nobody else does
    ref = plain.rows[b0, :m.dim] + 0.25
    o.update_blocks(plain, NB, obs_rows(g, m, B, 3))
    lw_in = pinned.lw[b0].copy()
    cs.pinned_update(o, pinned, NB, obs_rows(g, m, B, 3), ref)
    others = np.ones(N, bool); others[b0] = False
    assert np.array_equal(plain.rows[others], pinned.rows[others]) and np.array_equal(plain.lw[others], pinned.lw[others])
    assert np.array_equal(pinned.rows[b0, :m.dim], ref) and not np.array_equal(plain.lw[b0], pinned.lw[b0])
    assert np.array_equal(pinned.lw[b0], lw_in + cs.loglik_rows(o, pinned, pinned.rows[b0], obs_rows(g, m, B, 3)))


def test_spec_conditional_resample_differs_in_slot_0_of_resampled_blocks_only(g, o):
    m = g.models.lgssm2()
    B = (N + NB - 1) // NB
    b0 = cs.slot0(N, NB)
    plain = o.OracleFilter(m.model_id, m.params, N, SEED)
    o.initialize_blocks(plain, NB, obs_rows(g, m, B, 0))
    plain.lw[NB:2 * NB] = 0.0                                                                # block 1: even weights, its ESS test fails
    cond = o.OracleFilter(m.model_id, m.params, N, SEED)
    cond.rows, cond.lw, cond.epoch = plain.rows.copy(), plain.lw.copy(), plain.epoch
    before = plain.rows.copy()
    mask = np.asarray(o.resample_blocks(plain, NB, "multinomial", ess_frac=0.9, check=False), bool)
    mask_c = cs.conditional_resample(o, cond, NB, ess_frac=0.9)
    assert np.array_equal(mask, mask_c) and mask.any() and not mask[1]
    others = np.ones(N, bool); others[b0[mask]] = False
    assert np.array_equal(plain.rows[others], cond.rows[others]) and np.array_equal(plain.parents[others], cond.parents[others])
    assert np.array_equal(plain.lw, cond.lw) and plain.epoch == cond.epoch
    assert np.array_equal(cond.rows[b0[mask]], before[b0[mask]]) and np.all(cond.parents[b0[mask]] == 1)
    assert np.any(plain.parents[b0[mask]] != 1)                                              # (the plain call did move some slot 0)


# ----------------------------------------------------------------------------- invariance against the exact smoother, once on the CPU
def spec_steps(g, o, conditional):
    m = g.models.lgssm2()
    L = cs.ConditionalLoop(o, m, cs.INV_B * cs.INV_N, cs.INV_N, cs.INV_SEED, False)
    return (lambda ob, r: L.initialize(ob, r), lambda: L.resample(None, conditional=conditional), lambda ob, r: L.update(ob, r),
            lambda: L.sample_trajectories(1))


def test_smoother_is_the_kalman_smoother(g):
    """the joint-precision smoother against the forward filter's last marginal (models.kalman_loglik's recursion restated)"""
    m, ys, _, mu, Sigma = cs.invariance_setup(g.models)
    A, sq, sr, s0 = m.info["A"], m.info["sq"], m.info["sr"], m.info["s0"]
    mean, P = np.zeros(2), s0 ** 2 * np.eye(2)
    for t in range(len(ys)):
        if t > 0:
            mean, P = A @ mean, A @ P @ A.T + sq ** 2 * np.eye(2)
        K = P @ np.linalg.inv(P + sr ** 2 * np.eye(2))
        mean, P = mean + K @ (ys[t] - mean), (np.eye(2) - K) @ P
    np.testing.assert_allclose(mu[-1], mean, rtol=1e-10)
    np.testing.assert_allclose(Sigma[-2:, -2:], P, rtol=1e-10, atol=1e-14)


def test_invariance_against_the_exact_smoother_on_the_spec(g, o):
    """B = 4096 blocks of N = 8, T = 4: the conditional loop's drawn paths are exact smoother draws -- every mean within 5 standard errors, every
    variance within 5 sqrt(2 / B) relative (CPU run: worst 1.13 and 1.41 of those units) -- and the plain filter at the same shape fails the
    variance bound at t = 1 (CPU run: 219 units; path degeneracy at N = 8)"""
    zm, zv = cs.invariance_run(spec_steps(g, o, True), g.models, True)
    print("conditional: mean z", np.round(zm, 2).tolist(), "variance z", np.round(zv, 2).tolist())
    assert np.all(zm <= cs.INV_SIGMAS) and np.all(zv <= cs.INV_SIGMAS), (zm, zv)
    zm_p, zv_p = cs.invariance_run(spec_steps(g, o, False), g.models, False)
    print("plain: mean z", np.round(zm_p, 2).tolist(), "variance z", np.round(zv_p, 2).tolist())
    assert np.all(zv_p[0] > cs.INV_SIGMAS), zv_p
