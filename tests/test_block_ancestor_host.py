"""Ancestor sampling for conditional SMC per block (gpf.h gpf_resample_blocks_ancestor, gpf_block_ancestor_log_weights), the parts that need no GPU:
the two entry points exist in every layer (header with citation, definition and refusals; library; ctypes table; package; Julia glue); the NumPy
restatement of Model<M>::logtrans -- tests/block_ancestor_spec.py -- against the mpmath transition densities of tests/hp_reference.py (Ref.logtrans); the spec
reduces to the plain one where it must; and the invariance experiment of tests/test_gpu_block_ancestor.py run on the CPU through the spec, with the
negative control that shows the experiment can see a wrong ancestor density."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import block_ancestor_spec as asp
import block_conditional_spec as cs
import hp_reference as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "gpf_resample_blocks_ancestor": ["gpf_handle", "int32_t", "int64_t", "double", "int32_t", "constdouble*", "int32_t", "constdouble*", "int32_t",
                                     "int32_t*", "int64_t*"],
    "gpf_block_ancestor_log_weights": ["gpf_handle", "int64_t", "constdouble*", "int32_t", "constdouble*", "int32_t", "double*"],
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


def test_header_documents_the_ancestor_step():
    txt = header()
    end = txt.index("gpf_resample_blocks_ancestor(gpf_handle")
    doc = txt[txt.rindex("/*", 0, end):end]
    assert "Lindsten, Jordan & Schoen (2014)" in doc and "Particle Gibbs with ancestor sampling" in doc and "JMLR 15" in doc
    assert "proportional to  w_{t-1}^i f(x'_t | x_{t-1}^i)" in doc and "logtrans" in doc
    assert "OWN" in doc and "counter" in doc and "a_0 = 0" in doc                            # the counter used and the fallback
    assert "scratch of their own" in doc and "gpf_rejuvenate_blocks" in doc and "no copy and no mode" in doc
    for refusal in ("gpf_resample_blocks_conditional refuses", "NULL", "non-finite", "GPF_ERR_INVALID_ARGUMENT", "per-block parameters", "epoch included"):
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
    assert table["gpf_resample_blocks_ancestor"][1:] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_int32, pd, C.c_int32, pd, C.c_int32,
                                                                   C.POINTER(C.c_int32), C.POINTER(C.c_int64)])
    assert table["gpf_block_ancestor_log_weights"][1:] == (C.c_int, [C.c_void_p, C.c_int64, pd, C.c_int32, pd, C.c_int32, pd])


def test_package_exports_and_argument_checks(g):
    for kw in ("reference", "observations"):
        p = inspect.signature(g.pf_resample_blocks).parameters[kw]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(g.block_ancestor_log_weights)
    assert list(inspect.signature(g.block_ancestor_log_weights).parameters) == ["state", "block_size", "observations", "reference"]
    # refused before anything is called (no state needed)
    ref, obs = np.zeros((2, 2)), np.zeros((2, 2))
    with pytest.raises(ValueError, match="conditional=True"):
        g.pf_resample_blocks(None, 4, "multinomial", reference=ref, observations=obs)
    with pytest.raises(ValueError, match="observations="):
        g.pf_resample_blocks(None, 4, "multinomial", conditional=True, reference=ref)
    for method in ("residual", "stratified"):
        with pytest.raises(ValueError, match="not a valid conditional scheme"):
            g.pf_resample_blocks(None, 4, method, conditional=True, reference=ref, observations=obs)


def test_julia_glue_calls_the_entry_points():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:gpf_resample_blocks_ancestor, libgpf\), Cint,\s*\(Ptr\{Cvoid\}, Cint, Int64, Cdouble, Cint, Ptr\{Cdouble\}, Cint, "
                     r"Ptr\{Cdouble\}, Cint, Ptr\{Cint\}, Ptr\{Int64\}\)", jl)
    assert re.search(r"ccall\(\(:gpf_block_ancestor_log_weights, libgpf\), Cint, \(Ptr\{Cvoid\}, Int64, Ptr\{Cdouble\}, Cint, Ptr\{Cdouble\}, Cint, Ptr\{Cdouble\}\)", jl)
    assert re.search(r"^function pf_resample_blocks_ancestor!\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)
    assert re.search(r"^function block_ancestor_log_weights\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)


# ----------------------------------------------------------------------------- logtrans against the models' transition densities in mpmath
def _cases(m, rng, k=12):
    d = m.dim
    xs = rng.standard_normal((k, 3, d))                                                      # (xp_a, xp_b, x)
    if m.name == "object_motion":
        xs[..., 0] = rng.integers(0, 2, (k, 3))
    return xs


@pytest.mark.parametrize("name", ["lgssm2", "sv1", "bearings4", "object_motion"])
def test_logtrans_against_the_mpmath_transition_density(g, name):
    """the difference logtrans(xp_a) - logtrans(xp_b) at a fixed x -- normalising constants drop -- within the bound that first-order error propagation
    through the expression derives (tests/hp_reference.py), per value"""
    m = g.models.by_name(name)
    ref = hp.Ref(m)
    rng = np.random.default_rng(11)
    obs = np.array([0.3, 0.7, 0.0, 0.0])
    for xa, xb, x in _cases(m, rng):
        got = asp.logtrans(name, m.params, xa, x, obs)[0] - asp.logtrans(name, m.params, xb, x, obs)[0]
        want = ref.logtrans(xa, x, obs) - ref.logtrans(xb, x, obs)
        err, bound = hp.differs(got, want)
        assert np.isfinite(bound) and bound < 1e-9 * max(1.0, abs(float(want.v))), (name, bound)    # (the bound itself says something)
        assert err <= bound, (name, xa, xb, x, err, bound)


def test_logtrans_of_the_line_model_is_the_persistence_of_the_slope(g):
    m = g.models.by_name("line_model")
    xp = np.array([[1.0, 0.0], [1.0, 1.0], [-2.0, 0.0], [0.0, 1.0]])
    for out in (0.0, 1.0):                                                                   # (the outlier's probability does not depend on xp)
        assert np.array_equal(asp.logtrans("line_model", m.params, xp, np.array([1.0, out]), np.zeros(2)), [0.0, 0.0, -np.inf, -np.inf])


# ----------------------------------------------------------------------------- the restatement, on the CPU alone
N, NB, SEED = 3 * 7 + 5, 7, 31                                                              # three full blocks and a short one


def obs_rows(g, m, B, t, seed=3):
    base = np.asarray(g.models.simulate(m, t + 1))[t]
    return base[None, :] + 0.3 * np.random.default_rng(seed + t).standard_normal((B, base.size))


@pytest.mark.parametrize("name", ["sv1", "object_motion", "lgssm2", "bearings4"])
def test_spec_differs_from_the_conditional_spec_in_slot_0_only(g, o, name):
    """the ancestor loop and the conditional loop on the same incoming state: every particle but slot 0 of the resampled blocks, every weight and the
    epoch are the conditional spec's; slot 0's row is a pre-call row of its block and its parent says which; some a0 is not 0"""
    m = g.models.bearings4(sb=0.5) if name == "bearings4" else g.models.by_name(name)
    B = (N + NB - 1) // NB
    b0 = cs.slot0(N, NB)
    moved = 0
    for seed in range(SEED, SEED + 6):
        fa, fc, fp = (o.OracleFilter(m.model_id, m.params, N, seed, keep_prev=True) for _ in range(3))
        for f in (fa, fc, fp):
            o.initialize_blocks(f, NB, obs_rows(g, m, B, 0))
            o.update_blocks(f, NB, obs_rows(g, m, B, 1))
        before = fa.rows.copy()
        # the reference: what the plain filter makes of slot 0 in the step being entered
        o.resample_blocks(fp, NB, "multinomial", check=False)
        o.update_blocks(fp, NB, obs_rows(g, m, B, 2))
        ref = fp.rows[b0, :m.dim].copy()
        mask, a0 = asp.ancestor_resample(o, fa, NB, obs_rows(g, m, B, 2), ref)
        mask_c = cs.conditional_resample(o, fc, NB)
        assert np.array_equal(mask, mask_c) and mask.all()
        others = np.ones(N, bool); others[b0] = False
        assert np.array_equal(fa.rows[others], fc.rows[others]) and np.array_equal(fa.parents[others], fc.parents[others])
        assert np.array_equal(fa.lw, fc.lw) and fa.epoch == fc.epoch
        assert np.array_equal(fa.rows[b0], before[b0 + a0]) and np.array_equal(fa.parents[b0], a0 + 1)
        moved += int((a0 != 0).sum())
    assert moved > 0


def test_spec_falls_back_to_the_conditional_step(g, o):
    """line_model with a reference slope no particle holds: all ancestor weights are -Inf, a0 = 0; a block of one particle: a0 = 0"""
    m = g.models.by_name("line_model")
    B = (N + NB - 1) // NB
    f = o.OracleFilter(m.model_id, m.params, N, SEED)
    o.initialize_blocks(f, NB, np.tile([0.5, 1.0], (B, 1)))
    ref = np.tile([7.0, 0.0], (B, 1))
    mask, a0 = asp.ancestor_resample(o, f, NB, np.tile([1.0, 2.0], (B, 1)), ref)
    assert mask.all() and np.all(a0 == 0) and np.all(f.parents[cs.slot0(N, NB)] == 1)
    f1 = o.OracleFilter(m.model_id, m.params, 5, SEED)
    o.initialize_blocks(f1, 1, np.tile([0.5, 1.0], (5, 1)))
    mask, a0 = asp.ancestor_resample(o, f1, 1, np.tile([1.0, 2.0], (5, 1)), f1.rows[:, :2].copy())
    assert mask.all() and np.all(a0 == 0)


# ----------------------------------------------------------------------------- invariance against the exact smoother at T = 8, on the CPU
def spec_steps(g, o, density):
    m = g.models.lgssm2()
    L = asp.AncestorLoop(o, m, cs.INV_B * cs.INV_N, cs.INV_N, cs.INV_SEED, False)

    def resample(ob, r):
        assert L.resample(ob, r, None, density=density).all()

    return (lambda ob, r: L.initialize(ob, r), resample, lambda ob, r: L.update(ob, r), lambda: L.sample_trajectories(1))


def test_invariance_against_the_exact_smoother_on_the_spec(g, o):
    """lgssm2 defaults, B = 4096 blocks of N = 8, T = 8, references from the exact smoother: after pinned initialise, (ancestor resample, pinned update)
    x 7 and one trajectory draw per block, every mean is within 5 standard errors and every variance within 5 sqrt(2 / B) relative of the smoother's
    (CPU run of this test: worst mean z 1.36, worst variance z 2.31; 4.2 % of the blocks renewed x_1)"""
    zm, zv, renewed = asp.invariance_run(spec_steps(g, o, True), g.models)
    print("ancestor sampling: mean z", np.round(zm, 2).tolist(), "variance z", np.round(zv, 2).tolist(), "x_1 renewed", renewed)
    assert np.all(zm <= cs.INV_SIGMAS) and np.all(zv <= cs.INV_SIGMAS), (zm, zv)


def test_invariance_experiment_sees_a_wrong_ancestor_density(g, o):
    """the negative control: the same sweep with logtrans = 0 -- slot 0's ancestor in proportion to w alone, not a valid kernel -- must exceed the bound
    (CPU run of this test: worst mean z 10.42, worst variance z 9.46)"""
    zm, zv, renewed = asp.invariance_run(spec_steps(g, o, False), g.models)
    print("control: mean z", np.round(zm, 2).tolist(), "variance z", np.round(zv, 2).tolist(), "x_1 renewed", renewed)
    assert max(zm.max(), zv.max()) > cs.INV_SIGMAS, (zm, zv)
