"""Forward-only smoothing per block (gpf.h gpf_forward_enable_blocks, gpf_block_forward_moments), the parts that need no GPU: the entry points exist in
every layer (header, library, ctypes table, package, Julia glue); the NumPy restatement -- tests/block_forward_spec.py -- is what it must be where its
answer is known (T = 1: the oracle's block mean, and its block variance plus mean^2), and on the CPU oracle's filter it returns the sums over steps of
the pairwise smoother's restatement over a full store (tests/block_pairs_spec.py), an independent computation of the same quantities that walks backwards
from T -- in the plain filter, the nested filter, with a target on its fallback, with a dead candidate whose statistic is not finite, and without a
transition density; every bound is gamma(k) sum|terms| with k counted from the statements of both sides, and three wrong answers fail the same comparison.

The count.  A term enters the forward statistic at step s and is read after step T:
  entry      sum: one addition; second: a product and an addition; cross: q * x (1), at most bs additions into xb, the division by D (1), xbar * x (1), the
             addition (1): bs + 4 at most; first, first2: step 1, at most one product;
  each of the T - s later closes: q * T (1), at most bs additions into h, the division by D (1), the addition of the step's increment (1): bs + 3;
  the query  W = q / S (1), W * T (1), LEVELS additions up the tree.
  K_FWD = (bs + 4) + (T - 1)(bs + 3) + 2 + LEVELS <= T (bs + 3) + 3 + LEVELS.
The backward side (block_pairs_spec, a term of step s): r = q / D (1), t = W r (1), at most bs additions into W per walked step, T - s steps: (T - s)(bs +
2); then the moment -- second: two products + LEVELS; cross: t x (1), at most bs additions into A, x A (1), LEVELS -- and the T - 1 additions over the
steps formed here.  K_BWD = (T - 1)(bs + 2) + (bs + 2) + LEVELS + (T - 1) <= T (bs + 3) + LEVELS.
In the reals the two agree exactly: both use the same q_ij and D_j, and sum_j W_s^j q_ij / D_j = W_{s-1}^i is the backward recursion itself.
sum|terms|: sum_s sum_i W_s^i |x_s^i[a]| (sum), sum_s sum_i W_s^i |x_s^i[a] x_s^i[c]| (second), and for cross the Cauchy-Schwarz bound of
sum_ij t_ij |x_s^i[a]| |x_{s+1}^j[c]| under the pairwise weights' marginals (sum_j t_ij = W_s^i, sum_i t_ij = W_{s+1}^j):
sqrt(sum_i W_s^i x_s^i[a]^2  sum_j W_{s+1}^j x_{s+1}^j[c]^2), summed over the pairs."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import across_blocks_spec as xs
import block_backward_spec as bsp
import block_forward_spec as fsp
import block_pairs_spec as psp
import block_smooth_spec as ssp
from test_block_backward_host import small_loop
from test_block_smooth_host import gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = ["gpf_handle", "int64_t", "double*", "double*", "double*", "double*", "double*", "double*", "int32_t*"]
LEVELS = 11                                                                   # additions on a term's way up the tree of DESIGN.md 3.5 (2048 leaves)


def k_fwd(T, bs):
    return T * (bs + 3) + 3 + LEVELS


def k_bwd(T, bs):
    return T * (bs + 3) + LEVELS


def header():
    return open(os.path.join(ROOT, "include", "gpf.h")).read()


# ----------------------------------------------------------------------------- every layer
def test_header_declares_the_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"gpf_status\s+gpf_block_forward_moments\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "gpf_block_forward_moments is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", a.strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == PROTO
    assert re.search(r"gpf_status\s+gpf_forward_enable_blocks\s*\(\s*gpf_handle\s+h\s*\)\s*;", hdr)


def test_header_states_the_definition():
    txt = header()
    end = txt.index("gpf_status gpf_forward_enable_blocks(gpf_handle")
    doc = re.sub(r"\s*\n \*\s*", " ", txt[txt.rindex("/*", 0, end):end])     # (one line: a phrase may be broken across two of the comment's)
    for piece in ("Everything not named here is gpf_block_smooth's", "CLOSES the step that ends", "A refused block-wise call closes nothing", "cross = +0.0",
                  "pm_j = g_s[j]", "c' = pm_{c bs} / bs", "every entry of every T of block c is NaN", "CURRENT WHEN THE STEP IS CLOSED", "q_ij = exp_fix(lwa_ij - m_j, K)",
                  "D_j = 1", "ASCENDING order", "SKIPPED ENTIRELY", "h_j[f] = h_j[f] + (double)q_ij * T_{s-1}^i[f]", "xb_j[a] = xb_j[a] + (double)q_ij * x_{s-1}^i[a]",
                  "from +0.0", "no fused multiply-add", "cross[a][c] = e + xbar_j[a] * x_s^j[c]", "tree_j(W^j * T^j[f])", "tree_j((W^j * x^j[a]) * x^j[c])", "mirrored",
                  "nothing is committed", "second - last2", "second - first2", "NOT part of a checkpoint", "8 (2 F + d + 1) n bytes"):
        assert piece in doc, piece
    for refusal in ("GPF_ERR_STATE", "GPF_ERR_INVALID_ARGUMENT", "all outputs NULL", "2048", "gpf_step_ess", "gpf_checkpoint_load", "communicator", "views"):
        assert refusal in doc, refusal


def test_library_exports_the_entry_points(g):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    for name in ("gpf_forward_enable_blocks", "gpf_block_forward_moments"):
        assert hasattr(L, name), name + " is not exported by the built library"
    assert L.gpf_abi_version() == 1                                                          # additive: the ABI version stays


def test_ctypes_table(g):
    C = ctypes
    pd = C.POINTER(C.c_double)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_forward_enable_blocks"][1:] == (C.c_int, [C.c_void_p])
    assert table["gpf_block_forward_moments"][1:] == (C.c_int, [C.c_void_p, C.c_int64, pd, pd, pd, pd, pd, pd, C.POINTER(C.c_int32)])


def test_package_exports(g):
    assert list(inspect.signature(g.block_forward_moments).parameters) == ["state", "block_size"]
    assert inspect.signature(g.pf_initialize_blocks).parameters["forward"].default is False
    assert g.BlockForwardMoments._fields == ("sum", "second", "cross", "first", "first2", "last2", "n_steps") == fsp.Moments._fields


def test_julia_glue_calls_the_entry_points():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:gpf_forward_enable_blocks, libgpf\), Cint, \(Ptr\{Cvoid\},\)", jl)
    assert re.search(r"ccall\(\(:gpf_block_forward_moments, libgpf\), Cint, \(Ptr\{Cvoid\}, Int64, Ptr\{Cdouble\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}, "
                     r"Ptr\{Cdouble\}, Ptr\{Cdouble\}, Ref\{Cint\}\)", jl)
    assert re.search(r"^function block_forward_moments\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)


def test_the_layout_is_the_documented_one():
    assert [fsp.F_of(d) for d in (1, 2, 4)] == [5, 14, 44]
    assert fsp.offsets(2) == (0, 2, 5, 9, 11, 14)


# ----------------------------------------------------------------------------- T = 1
@pytest.mark.parametrize("name,n,bs", [("lgssm2", 26, 7), ("bearings4", 1031, 513), ("sv1", 300, 129)])
def test_at_one_step_it_is_the_oracles_block_mean_and_variance_plus_mean_squared(g, o, name, n, bs):
    """sum and first are the oracle's block mean bit for bit; second = first2 = tree(w (x x)) and last2 = tree((w x) x) -- two products and LEVELS additions
    either way -- have the oracle's block variance plus mean^2 on their diagonal, within the bound tests/test_block_pairs_host.py derives for the latter"""
    m, L = small_loop(g, o, name, n, bs, 1)
    S = L.store
    r = fsp.forward(o, name, m.params, S)
    assert r.n_steps == 1 and np.all(r.cross == 0.0) and not np.any(np.signbit(r.cross))
    assert np.array_equal(r.first, r.sum) and np.array_equal(r.second, r.first2)
    assert np.array_equal(r.last2, psp.pairs(o, name, m.params, S)[1][:, 0])
    f = L.L.f[0]
    worst = 0.0
    for b in range(S.B):
        b0, b1 = b * bs, min((b + 1) * bs, n)
        s = o.WeightSummary(np.ascontiguousarray(f.lw[b0:b1]), b1 - b0)
        w = s.q.astype(np.float64) / np.float64(s.S)
        rows_b = np.ascontiguousarray(f.rows[b0:b1])
        for col in range(m.dim):
            x = rows_b[:, col]
            mu = o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, b1 - b0, 1, 0.0)
            var = o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, b1 - b0, 2, mu)
            assert r.sum[b, col] == mu, (b, col)
            bound = (gamma(2 + LEVELS) * np.sum(w * x * x) + gamma(4 + LEVELS) * np.sum(w * (x - mu) ** 2) + 2 * abs(mu) * gamma(1 + LEVELS) * np.sum(w * np.abs(x))
                     + mu * mu * gamma(1) + gamma(2) * (var + mu * mu))
            for moment in (r.second, r.last2):
                err = abs(moment[b, col, col] - (var + mu * mu))
                worst = max(worst, err / bound)
                assert err <= bound, (b, col, err, bound)
    print("T = 1, second's diagonal against var + mean^2: worst error / bound", worst)


# ----------------------------------------------------------------------------- the six identities against the pairwise smoother over a full store
def identities(o, name, P, S, got=None, back=None, **kw):
    """(worst error / bound per output) of the forward restatement (or `got`) against the sums over steps of block_pairs_spec.pairs on the same Store (or
    `back` = (mean, second, cross, blocks, smoothing weights) of the same walk from elsewhere: the device's, tests/test_gpu_block_forward.py)"""
    T, bs, d = S.steps, S.bs, S.d
    r = fsp.forward(o, name, P, S, **kw) if got is None else got
    mean, second, cross, blocks, W = back if back is not None else psp.pairs(o, name, P, S, **kw) + (ssp.smooth(o, name, P, S, **kw)[2],)
    assert np.all(blocks >= 1), "an undefined lineage: nothing to compare"
    B = S.B
    a_sum, a_sec, a_cross = np.zeros((B, d)), np.zeros((B, d, d)), np.zeros((B, d, d))
    a_first, a_first2 = np.zeros((B, d)), np.zeros((B, d, d))
    for b in range(B):
        s2 = []
        for s in range(1, T + 1):
            c0 = (blocks[b, s - 1] - 1) * bs
            c1 = min(c0 + bs, S.n)
            x, w = S.x(s)[c0:c1], W[b, s - 1, :c1 - c0]
            ax, axx = (w[:, None] * np.abs(x)).sum(axis=0), (w[:, None, None] * np.abs(x[:, :, None] * x[:, None, :])).sum(axis=0)
            a_sum[b] += ax; a_sec[b] += axx
            if s == 1:
                a_first[b], a_first2[b] = ax, axx
            s2.append((w[:, None] * x * x).sum(axis=0))
        for s in range(T - 1):
            a_cross[b] += np.sqrt(np.outer(s2[s], s2[s + 1]))
    gk = gamma(k_fwd(T, bs)) + gamma(k_bwd(T, bs))
    pairs_of = {"sum": (r.sum, mean.sum(axis=1), a_sum), "second": (r.second, second.sum(axis=1), a_sec), "cross": (r.cross, cross.sum(axis=1), a_cross),
                "first": (r.first, mean[:, 0], a_first), "first2": (r.first2, second[:, 0], a_first2)}
    ratios = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for what, (a, w, mass) in pairs_of.items():
            err = np.abs(a - w)
            ratios[what] = float(np.nanmax(np.where(err == 0, 0.0, err / (gk * mass)))) if np.all(np.isfinite(a)) else np.inf
    ratios["last2"] = 0.0 if np.array_equal(r.last2, second[:, T - 1]) else np.inf        # (the same statement on the same doubles: bit for bit)
    assert r.n_steps == T
    return ratios


def assert_inside(ratios, where):
    print(where, "worst error / bound:", {k: float("%.3g" % v) for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), (where, ratios)


@pytest.mark.parametrize("name,n,bs,ess", [("lgssm2", 26, 7, 0.5), ("lgssm2", 26, 7, None), ("bearings4", 300, 129, None), ("sv1", 40, 7, None), ("object_motion", 26, 7, None)])
def test_on_the_oracles_filter_it_is_the_sum_over_steps_of_the_pairwise_smoother(g, o, name, n, bs, ess):
    m, L = small_loop(g, o, name, n, bs, 4, ess_frac=ess)
    assert_inside(identities(o, name, m.params, L.store), (name, n, bs, ess))
    for t in (1, 2, 3):                                                       # the query after every step is the whole query of a shorter store
        assert fsp.forward(o, name, m.params, L.store, t).n_steps == t


def nested_loop(g, o, n, bs, T):
    """block resample, then resampling across blocks, every step, on the oracle (tests/across_blocks_spec.py), recorded into the Store"""
    from test_gpu_block_conditional import block_obs, model_of
    m = model_of(g, "lgssm2")
    ys = block_obs(g, m, n // bs, T)
    L = bsp.StoreLoop(o, m, n, bs, 17)
    L.initialize(ys[:, 0])
    fired = 0
    for t in range(1, T):
        L.resample(0.8)
        f = L.L.f[0]
        plan = xs.resample_across_blocks(o, f, bs, "multinomial", check=False)
        if plan.resampled:
            fired += 1
            L.store.resample_across(f.parents, plan.A + 1)
            L._end()
        L.update(ys[:, t])
    return m, L, fired


def test_the_nested_filter(g, o):
    m, L, fired = nested_loop(g, o, 6 * 8, 8, 4)
    assert fired > 0
    blocks = psp.pairs(o, "lgssm2", m.params, L.store)[3]
    assert np.any(blocks != blocks[:, -1:])                                   # (some lineage changed its block)
    assert_inside(identities(o, "lgssm2", m.params, L.store), "nested")


def fallback_store():
    """line_model, one block of four, three steps: at step 2 the targets 0 and 2 hold slope 7, which no candidate of step 1 leads to -- they take their
    recorded parent; target 1 has weight -Inf at step 2 (a dead candidate of the close of step 3) and target 3 shares the candidates of slope 1"""
    S = bsp.Store(4, 4, 2)
    x1 = np.array([[1.0, 0.0], [1.0, 1.0], [2.0, 0.0], [-1.0, 0.0]])
    x2 = np.array([[7.0, 0.5], [1.0, 0.25], [7.0, 1.0], [1.0, 1.5]])
    x3 = np.array([[7.0, 0.75], [1.0, 2.0], [1.0, -0.5], [7.0, 0.125]])
    S.begin_step(np.zeros((1, 2))); S.end_step(x1, np.zeros(4))
    S.begin_step(np.zeros((1, 2))); S.resample_blocks(np.array([3, 4, 1, 2]), np.array([True])); S.end_step(x2, np.array([np.log(0.2), -np.inf, np.log(0.3), np.log(0.5)]))
    S.begin_step(np.zeros((1, 2))); S.end_step(x3, np.log(np.array([0.1, 0.2, 0.3, 0.4])))
    return S


def test_a_step_with_a_target_on_its_fallback(g, o):
    m = g.models.line_model()
    S = fallback_store()
    T2 = fsp.statistics(o, "line_model", m.params, S, 2)
    o_cross = fsp.offsets(2)[2]
    # target 0 of step 2: slope 7, recorded parent 2 of step 1 -- its statistic is the parent's plus its own increment, and xbar is the parent's row
    T1 = fsp.first(S.x(1))
    want = T1[2].copy()
    want[0:2] += S.x(2)[0]; want[2:5] += fsp.triangle(S.x(2)[0]); want[o_cross:o_cross + 4] += np.outer(S.x(1)[2], S.x(2)[0]).ravel()
    assert np.array_equal(T2[0], want)
    assert_inside(identities(o, "line_model", m.params, S), "fallback")
    assert_inside(identities(o, "line_model", m.params, S, fallback=True), "every target on its fallback")


def test_a_dead_candidate_with_a_non_finite_statistic_is_skipped(g, o):
    """candidate 1 of step 2 has weight -Inf: q = 0 for every target of step 3, so whatever its statistic holds never reaches a sum (0 * inf is NaN)"""
    m = g.models.line_model()
    S = fallback_store()
    T2 = fsp.statistics(o, "line_model", m.params, S, 2)
    args = (S.x(2), S.lw[1], S.x(3), S.step_map(3), S.obs[2], S.bs)
    clean = fsp.close(o, "line_model", m.params, T2, *args)
    for poison in (np.inf, -np.inf, np.nan):
        bad = T2.copy()
        bad[1] = poison
        T3 = fsp.close(o, "line_model", m.params, bad, *args)
        assert np.all(np.isfinite(T3)) and np.array_equal(T3, clean), poison
    r = fsp.query(o, clean, S.x(3), S.lw[2], S.bs, 3)
    assert all(np.all(np.isfinite(a)) for a in r[:6])
    # ... and on the oracle's filter: a particle of step 2 made dead in the Store is a target of weight 0 backwards and a candidate with q = 0 forwards
    m, L = small_loop(g, o, "lgssm2", 26, 7, 4)
    L.store.lw[1][[1, 3, 9, 22]] = -np.inf
    assert_inside(identities(o, "lgssm2", m.params, L.store), "dead candidates")


def test_without_a_transition_density_cross_is_the_sum_of_outer_products_of_two_means(g, o):
    """logtrans = 0: q_ij / D_j = r_i, the step's own normalised weight whatever j, so xbar_j = F_s, the FILTERING mean of step s, and in exact arithmetic
    cross = sum_s F_s (x) M_{s+1} with M the smoothed mean.  sum|terms| of the pair (s, s + 1) is the product of the two absolute means exactly (the
    pairs are independent); the outer products formed here: each mean a product + LEVELS additions, their product, T - 1 additions"""
    m, L = small_loop(g, o, "lgssm2", 26, 7, 4, ess_frac=0.5)
    S = L.store
    T, bs = S.steps, S.bs
    assert_inside(identities(o, "lgssm2", m.params, S, trans=False), "no transition density")
    r = fsp.forward(o, "lgssm2", m.params, S, trans=False)
    M = psp.pairs(o, "lgssm2", m.params, S, trans=False)[0]
    W = ssp.smooth(o, "lgssm2", m.params, S, trans=False)[2]
    worst = 0.0
    for b in range(S.B):
        b0, b1 = b * bs, min((b + 1) * bs, S.n)
        want, mass = np.zeros((2, 2)), np.zeros((2, 2))
        for s in range(1, T):
            ws = o.WeightSummary(np.ascontiguousarray(S.lw[s - 1][b0:b1]), b1 - b0)
            rr = ws.q.astype(np.float64) / np.float64(ws.S)
            xs_, xn, Wn = S.x(s)[b0:b1], S.x(s + 1)[b0:b1], W[b, s, :b1 - b0]
            want += np.outer([ssp.tree_sum(rr * xs_[:, a]) for a in range(2)], M[b, s])
            mass += np.outer((rr[:, None] * np.abs(xs_)).sum(axis=0), (Wn[:, None] * np.abs(xn)).sum(axis=0))
        bound = (gamma(k_fwd(T, bs)) + gamma(2 * (1 + LEVELS) + 1 + (T - 1) + k_bwd(T, bs))) * mass
        err = np.abs(r.cross[b] - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (b, err, bound)
    print("no transition density, cross against sum_s F_s (x) M_{s+1}: worst error / bound", worst)
    assert not np.array_equal(r.cross, fsp.forward(o, "lgssm2", m.params, S).cross)          # (the density matters)


# ----------------------------------------------------------------------------- three wrong answers
def test_three_wrong_answers_fail_the_same_comparison(g, o):
    m, L = small_loop(g, o, "lgssm2", 26, 7, 4, ess_frac=0.5)
    S = L.store
    good = fsp.forward(o, "lgssm2", m.params, S)
    assert_inside(identities(o, "lgssm2", m.params, S, got=good), "the right answer")
    transposed = good._replace(cross=good.cross.transpose(0, 2, 1))
    parent = fsp.forward(o, "lgssm2", m.params, S, parent_x=True)            # the increment taken with x_{s-1} of the recorded parent instead of xbar
    undivided = fsp.forward(o, "lgssm2", m.params, S, divide=False)          # no division by D
    for what, bad in (("cross transposed", transposed), ("the recorded parent's row for xbar", parent), ("no division by D", undivided)):
        ratios = identities(o, "lgssm2", m.params, S, got=bad)
        print(what, "worst error / bound:", {k: float("%.3g" % v) for k, v in ratios.items()})
        assert ratios["cross"] > 1.0, (what, ratios)
    assert identities(o, "lgssm2", m.params, S, got=parent)["second"] <= 1.0   # (only the cross moment reads xbar)
