"""Pairwise smoothing per block (gpf.h gpf_block_smooth_pairs), the parts that need no GPU: the entry point exists in every layer (header, library,
ctypes table, package, Julia glue); the NumPy restatement -- tests/block_pairs_spec.py -- reduces to what it must where its answer is known (its mean
is the marginal smoother's; T = 1: the oracle's block variance plus mean^2; no transition density: the outer product of two means; every target on its
fallback: the genealogy's pairs; sum_i A_i: the next step's smoothed mean), every bound derived as gamma(k) sum|terms| with k counted from the
statements; and the law experiment of tests/test_gpu_block_pairs.py passes on the CPU oracle's filter while three wrong answers do not."""
import ctypes
import inspect
import os
import re
import time

import numpy as np
import pytest

import block_backward_spec as bsp
import block_pairs_spec as psp
import block_smooth_spec as ssp
from test_block_backward_host import small_loop
from test_block_smooth_host import gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = ["gpf_handle", "int64_t", "int32_t", "int32_t", "double*", "double*", "double*", "int64_t*"]
LEVELS = 11                                                                   # additions on a term's way up the tree of DESIGN.md 3.5 (2048 leaves)


def header():
    return open(os.path.join(ROOT, "include", "gpf.h")).read()


# ----------------------------------------------------------------------------- every layer
def test_header_declares_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"gpf_status\s+gpf_block_smooth_pairs\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "gpf_block_smooth_pairs is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", a.strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == PROTO


def test_header_states_the_definition():
    txt = header()
    end = txt.index("gpf_status gpf_block_smooth_pairs(gpf_handle")
    doc = re.sub(r"\s*\n \*\s*", " ", txt[txt.rindex("/*", 0, end):end])     # (one line: a phrase may be broken across two of the comment's)
    for piece in ("gpf_block_smooth's, word for word", "ASCENDING order", "SKIPPED ENTIRELY", "t = W_{s+1}^j * r_ij", "W_s^i = W_s^i + t",
                  "A_i[c] = A_i[c] + t * x_{s+1}^j[c]", "from +0.0", "no fused multiply-add", "gpf_block_smooth's mean_out bit for bit",
                  "tree_i((W_s^i * x_s^i[a]) * x_s^i[c])", "mirrored", "tree_i(x_s^i[a] * A_i[c])", "[n_blocks][n_steps - 1][d][d]", "the pair (s, s+1), s = step_lo + o",
                  "every pair whose lower step is <= s", "the epoch does not advance", "not allocated on the device"):
        assert piece in doc, piece
    for refusal in ("GPF_ERR_STATE", "GPF_ERR_INVALID_ARGUMENT", "all outputs NULL", "step_lo == step_hi", "n_blocks * n_steps * d * d >= 2^31", "2048"):
        assert refusal in doc, refusal


def test_library_exports_the_entry_point(g):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, "gpf_block_smooth_pairs"), "gpf_block_smooth_pairs is not exported by the built library"
    assert L.gpf_abi_version() == 1                                                          # additive: the ABI version stays


def test_ctypes_table(g):
    C = ctypes
    pd = C.POINTER(C.c_double)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_block_smooth_pairs"][1:] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, pd, pd, pd, C.POINTER(C.c_int64)])


def test_package_exports_and_argument_checks(g):
    assert list(inspect.signature(g.block_smoothed_pair_moments).parameters) == ["state", "block_size", "steps", "return_blocks"]

    class NoStore:
        history_blocks = True
    with pytest.raises(g.ErrorException, match="history_weights=True"):                      # the message names the keyword
        g.block_smoothed_pair_moments(NoStore(), 4)


def test_julia_glue_calls_the_entry_point():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:gpf_block_smooth_pairs, libgpf\), Cint, \(Ptr\{Cvoid\}, Int64, Cint, Cint, Ptr\{Cdouble\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}, Ptr\{Int64\}\)", jl)
    assert re.search(r"^function block_smoothed_pair_moments\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)


# ----------------------------------------------------------------------------- the restatement where its answer is known
def blocks_of(S):
    for b in range(S.B):
        yield b, b * S.bs, min((b + 1) * S.bs, S.n)


@pytest.mark.parametrize("name,n,bs,ess", [("lgssm2", 26, 7, None), ("lgssm2", 26, 7, 0.5), ("bearings4", 300, 129, None), ("sv1", 40, 7, None)])
def test_its_mean_and_blocks_are_the_marginal_smoothers(g, o, name, n, bs, ess):
    m, L = small_loop(g, o, name, n, bs, 4, ess_frac=ess)
    full = psp.pairs(o, name, m.params, L.store)
    for lo, hi in ((1, 4), (2, 3), (4, 4)):
        mean, second, cross, blocks = psp.pairs(o, name, m.params, L.store, lo, hi)
        for k, part in enumerate((mean, second, cross, blocks)):               # a sub-range is that part of the whole walk (one pair fewer than steps)
            assert np.array_equal(part, full[k][:, lo - 1:hi - (k == 2)])
        want = ssp.smooth(o, name, m.params, L.store, lo, hi)
        assert np.array_equal(mean, want[0]) and np.array_equal(blocks, want[3])
        assert second.shape == (L.store.B, hi - lo + 1, m.dim, m.dim) and cross.shape == (L.store.B, hi - lo, m.dim, m.dim)
        assert np.array_equal(second, second.transpose(0, 1, 3, 2)) and np.all(np.isfinite(second)) and np.all(np.isfinite(cross))
    for kw in (dict(trans=False), dict(fallback=True)):
        assert np.array_equal(psp.pairs(o, name, m.params, L.store, **kw)[0], ssp.smooth(o, name, m.params, L.store, **kw)[0])


@pytest.mark.parametrize("name,n,bs", [("lgssm2", 26, 7), ("bearings4", 1031, 513), ("sv1", 300, 129)])
def test_at_one_step_the_diagonal_is_the_oracles_block_variance_plus_mean_squared(g, o, name, n, bs):
    """T = 1.  With w, x exact, m = sum w x, v = sum w (x - mu)^2 for the oracle's ROUNDED mean mu:  sum w x^2 = v + mu^2 + 2 mu (m - mu) + mu^2 (sum w - 1).
    Roundings: second = tree((w x) x): 2 products + LEVELS additions; the oracle's var = tree(w (x - mu)^2): a difference, a square of it (2 + 1), a
    product, LEVELS additions; its mean: 1 product + LEVELS additions, so |m - mu| <= gamma(1 + LEVELS) sum |w x|; w = q / S, one rounding each of
    quotients that sum to 1: |sum w - 1| <= gamma(1); var + mu * mu formed here: 2 roundings"""
    m, L = small_loop(g, o, name, n, bs, 1)
    S = L.store
    second = psp.pairs(o, name, m.params, S)[1]
    f = L.L.f[0]
    worst = 0.0
    for b, b0, b1 in blocks_of(S):
        s = o.WeightSummary(np.ascontiguousarray(f.lw[b0:b1]), b1 - b0)
        w = s.q.astype(np.float64) / np.float64(s.S)
        rows_b = np.ascontiguousarray(f.rows[b0:b1])
        for col in range(m.dim):
            x = rows_b[:, col]
            mu = o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, b1 - b0, 1, 0.0)
            var = o.lib().o_wsum(s.q, s.S, rows_b, f.W, col, b1 - b0, 2, mu)
            bound = (gamma(2 + LEVELS) * np.sum(w * x * x) + gamma(4 + LEVELS) * np.sum(w * (x - mu) ** 2) + 2 * abs(mu) * gamma(1 + LEVELS) * np.sum(w * np.abs(x))
                     + mu * mu * gamma(1) + gamma(2) * (var + mu * mu))
            err = abs(second[b, 0, col, col] - (var + mu * mu))
            worst = max(worst, err / bound)
            assert err <= bound, (b, col, err, bound)
    print("T = 1, second's diagonal against var + mean^2: worst error / bound", worst)


def loop_and_weights(g, o, **kw):
    n, bs, T = 3 * 7 + 5, 7, 4
    m, L = small_loop(g, o, "lgssm2", n, bs, T, ess_frac=0.5)                 # (the ESS gate leaves unequal stored weights in some blocks)
    S = L.store
    out = psp.pairs(o, "lgssm2", m.params, S, return_A=True, **kw)
    W = ssp.smooth(o, "lgssm2", m.params, S, **kw)[2]                          # the smoothing weights of the same walk
    return m, S, T, out, W


def test_without_a_transition_density_cross_is_the_outer_product_of_two_means(g, o):
    """logtrans = 0: r_ij = r_i = the step's own normalised weight whatever j, so in exact arithmetic cross_s[a][c] = (sum_i r_i x_s^i[a]) (sum_j W_j x_{s+1}^j[c])
    = F[a] M[c], the filtering mean of step s times the smoothed mean of step s + 1.  Both sides are sums over (i, j) of x_i[a] r_i W_j x_j[c] with r, W
    and x the same doubles.  Roundings per term: cross -- t = W r (1), t x (1), at most cnt_t additions into A, x A (1), LEVELS additions; F M -- each mean 1
    product + LEVELS additions, one product of the two"""
    m, S, T, (mean, second, cross, blocks, As), W = loop_and_weights(g, o, trans=False)
    worst = 0.0
    for b, b0, b1 in blocks_of(S):
        cnt = b1 - b0
        for s in range(1, T):
            ws = o.WeightSummary(np.ascontiguousarray(S.lw[s - 1][b0:b1]), cnt)
            r = ws.q.astype(np.float64) / np.float64(ws.S)
            xs, xn, Wn = S.x(s)[b0:b1], S.x(s + 1)[b0:b1], W[b, s, :cnt]
            F = np.array([ssp.tree_sum(r * xs[:, a]) for a in range(2)])
            M = mean[b, s]
            k = (3 + cnt + LEVELS, 2 * (1 + LEVELS) + 1)
            bound = (gamma(k[0]) + gamma(k[1])) * np.outer((r[:, None] * np.abs(xs)).sum(axis=0), (Wn[:, None] * np.abs(xn)).sum(axis=0))
            err = np.abs(cross[b, s - 1] - np.outer(F, M))
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (b, s, err, bound)
    print("no transition density, cross against the outer product of the means: worst error / bound", worst)


def test_with_every_target_on_its_fallback_cross_is_the_genealogys(g, o):
    """r_ij = [i is j's recorded parent]: cross_s[a][c] = sum_j W_j x_s^{parent(j)}[a] x_{s+1}^j[c] in exact arithmetic.  Roundings per term: cross -- t = W 1 (exact,
    counted 1), t x (1), at most cnt_t additions into A, x A (1), LEVELS additions; the sum formed here -- 2 products and cnt_t - 1 additions"""
    m, S, T, (mean, second, cross, blocks, As), W = loop_and_weights(g, o, fallback=True)
    worst = 0.0
    for b, b0, b1 in blocks_of(S):
        cnt = b1 - b0
        for s in range(1, T):
            pm = S.step_map(s + 1)[b0:b1]
            assert np.all(pm // S.bs == b)
            xp, xn, Wn = S.x(s)[pm], S.x(s + 1)[b0:b1], W[b, s, :cnt]
            want = ((Wn[:, None] * xp)[:, :, None] * xn[:, None, :]).sum(axis=0)
            bound = (gamma(3 + cnt + LEVELS) + gamma(1 + cnt)) * ((Wn[:, None] * np.abs(xp))[:, :, None] * np.abs(xn)[:, None, :]).sum(axis=0)
            err = np.abs(cross[b, s - 1] - want)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (b, s, err, bound)
    print("every target on its fallback, cross against the genealogy's pairs: worst error / bound", worst)
    assert not np.array_equal(cross, psp.pairs(o, "lgssm2", m.params, S)[2])                 # (the density matters)


def test_the_pair_sums_of_a_step_add_up_to_the_next_steps_smoothed_mean(g, o):
    """sum_i A_i[c] = sum_j W_j x_j[c] sum_i r_ij, and sum_i q_ij / D_j = 1 exactly.  Roundings per term (i, j): r = q / D (1), t = W r (1), t x (1), at most
    cnt_t additions into A, cnt_c - 1 additions over i here; the smoothed mean: 1 product + LEVELS additions.  sum |terms| = sum_j W_j |x_j[c]|"""
    m, S, T, (mean, second, cross, blocks, As), W = loop_and_weights(g, o)
    worst = 0.0
    for b, b0, b1 in blocks_of(S):
        cnt = b1 - b0
        for s in range(1, T):
            xn, Wn = S.x(s + 1)[b0:b1], W[b, s, :cnt]
            bound = (gamma(3 + cnt + cnt - 1) + gamma(1 + LEVELS)) * (Wn[:, None] * np.abs(xn)).sum(axis=0)
            err = np.abs(As[(b, s)].sum(axis=0) - mean[b, s])
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (b, s, err, bound)
    print("sum_i A_i against the next step's smoothed mean: worst error / bound", worst)


def test_a_target_of_weight_zero_is_skipped_entirely(g, o):
    """the hand-built store of tests/test_block_smooth_host.py with a target of weight 0 whose row holds an infinity: nothing of it reaches A, and the
    pair sums are those of the three live targets (line_model: slope 7 goes to the recorded parent, slope 1 is shared by the candidates of slope 1)"""
    m = g.models.line_model()
    S = bsp.Store(4, 4, 2)
    x1 = np.array([[1.0, 0.0], [1.0, 1.0], [2.0, 0.0], [-1.0, 0.0]])
    x2 = np.array([[7.0, 0.5], [1.0, np.inf], [7.0, 1.0], [1.0, 1.5]])
    S.begin_step(np.zeros((1, 2))); S.end_step(x1, np.zeros(4))
    S.begin_step(np.zeros((1, 2))); S.resample_blocks(np.array([3, 4, 1, 2]), np.array([True])); S.end_step(x2, np.array([np.log(0.2), -np.inf, np.log(0.3), np.log(0.5)]))
    mean, second, cross, blocks, As = psp.pairs(o, "line_model", m.params, S, return_A=True)
    w2 = ssp.smooth(o, "line_model", m.params, S)[2][0, 1]
    assert w2[1] == 0.0 and np.all(np.isfinite(cross)) and np.isnan(second[0, 1, 1, 1]) and np.isnan(mean[0, 1, 1])     # (0 * inf at step 2 itself, as the marginal smoother)
    A = np.zeros((4, 2))
    A[2] = A[2] + w2[0] * x2[0]                                               # target 0: slope 7, recorded parent 2
    A[0] = A[0] + w2[2] * x2[2]                                               # target 2: slope 7, recorded parent 0
    A[0] = A[0] + (w2[3] * 0.5) * x2[3]; A[1] = A[1] + (w2[3] * 0.5) * x2[3]  # target 3: slope 1, candidates 0 and 1
    assert np.array_equal(As[(0, 1)], A)


# ----------------------------------------------------------------------------- the law experiment on the CPU, and three wrong answers
def law_run(g, o, N):
    """(second [B, T, 2, 2], cross [B, T - 1, 2, 2], mean [B, T, 2]) of the restatement on the oracle's filter, the exact (second, cross)"""
    m, ys, mu, Sigma = bsp.law_setup(g.models)
    L = bsp.StoreLoop(o, m, psp.LAW_B * N, N, psp.LAW_SEED)
    obs = lambda t: np.tile(ys[t], (psp.LAW_B, 1))
    L.initialize(obs(0))
    for t in range(1, psp.LAW_T):
        L.resample()
        L.update(obs(t))
    mean, second, cross, _ = psp.pairs(o, "lgssm2", m.params, L.store)
    return second, cross, mean, psp.law_exact(mu, Sigma)


def test_law_experiment_on_the_restatement_and_three_rejected_controls(g, o):
    """the experiment of tests/test_gpu_block_pairs.py::test_pair_moments_follow_the_exact_smoother on the oracle's filter, at the block size that test
    fixes: the across-block average of every entry of cross_s and second_s within 5 across-block standard errors of the exact one -- and each of three
    wrong answers outside, on the same run (lgssm2's default rotation theta = 0.1 exposes the transposition)"""
    t0 = time.time()
    second, cross, mean, (exact_second, exact_cross) = law_run(g, o, psp.LAW_N)
    zs, zc = psp.law_units(second, exact_second), psp.law_units(cross, exact_cross)
    worst = max(float(zs.max()), float(zc.max()))
    bad = psp.law_controls(cross, mean, exact_cross)
    print("pairwise smoothing, restatement, N =", psp.LAW_N, ": second worst", round(float(zs.max()), 2), "cross worst", round(float(zc.max()), 2),
          "controls", {k: round(v, 2) for k, v in bad.items()}, "in", round(time.time() - t0, 1), "s")
    assert worst <= psp.LAW_SIGMAS, (zs, zc)
    assert round(worst, 2) == psp.LAW_REHEARSED[psp.LAW_N]
    for k, v in bad.items():
        assert v > psp.LAW_SIGMAS, (k, v)
