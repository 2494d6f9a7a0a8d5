"""The weight side of the filter -- normalised weights, resampling uniforms, ancestors, the weights after a resample, the log-ML
bookkeeping, ESS, mean / var / proportions -- restated from the DEFINITIONS in mpmath, next to tests/hp_reference.py and under its rules.

Written from src/resample.jl, src/resize.jl, src/utils.jl and src/statistics.jl of the reference, not from the integer spec of DESIGN.md 3.3:

  * w_i = exp(lp_i - max lp) / sum (utils.jl:117-140; all -Inf: the uniform fallback and `invalid`), PREC-bit mpmath;
  * u_j = U_j / 2^64 exactly, U_j the 64-bit word pair of resample slot j, Philox in Python integers;
  * multinomial: the inverse CDF of w at u_j (resample.jl:59); stratified: at (j + u_j) / N over the particles as they stand or in
    descending order of priority (:155-170); residual: floor(N w_i) copies in particle order, then slot j from the categorical over
    N w_i - floor(N w_i) (:96-115); pf_resize the same with n_new slots (resize.jl:46-124);
  * after the resample (resample.jl:190-202): 0, or lw[a] - lp[a] + log N - logsumexp(...) under a priority; the log-ML estimate grows by
    logsumexp(lw) - log N of the RAW weights (:178-182).

The spec computes these on integers.  How far it may sit from real arithmetic is bounded from the quantisation steps DESIGN.md 3.3
documents, per particle, in counts of the fixed-point weight q_i ~ exp(lp_i - m) 2^K:

    delta_i = 1/2                                   rounding to the nearest count
            + q_i (2 * 2^-52                        exp_'s 2 ulp
                   + ulp(lp_i - m) / 2              the Float64 subtraction in front of exp_: an absolute error of the exponent
                   + 2^-53)                         the rounding of the `+ 0.5` before the truncation
    D = sum delta_i,   S >= S~ - D   (S~ = sum exp(lp_i - m) 2^K in real arithmetic)

    multinomial   |cdf[a] / S - CDF(a)| <= 2 D / S.  The floor in T = floor(U S / 2^64) costs nothing: cdf[a] is an integer, so
                  T < cdf[a] <=> U S / 2^64 < cdf[a].
    stratified    the same + 3 counts: the floor in T, in L_j = floor(j S / N) and the length L_{j+1} - L_j off S / N by less than one.
    residual      N q_i / S is off N w_i by at most e_i = N (delta_i + w_i D) / S: particle i is decidable when N w_i is further than that
                  from the integer above it (and from the one below, unless that is 0: N q_i / S is never negative).  The tail weights
                  r_i 2^sh / S are off the fractional parts by h_i = e_i + 2^sh / S (the shift drops less than 2^sh counts), their sum R 2^sh / S
                  off F = N - sum floor(N w_i) by H = sum h_i: |tail cdf - CDF| <= (2 H + 2^sh / S) / (F - H), the last term the count of R's floor.
    uniform fallback (all -Inf): q_i = 1, S = N: no quantisation at all, every bound is 0.

A slot whose target lies within the bound of a CDF boundary of THIS reference is undecidable and is not compared.  No figure here is fitted
to an output of the oracle or of the device.

The sorted multinomial (the header comment of o_targets_sorted; this project's own construction, no line of resample.jl behind
it).  In the reals: e_i = -log((k_i + 1/2) 2^-52), k_i the top 52 bits of the 64-bit word pair of resample slot slot0 + i, i = 0 .. n; tiles of
2048 consecutive slots; gamma_t the Marsaglia-Tsang variate of shape c_t (c_t + 1 in the last tile) from the blocks 1 + 2k / 2 + 2k of counter
(slot0 + first, ., epoch, resample tag); V_t = sum_{r<t} gamma_r / sum gamma_r; slot j of tile t at x_j = V_t + (V_{t+1} - V_t) p_j / s_t, p_j the
tile's spacings up to and including j, s_t the tile's sum (+ e_n in the last tile); the ancestor is the inverse CDF of w at x_j.  The spec
computes x_j as the integer T_j against the integer CDF.  With S the integer sum of the weights (S >= S_lo), how far T_j / S may sit from x_j:

    gamma         every Float64 operation of gamma_tile carried as an E (d = shape - fl(1/3), c = 1 / sqrt(9 d), Box-Muller's x, v1 = 1 + c x,
                  v = (v1 v1) v1, d v): |fl(d v) - gamma_t| <= eg_t.  The two DECISIONS, v1 > 0 and log u < ((x^2 / 2 + d) - d v) + d log v, are
                  decidable when the two sides differ by more than their summed E bounds (the right side's bound carries the cancellation of
                  (x^2 / 2 + d) - d v at d ~ 2048: half an ulp of 2048 per term, ~7e-13, against |log u - right side| of order 1); asserted
                  decidable in every case, never skipped.  G_t = trunc(fl(d v) 2^Eg): a_t = eg_t + 2^-Eg, Eg = min(48, 50 - ceil(log2 ntl)),
                  read only to size the bound.
    V_t           Gpre_t / Gtot against A / B (A = sum_{r<t} gamma_r, B = sum gamma_r): |dA| <= sum_{r<t} a_r, |dB| <= sum a_r + 2^-Eg (the + 1
                  of Gtot), so |Gpre_t / Gtot - V_t| <= (|dA| + V_t |dB|) / (B - |dB|) = dV_t; the floor of Vlo_t 2^-64 on top.
    Tlo_t         floor(Vlo_t S / 2^64): one count of S.  b_t = dV_t + 2^-64 + 1 / S_lo bounds |Tlo_t / S - V_t| (b_0 = 0: Tlo_0 = 0 = V_0
                  exactly), and |Tw_t / S - (V_{t+1} - V_t)| <= b_t + b_{t+1} = dW_t.
    p_j / s_t     per spacing c = 1e-11 (neglog_u52's absolute bound, the figure tests/test_hp_math.py pins: passed in, the only imported
                  constant) + 2^-44 (the truncation): |p_j 2^-44 - P_j| <= (k + 1) c for the k + 1 spacings summed, |s_t 2^-44 - s^_t| <=
                  m c + 2^-44 for the tile's m spacings and its + 1; the ratio r = p / s against r^ = P / s^:
                  dr_j = ((k + 1) c + r^ (m c + 2^-44)) / (s^ - m c - 2^-44).
    the product   fl(fl(fl(p) fl(1 / fl(s))) fl(Tw)): the four roundings of the quotient (two conversions, the reciprocal, the product), the
                  conversion of Tw (it may exceed 2^53) and the last product, eta = expm1(6 * 2^-53) relative.  The clamp min(Tw, .) costs
                  nothing: p_j < s_t, the clamp only moves a rounded-up value back towards the real one.
    the last truncation: one count of S, 1 / S_lo.

    eps_j = 2 D / S_lo                                                     the weight side, as for `multinomial`
          + b_t + dr_j (W_t + dW_t) + r^_j dW_t + eta (W_t + dW_t) + 1 / S_lo,     W_t = V_{t+1} - V_t

computed per slot; a slot whose x_j lies within eps_j of a CDF boundary of this reference is undecidable.  Under the uniform fallback (all
-Inf) the spec's weights are q_i = 1 and S = n; it places the targets on the grid of S 2^K and drops the K bits again, so a
count is 2^-K / n there: S_lo = n 2^K, D = 0.  (On the grid of S = n a count is a whole particle: b_t + dW_t + 1 / S_lo is a few cells wide and
every slot undecidable by this derivation.  That is how these tests found that the spec had used that grid, had moved 903 of 2049 ancestors
by one against the construction and could never draw the last particle.)

Inexact log-weights (Softmax.inexact): the ancestor weights lwa_i = lw_i + logtrans_i of PGAS, backward simulation and smoothing are not
Float64 inputs but Float64 RESULTS: the device holds l_i with |l_i - a_i| <= e_i, a_i the real value (an E of tests/hp_reference.py).  The
reference is safe_softmax of the a_i; the device subtracts ITS maximum m = max l_i.  With a* = max a_i and mu = m - a*:

    |mu| <= e_max = max e_i     m = l_k <= a_k + e_k <= a* + e_k for the k that attains it, and m >= l_i* >= a* - e_i* for the real maximiser i*.
    l_i - m = (a_i - a*) + (l_i - a_i) - mu: the device's count is round(T_i exp(l_i - a_i) (1 + roundings)), T_i = exp(a_i - a*) exp(-mu) 2^K.
    The factor exp(-mu) is COMMON to all i: the T_i have the normalised weights and the CDF of the definition exactly.  So the bounds above
    hold with q~_i replaced by T_i <= q~_i exp(e_max) and the absolute error e_i of the exponent entering as a relative error of the count:

    delta_i = 1/2 + q~_i exp(e_max) expm1(e_i + 2 * 2^-52 + ulp(|a_i - a*| + e_i + e_max) / 2 + 2^-53)
              ((1 + a)(1 + b) <= exp(a + b): the product of the relative factors is inside expm1 of the sum of their exponents)
    S >= S~ exp(-e_max) - D,  D = sum delta_i

    and |cdf[a] / S - CDF(a)| <= 2 D / S, w_err and lse's relative bound of S follow as before from delta, D and this S_lo.  exp_'s flush:
    l_i - m < -708 is certain when a_i - a* < -708 - e_i - e_max (`dead`); a flushed count is 0 and T_i < 2^K exp(-708 + 2 e_max) < 1/2: inside
    delta_i either way.  -Inf is exact (lw = -Inf, or line_model's logtrans): count 0, delta 0.  With every e_i = 0 this is the bound above;
    Softmax(lp) on Float64 input takes the old statements and returns the old numbers.

ancestor_draw, backward_step and smooth_step restate PGAS' ancestor draw (Lindsten, Jordan & Schoen 2014), one transition of FFBSi (Godsill,
Doucet & West 2004) and one of FFBSm (Doucet, Godsill & Andrieu 2000) from these: the inverse CDF of w_i f(x' | x_i) / sum at the exact uniform
with eps = 2 D / S_lo, and W_s^i = sum_j W_{s+1}^j r_ij with r_ij = E(p_i, w_err_i), accumulated by E arithmetic (one multiply and one add per
term at half an ulp each, W_{s+1}'s own bound carried through the product).  Flagged ancestor weights (NaN, +Inf, all -Inf) are the spec's
exact fallback -- the recorded parent -- and are reported as such, not bounded.  The pairwise smoother comes out of the same
transition: smooth_step(pairs=True) accumulates A_i[c] = sum_j t_ij x_{s+1}^j[c], t_ij = W_{s+1}^j r_ij, beside W_s; `cross` and `second` at the
end of this module turn A and W into the raw lag-one and second moments, each an E.

The rest of the resize family, from src/resize.jl of the reference:

  * pf_optimal_resize! (:149-219): w = safe_softmax(lw); find_inv_w_threshold is the ascending loop `A -= 1; B += kappa`, the first kappa with
    B / kappa + A <= n', then c = (n' - A) / B, else c = n'; keep_i <=> c w_i >= 1; the rest by the literal systematic loop of :170-178 over
    safe_softmax(lw[strat]) from u0 = U / 2^64 of resample slot 0; kept slots carry lw + (log n' - log n), the others logsumexp(lw) - log c + that.
  * pf_dereplicate!(method = :sample) (:281-293): per group of k replicates the inverse CDF of softmax(lw[group]) at the group's uniform, and
    logsumexp(group) - log k.  Output j reads words (0,1) of the block with counter (j, 0, epoch, resample tag).
  * pf_coalesce! (:309-334): groups by equality of the key, log sum_{i in g} exp(w_i) + log G - log n_old.

Their bounds, in the counts of above (q~_i = exp(lp_i - m) 2^K real, q_i the integer, |q_i - q~_i| <= delta_i):

    threshold     the spec sums integers: over the set summed so far |B - B~| <= dB = sum delta_i, and the candidate kappa is off by delta_k, so
                  |B / q_k - B~ / q~_k| <= (dB + (B~ / q~_k) delta_k) / (q~_k - delta_k): kappa is decidable when n_check is further than that
                  from n'.  B contains kappa, so n_check >= 1 + A in real and in integer arithmetic alike: a kappa with 1 + A > n' is no threshold,
                  exactly.  A zero weight gives 0 / 0, which `<=` rejects.  At the smallest positive weight B = kappa and n_check = 1 + A is an
                  identity of integers, decided exactly.
    keep set      c w_i >= 1 <=> a q_i >= B, a = n' - A an exact integer: decidable when |a q~_i - B~| > a delta_i + dB.  The threshold
                  particle at the smallest positive weight (B = kappa, a >= 1) is kept exactly; the uniform fallback has no quantisation.
    picks         the loop's test `u < 0` at particle i of the unkept set is cdf'_i > (m + u0) / n_res on the normalised CDF of the unkept
                  weights, m the picks so far: the stratified bound over that set, (2 D' + 3) / S'_lo with D' = sum of its delta_i and
                  S'_lo = S~' - D'.  The spec reads all 64 bits of U.  Unkept weights all zero: the uniform weights are exact, the bound is 0.
                  Unkept weights all the same Float64: the same input gives the same count q, the normalised CDF is i / n_strat whatever q
                  is, and the floors cost nothing against the integer i q: the bound is 0 as well (`dominant`, `equal`).
    weights       log_ of (double)B 2^-K: B's relative bound dB / (B~ - dB), the conversion, log_'s 2 ulp; every + and - half an ulp (E).
    dereplicate   the multinomial bound 2 D / S_lo of the group's own Softmax at K = fix_K(k); logsumexp as Softmax.lse().
    coalesce      Softmax(w[g], K = fix_K(n_old)).lse() of the group, then the additions.

Helper module, no tests."""
import bisect
import math

import numpy as np

import hp_reference as hp
from hp_reference import E, M, mpf

U = 2.0 ** -53                    # half an ulp, relative: one correctly rounded operation
TREE_CHUNK = 2048


def fix_K(n):
    """K = min(52, 62 - ceil(log2 N)): read only to size the bounds"""
    return min(52, 62 - (int(n) - 1).bit_length())


def resample_u64(seed, slot, epoch):
    """resample slot s reads the block with counter (s >> 1, 0, epoch, resample tag); words (0,1) for even s, (2,3) for odd s,
    the first word of the pair the high half"""
    w = hp.block(seed, slot >> 1, 0, epoch, hp.TAG_RESAMPLE)
    return hp.u64(w[2], w[3]) if slot & 1 else hp.u64(w[0], w[1])


def uniform(seed, slot, epoch):
    return M.ldexp(mpf(resample_u64(seed, slot, epoch)), -64)          # exact: 64 bits in PREC


# ------------------------------------------------------------------------------------------- the normalised weights
class Softmax:
    """safe_softmax of a Float64 vector in mpmath, with the per-particle quantisation bound of the module docstring"""

    def __init__(self, lp, K=None, real=None, err=None):
        """`real`, `err`: only through Softmax.inexact"""
        lp = np.ascontiguousarray(lp, np.float64)
        assert lp.size >= 1 and not np.isnan(lp).any() and not (lp == np.inf).any()
        self.lp, self.n = lp, lp.size
        self.K = fix_K(self.n) if K is None else int(K)
        m = float(lp.max())
        self.m, self.invalid = m, m == -np.inf
        self.e_max = 0.0
        if self.invalid:                                             # utils.jl:123-126: uniform weights
            self.W = [mpf(1)] * self.n
            self.delta = np.zeros(self.n)
            self.St = float(self.n)
        elif real is None:
            mm = mpf(m)
            self.W = [M.exp(mpf(float(x)) - mm) if x != -np.inf else mpf(0) for x in lp]
            with np.errstate(invalid="ignore"):
                d = np.where(lp == -np.inf, 0.0, np.abs(lp - m))
            qt = np.array([float(M.ldexp(w, self.K)) for w in self.W])
            ulp_d = np.array([math.ulp(x) for x in d])
            self.delta = np.where(lp == -np.inf, 0.0, 0.5 + qt * (4 * U + 0.5 * ulp_d + U))
            self.St = float(M.ldexp(M.fsum(self.W), self.K))
        else:                                                        # the module docstring, "Inexact log-weights"
            err = np.where(lp == -np.inf, 0.0, np.asarray(err, np.float64))
            assert np.isfinite(err).all()
            mm = max(real)
            self.e_max = em = float(err[lp != -np.inf].max())
            self.W = [M.exp(a - mm) if x != -np.inf else mpf(0) for a, x in zip(real, lp)]
            d = np.array([float(mm - a) if x != -np.inf else 0.0 for a, x in zip(real, lp)])
            qt = np.array([float(M.ldexp(w, self.K)) for w in self.W])
            ulp_d = np.array([math.ulp(x) for x in d + err + em])
            self.delta = np.where(lp == -np.inf, 0.0, 0.5 + qt * math.exp(em) * np.expm1(err + 4 * U + 0.5 * ulp_d + U))
            self.St = float(M.ldexp(M.fsum(self.W), self.K)) * math.exp(-em)
            self.margin = err + em
        self.tot = M.fsum(self.W)
        self.D = float(self.delta.sum())
        self.S_lo = self.St - self.D                                 # the integer S is not below this
        if self.invalid:
            self.dead = np.zeros(self.n, bool)
        elif real is None:
            self.dead = lp - m < -708.0                              # exp_ flushes them; -Inf included
        else:
            self.dead = (lp == -np.inf) | (-d < -708.0 - self.margin)
        self._p = self._pf = None

    @classmethod
    def inexact(cls, a, K=None):
        """`a`: one E per particle -- the real log-weight and the bound of the Float64 the device forms -- or -Inf (float) where it is exactly -Inf"""
        real = [x.v if isinstance(x, E) else mpf(x) for x in a]
        err = [x.e if isinstance(x, E) else 0.0 for x in a]
        return cls([float(r) for r in real], K, real=real, err=err)

    @property
    def p(self):
        if self._p is None:
            self._p = [w / self.tot for w in self.W]
        return self._p

    @property
    def pf(self):
        if self._pf is None:
            self._pf = np.array([float(x) for x in self.p])
        return self._pf

    def cdf(self, order=None):
        """normalised inclusive CDF over the particles in `order`"""
        W = self.W if order is None else [self.W[i] for i in order]
        out, s = [], mpf(0)
        for w in W:
            s += w
            out.append(s / self.tot)
        return out

    def rel_S(self):
        """relative bound of the integer sum S against S~"""
        return self.D / self.S_lo

    def w_err(self):
        """|(double)q_i / (double)S - w_i|: the count bound over S, S's own bound, two conversions and the division"""
        return self.delta / self.S_lo + self.pf * (self.rel_S() + 3 * U)

    # ---- logsumexp = m + log_(S 2^-K) as an E
    def lse(self, in_err=0.0):
        if self.invalid:
            return E(-M.inf)
        arg = E(self.tot, float(self.tot) * (self.rel_S() + U))       # (double)S, scaled exactly
        r = E(self.m) + arg.log(2.0)
        return E(r.v, r.e + in_err)

    # ---- ESS = S^2 / Q, Q = sum q^2 exact in 128 bits
    def ess(self):
        if self.invalid:
            return None
        q = np.array([float(M.ldexp(w, self.K)) for w in self.W])
        Q = M.fsum([w * w for w in self.W])
        val = self.tot * self.tot / Q
        relQ = float(np.sum(2 * q * self.delta + self.delta ** 2)) / (float(M.ldexp(Q, 2 * self.K)) - float(np.sum(2 * q * self.delta)))
        # conversions of S, Qhi, Qlo, the product, the sum of the two halves and the division: 7 roundings
        rel = 2 * self.rel_S() + relQ + 7 * U
        return E(val, float(val) * rel * (1 + rel))


# ------------------------------------------------------------------------------------------- ancestors
class Ancestors:
    def __init__(self, anc, undecidable, eps, ties=None):
        self.anc, self.undecidable, self.eps = anc, undecidable, eps
        self.ties = ties                              # sorted stratified: lp; equal priorities may be permuted (check_ancestors)


def _inverse_cdf(cdf, xs, eps):
    """first a with cdf[a] > x per target; undecidable when x is within eps of the boundary below or above (0 and 1 are exact).  `eps`: one
    bound for all targets, or one per target"""
    n, anc, und = len(cdf), [], []
    per_slot = None if np.isscalar(eps) else eps
    for j, x in enumerate(xs):
        if per_slot is not None:
            eps = per_slot[j]
        a = min(bisect.bisect_right(cdf, x), n - 1)
        near = (a > 0 and x - cdf[a - 1] <= eps) or (a < n - 1 and cdf[a] - x <= eps)
        anc.append(a)
        if near:
            und.append(j)
    return anc, und


def multinomial(sm, seed, epoch, n_slots=None, slot0=0):
    n_slots = sm.n if n_slots is None else n_slots
    eps = 0.0 if sm.invalid else 2 * sm.D / sm.S_lo
    anc, und = _inverse_cdf(sm.cdf(), [uniform(seed, slot0 + j, epoch) for j in range(n_slots)], eps)
    return Ancestors(anc, und, eps)


# ------------------------------------------------------------------------------------------- the sorted multinomial
SP_TILE = 2048                    # slots per tile
SP_ATTEMPTS = 8                   # Marsaglia-Tsang attempts per tile total, then the value d
SP_FRAC = 44                      # a spacing is truncated at 2^-44
NEGLOG_ABS = 1e-11                # neglog_u52's absolute bound: the figure tests/test_hp_math.py asserts, not measured here
MUTATIONS = ("attempt_blocks", "accept_words23", "last_shape", "no_e_n", "tile_id_local", "spacing_slot0", "spacing_pair", "d_half",
             "second_normal", "exclusive", "boundary_next")      # what the negative controls hand the checker; never a truth for the device
SORTED_MAX = {}                   # largest derived bound per quantity over the calls so far (`python tests/test_hp_sorted_multinomial.py`)


def _worst(what, x):
    SORTED_MAX[what] = max(SORTED_MAX.get(what, 0.0), float(x))


def gamma_E(ntl):
    """Eg = min(48, 50 - ceil(log2 ntl)): read only to size the bound, as fix_K is"""
    return min(48, 50 - (int(ntl) - 1).bit_length())


class GammaTile:
    """one tile total: .value the E of fl(d v) (its .v the real gamma_t of the construction), .attempt the accepted attempt (SP_ATTEMPTS: none,
    the value is d), .negative how many attempts had 1 + c x <= 0, .margin the smallest |side - side| - bound over its decisions"""

    def __init__(self, value, attempt, negative, margin):
        self.value, self.attempt, self.negative, self.margin = value, attempt, negative, margin


def gamma_tile(seed, gid, epoch, shape, mutate=None):
    """Marsaglia & Tsang (2000), Gamma(shape, 1) for an integer shape >= 1, every Float64 operation an E.  Attempt k: x the first Box-Muller
    normal of block 1 + 2k, u the 52-bit uniform of words (0,1) of block 2 + 2k, both of counter (gid, ., epoch, resample tag); reject when
    1 + c x <= 0, accept when log u < ((x^2 / 2 + d) - d v) + d log v, v = (1 + c x)^3.  A decision closer than its bounds is an error: the
    reference cannot say which attempt the spec takes."""
    d = E(float(shape)) - (E(1.0) / E(2.0 if mutate == "d_half" else 3.0))
    c = E(1.0) / (E(9.0) * d).sqrt()
    negative, margin = 0, math.inf
    for k in range(SP_ATTEMPTS):
        bx, bu = (1 + k, 2 + k) if mutate == "attempt_blocks" else (1 + 2 * k, 2 + 2 * k)
        x = hp.box_muller(hp.block(seed, gid, bx, epoch, hp.TAG_RESAMPLE))[1 if mutate == "second_normal" else 0]
        w = hp.block(seed, gid, bu, epoch, hp.TAG_RESAMPLE)
        u = hp.u52(w[2], w[3]) if mutate == "accept_words23" else hp.u52(w[0], w[1])
        v1 = E(1.0) + c * x
        gap = abs(float(v1.v)) - v1.e
        assert gap > 0.0, f"gamma_tile(gid {gid}, epoch {epoch}, shape {shape}) attempt {k}: the sign of 1 + c x = {v1} is not decidable"
        margin = min(margin, gap)
        if v1.v <= 0:
            negative += 1
            continue
        v = (v1 * v1) * v1
        lhs = E(u).log()
        rhs = (((x * x).scale2(-1) + d) - d * v) + d * v.log()
        gap = abs(float(lhs.v - rhs.v)) - (lhs.e + rhs.e)
        assert gap > 0.0, f"gamma_tile(gid {gid}, epoch {epoch}, shape {shape}) attempt {k}: log u = {lhs} against {rhs} is not decidable"
        margin = min(margin, gap)
        _worst("gamma_tile: bound of the acceptance test's right side", rhs.e)
        if lhs.v < rhs.v:
            return GammaTile(d * v, k, negative, margin)
    return GammaTile(d, SP_ATTEMPTS, negative, margin)


def spacing(seed, slot, epoch, mutate=None):
    """e = -log((k + 1/2) 2^-52), k the top 52 bits of the slot's 64-bit uniform"""
    if mutate == "spacing_pair":
        w = hp.block(seed, slot >> 1, 0, epoch, hp.TAG_RESAMPLE)
        bits = hp.u64(w[0], w[1]) if slot & 1 else hp.u64(w[2], w[3])
    else:
        bits = resample_u64(seed, slot, epoch)
    return -M.log(M.ldexp(mpf(2 * (bits >> 12) + 1), -53))


class SortedTargets:
    """x[j], eps[j] (the target side of the module docstring's eps_j, without 2 D / S_lo) for the slots j of the tiles asked for; .tiles the
    GammaTile of every tile; .V the tile boundaries"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def sorted_targets(seed, epoch, n, slot0, S_lo, mutate=None, tiles=None):
    """the construction of DESIGN.md 3.6 in the reals with the bound of the module docstring per slot.  `S_lo`: what the integer sum of the
    weights is not below (a count of S is at most 1 / S_lo).  `tiles`: the tiles whose slots are placed (None: all); the totals of ALL tiles
    are drawn either way -- they place every boundary."""
    assert mutate is None or mutate in MUTATIONS, mutate
    ntl = (n + SP_TILE - 1) // SP_TILE
    Eg = gamma_E(ntl)
    gid0 = 0 if mutate == "tile_id_local" else slot0
    sp0 = 0 if mutate == "spacing_slot0" else slot0
    G = []
    for t in range(ntl):
        first = t * SP_TILE
        cnt = min(SP_TILE, n - first)
        last = t == ntl - 1 and mutate != "last_shape"
        G.append(gamma_tile(seed, gid0 + first, epoch, cnt + (1 if last else 0), mutate))
    a = [g.value.e + 2.0 ** -Eg for g in G]
    B = M.fsum(g.value.v for g in G)
    dB = sum(a) + 2.0 ** -Eg
    B_lo = float(B) - dB
    assert B_lo > 0.0
    V, b, A, dA = [], [], mpf(0), 0.0
    for t in range(ntl + 1):
        Vt = A / B
        V.append(Vt)
        # Tlo_0 = 0 and V_0 = 0 exactly; past the last tile nothing is floored twice, but the bound is kept uniform
        b.append(0.0 if t == 0 else (dA + float(Vt) * dB) / B_lo + 2.0 ** -64 + 1.0 / S_lo)
        if t < ntl:
            A += G[t].value.v
            dA += a[t]
    for t in range(ntl):
        _worst("gamma_t: |fl(d v) - gamma| / gamma", G[t].value.e / float(G[t].value.v))
        _worst("V_t: |Gpre / Gtot - V_t|", b[t] - (2.0 ** -64 + 1.0 / S_lo if t else 0.0))
    eta = math.expm1(6 * U)
    c1 = NEGLOG_ABS + 2.0 ** -SP_FRAC
    x, eps = {}, {}
    for t in (range(ntl) if tiles is None else tiles):
        first = t * SP_TILE
        cnt = min(SP_TILE, n - first)
        e = [spacing(seed, sp0 + first + k, epoch, mutate) for k in range(cnt)]
        m = cnt
        s = M.fsum(e)
        if t == ntl - 1 and mutate != "no_e_n":
            s += spacing(seed, sp0 + n, epoch, mutate)
            m += 1
        ds = m * c1 + 2.0 ** -SP_FRAC                                        # the tile's spacings and the + 1 of s_t
        s_lo = float(s) - ds
        assert s_lo > 0.0
        lo, hi = (V[t + 1], V[min(t + 2, ntl)]) if mutate == "boundary_next" else (V[t], V[t + 1])
        W, dW = hi - lo, b[t] + b[t + 1]
        Wf = float(W)
        p = mpf(0)
        for k in range(cnt):
            pk = p if mutate == "exclusive" else p + e[k]
            p += e[k]
            r = pk / s
            rf = float(r)
            dr = ((k + 1) * c1 + rf * ds) / s_lo
            x[first + k] = lo + W * r
            eps[first + k] = b[t] + dr * (Wf + dW) + rf * dW + eta * (Wf + dW) + 1.0 / S_lo
            _worst("p_j / s_t: |p / s - P / s^|", dr)
    return SortedTargets(x=x, eps=eps, tiles=G, V=V, Eg=Eg)


def sorted_multinomial(sm, seed, epoch, n_slots=None, slot0=0, mutate=None):
    """the ancestors of GPF_RESAMPLE_MULTINOMIAL_SORTED: the inverse CDF of w at the x_j of sorted_targets, each slot with its own eps_j.
    `mutate`: one of MUTATIONS, for the negative controls only.  Beside the fields of Ancestors: .targets (SortedTargets)"""
    n_slots = sm.n if n_slots is None else n_slots
    st = sorted_targets(seed, epoch, n_slots, slot0, math.ldexp(sm.n, sm.K) if sm.invalid else sm.S_lo, mutate)
    weight_side = 0.0 if sm.invalid else 2 * sm.D / sm.S_lo
    eps = [weight_side + st.eps[j] for j in range(n_slots)]
    anc, und = _inverse_cdf(sm.cdf(), [st.x[j] for j in range(n_slots)], eps)
    for e in eps:
        _worst("eps_j: the slot's whole bound", e)
    out = Ancestors(anc, und, max(eps))
    out.targets = st
    return out


def sort_order(lp):
    """sortperm(lp, rev=true) (resample.jl:156-157), stable: ties keep particle order -- the order the oracle uses; the checks accept any"""
    return [int(i) for i in np.argsort(-np.asarray(lp, np.float64), kind="stable")]


def stratified(sm, seed, epoch, sort_particles, slot0=0):
    """`slot0`: a view's first particle -- the strata are local to the view (stratum j of n: resample.jl:155-162 on the sub-state's own
    n_particles), the uniform of stratum j is that of resample slot slot0 + j"""
    n = sm.n
    eps = 0.0 if sm.invalid else (2 * sm.D + 3) / sm.S_lo
    order = sort_order(sm.lp) if sort_particles else None
    xs = [(j + uniform(seed, slot0 + j, epoch)) / n for j in range(n)]
    k, und = _inverse_cdf(sm.cdf(order), xs, eps)
    anc = [order[i] for i in k] if order is not None else k
    return Ancestors(anc, und, eps, ties=sm.lp if sort_particles else None)


def residual(sm, seed, epoch, n_slots=None):
    """(Ancestors, undecidable particles): head = floor(n_slots w_i) copies in particle order; tail slot j reads the uniform of slot j"""
    n_slots = sm.n if n_slots is None else n_slots
    if sm.invalid:
        e = np.zeros(sm.n)
    else:
        e = n_slots * (sm.delta + sm.pf * sm.D) / sm.S_lo
    if sm.invalid:                                                   # n_slots / n exactly
        c, frac, bad = [n_slots // sm.n] * sm.n, [mpf(n_slots % sm.n) / sm.n] * sm.n, []
    else:
        x = [n_slots * p for p in sm.p]
        c = [int(M.floor(v)) for v in x]
        frac = [v - k for v, k in zip(x, c)]
        bad = [i for i in range(sm.n) if float(1 - frac[i]) <= e[i] or (c[i] >= 1 and float(frac[i]) <= e[i])]
    anc = [i for i in range(sm.n) for _ in range(c[i])]
    n_res = len(anc)
    und, eps = [], 0.0
    if n_res < n_slots:
        F = n_slots - n_res
        cl = (n_slots - 1).bit_length()
        sh = max(0, int(math.ceil(sm.St + sm.D)).bit_length() + cl - 62)              # the residual CDF fits 62 bits
        step = 2.0 ** sh / sm.S_lo
        H = float(np.sum(e + step))
        eps = (2 * H + step) / (F - H) if F > H else math.inf
        tot, s, cdf = M.fsum(frac), mpf(0), []
        for f in frac:
            s += f
            cdf.append(s / tot)
        tail, und = _inverse_cdf(cdf, [uniform(seed, j, epoch) for j in range(n_res, n_slots)], eps)
        anc += tail
        und = [n_res + j for j in und]
    return Ancestors(anc, und, eps), bad


def reference_ancestors(lp, method, seed, epoch, n_slots=None, sort_particles=True, K=None, slot0=0):
    """(Softmax, Ancestors, undecidable particles) of one resample / resize call; `slot0`: the first particle of a view"""
    sm = Softmax(lp, K)
    if method == "multinomial":
        return sm, multinomial(sm, seed, epoch, n_slots, slot0), []
    if method == "multinomial_sorted":
        assert n_slots in (None, sm.n)
        return sm, sorted_multinomial(sm, seed, epoch, slot0=slot0), []
    if method == "stratified":
        assert n_slots in (None, sm.n)
        return sm, stratified(sm, seed, epoch, sort_particles, slot0), []
    assert slot0 == 0
    if method == "residual":
        a, bad = residual(sm, seed, epoch, n_slots)
        return sm, a, bad
    raise ValueError(method)


def check_ancestors(ref: Ancestors, parents0, sm, label):
    """`parents0`: 0-based ancestors under test.  Every decidable slot must hold the reference's ancestor (sorted stratified: a particle of the
    same priority); no slot may hold a particle whose weight exp_ flushes.  Returns the number of undecidable slots."""
    parents0 = np.asarray(parents0)
    assert parents0.shape == (len(ref.anc),), (label, parents0.shape, len(ref.anc))
    assert ((parents0 >= 0) & (parents0 < sm.n)).all(), label
    skip, wrong, fwd, inv = set(ref.undecidable), [], {}, {}
    for j, (got, want) in enumerate(zip(parents0, ref.anc)):
        if j in skip:
            continue
        if ref.ties is not None:
            # particles of equal priority may stand in any order inside their run of the sorted CDF, but in ONE order: the answers must
            # be those of the reference under a permutation inside each priority class (same position -> same particle, and only it)
            got = int(got)
            if ref.ties[got] != ref.ties[want] or fwd.setdefault(want, got) != got or inv.setdefault(got, want) != want:
                wrong.append((j, got, want))
        elif got != want:
            wrong.append((j, int(got), want))
    assert not wrong, f"{label}: {len(wrong)} ancestors off the reference (eps {ref.eps:.3g}), first (slot, got, want) {wrong[:4]}"
    if not sm.invalid:
        assert not sm.dead[parents0].any(), f"{label}: a particle more than 708 below the maximum was chosen"
    return len(ref.undecidable)


# ------------------------------------------------------------------------------------------- weights and log-ML after the resample
def log_n(n):
    return E(float(n)).log(2.0)


def weights_after(lw, lp, parents0, n_new=None, total=None):
    """update_weights! (resample.jl:190-202) under a priority: lw[a] - lp[a] + log N - logsumexp(lw[a] - lp[a]), one E per slot.  The spec
    sums its own ROUNDED differences: their half ulp enters the logsumexp's bound.  `total`: the sub-state form (:205-218) -- the
    logsumexp of the view's weights before the call, as an E, in the place of log N."""
    lw, lp, a = np.asarray(lw), np.asarray(lp), np.asarray(parents0)
    n_new = a.size if n_new is None else n_new
    with np.errstate(invalid="ignore"):
        ws = lw[a] - lp[a]
    if np.isnan(ws).any():
        return None
    sm = Softmax(ws, fix_K(n_new))
    in_err = 0.5 * max(math.ulp(abs(float(x))) for x in ws if np.isfinite(x))
    shift = (log_n(n_new) if total is None else total) - sm.lse(in_err)
    return [(E(float(lw[i])) - E(float(lp[i]))) + shift for i in a]


def lml_estimate_from(lml_est: E, sm):
    """log_ml_estimate (utils.jl:171-178): lml_est + logsumexp(lw) - log N, `lml_est` the running estimate with its own bound; the bound holds
    for either association of the two additions"""
    lse, ln = sm.lse(), log_n(sm.n)
    a, b = (lml_est + lse) - ln, lml_est + (lse - ln)
    return E(a.v, max(a.e, b.e))


# ------------------------------------------------------------------------------------------- weighted sums (statistics.jl:13-14, 48-50, 91-101)
def tree_levels(n):
    """roundings on the path of one term through the summation tree of DESIGN.md 3.5: a chunk of 2048, then the chunks' partials"""
    chunks = (n + TREE_CHUNK - 1) // TREE_CHUNK
    return (min(n, TREE_CHUNK) - 1).bit_length() + (chunks - 1).bit_length()


def _tree_err(n, abs_terms_sum):
    L = tree_levels(n) * U
    return L * abs_terms_sum / (1 - L)


def mean(sm, x):
    """sum w_i x_i as an E: each term carries w_i's bound and the product's rounding, the tree one rounding per level over sum |terms|"""
    x = np.asarray(x, np.float64)
    v = M.fsum([p * mpf(float(t)) for p, t in zip(sm.p, x)])
    at = float(np.sum(sm.pf * np.abs(x)))
    term_err = float(np.sum(np.abs(x) * sm.w_err())) + U * at
    return E(v, term_err + _tree_err(sm.n, at + term_err))


def var(sm, x):
    """sum w_i (x_i - mu)^2, population form, centred on the weighted mean mu.  The spec centres on its COMPUTED mean: sum w (x - c)^2 =
    var + (c - mu)^2 for weights that sum to one, bounded here term by term with |c - mu| <= the mean's bound."""
    x = np.asarray(x, np.float64)
    mu = mean(sm, x)
    dv = [mpf(float(t)) - mu.v for t in x]
    v = M.fsum([p * d * d for p, d in zip(sm.p, dv)])
    ad = np.array([abs(float(d)) for d in dv])
    de = mu.e + 0.5 * np.array([math.ulp(t + mu.e) for t in ad])                       # x - c: c's distance from mu, one rounding
    sq = ad * ad
    sq_err = 2 * ad * de + de * de + 2 * U * (ad + de) ** 2                             # the square and its rounding
    at = float(np.sum(sm.pf * (sq + sq_err)))
    term_err = float(np.sum((sq + sq_err) * sm.w_err())) + float(np.sum(sm.pf * sq_err)) + U * at
    return E(v, term_err + _tree_err(sm.n, at + term_err))


def proportion(sm, x, value):
    x = np.asarray(x, np.float64)
    hit = x == value
    v = M.fsum([p for p, h in zip(sm.p, hit) if h])
    term_err = float(np.sum(sm.w_err()[hit]))
    return E(v, term_err + _tree_err(sm.n, float(v) + term_err))


def log_norm_weights(sm):
    lse = sm.lse()
    return [E(float(t)) - lse for t in sm.lp]


def norm_weights(sm):
    return [E(p, e) for p, e in zip(sm.p, sm.w_err())]


# ------------------------------------------------------------------------------------------- pf_optimal_resize! (resize.jl:149-219)
class OptimalResize:
    """what the definition says of one call: the kept particles (ascending), the systematic picks with their undecidable slots, one
    expected weight per new slot (None: -Inf), and where the reference itself cannot decide the threshold or a keep test"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _lse_counts(sm, B, dB):
    """m + log_((double)B 2^-K) of an integer sum B of counts whose real value is `B` (in units of exp(lp - m)), off by at most dB counts"""
    Bt = float(M.ldexp(B, sm.K))
    return E(sm.m) + E(B, float(B) * (dB / (Bt - dB) + U)).log(2.0)


def optimal_resize(lw, n_new, seed, epoch, K=None, threshold_shift=0):
    """`threshold_shift`: take the threshold that many positions further up the ascending order -- only the negative controls of
    tests/test_hp_weights.py pass it"""
    sm = Softmax(lw, K)
    n, W, delta = sm.n, sm.W, sm.delta
    assert 1 <= n_new <= n
    order = [int(i) for i in np.argsort(sm.lp, kind="stable")]                 # sort(weights), :204
    # ---- find_inv_w_threshold (:203-219)
    A, B, dB, thr, exact, und_thr = n, mpf(0), 0.0, None, False, []
    for pos, i in enumerate(order):
        A -= 1
        B += W[i]
        dB += float(delta[i])
        if A + 1 > n_new or W[i] == 0:                                         # n_check >= 1 + A;  0 / 0 is NaN and `<=` is false
            continue
        if B == W[i]:                                                          # n_check = 1 + A <= n': an identity of integers
            thr, exact = pos, True
            break
        r = B / W[i]
        qk = float(M.ldexp(W[i], sm.K))
        bound = (dB + float(r) * float(delta[i])) / (qk - float(delta[i])) if qk > delta[i] else math.inf
        if bound > 0.0 and abs(float(r + A - n_new)) <= bound:
            und_thr.append(i)
        if r + A <= n_new:
            thr = pos
            break
    if thr is not None and threshold_shift:
        thr, exact = thr + threshold_shift, False
        A, B, dB = n - thr - 1, M.fsum(W[i] for i in order[:thr + 1]), float(sum(delta[i] for i in order[:thr + 1]))
    if thr is None:
        a, B, dB = n_new, sm.tot, sm.D                                         # float(n_particles), :218
    else:
        a = n_new - A                                                          # c = (n' - A) / B, :215
    # ---- keep_idxs = c .* weights .>= 1 (:156)
    keep, und_keep = [], []
    for i in range(n):
        if exact and sm.lp[i] == sm.lp[order[thr]]:
            keep.append(i)
            continue
        lhs = a * W[i] - B
        bound = a * float(delta[i]) + dB
        if bound > 0.0 and abs(float(M.ldexp(lhs, sm.K))) <= bound:
            und_keep.append(i)
        if lhs >= 0:
            keep.append(i)
    kept = set(keep)
    strat = [i for i in range(n) if i not in kept]
    n_keep = len(keep)
    n_res = n_new - n_keep
    assert n_res >= 0, "not a case: more kept particles than slots"
    # ---- the systematic loop (:170-178) over safe_softmax(lw[strat])
    picks, und, eps, rest_uniform = [], [], 0.0, False
    if n_res > 0:
        Ws = [W[i] for i in strat]
        tot = M.fsum(Ws)
        if tot == 0:                                                           # safe_softmax of the rest: uniform, `invalid`
            Ws, tot, rest_uniform = [mpf(1)] * len(strat), mpf(len(strat)), True
        elif not sm.invalid and len({float(sm.lp[i]) for i in strat}) > 1:       # (one value: equal counts, the CDF is i / n exactly)
            Dp = float(sum(delta[i] for i in strat))
            eps = (2 * Dp + 3) / (float(M.ldexp(tot, sm.K)) - Dp)
        step = mpf(1) / n_res
        u = uniform(seed, 0, epoch) * step
        for i, w in zip(strat, Ws):
            u -= w / tot
            if eps > 0.0 and abs(float(u)) <= eps and len(picks) < n_res:
                und.append(len(picks))
            if u < 0:
                picks.append(i)
                u += step
    assert len(picks) == n_res, "not a case: the reference's own @assert (:181) throws"
    # ---- the weights (:189-195)
    ratio = log_n(n_new) - log_n(n)
    weights = [E(float(lw[i])) + ratio for i in keep]
    if sm.invalid:
        weights += [None] * n_res
    elif n_res:
        weights += [(_lse_counts(sm, B, dB) - log_n(a)) + ratio] * n_res
    return OptimalResize(sm=sm, keep=keep, n_keep=n_keep, picks=Ancestors(picks, sorted(set(und)), eps), weights=weights, a=a,
                         und_threshold=und_thr, und_keep=und_keep, invalid=sm.invalid or rest_uniform, rest_uniform=rest_uniform)


# ------------------------------------------------------------------------------------------- pf_dereplicate!(method = :sample) (resize.jl:281-293)
def dereplicate_u64(seed, j, epoch, block_of=lambda j: j):
    """output j reads words (0,1) of the block with counter (j, 0, epoch, resample tag) -- block j, not j >> 1"""
    w = hp.block(seed, block_of(j), 0, epoch, hp.TAG_RESAMPLE)
    return hp.u64(w[0], w[1])


def replicate_groups(n_old, k, layout):
    n_new = n_old // k
    if layout == "contiguous":
        return [list(range(j * k, (j + 1) * k)) for j in range(n_new)]
    return [list(range(j, n_old, n_new)) for j in range(n_new)]


def dereplicate_sample(lw, k, layout, seed, epoch, block_of=lambda j: j):
    """(Ancestors over the n_new outputs as global 0-based indices, expected weights (None: -Inf), the groups' Softmax)"""
    lw = np.asarray(lw, np.float64)
    assert lw.size % k == 0
    anc, und, weights, sms, eps = [], [], [], [], 0.0
    for j, idx in enumerate(replicate_groups(lw.size, k, layout)):
        sm = Softmax(lw[idx], fix_K(k))
        e = 0.0 if sm.invalid else 2 * sm.D / sm.S_lo
        a, ud = _inverse_cdf(sm.cdf(), [M.ldexp(mpf(dereplicate_u64(seed, j, epoch, block_of)), -64)], e)
        assert sm.invalid or not sm.dead[a[0]] or ud, "the definition draws a particle the fixed point cannot see: not a case"
        anc.append(idx[a[0]])
        if ud:
            und.append(j)
        weights.append(None if sm.invalid else sm.lse() - log_n(k))
        sms.append(sm)
        eps = max(eps, e)
    return Ancestors(anc, und, eps), weights, sms


# ------------------------------------------------------------------------------------------- pf_coalesce! (resize.jl:309-334)
def coalesce(rows, lw, cols, drop_smallest_of=None):
    """(first members, expected weights (None: -Inf), groups): the groups of a dict over the key columns' bit patterns, in order of first
    occurrence (the deviation include/gpf.h documents).  `drop_smallest_of`: a group whose sum leaves out its smallest member -- only the
    negative controls pass it."""
    rows, lw = np.ascontiguousarray(rows, np.float64), np.asarray(lw, np.float64)
    groups = {}
    for i in range(lw.size):
        groups.setdefault(rows[i, list(cols)].tobytes(), []).append(i)
    groups = list(groups.values())
    K = fix_K(lw.size)
    ratio = log_n(len(groups)) - log_n(lw.size)
    weights = []
    for g, idx in enumerate(groups):
        if g == drop_smallest_of:
            idx = sorted(idx, key=lambda i: lw[i])[1:]
        sm = Softmax(lw[idx], K)
        weights.append(None if sm.invalid else sm.lse() + ratio)
    return [idx[0] for idx in groups], weights, groups


# ------------------------------------------------------------------------------------------- ancestor sampling, backward simulation, smoothing
FALLBACK = "recorded parent"          # flagged ancestor weights (NaN, +Inf, all -Inf): the spec's exact fallback, not a draw


def ancestor_weights(ref, lw, xs, x_next, obs):
    """lwa_i = lw_i + log f(x_next | xs_i) per candidate: an E (the real value, the bound of the Float64 sum of the two Float64 terms), -Inf
    where either term is -Inf, or None where the recorded weight is NaN / +Inf.  `ref`: the hp_reference.Ref of the block's parameters."""
    out = []
    for w, x in zip(np.asarray(lw, np.float64), np.asarray(xs, np.float64)):
        if np.isnan(w) or w == np.inf:
            out.append(None)
            continue
        lt = ref.logtrans(list(x), list(x_next), obs)
        out.append(-np.inf if (w == -np.inf or lt.v == -M.inf) else E(float(w)) + lt)
    return out


def ancestor_softmax(ref, lw, xs, x_next, obs, K=None):
    """the Softmax over a block's ancestor weights, or FALLBACK"""
    a = ancestor_weights(ref, lw, xs, x_next, obs)
    if any(x is None for x in a) or all(not isinstance(x, E) for x in a):
        return FALLBACK
    return Softmax.inexact(a, fix_K(len(a)) if K is None else K)


def _draw(sm, seed, slot, epoch):
    """(index, undecidable) of the inverse CDF of sm at the uniform of resample slot `slot`"""
    anc, und = _inverse_cdf(sm.cdf(), [uniform(seed, slot, epoch)], 2 * sm.D / sm.S_lo)
    return anc[0], bool(und)


def ancestor_draw(ref, lw, xs, x_ref, obs, seed, epoch, slot):
    """PGAS: a_0 of a block = the inverse CDF of w_i f(x_ref | x_i) / sum over the block's particles (lw, xs: its weights and latents before
    the call) at the uniform of slot 0's own resample counter `slot` (its global index) of the call's epoch.  Invalid ancestor weights keep the
    predecessor: (0, False, FALLBACK).  Returns (a_0, undecidable, Softmax)."""
    sm = ancestor_softmax(ref, lw, xs, x_ref, obs)
    if sm is FALLBACK:
        return 0, False, FALLBACK
    a, und = _draw(sm, seed, slot, epoch)
    return a, und, sm


def backward_step(ref, lw, xs, x_held, obs, seed, epoch, slot, sm=None):
    """one transition of FFBSi: the local index at step s among the candidates (lw, xs: the recorded weights and latents of the block of the
    held particle's recorded parent in snapshot s), given the particle held at step s + 1 (x_held; obs: the observation row step s + 1 of ITS
    block was entered with), at the uniform of resample slot b n_samples + j under the epoch of that step.  `sm`: the ancestor_softmax of the same
    held particle where a caller has it already (draws that hold one particle share it).  Returns (index | FALLBACK, undecidable, Softmax |
    FALLBACK)."""
    sm = ancestor_softmax(ref, lw, xs, x_held, obs) if sm is None else sm
    if sm is FALLBACK:
        return FALLBACK, False, FALLBACK
    a, und = _draw(sm, seed, slot, epoch)
    return a, und, sm


def smooth_step(ref, W_next, x_next, lw, xs, obs, parents, pairs=False):
    """one transition of FFBSm: W_s^i = sum_j W_{s+1}^j w_s^i f(x_{s+1}^j | x_s^i) / sum_l w_s^l f(x_{s+1}^j | x_s^l), one E per candidate i.
    W_next: one E per target j; x_next: the targets' latents; lw, xs: the candidates' recorded weights and latents; parents[j]: the local index
    of target j's recorded parent among the candidates, read only on the fallback.  A target of weight exactly 0 adds nothing, and neither does a
    candidate that is -Inf or certainly flushed (Softmax.dead: more than 708 plus the bounds below the maximum) -- its W stays E(0, 0), which the
    check compares exactly.  Returns (W_s,
    the targets that took the fallback, the largest bound e_max of an ancestor weight met).

    pairs=True: the pairwise smoother's sums of the same transition from the SAME loop and the same ancestor softmax, computed once
    per target: A_i[c] = sum_j t_ij x_{s+1}^j[c] with the pairwise smoothing weight t_ij = W_{s+1}^j p_ij, one E per candidate and latent column,
    returned as a fourth value.  Value: the real t_ij (the real W_{s+1}^j times the real p_ij) times the Float64 x, summed exactly.  Bound, in E
    arithmetic, per term: W_{s+1}^j's own bound and p_ij's (w_err: the counts, their sum, two conversions and the division that is r) through the
    product, one rounding for t = W r, one for t * x (x is a Float64: exact), and one per addition into A in ascending j over the live targets --
    half an ulp of the largest magnitude the partial sum can have, its real value plus its bound, which the sum of |terms| plus their bounds is
    never below: the terms are signed and nothing is taken from their cancellation.  A target of weight exactly 0 is skipped before its row is
    read (its row may hold anything, an infinity included); a dead or certainly flushed candidate keeps A_i = E(0, 0); a target on its fallback
    gives its whole W_j to the recorded parent: t = W_j for that pair and no other."""
    acc, fell, e_max = [E(0.0) for _ in range(len(lw))], [], 0.0
    A = [[E(0.0)] * len(x_next[0]) for _ in range(len(lw))] if pairs else None

    def add(i, t, xj):
        acc[i] = acc[i] + t
        if pairs:
            A[i] = [a + t * x for a, x in zip(A[i], xj)]

    for j, Wj in enumerate(W_next):
        if Wj.v == 0 and Wj.e == 0.0:
            continue
        sm = ancestor_softmax(ref, lw, xs, x_next[j], obs)
        xj = [E(float(x)) for x in x_next[j]] if pairs else None
        if sm is FALLBACK:
            add(parents[j], Wj * E(1.0), xj)
            fell.append(j)
            continue
        p, we, e_max = sm.p, sm.w_err(), max(e_max, sm.e_max)
        for i in range(len(acc)):
            if sm.dead[i]:
                continue                                                       # -Inf, or certainly flushed by exp_: r = 0 EXACTLY, the term is +0.0
            add(i, Wj * E(p[i], we[i]), xj)
    return (acc, fell, e_max, A) if pairs else (acc, fell, e_max)


class Weighted:
    """weights given as E values, for mean / var below: .p the real weights, .pf their floats, .w_err() their bounds, .n"""

    def __init__(self, W):
        self.p, self.n = [w.v for w in W], len(W)
        self.pf = np.array([float(w.v) for w in W])
        self._e = np.array([w.e for w in W])

    def w_err(self):
        return self._e


def second(ws, x, a, c):
    """sum_i W_i x_i[a] x_i[c] as an E, for the statement (W x[a]) x[c] of DESIGN.md 5.7: each term carries W_i's bound times |x[a] x[c]| and
    the two products' roundings ((1 + u)^2 - 1 = 2u + u^2 of the largest magnitude the term can have), the tree one rounding per level over
    sum |terms|.  `x`: [n, d]"""
    x = np.asarray(x, np.float64)
    g = [mpf(float(s)) * mpf(float(t)) for s, t in zip(x[:, a], x[:, c])]
    v = M.fsum([p * t for p, t in zip(ws.p, g)])
    ag = np.array([abs(float(t)) for t in g])
    we = ws.w_err()
    at = float(np.sum(np.abs(ws.pf) * ag))
    w_part = float(np.sum(ag * we))
    term_err = w_part + (2 * U + U * U) * (at + w_part)
    return E(v, term_err + _tree_err(ws.n, at + term_err))


def cross(x, A, a, c):
    """cross_s[a][c] = sum_i x_s^i[a] A_i[c] as an E (A: smooth_step's fourth value, the sums over the targets of step s + 1): A_i[c]'s bound
    times |x|, one rounding for the product x * A, the tree of DESIGN.md 3.5 one rounding per level over sum |terms| (tree_levels)"""
    xa = np.asarray(x, np.float64)[:, a]
    v = M.fsum([mpf(float(t)) * Ai[c].v for t, Ai in zip(xa, A)])
    at = float(sum(abs(float(t)) * abs(float(Ai[c].v)) for t, Ai in zip(xa, A)))
    a_part = float(sum(abs(float(t)) * Ai[c].e for t, Ai in zip(xa, A)))
    term_err = a_part + U * (at + a_part)
    return E(v, term_err + _tree_err(len(A), at + term_err))
