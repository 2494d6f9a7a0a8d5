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
to an output of the oracle or of the device.  Helper module, no tests."""
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

    def __init__(self, lp, K=None):
        lp = np.ascontiguousarray(lp, np.float64)
        assert lp.size >= 1 and not np.isnan(lp).any() and not (lp == np.inf).any()
        self.lp, self.n = lp, lp.size
        self.K = fix_K(self.n) if K is None else int(K)
        m = float(lp.max())
        self.m, self.invalid = m, m == -np.inf
        if self.invalid:                                             # utils.jl:123-126: uniform weights
            self.W = [mpf(1)] * self.n
            self.delta = np.zeros(self.n)
            self.St = float(self.n)
        else:
            mm = mpf(m)
            self.W = [M.exp(mpf(float(x)) - mm) if x != -np.inf else mpf(0) for x in lp]
            with np.errstate(invalid="ignore"):
                d = np.where(lp == -np.inf, 0.0, np.abs(lp - m))
            qt = np.array([float(M.ldexp(w, self.K)) for w in self.W])
            ulp_d = np.array([math.ulp(x) for x in d])
            self.delta = np.where(lp == -np.inf, 0.0, 0.5 + qt * (4 * U + 0.5 * ulp_d + U))
            self.St = float(M.ldexp(M.fsum(self.W), self.K))
        self.tot = M.fsum(self.W)
        self.D = float(self.delta.sum())
        self.S_lo = self.St - self.D                                 # the integer S is not below this
        self.dead = (lp - m < -708.0) if not self.invalid else np.zeros(self.n, bool)      # exp_ flushes them; -Inf included
        self._p = self._pf = None

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
    """first a with cdf[a] > x per target; undecidable when x is within eps of the boundary below or above (0 and 1 are exact)"""
    n, anc, und = len(cdf), [], []
    for j, x in enumerate(xs):
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


def sort_order(lp):
    """sortperm(lp, rev=true) (resample.jl:156-157), stable: ties keep particle order -- the order the oracle uses; the checks accept any"""
    return [int(i) for i in np.argsort(-np.asarray(lp, np.float64), kind="stable")]


def stratified(sm, seed, epoch, sort_particles):
    n = sm.n
    eps = 0.0 if sm.invalid else (2 * sm.D + 3) / sm.S_lo
    order = sort_order(sm.lp) if sort_particles else None
    xs = [(j + uniform(seed, j, epoch)) / n for j in range(n)]
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


def reference_ancestors(lp, method, seed, epoch, n_slots=None, sort_particles=True, K=None):
    """(Softmax, Ancestors, undecidable particles) of one resample / resize call"""
    sm = Softmax(lp, K)
    if method == "multinomial":
        return sm, multinomial(sm, seed, epoch, n_slots), []
    if method == "stratified":
        assert n_slots in (None, sm.n)
        return sm, stratified(sm, seed, epoch, sort_particles), []
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


def weights_after(lw, lp, parents0, n_new=None):
    """update_weights! (resample.jl:190-202) under a priority: lw[a] - lp[a] + log N - logsumexp(lw[a] - lp[a]), one E per slot.  The spec
    sums its own ROUNDED differences: their half ulp enters the logsumexp's bound."""
    lw, lp, a = np.asarray(lw), np.asarray(lp), np.asarray(parents0)
    n_new = a.size if n_new is None else n_new
    with np.errstate(invalid="ignore"):
        ws = lw[a] - lp[a]
    if np.isnan(ws).any():
        return None
    sm = Softmax(ws, fix_K(n_new))
    in_err = 0.5 * max(math.ulp(abs(float(x))) for x in ws if np.isfinite(x))
    shift = log_n(n_new) - sm.lse(in_err)
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
