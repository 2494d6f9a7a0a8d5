"""An arbitrary-precision restatement of the five native models, of the counter-based random stream and of the
pf_* operations built on them -- the one reference of this suite that is NOT a twin of the C / HIP code.

Written from the definitions:
  * the models as Gen programs (README.md:43-55 and test/runtests.jl:3-16 of the reference; BASELINE configs 2-5), their
    densities as Gen's distributions: normal(mu, sigma) logpdf = -(x - mu)^2 / (2 sigma^2) - log sigma - log(2 pi) / 2,
    bernoulli, uniform_discrete;
  * only the NATURAL parameters in `model.info` are read (A, sq, sr, s0 | mu, s, sp, sv, sb | mu, phi, sigma |
    p_stay, p_start, sy, sobs | p_out, s_in, s_out, slopes); `model.params` -- the packed vector both the oracle and the
    kernels consume -- is never touched;
  * the random stream of DESIGN.md 3.1: Philox4x32-10 in Python integers, counter = (particle id, block, epoch, tag),
    key = seed; u52 = (k + 1/2) 2^-52; Box-Muller sqrt(-2 ln u1) (cos, sin)(2 pi u2).  The reference therefore predicts
    the SAMPLED VALUES, not only their scores.

Every quantity is a pair (value, bound): `E.v` is the value of the definition in mpmath (PREC bits), `E.e` is a bound on
how far a Float64 evaluation of the same expression may land from it.  The bound is DERIVED, by running first-order error
propagation through the expression, from the bounds the project asserts for its primitives:

    + - * / sqrt                    half an ulp of the result
    exp_, log_                      2 ulp            (tests/test_oracle_math.py, tests/test_hp_math.py)
    sincos2pi                       1e-15 absolute
    atan2_                          4 ulp
    libm log / log1p / cos / sin    1 ulp            (the host's libm, used by models.py when it packs constants)
    packed constants                the roundings of the expression that builds them in models.py, propagated the same way
    Float64 constants PI, TWOPI     their distance from pi, 2 pi

No factor in this file is fitted to the output of the oracle or of the device.
"""
import math

import mpmath

PREC = 160
M = mpmath.mp.clone()
M.prec = PREC
mpf = M.mpf
PI = +M.pi
HALF_LOG_2PI = M.log(2 * PI) / 2

TAG_INIT, TAG_UPDATE, TAG_RESAMPLE, TAG_MOVE, TAG_REWEIGHT = 1, 2, 3, 4, 5
NBLK = {"lgssm2": 1, "bearings4": 2, "sv1": 1, "object_motion": 2, "line_model": 1}
DISCRETE = {"lgssm2": (), "bearings4": (), "sv1": (), "object_motion": (0,), "line_model": (0, 1)}
DBL_MAX = 1.7976931348623157e308


# ------------------------------------------------------------------------------------------- value + derived bound
def _ulp(v, e=0.0):
    """ulp of the largest Float64 magnitude the computed result can have"""
    a = abs(float(v)) + e
    if not a < DBL_MAX:
        return math.inf
    return math.ulp(a)


class E:
    """a real number `v` (mpmath) and a bound `e` on |Float64 evaluation - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = v if isinstance(v, M.mpf) else mpf(v)
        self.e = float(e)

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(x)

    def _rounded(self, v, e):            # the result of one correctly rounded operation
        return E(v, e + 0.5 * _ulp(v, e))

    def __neg__(self):
        return E(-self.v, self.e)

    def __abs__(self):
        return E(abs(self.v), self.e)

    def __add__(self, o):
        o = E.lift(o)
        return self._rounded(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = E.lift(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.lift(o) - self

    def __mul__(self, o):
        o = E.lift(o)
        return self._rounded(self.v * o.v, float(abs(self.v)) * o.e + float(abs(o.v)) * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.lift(o)
        den = float(abs(o.v)) - o.e
        if not den > 0.0:
            return E(self.v / o.v if o.v != 0 else M.inf, math.inf)
        q = self.v / o.v
        return self._rounded(q, (self.e + float(abs(q)) * o.e) / den)

    def __rtruediv__(self, o):
        return E.lift(o) / self

    def scale2(self, k):
        """times 2^k: exact in binary floating point (no underflow at the magnitudes used here)"""
        return E(M.ldexp(self.v, k), math.ldexp(self.e, k))

    def sqrt(self):
        lo = float(self.v) - self.e
        if not lo > 0.0:
            return E(M.sqrt(max(self.v, 0)), math.inf if self.e > 0 else 0.0)
        r = M.sqrt(self.v)
        return self._rounded(r, self.e / (2.0 * math.sqrt(lo)))

    def log(self, ulps=2.0):
        lo = float(self.v) - self.e
        if not lo > 0.0:
            return E(M.log(self.v), math.inf)
        r = M.log(self.v)
        e = self.e / lo
        return E(r, e + ulps * _ulp(r, e))

    def log1p(self, ulps=1.0):
        lo = 1.0 + float(self.v) - self.e
        r = M.log1p(self.v)
        e = self.e / lo
        return E(r, e + ulps * _ulp(r, e))

    def exp(self, ulps=2.0):
        r = M.exp(self.v)
        e = 0.0 if self.e == 0.0 else (float(r) * math.expm1(self.e) if self.e < 700 else math.inf)
        return E(r, e + ulps * _ulp(r, e))

    def __repr__(self):
        return f"E({M.nstr(self.v, 20)} +- {self.e:.3g})"


def atan2(y, x, ulps=4.0):
    y, x = E.lift(y), E.lift(x)
    r = M.atan2(y.v, x.v)
    h2 = float(x.v * x.v + y.v * y.v)
    e = (float(abs(x.v)) * y.e + float(abs(y.v)) * x.e) / h2 if (y.e or x.e) else 0.0
    return E(r, e + ulps * _ulp(r, e))


def differs(got, want: E):
    """(|got - want.v|, want.e) as floats; the caller asserts first <= second"""
    return float(abs(mpf(float(got)) - want.v)), want.e


def rel_tol(want: E):
    return want.e / max(1.0, abs(float(want.v)))


# log(2 pi) / 2 as models.py packs it, 0.5 * math.log(2.0 * math.pi): math.pi is pi rounded, libm's log adds its ulp, the two scalings are exact
HL2P = E(PI, 0.5 * _ulp(PI)).scale2(1).log(1.0).scale2(-1)


# ------------------------------------------------------------------------------------------- the random stream
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC11), Philox4x32 with 10 rounds"""
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def block(seed, gid, blk, epoch, tag):
    """counter = (particle id, block, epoch, tag), key = seed"""
    return philox4x32_10(gid & _MASK, blk & _MASK, epoch & _MASK, tag, seed & _MASK, (seed >> 32) & _MASK)


def mix(seed, epoch):
    """the seed of the streams of pf_introduce's new particles, as the comment of include/gpf.h gpf_introduce states it:
    z = s ^ (e * 0x9e3779b97f4a7c15 + 0xd1b54a32d192ed03); z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9; z = (z ^ z >> 27) * 0x94d049bb133111eb;
    mix = z ^ z >> 31, in 64-bit wrap-around arithmetic"""
    m64 = (1 << 64) - 1
    z = seed ^ ((epoch * 0x9e3779b97f4a7c15 + 0xd1b54a32d192ed03) & m64)
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & m64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & m64
    return z ^ (z >> 31)


def u52(hi, lo):
    """(k + 1/2) 2^-52, k = the top 52 of the 64 bits hi:lo -- a Float64 without rounding, strictly inside (0, 1)"""
    k = (hi << 20) | (lo >> 12)
    return (k + 0.5) * 2.0 ** -52


def u64(hi, lo):
    return (hi << 32) | lo


def mulhi64(a, b):
    return (a * b) >> 64


def box_muller(words):
    """(z0, z1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2), u1 from words (0,1), u2 from words (2,3)"""
    u1, u2 = u52(words[0], words[1]), u52(words[2], words[3])
    r = (-(E(u1).log())).scale2(1).sqrt()
    a = 2 * PI * mpf(u2)
    return r * E(M.cos(a), 1e-15), r * E(M.sin(a), 1e-15)


class Stream:
    """the blocks one particle reads in one operation: block j of the operation is block blk0 + j of (gid, epoch, tag)"""

    def __init__(self, seed, gid, epoch, tag, blk0=0):
        self.seed, self.gid, self.epoch, self.tag, self.blk0 = seed, gid, epoch, tag, blk0

    def words(self, j):
        return block(self.seed, self.gid, self.blk0 + j, self.epoch, self.tag)

    def normal2(self, j):
        return box_muller(self.words(j))


# ------------------------------------------------------------------------------------------- Gen's distributions
def _sigma_consts(sigma):
    """1 / sigma and log sigma + log(2 pi)/2 as models.py packs them (one division; libm log, one addition of the rounded constant)"""
    s = E.lift(sigma)
    return 1.0 / s, s.log(1.0) + HL2P


def normal_logpdf(x, mu, sigma, consts=None):
    """Gen.normal: -(x - mu)^2 / (2 sigma^2) - log sigma - log(2 pi)/2, evaluated as -z^2 / 2 - c with z = (x - mu) (1 / sigma)"""
    inv, c = consts or _sigma_consts(sigma)
    z = (E.lift(x) - mu) * inv
    return -(z * z).scale2(-1) - c


def normal2_logpdf(x0, x1, mu0, mu1, sigma, consts=None):
    """two independent normals with one sigma: -(z0^2 + z1^2) / 2 - 2 (log sigma + log(2 pi)/2)"""
    inv, c = consts or _sigma_consts(sigma)
    z0, z1 = (E.lift(x0) - mu0) * inv, (E.lift(x1) - mu1) * inv
    return -(z0 * z0 + z1 * z1).scale2(-1) - c.scale2(1)


def log_bernoulli(p, value):
    """Gen.bernoulli: log p or log(1 - p); models.py packs them with libm log / log1p"""
    return E(p).log(1.0) if value else E(-p).log1p(1.0)


# ------------------------------------------------------------------------------------------- the five models
def _f(x):
    return float(x.v) if isinstance(x, E) else float(x)


class Ref:
    """the model `m` (a NativeModel; only `m.name` and `m.info` are read) as a Gen program in arbitrary precision"""

    def __init__(self, m):
        self.name, self.info = m.name, m.info
        self.nblk, self.dim = NBLK[m.name], m.dim
        self._c = {}
        assert set(m.info) - {"strata_address"} <= {"A", "sq", "sr", "s0", "mu", "s", "sp", "sv", "sb", "phi", "sigma", "p_stay", "p_start", "sy",
                                                    "sobs", "p_out", "s_in", "s_out", "slopes"}

    def sc(self, key, sigma=None):
        if key not in self._c:
            self._c[key] = _sigma_consts(self.info[key] if sigma is None else sigma)
        return self._c[key]

    # ---- x_t ~ p(. | x_{t-1}) (first: the prior); `s` is the particle's Stream.  Returns the new latent columns.
    def sample(self, first, xp, obs, s):
        I = self.info
        if self.name == "lgssm2":
            z0, z1 = s.normal2(0)
            if first:
                return [I["s0"] * z0, I["s0"] * z1]
            A = I["A"]
            t0 = E(float(A[0][0])) * xp[0] + E(float(A[0][1])) * xp[1]
            t1 = E(float(A[1][0])) * xp[0] + E(float(A[1][1])) * xp[1]
            return [t0 + I["sq"] * z0, t1 + I["sq"] * z1]
        if self.name == "bearings4":
            z = list(s.normal2(0)) + list(s.normal2(1))
            if first:
                return [E(I["mu"][k]) + I["s"][k] * z[k] for k in range(4)]
            return [(E.lift(xp[0]) + xp[2]) + I["sp"] * z[0], (E.lift(xp[1]) + xp[3]) + I["sp"] * z[1],
                    E.lift(xp[2]) + I["sv"] * z[2], E.lift(xp[3]) + I["sv"] * z[3]]
        if self.name == "sv1":
            z0, _ = s.normal2(0)
            mu, phi, sg = I["mu"], I["phi"], I["sigma"]
            if first:                                                        # the stationary law N(mu, sigma^2 / (1 - phi^2))
                if "sd0" not in self._c:
                    self._c["sd0"] = E(sg) / (1.0 - E(phi) * phi).sqrt()
                return [E(mu) + self._c["sd0"] * z0]
            return [(E(mu) + E(phi) * (E.lift(xp[0]) - mu)) + sg * z0]
        if self.name == "object_motion":
            w = s.words(0)
            z0, _ = s.normal2(1)
            pm, py = (0.0, 0.0) if first else (_f(xp[0]), xp[1])                  # (the indicator is exact; xp may come as E: pf_introduce's chain)
            mv = u52(w[0], w[1]) < (I["p_stay"] if pm != 0.0 else I["p_start"])
            return self._om_row(mv, py, obs, z0)
        if self.name == "line_model":
            w = s.words(0)
            slopes = I["slopes"]
            slope = float(slopes[mulhi64(u64(w[0], w[1]), len(slopes))]) if first else xp[0]      # uniform_discrete
            out = obs[1] != 0.0 and u52(w[2], w[3]) < I["p_out"]                                  # bernoulli(p_out); no step at x_t = 0
            return [E.lift(slope), E(1.0 if out else 0.0)]
        raise ValueError(self.name)

    def _om_row(self, moving, py, obs, z0):
        vel = obs[1] if moving else 0.0
        return [E(1.0 if moving else 0.0), (E.lift(py) + vel) + self.info["sy"] * z0]

    # ---- log p(y_t | x_t)
    def loglik(self, x, obs, wraps=None):
        I = self.info
        if self.name == "lgssm2":
            return normal2_logpdf(obs[0], obs[1], x[0], x[1], I["sr"], self.sc("sr"))
        if self.name == "bearings4":
            r = E(obs[0]) - atan2(x[1], x[0])
            r = self.wrap(r, wraps)
            inv, c = self.sc("sb")
            z = r * inv
            return -(z * z).scale2(-1) - c
        if self.name == "sv1":
            # y ~ normal(0, exp(h / 2)): -y^2 exp(-h) / 2 - h / 2 - log(2 pi)/2
            y, h = E(obs[0]), E.lift(x[0])
            return (-((y * y) * (-h).exp()).scale2(-1) - h.scale2(-1)) - HL2P
        if self.name == "object_motion":
            return normal_logpdf(obs[0], x[1], I["sobs"], self.sc("sobs"))
        if self.name == "line_model":
            if obs[1] == 0.0:
                return E(0.0)
            out = _f(x[1]) != 0.0
            return normal_logpdf(obs[0], E(obs[1]) * x[0], I["s_out"] if out else I["s_in"], self.sc("s_out" if out else "s_in"))
        raise ValueError(self.name)

    # ---- log f(x_t = x | x_{t-1} = xp): the transition density of the Gen program
    def logtrans(self, xp, x, obs, full=False):
        """log f(x | xp) up to terms free of xp (ancestor sampling, backward simulation and smoothing normalise over xp: they cancel): the
        value of the definition and the bound of a Float64 evaluation that divides the residuals by sigma (one rounding each; lgssm2
        multiplies by 1 / sq as models.py packs it) and drops the normalising constants of the normals.  object_motion keeps the Bernoulli
        term of `moving`: it depends on xp.  line_model: the slope persists -- exactly 0, or -Inf where xp holds another slope (the outlier's
        probability is free of xp).  `full`: the complete Gen log-density, constants included (normal_logpdf, log_bernoulli)."""
        I = self.info
        if full:
            return self._logtrans_full(xp, x, obs)
        nq = lambda r, sigma: r / E(sigma)                                                      # (x - mean) / sigma
        if self.name == "lgssm2":
            A = I["A"]
            if "inv_sq" not in self._c:
                self._c["inv_sq"] = 1.0 / E(I["sq"])
            inv = self._c["inv_sq"]
            t0 = E(float(A[0][0])) * xp[0] + E(float(A[0][1])) * xp[1]
            t1 = E(float(A[1][0])) * xp[0] + E(float(A[1][1])) * xp[1]
            a0, a1 = (E(x[0]) - t0) * inv, (E(x[1]) - t1) * inv
            return -(a0 * a0 + a1 * a1).scale2(-1)
        if self.name == "sv1":
            z = nq(E(x[0]) - (E(I["mu"]) + E(I["phi"]) * (E(xp[0]) - I["mu"])), I["sigma"])
            return -(z * z).scale2(-1)
        if self.name == "bearings4":
            z0, z1 = nq(E(x[0]) - (E(xp[0]) + xp[2]), I["sp"]), nq(E(x[1]) - (E(xp[1]) + xp[3]), I["sp"])
            z2, z3 = nq(E(x[2]) - xp[2], I["sv"]), nq(E(x[3]) - xp[3], I["sv"])
            return -((z0 * z0 + z1 * z1) + (z2 * z2 + z3 * z3)).scale2(-1)
        if self.name == "object_motion":
            mv = x[0] != 0.0
            lp = log_bernoulli(I["p_stay"] if xp[0] != 0.0 else I["p_start"], mv)
            z = nq(E(x[1]) - (E(xp[1]) + (obs[1] if mv else 0.0)), I["sy"])
            return lp + (-(z * z).scale2(-1))
        if self.name == "line_model":
            return E(0.0) if xp[0] == x[0] else E(-M.inf)
        raise ValueError(self.name)

    def _logtrans_full(self, xp, x, obs):
        I = self.info
        if self.name == "lgssm2":
            mu0, mu1 = self._prior_mean(False, xp)
            return normal2_logpdf(x[0], x[1], mu0, mu1, I["sq"], self.sc("sq"))
        if self.name == "sv1":
            return normal_logpdf(x[0], E(I["mu"]) + E(I["phi"]) * (E(xp[0]) - I["mu"]), I["sigma"], self.sc("sigma"))
        if self.name == "bearings4":
            return (normal2_logpdf(x[0], x[1], E(xp[0]) + xp[2], E(xp[1]) + xp[3], I["sp"], self.sc("sp"))
                    + normal2_logpdf(x[2], x[3], E(xp[2]), E(xp[3]), I["sv"], self.sc("sv")))
        if self.name == "object_motion":
            mv = x[0] != 0.0
            lp = log_bernoulli(I["p_stay"] if xp[0] != 0.0 else I["p_start"], mv)
            return lp + normal_logpdf(x[1], E(xp[1]) + (obs[1] if mv else 0.0), I["sy"], self.sc("sy"))
        if self.name == "line_model":                                        # slope: a point mass on xp's; outlier ~ bernoulli(p_out) once a step has happened
            if xp[0] != x[0]:
                return E(-M.inf)
            return log_bernoulli(I["p_out"], x[1] != 0.0) if obs[1] != 0.0 else E(0.0)
        raise ValueError(self.name)

    @staticmethod
    def wrap(r, wraps=None):
        """the bearing residual wrapped to (-pi, pi].  wraps = 1: ONE subtraction / addition of 2 pi, which is what the spec does (enough
        for |r| <= 3 pi); None: as many as needed.  The Float64 PI / TWOPI differ from pi / 2 pi by < 1.3e-16 / 2.5e-16: counted."""
        k = M.ceil((r.v - PI) / (2 * PI))
        if wraps is not None:
            k = max(-wraps, min(wraps, k))
        if k == 0:
            return r
        return E(r.v - 2 * PI * k, r.e + float(abs(k)) * 2.5e-16 + 0.5 * _ulp(r.v - 2 * PI * k, r.e))

    # ---- the LG-SSM's locally optimal proposal, from Gaussian conjugacy: prior N(mu, s^2 I), y = x + N(0, sr^2 I)
    #      => x | y ~ N(mu + s^2 / (s^2 + sr^2) (y - mu), s^2 sr^2 / (s^2 + sr^2) I)
    def _lo(self, first):
        key = ("lo", first)
        if key not in self._c:
            s, sr = E(self.info["s0"] if first else self.info["sq"]), E(self.info["sr"])
            s2, r2 = s * s, sr * sr
            gain = s2 / (s2 + r2)
            sd = ((s2 * r2) / (s2 + r2)).sqrt()
            self._c[key] = (gain, sd, _sigma_consts(sd), _sigma_consts(s))
        return self._c[key]

    def _prior_mean(self, first, xp):
        if first:
            return E(0.0), E(0.0)
        A = self.info["A"]
        return (E(float(A[0][0])) * xp[0] + E(float(A[0][1])) * xp[1], E(float(A[1][0])) * xp[0] + E(float(A[1][1])) * xp[1])

    def proposal_weight(self, first, xp, obs, x):
        """[log p(x | x') + log p(y | x)] - log q(x | x', y)"""
        if self.name == "line_model":
            raise ValueError
        gain, sd, csd, cs = self._lo(first)
        mu0, mu1 = self._prior_mean(first, xp)
        m0, m1 = mu0 + gain * (E(obs[0]) - mu0), mu1 + gain * (E(obs[1]) - mu1)
        lt = normal2_logpdf(x[0], x[1], mu0, mu1, None, cs)
        lq = normal2_logpdf(x[0], x[1], m0, m1, None, csd)
        return (lt + self.loglik(x, obs)) - lq

    def propose(self, first, xp, obs, s):
        """the native proposal of pf_initialize / pf_update with a proposal: (new latent, log weight)"""
        if self.name == "line_model":
            # slope ~ uniform_discrete(0, 0) at the first step, outlier ~ bernoulli(0.0) (test/initialize.jl:16-19, test/update.jl:42-43):
            # deterministic, proposal score 0; weight = log p(slope = 0) [first] + log p(outlier = false) + log p(y | .)
            x = [E(0.0 if first else xp[0]), E(0.0)]
            w = -E(float(len(self.info["slopes"]))).log(1.0) if first else E(0.0)
            if obs[1] != 0.0:
                w = (w + log_bernoulli(self.info["p_out"], False)) + self.loglik(x, obs)
            return x, w
        gain, sd, _, _ = self._lo(first)
        z0, z1 = s.normal2(0)
        mu0, mu1 = self._prior_mean(first, xp)
        m0, m1 = mu0 + gain * (E(obs[0]) - mu0), mu1 + gain * (E(obs[1]) - mu1)
        return [m0 + sd * z0, m1 + sd * z1], None        # the weight is a function of the STORED row: proposal_weight

    def marginal_loglik(self, first, xp, obs):
        """log N(y; A x', (sq^2 + sr^2) I) (first: N(y; 0, (s0^2 + sr^2) I)): what the locally optimal proposal's weight must equal for ANY x"""
        s, sr = mpf(self.info["s0"] if first else self.info["sq"]), mpf(self.info["sr"])
        v = s * s + sr * sr
        if first:
            mu = (mpf(0), mpf(0))
        else:
            A = self.info["A"]
            mu = (mpf(float(A[0][0])) * mpf(xp[0]) + mpf(float(A[0][1])) * mpf(xp[1]), mpf(float(A[1][0])) * mpf(xp[0]) + mpf(float(A[1][1])) * mpf(xp[1]))
        d0, d1 = mpf(obs[0]) - mu[0], mpf(obs[1]) - mu[1]
        return -(d0 * d0 + d1 * d1) / (2 * v) - M.log(v) - M.log(2 * PI)

    # ---- stratified generate / update: the stratified discrete choice is constrained to `value`; returns (row, log p(choice = value | .))
    def sample_stratum(self, first, xp, obs, value, s):
        I = self.info
        if self.name == "object_motion":
            z0, _ = s.normal2(1)
            pm, py = (0.0, 0.0) if first else (xp[0], xp[1])
            mv = value != 0.0
            return self._om_row(mv, py, obs, z0), log_bernoulli(I["p_stay"] if pm != 0.0 else I["p_start"], mv)
        if self.name == "line_model":
            w = s.words(0)
            if first:                                                    # strata over `slope`; the outlier is sampled as usual
                out = obs[1] != 0.0 and u52(w[2], w[3]) < I["p_out"]
                return [E(value), E(1.0 if out else 0.0)], -E(float(len(I["slopes"]))).log(1.0)
            return [E(xp[0]), E(1.0 if value != 0.0 else 0.0)], log_bernoulli(I["p_out"], value != 0.0)      # strata over the step's outlier
        raise ValueError(self.name)

    def propose_stratum(self, obs, value):
        """stratified initialise with line_model's fixed proposal (initialize.jl:111-129 as test/initialize.jl:66-90 uses it)"""
        x = [E(value), E(0.0)]
        w = -E(float(len(self.info["slopes"]))).log(1.0)
        if obs[1] != 0.0:
            w = (w + log_bernoulli(self.info["p_out"], False)) + self.loglik(x, obs)
        return x, w

    # ---- move proposals: (new latent, rel_weight = weight - fwd_score + bwd_score, rejuvenate.jl:134-148)
    def move_propose(self, first, xp, x, obs, s, q=None):
        if self.name == "lgssm2":
            xn, _ = self.propose(first, xp, obs, s)
            return xn, None
        if self.name == "line_model":
            w = s.words(0)
            if obs[1] == 0.0:
                return [E.lift(x[0]), E(0.0)], E(0.0)
            on, oo = u52(w[2], w[3]) < q, _f(x[1]) != 0.0
            xn = [E.lift(x[0]), E(1.0 if on else 0.0)]
            wn = log_bernoulli(self.info["p_out"], on) + self.loglik(xn, obs)
            wo = log_bernoulli(self.info["p_out"], oo) + self.loglik(x, obs)
            return xn, ((wn - wo) - log_bernoulli(q, on)) + log_bernoulli(q, oo)
        raise ValueError(self.name)


def stratum_of(ref: Ref, i, n, K, interleaved, seed, gid, epoch, tag):
    """stratified_map! (src/utils.jl:29-55 of the reference): block size B = n div K; particle i < K B belongs to stratum i div B
    (contiguous) or i mod K (interleaved); the others draw one uniformly, from words (0,1) of the block after the model's own"""
    B = n // K
    if i < K * B:
        return i % K if interleaved else i // B
    w = block(seed, gid, ref.nblk, epoch, tag)
    return mulhi64(u64(w[0], w[1]), K)


# ------------------------------------------------------------------------------------------- the operations, per particle
# Each returns (row, weight): `row` the expected new latent columns (list of E), `weight` a function stored_row -> E giving the
# expected log-weight INCREMENT as the density of the row actually stored (so a rounding of the row is not counted twice).
def initialize(ref, seed, epoch, gid, obs):
    return ref.sample(True, None, obs, Stream(seed, gid, epoch, TAG_INIT)), lambda x: ref.loglik(x, obs)


def update(ref, seed, epoch, gid, xp, obs):
    return ref.sample(False, xp, obs, Stream(seed, gid, epoch, TAG_UPDATE)), lambda x: ref.loglik(x, obs)


def update_proposal(ref, seed, epoch, gid, xp, obs, first=False):
    x, w = ref.propose(first, xp, obs, Stream(seed, gid, epoch, TAG_INIT if first else TAG_UPDATE))
    if w is not None:
        return x, lambda _x: w
    return x, lambda xs: ref.proposal_weight(first, xp, obs, xs)


def _log_n(K):
    return E(float(K)).log(2.0)         # the caller's + log n_strata, by the spec's log_


def update_stratified(ref, seed, epoch, gid, i, n, xp, obs, values, interleaved, first=False):
    tag = TAG_INIT if first else TAG_UPDATE
    v = values[stratum_of(ref, i, n, len(values), interleaved, seed, gid, epoch, tag)]
    x, lp = ref.sample_stratum(first, xp, obs, v, Stream(seed, gid, epoch, tag))
    return x, lambda xs: (lp + ref.loglik(xs, obs)) + _log_n(len(values))


def initialize_stratified(ref, seed, epoch, gid, i, n, obs, values, interleaved, proposal=False):
    if not proposal:
        return update_stratified(ref, seed, epoch, gid, i, n, None, obs, values, interleaved, first=True)
    v = values[stratum_of(ref, i, n, len(values), interleaved, seed, gid, epoch, TAG_INIT)]
    x, w = ref.propose_stratum(obs, v)
    return x, lambda _x: w + _log_n(len(values))


def move_reweight_iter(ref, seed, epoch, gid, it, first, xp, x, obs, q=None, proposal=False):
    """one iteration of pf_move_reweight!: (proposed latent, rel_weight as a function of the stored proposal)"""
    s = Stream(seed, gid, epoch, TAG_REWEIGHT, it * ref.nblk)
    if not proposal:                                 # move_reweight(trace, selection): regenerate from the model; weight = log p(y|x') - log p(y|x)
        xn = ref.sample(first, xp, obs, s)
        return xn, lambda xs: ref.loglik(xs, obs) - ref.loglik(x, obs)
    xn, rw = ref.move_propose(first, xp, x, obs, s, q)
    if rw is not None:
        return xn, lambda _x: rw
    return xn, lambda xs: ref.proposal_weight(first, xp, obs, xs) - ref.proposal_weight(first, xp, obs, x)


def mh_move(ref, seed, epoch, gid, it, first, xp, x, obs, q=None, proposal=False):
    """one iteration of Gen.mh under pf_move_accept!: (proposed latent, alpha as a function of the stored proposal, log u).  The accept
    uniform is words (0,1) of the block after the proposal's own: block blk0 + NBLK of the move stream, blk0 = it (NBLK + 1)."""
    blk0 = it * (ref.nblk + 1)
    s = Stream(seed, gid, epoch, TAG_MOVE, blk0)
    if not proposal:
        xn = ref.sample(first, xp, obs, s)
        alpha = lambda xs: ref.loglik(xs, obs) - ref.loglik(x, obs)
    else:
        xn, rw = ref.move_propose(first, xp, x, obs, s, q)
        if rw is not None:
            alpha = lambda _x: rw
        else:
            alpha = lambda xs: ref.proposal_weight(first, xp, obs, xs) - ref.proposal_weight(first, xp, obs, x)
    w = s.words(ref.nblk)
    return xn, alpha, E(u52(w[0], w[1])).log(2.0)
