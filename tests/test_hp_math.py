"""The math spec against mpmath, on BOTH CPU builds: the oracle's copy (oracle/gpf_oracle_math.h through o_math_vec) and the
host build of the kernels' own header (csrc/gpf_math.hpp through gpf_host_math).  Accuracy at the points where such functions go wrong --
every range-reduction switch, the domain's ends, the table boundaries -- to the bounds the project claims (exp_, log_ 2 ulp; sincos2pi
1e-15 absolute; atan2_ 4 ulp; neglog_u52 1e-11 absolute); the behaviour OUTSIDE the domain pinned bit for bit, row by row of the table in
DESIGN.md 3.2; and every call site of log_ shown to stay inside "positive normal"."""
import math

import numpy as np
import pytest

import hp_checks as hc
import hp_reference as hp

M, mpf = hp.M, hp.mpf
BUILDS = ["oracle", "host"]


def call(g, o, build, which, a, b=None):
    a = np.ascontiguousarray(a, np.float64)
    b = a if b is None else np.ascontiguousarray(b, np.float64)
    o1, o2 = np.empty_like(a), np.zeros_like(a)
    if build == "oracle":
        o.lib().o_math_vec(which, a, b, a.size, o1, o2)
    else:
        C = g._lib.C
        pd = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))                  # noqa: E731
        g._lib.load().gpf_host_math(which, pd(a), pd(b), a.size, pd(o1), pd(o2))
    return o1, o2


def ulps(got, want_mp):
    """|got - want| in ulps of the correctly rounded want, per element (want: mpmath values)"""
    out = np.empty(len(got))
    for i, (gv, w) in enumerate(zip(got, want_mp)):
        wr = float(w)
        if wr == 0.0:
            out[i] = 0.0 if gv == 0.0 else math.inf
        else:
            out[i] = float(abs(mpf(float(gv)) - w) / mpf(math.ulp(wr)))
    return out


def report(name, x, err, bound):
    i = int(np.argmax(err))
    print(f"{name}: max error {err[i]:.3g} (bound {bound}) at {x[i]!r}, {len(err)} points")
    assert err[i] <= bound, (name, x[i], err[i])


@pytest.mark.parametrize("build", BUILDS)
def test_exp(g, o, build):
    x = hc.exp_points(np.random.default_rng(1))
    got, _ = call(g, o, build, 0, x)
    report("exp_", x, ulps(got, [M.exp(mpf(float(v))) for v in x]), 2.0)


@pytest.mark.parametrize("build", BUILDS)
def test_log(g, o, build):
    x = hc.log_points(np.random.default_rng(2))
    assert (x >= hc.DBL_MIN).all() and np.isfinite(x).all()
    got, _ = call(g, o, build, 1, x)
    report("log_", x, ulps(got, [M.log(mpf(float(v))) for v in x]), 2.0)


@pytest.mark.parametrize("build", BUILDS)
def test_sincos2pi(g, o, build):
    u = hc.sincos_points(np.random.default_rng(3))
    s, c = call(g, o, build, 2, u)
    es, ec, circ = np.empty(u.size), np.empty(u.size), np.empty(u.size)
    for i, v in enumerate(u):
        a = 2 * hp.PI * mpf(float(v))
        es[i], ec[i] = abs(mpf(float(s[i])) - M.sin(a)), abs(mpf(float(c[i])) - M.cos(a))
        circ[i] = abs(mpf(float(s[i])) ** 2 + mpf(float(c[i])) ** 2 - 1)
    report("sin(2 pi u)", u, es, 1e-15)
    report("cos(2 pi u)", u, ec, 1e-15)
    # two values within 1e-15 of a point of the unit circle: |s^2 + c^2 - 1| <= 2 (|sin| + |cos|) 1e-15 + 2e-30 <= 2 sqrt(2) 1e-15 + 2e-30
    report("sin^2 + cos^2 - 1", u, circ, 2 * math.sqrt(2) * 1e-15 + 2e-30)


@pytest.mark.parametrize("build", BUILDS)
def test_atan2(g, o, build):
    y, x = hc.atan2_points(np.random.default_rng(4))
    got, _ = call(g, o, build, 3, y, x)
    report("atan2_", list(zip(y, x)), ulps(got, [M.atan2(mpf(float(a)), mpf(float(b))) for a, b in zip(y, x)]), 4.0)


@pytest.mark.parametrize("build", BUILDS)
def test_neglog_u52(g, o, build):
    U = hc.neglog_points(np.random.default_rng(5))
    got, _ = call(g, o, build, 7, U.view(np.float64))
    k = U >> np.uint64(12)
    err = np.array([abs(mpf(float(gv)) + M.log((mpf(int(kk)) + 0.5) / 2 ** 52)) for gv, kk in zip(got, k)], dtype=float)
    report("neglog_u52", U, err, 1e-11)
    assert (got >= 0.0).all()


def test_builds_agree_on_every_edge_vector(g, o):
    rng = [np.random.default_rng(s) for s in (1, 2, 3, 4, 5)]
    y, x = hc.atan2_points(rng[3])
    for which, a, b in [(0, hc.exp_points(rng[0]), None), (1, hc.log_points(rng[1]), None), (2, hc.sincos_points(rng[2]), None), (3, y, x),
                        (7, hc.neglog_points(rng[4]).view(np.float64), None)]:
        r, h = call(g, o, "oracle", which, a, b), call(g, o, "host", which, a, b)
        assert hc.bits_equal_nan(r[0], h[0]).all() and hc.bits_equal_nan(r[1], h[1]).all(), which


# ------------------------------------------------------------------------------------------- the domain is a tested statement
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("row", range(len(hc.DOMAIN_TABLE)))
def test_domain_table(g, o, build, row):
    """one row of the table "input class -> result" of DESIGN.md 3.2, exactly"""
    fn, args, want = hc.DOMAIN_TABLE[row]
    o1, o2 = call(g, o, build, hc.WHICH[fn], [args[0]], [args[-1]])
    if fn == "sincos":
        assert hc.same_bits(o1[0], want[0]) and hc.same_bits(o2[0], want[1]), (fn, args, o1[0], o2[0], want)
    else:
        assert hc.same_bits(o1[0], want), (fn, args, float(o1[0]).hex(), want)


def test_exp_cutoffs_against_the_true_thresholds(g, o):
    """what the cut-offs cost, as a statement: e^x is a NORMAL number for -708.396 < x < -708 (returned: 0) and FINITE for 709 < x <= 709.78
    (returned: +Inf).  Between the cut-offs the result is within 2 ulp (test_exp); a caller needing the margins must not use exp_."""
    assert M.exp(mpf(-708.39)) > mpf(hc.DBL_MIN) and M.exp(mpf(709.78)) < mpf(hc.DBL_MAX)
    assert M.exp(mpf(-708.4)) < mpf(hc.DBL_MIN) and M.exp(mpf(709.79)) > mpf(hc.DBL_MAX)
    for build in BUILDS:
        got, _ = call(g, o, build, 0, [-708.39, 709.78, -708.0, 709.0])
        assert got[0] == 0.0 and got[1] == math.inf and got[2] >= hc.DBL_MIN and got[3] < math.inf


# ------------------------------------------------------------------------------------------- log_'s call sites stay inside its domain
def _positive_normal(x):
    return np.isfinite(x).all() and (np.asarray(x) >= hc.DBL_MIN).all()


@pytest.mark.parametrize("build", BUILDS)
def test_log_call_site_arguments_are_positive_normal(g, o, build):
    """every argument class a call site can produce: u52 values (Box-Muller, the MH accept, gamma_tile's uniform), (double)n for a count
    n >= 1 (log N, log n_strata, the resize ratios, a block's particle count, the optimal resize's a), S 2^-K for S >= 1, K <= 52 (lse_from,
    behind its flag check), and gamma_tile's v > 0 (v = (1 + c x)^3 with 1 + c x > 0 checked first)"""
    u = hc.u52_extremes()
    counts = np.concatenate([np.arange(1.0, 4097.0), 2.0 ** np.arange(0, 63), [2.0 ** 31 - 1, 2.0 ** 62 - 1024]])
    sums = np.array([float(S) * 2.0 ** -K for K in range(31, 53) for S in (1, 2, 3, 2 ** K, 2 ** 62 - 1)])
    for x in (u, counts, sums):
        assert _positive_normal(x)
        got, _ = call(g, o, build, 1, x)
        report("log_ at call-site arguments", x, ulps(got, [M.log(mpf(float(v))) for v in x]), 2.0)
    assert call(g, o, build, 1, [1.0])[0][0] == 0.0                          # a one-particle filter: log N = 0 exactly
    # gamma_tile: 1 + c x > 0 in Float64 means >= 2^-53 (c x is a Float64 >= -1 + 2^-53), so v = (v1 v1) v1 >= 2^-159: normal
    assert (2.0 ** -53 * 2.0 ** -53) * 2.0 ** -53 >= hc.DBL_MIN


def test_optimal_resize_counts_reach_log_as_positive_integers(g, o):
    """pf_resize(state, n, "optimal") down to 1 and 2 particles: opt_a = n - d >= 1 and opt_B > 0 whatever the weights"""
    m = g.models.lgssm2()
    y = g.models.simulate(m, 1)[0]
    for n_old, n_new, what, lw in hc.optimal_resize_cases():
        f = o.OracleFilter(m.model_id, m.params, n_old, 3).initialize(y)
        f.lw = lw.copy()
        f.resize(n_new, "optimal", check=False)
        assert f.n == n_new and f.lw.size == n_new
        hc.check_no_log_garbage(f.lw, lw)


def test_blockwise_resample_with_a_dead_block(g, o):
    """one block's weights all -Inf: that block takes the documented uniform fallback (its weights stay -Inf: logsumexp = -Inf), every
    other block's weights are its finite block average; no log_ of a zero count anywhere"""
    m = g.models.lgssm2()
    y = g.models.simulate(m, 1)[0]
    f = o.OracleFilter(m.model_id, m.params, 64, 3).initialize(y)
    lw = f.lw.copy(); lw[16:32] = -np.inf
    f.lw = lw.copy()
    o.resample_blocks(f, 16, "multinomial", check=False)
    out = f.lw
    assert (out[16:32] == -np.inf).all()
    for a in (0, 32, 48):
        assert np.isfinite(out[a:a + 16]).all() and (out[a:a + 16] == out[a]).all()
        assert abs(out[a] - (hc.lse(lw[a:a + 16]) - math.log(16))) < 1e-12
    assert (1 <= f.parents).all() and (f.parents <= 16).all()


def test_bearings_density_is_blind_to_the_sign_of_zero(g, o):
    """atan2_(-0, x < 0) = +pi (IEEE: -pi).  The bearing is wrapped, so both are the same angle: the density of a particle exactly on the
    negative x axis does not depend on the sign of its zero, and is the mpmath density"""
    m = g.models.bearings4()
    ref = hp.Ref(m)
    W = m.row_width(True)
    rows = np.zeros((2, W)); rows[:, 0] = -2.0; rows[0, 1], rows[1, 1] = 0.0, -0.0
    for yobs in (3.0, -3.0, 0.5):
        out = np.empty(2)
        o.lib().o_loglik_rows(m.model_id, np.ascontiguousarray(m.params), rows, W, 2, np.array([yobs]), out)
        assert out[0] == out[1]
        d, t = hp.differs(out[0], ref.loglik([-2.0, 0.0, 0.0, 0.0], [yobs]))
        assert d <= t
