"""The CPU oracle's five models -- sampled values, densities, proposals, stratified weights, both moves, per-block parameters -- against
tests/hp_reference.py: an mpmath restatement of the model definitions that reads only the natural parameters and predicts every
particle's row from (seed, particle id, epoch, previous row).  Every compared value carries its own derived bound (hp_reference's error
propagation); the median bound of every case is asserted below 1e-12.  tests/test_gpu_hp.py runs the same checks on the device.

What the cases catch that "device == oracle" cannot: anything the two twins have in common -- a wrong packed constant, a wrong sign or
operand in a transition, a dropped density term, a bearing wrapped the wrong way, an accept uniform read from the wrong words."""
import math

import numpy as np
import pytest

import hp_checks as hc
import hp_reference as hp
from hp_reference import E

MODELS = ["lgssm2", "bearings4", "sv1", "object_motion", "line_model"]
N, SEED = 2000, 20240917


def _run(g, o, name, n=N, seed=SEED, **kw):
    m = getattr(g.models, name)(**kw) if kw else g.models.by_name(name)
    return hc.Run(hc.OracleAdapter(g, o, m, n, seed), m, n, seed), hc.case_data(g, m, 4)


def drive_filter(r, ys):
    """initialize, then three (resample, update): the ancestors are not the identity"""
    r.initialize(ys[0])
    for t, method in zip((1, 2, 3), ("multinomial", "residual", "stratified")):
        r.resample(method)
        r.update(ys[t])


def test_reference_stream_known_answers(o):
    """the reference's own Philox4x32-10 on the Random123 known-answer vectors (the three of tests/test_oracle_math.py), and its Box-Muller
    against the oracle's normal2 within the derived bound"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert hp.philox4x32_10(*ctr, *key) == want
    import ctypes as C
    seed = (0x1234 << 32) | 0x9abcdef1                       # both key words in use
    for gid in range(300):
        z0, z1 = C.c_double(), C.c_double()
        o.lib().o_normal2_d(seed, gid, 2, 5, hp.TAG_MOVE, C.byref(z0), C.byref(z1))
        w0, w1 = hp.box_muller(hp.block(seed, gid, 2, 5, hp.TAG_MOVE))
        for got, want in ((z0.value, w0), (z1.value, w1)):
            d, t = hp.differs(got, want)
            assert d <= t and t < 1e-14, (gid, got, want)
        assert o.lib().o_u52_d(seed, gid, 2, 5, hp.TAG_MOVE) == hp.u52(*hp.block(seed, gid, 2, 5, hp.TAG_MOVE)[:2])


@pytest.mark.parametrize("name", MODELS)
def test_initialize_and_updates(g, o, name):
    r, ys = _run(g, o, name)
    drive_filter(r, ys)


def drive_lgssm2_proposal(r, ys):
    r.initialize(ys[0], proposal=True)
    r.check_conjugacy(None, None, first=True)
    for t in (1, 2):
        r.resample("multinomial")
        rows0, lw0 = r.a.rows, r.a.lw
        r.update(ys[t], proposal=True)
        r.check_conjugacy(rows0, lw0, first=False)


def test_lgssm2_locally_optimal_proposal_and_conjugacy(g, o):
    """rows and weights of the native proposal, from the conjugacy formulas; and log p(x|x') + log p(y|x) - log q(x) = log N(y; A x',
    (sq^2 + sr^2) I) for every particle: all twelve packed proposal constants without reading one"""
    r, ys = _run(g, o, "lgssm2")
    drive_lgssm2_proposal(r, ys)
    r, ys = _run(g, o, "lgssm2", theta=0.7, rho=0.9, sq=0.3, sr=0.05, s0=2.5, seed=5)
    drive_lgssm2_proposal(r, ys)


def drive_line_proposal(r, ys):
    r.initialize(ys[0], proposal=True)
    r.update(ys[1], proposal=True)
    r.initialize(np.array([0.0, 0.0]), proposal=True)          # model args (0,): no step yet, weight = log(1/5)
    r.update(ys[0], proposal=True)


def test_line_model_fixed_proposal(g, o):
    r, ys = _run(g, o, "line_model", n=500)
    drive_line_proposal(r, ys)


STRATA_CASES = [("object_motion", 2000, "contiguous"), ("object_motion", 1999, "interleaved"), ("line_model", 2000, "contiguous"),
                ("line_model", 1998, "interleaved")]


def drive_strata(r, ys, name, layout):
    """stratified initialise / update: the increment includes log n_strata; 1999 / 1998 particles leave a remainder that draws its stratum"""
    first = [0.0, 1.0] if name == "object_motion" else [-2.0, -1.0, 0.0, 1.0, 2.0]
    r.initialize(ys[0], strata=first, layout=layout)
    r.update(ys[1], strata=[0.0, 1.0], layout=layout)
    r.resample("multinomial")
    r.update(ys[2], strata=[1.0, 0.0], layout="interleaved" if layout == "contiguous" else "contiguous")


@pytest.mark.parametrize("name,n,layout", STRATA_CASES)
def test_stratified(g, o, name, n, layout):
    r, ys = _run(g, o, name, n=n)
    drive_strata(r, ys, name, layout)


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_line_model_stratified_with_proposal(g, o, layout):
    r, ys = _run(g, o, "line_model", n=1003)
    r.initialize(ys[0], proposal=True, strata=[-2.0, -1.0, 0.0, 1.0, 2.0], layout=layout)


def _moves_q(g, name, proposal):
    if not proposal:
        return None
    return () if name == "lgssm2" else g.outlier_propose(0.9).params


MOVE_CASES = [(m, False) for m in MODELS] + [("lgssm2", True), ("line_model", True)]


def drive_reweight(r, ys, q):
    r.initialize(ys[0])
    r.reweight(1, q)                              # before any update: the move regenerates from the prior
    r.update(ys[1])
    r.reweight(1, q)
    r.resample("multinomial")
    r.update(ys[2])
    r.reweight(2, q)


@pytest.mark.parametrize("name,proposal", MOVE_CASES)
def test_move_reweight(g, o, name, proposal):
    """the weight increment is the reference's sum of relative weights (for lgssm2's Gibbs move: 0 within the bound)"""
    r, ys = _run(g, o, name, n=1000)
    drive_reweight(r, ys, _moves_q(g, name, proposal))


def drive_mh(r, ys, q):
    r.initialize(ys[0])
    left_out = r.mh(1, q)
    r.update(ys[1])
    left_out += r.mh(1, q)
    r.resample("multinomial")
    r.update(ys[2])
    return left_out + r.mh(2, q)


@pytest.mark.parametrize("name,proposal", MOVE_CASES)
def test_mh_move(g, o, name, proposal):
    """per particle: the stored row is the proposal iff log u < alpha, n_accepted is the count; no committed case leaves a particle out"""
    r, ys = _run(g, o, name, n=1000)
    assert drive_mh(r, ys, _moves_q(g, name, proposal)) == 0


def drive_move_then_update(r, ys):
    r.initialize(ys[0])
    r.update(ys[1])
    r.resample("multinomial")
    return r.mh_then_update(ys[2]) + r.mh_then_update(ys[3], n_iters=2)


@pytest.mark.parametrize("name", ["lgssm2", "bearings4", "object_motion"])
def test_move_then_update(g, o, name):
    """pf_rejuvenate followed at once by pf_update (the pair the device fuses into one kernel): same expected rows as the separate calls"""
    r, ys = _run(g, o, name, n=1000)
    assert drive_move_then_update(r, ys) == 0


def drive_step_ess(r, ys):
    r.initialize(ys[0])
    return [r.step_ess(ys[t]) for t in (1, 2, 3)]


def test_step_ess_bearings(g, o):
    """three iterations of the README loop (resample below ESS = N/2, update) in one call each, on the model with the sharpest likelihood"""
    r, ys = _run(g, o, "bearings4")
    assert any(drive_step_ess(r, ys))


# ------------------------------------------------------------------------------------------- rows placed by hand
def _loglik(o, m, rows, obs):
    W = m.row_width(True)
    buf = np.zeros((len(rows), W))
    buf[:, :m.dim] = rows
    out = np.empty(len(rows))
    o.lib().o_loglik_rows(m.model_id, np.ascontiguousarray(m.params), buf, W, len(rows), np.ascontiguousarray(obs, np.float64), out)
    return out


def _against_ref(o, m, rows, obs, wraps=None):
    got, ref, v = _loglik(o, m, rows, obs), hp.Ref(m), hc.Violations()
    for i, x in enumerate(rows):
        v.value(f"{m.name} loglik{tuple(x)} obs {tuple(obs)}", i, got[i], ref.loglik(list(x), obs, wraps))
    v.finish(f"{m.name} placed rows")
    return got


def test_bearings_on_the_branch_cut(g, o):
    """particles on the negative x axis (py = +-tiny, +-0) with the observation at +-(pi - 1e-4): the wrap fires in both directions.
    atan2_(-0, x < 0) returns +pi where IEEE atan2 returns -pi: the wrapped residual is the same, so is the density."""
    m = g.models.bearings4()
    tiny = 5e-324
    rows = [(-1.5, py, 0.0, 0.0) for py in (tiny, -tiny, 0.0, -0.0, 1e-300, -1e-300, 1e-9, -1e-9)]
    for y in (math.pi - 1e-4, -(math.pi - 1e-4)):
        got = _against_ref(o, m, rows, [y])
        assert got[2] == got[3]                                             # each sign of zero: one density
    # ... which is the density of the definition whichever of -pi / +pi the bearing is taken to be
    ref = hp.Ref(m)
    inv_sb = 1 / hp.mpf(m.info["sb"])
    for y in (math.pi - 1e-4, -(math.pi - 1e-4)):
        vals = [hp.Ref.wrap(E(hp.mpf(y) - b)).v for b in (hp.PI, -hp.PI)]
        assert abs(abs(vals[0]) - abs(vals[1])) < hp.mpf(2) ** -150
        want = -(vals[0] * inv_sb) ** 2 / 2 - hp.M.log(hp.mpf(m.info["sb"])) - hp.HALF_LOG_2PI
        assert abs(ref.loglik([-1.5, -0.0, 0.0, 0.0], [y]).v - want) < hp.mpf(2) ** -120 * abs(want)


def test_bearings_residual_exactly_pi(g, o):
    """r = +PI stays, r = -PI is wrapped to +PI (the interval is (-pi, pi]); the density is even in r, so both are the density at |r| = pi"""
    m = g.models.bearings4()
    PI = 3.14159265358979311600e+00
    rows = [(1.0, 0.0, 0.0, 0.0)]                                            # bearing exactly 0
    a, b = _against_ref(o, m, rows, [PI])[0], _against_ref(o, m, rows, [-PI])[0]
    assert a == b
    for y in (math.nextafter(PI, 4), math.nextafter(PI, 0), -math.nextafter(PI, 4), -math.nextafter(PI, 0)):
        _against_ref(o, m, rows, [y])


def test_bearings_observation_outside_the_circle(g, o):
    """the spec wraps ONCE: right for |y - bearing| <= 3 pi, i.e. any observation in [-2 pi, 2 pi]; beyond, the residual stays outside
    (-pi, pi] and the density is that of the unwrapped distance (DESIGN.md 3.2 states the domain)"""
    m = g.models.bearings4()
    rows = [(1.0, 0.5, 0.0, 0.0), (-1.0, -0.2, 0.0, 0.0), (0.3, -2.0, 0.0, 0.0)]
    for y in (4.0, -4.0, 6.28, -6.28):
        _against_ref(o, m, rows, [y])                                        # inside the domain: the definition
    ref = hp.Ref(m)
    for y in (13.0, -13.0):
        got = _against_ref(o, m, rows, [y], wraps=1)                         # outside: one wrap only
        assert all(abs(ref.loglik(list(x), [y]).v - got[i]) > 1.0 for i, x in enumerate(rows))


def test_sv1_extremes(g, o):
    """y^2 under- and overflows, h at the cut-offs of exp_.  Inside the documented domain (|h| <= 708, |y| < 1.3e154) the definition;
    outside it the stated saturation"""
    m = g.models.sv1()
    hs = [(-700.0,), (-20.0,), (0.0,), (3.0,), (700.0,), (708.0,), (-708.0,)]
    for y in (0.0, 1e-160, -1e-160, 1e-170, 0.37, -1.25):
        assert np.isfinite(_against_ref(o, m, hs, [y])).all()
    for y in (1e100, 1e150):                                                 # y^2 e^-h stays below DBL_MAX for h >= 0
        assert np.isfinite(_against_ref(o, m, [h for h in hs if h[0] >= 0.0], [y])).all()
    c = m.params[4]
    # h = 710 > 708: exp_(-h) flushes to 0 where e^-710 = 4.5e-309 is a subnormal: the term y^2 e^-h / 2 is dropped (it is below half an ulp of
    # h / 2 for |y| < 1e146, so the result is still the definition's)
    _against_ref(o, m, [(710.0,)], [1.0])
    assert _loglik(o, m, [(710.0,)], [1.0])[0] == -0.5 * 710.0 - c
    # h = -710 < -709: exp_(-h) saturates to +Inf where e^710 = 2.2e308 overflows too: -Inf for y != 0, NaN (0 * Inf) for y = 0
    assert _loglik(o, m, [(-710.0,)], [1.0])[0] == -np.inf
    assert np.isnan(_loglik(o, m, [(-710.0,)], [0.0])[0])
    # |y| = 1e160: y * y overflows: -Inf (the definition's value is below -DBL_MAX for every h <= 708)
    assert (_loglik(o, m, hs, [1e160]) == -np.inf).all()


@pytest.mark.parametrize("sigma", [1e-150, 1e150])
def test_gaussian_terms_far_from_one(g, o, sigma):
    """log sigma and 1 / sigma away from 1, in every Gaussian observation term"""
    k = sigma
    m = g.models.lgssm2(sr=sigma)
    _against_ref(o, m, [(0.0, 0.0), (k, -2 * k), (-0.5 * k, 3 * k)], [3 * k, 0.1 * k])
    m = g.models.object_motion(sobs=sigma)
    _against_ref(o, m, [(1.0, 0.0), (0.0, 2 * k), (1.0, -k)], [1.5 * k, 0.0])
    m = g.models.line_model(s_in=sigma, s_out=sigma * 8)
    _against_ref(o, m, [(1.0, 0.0), (-2.0, 1.0), (0.0, 1.0)], [2.5 * k, k])
    m = g.models.bearings4(sb=sigma)
    _against_ref(o, m, [(1.0, 0.0, 0.0, 0.0), (1.0, 2e-150, 0.0, 0.0)], [3e-150 if sigma < 1 else 1.0])


# ------------------------------------------------------------------------------------------- per-block parameters
def block_models(g, name):
    if name == "lgssm2":
        return [g.models.lgssm2(theta=0.05 + 0.1 * k, rho=0.9 + 0.012 * k, sq=0.05 + 0.03 * k, sr=0.2 + 0.1 * k, s0=0.5 + 0.25 * k) for k in range(8)]
    return [g.models.sv1(mu=-1.5 + 0.3 * k, phi=0.8 + 0.024 * k, sigma=0.05 + 0.04 * k) for k in range(8)]


def drive_blocks(g, br, models):
    rng = np.random.default_rng(3)
    od = models[0].obs_dim
    br.initialize(rng.normal(size=(8, od)))
    br.update(rng.normal(size=(8, od)))
    if models[0].name == "lgssm2":
        br.update(rng.normal(size=(8, od)), proposals=[k % 2 == 0 for k in range(8)])
    else:
        br.update(rng.normal(size=(8, od)))


@pytest.mark.parametrize("name", ["lgssm2", "sv1"])
def test_block_params(g, o, name):
    """a theta grid of 8 parameter rows, 64 particles per block: each block against the reference built from THAT block's natural parameters"""
    models = block_models(g, name)
    drive_blocks(g, hc.BlockRun(hc.OracleBlocks(g, o, models, 512, 64, 77), models, 512, 64, 77), models)
