"""The device filter against tests/hp_reference.py -- the mpmath restatement of the models, of the random stream and of the math spec -- through
the same check functions as tests/test_hp_models.py (there: the CPU oracle).  Device == oracle is asserted bit for bit elsewhere; this file is
the device's own witness that what both compute is what the model definitions say.  One case per model and operation at N = 2000 and at a
ragged size (N = 2051: odd, just past one 2048-particle tile), per-block parameters, the move fused into the update kernel, pf_step_ess;
the math spec on the edge vectors of tests/test_hp_math.py, special values included, bit for bit against the oracle; Box-Muller from
counters against mpmath."""
import math

import numpy as np
import pytest

import hp_checks as hc
import hp_reference as hp
import test_hp_models as cpu

pytestmark = pytest.mark.gpu

SIZES = [2000, 2051]
SEED = 20240917


def _run(g, o, name, n, seed=SEED, **kw):
    m = getattr(g.models, name)(**kw) if kw else g.models.by_name(name)
    return hc.Run(hc.DeviceAdapter(g, o, m, n, seed), m, n, seed), hc.case_data(g, m, 4)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", cpu.MODELS)
def test_initialize_and_updates(g, o, name, n):
    r, ys = _run(g, o, name, n)
    cpu.drive_filter(r, ys)


@pytest.mark.parametrize("n", SIZES)
def test_lgssm2_locally_optimal_proposal_and_conjugacy(g, o, n):
    r, ys = _run(g, o, "lgssm2", n)
    cpu.drive_lgssm2_proposal(r, ys)


def test_line_model_fixed_proposal(g, o):
    r, ys = _run(g, o, "line_model", 2051)
    cpu.drive_line_proposal(r, ys)


@pytest.mark.parametrize("name,n,layout", cpu.STRATA_CASES + [("object_motion", 2051, "contiguous"), ("line_model", 2051, "interleaved")])
def test_stratified(g, o, name, n, layout):
    r, ys = _run(g, o, name, n)
    cpu.drive_strata(r, ys, name, layout)


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_line_model_stratified_with_proposal(g, o, layout):
    r, ys = _run(g, o, "line_model", 2051)
    r.initialize(ys[0], proposal=True, strata=[-2.0, -1.0, 0.0, 1.0, 2.0], layout=layout)


@pytest.mark.parametrize("name,proposal", cpu.MOVE_CASES)
def test_move_reweight(g, o, name, proposal):
    r, ys = _run(g, o, name, 2051 if proposal else 2000)
    cpu.drive_reweight(r, ys, cpu._moves_q(g, name, proposal))


@pytest.mark.parametrize("name,proposal", cpu.MOVE_CASES)
def test_mh_move(g, o, name, proposal):
    r, ys = _run(g, o, name, 2000 if proposal else 2051)
    assert cpu.drive_mh(r, ys, cpu._moves_q(g, name, proposal)) <= hc.MAX_UNDECIDABLE


@pytest.mark.parametrize("name", ["lgssm2", "bearings4", "object_motion"])
def test_move_fused_into_update(g, o, name):
    """pf_rejuvenate without `count` followed by pf_update: the move runs inside the update kernel; same expected rows"""
    r, ys = _run(g, o, name, 2051)
    assert cpu.drive_move_then_update(r, ys) <= hc.MAX_UNDECIDABLE


def test_step_ess_bearings(g, o):
    r, ys = _run(g, o, "bearings4", 2051)
    assert any(cpu.drive_step_ess(r, ys))


@pytest.mark.parametrize("name", ["lgssm2", "sv1"])
def test_block_params(g, o, name):
    models = cpu.block_models(g, name)
    cpu.drive_blocks(g, hc.BlockRun(hc.DeviceBlocks(g, o, models, 512, 64, 77), models, 512, 64, 77), models)


# ------------------------------------------------------------------------------------------- the math spec on the device
def _edge_vectors():
    rng = [np.random.default_rng(s) for s in (1, 2, 3, 4, 5)]
    y, x = hc.atan2_points(rng[3])
    table = {fn: [r for r in hc.DOMAIN_TABLE if r[0] == fn] for fn in hc.WHICH}
    special = lambda fn, k: np.array([r[1][k] for r in table[fn]])                            # noqa: E731
    return {
        0: (np.concatenate([hc.exp_points(rng[0]), special("exp", 0)]), None),
        1: (np.concatenate([hc.log_points(rng[1]), special("log", 0)]), None),
        2: (np.concatenate([hc.sincos_points(rng[2]), special("sincos", 0)]), None),
        3: (np.concatenate([y, special("atan2", 0)]), np.concatenate([x, special("atan2", -1)])),
        7: (hc.neglog_points(rng[4]).view(np.float64), None),
    }


@pytest.mark.parametrize("which", [0, 1, 2, 3, 7])
def test_device_math_on_the_edge_vectors(g, o, which):
    """exactly the vectors of tests/test_hp_math.py plus every input of the domain table (NaN, +-Inf, +-0, subnormals, negative arguments of
    log_, the cut-offs of exp_ with the last argument on each side): device == oracle on the uint64 views, any NaN equal to any NaN (the sign
    of a NaN an operation produces is x86's or gfx950's, not the spec's)"""
    a, b = _edge_vectors()[which]
    st = g.DeviceParticleFilterState(g.models.lgssm2(), 16)
    d1, d2 = st.debug_math(which, a, b)
    o1, o2 = np.empty(a.size), np.zeros(a.size)
    o.lib().o_math_vec(which, np.ascontiguousarray(a), np.ascontiguousarray(a if b is None else b), a.size, o1, o2)
    bad = np.flatnonzero(~hc.bits_equal_nan(d1, o1))
    assert bad.size == 0, [(float(a[i]).hex(), None if b is None else float(b[i]).hex(), float(d1[i]).hex(), float(o1[i]).hex()) for i in bad[:5]]
    if which == 2:
        bad = np.flatnonzero(~hc.bits_equal_nan(d2, o2))
        assert bad.size == 0, [(float(a[i]).hex(), float(d2[i]).hex(), float(o2[i]).hex()) for i in bad[:5]]


@pytest.mark.parametrize("fn", ["exp", "log", "sincos", "atan2"])
def test_device_domain_table(g, o, fn):
    """every row of the table "input class -> result" of DESIGN.md 3.2, exactly, on the device (one launch per function)"""
    rows = [r for r in hc.DOMAIN_TABLE if r[0] == fn]
    st = g.DeviceParticleFilterState(g.models.lgssm2(), 16)
    d1, d2 = st.debug_math(hc.WHICH[fn], [r[1][0] for r in rows], [r[1][-1] for r in rows])
    for i, (_, args, want) in enumerate(rows):
        if fn == "sincos":
            assert hc.same_bits(d1[i], want[0]) and hc.same_bits(d2[i], want[1]), (fn, args, d1[i], d2[i], want)
        else:
            assert hc.same_bits(d1[i], want), (fn, args, float(d1[i]).hex(), want)


def test_device_box_muller_against_mpmath(g, o):
    """normal2 from counters (debug_math 6) for 4096 consecutive ids on two blocks.  Derived bound: log_ to 2 ulp moves r = sqrt(-2 ln u1) by
    2^-52 r <= 2 ulp(r), the square root adds half an ulp, sincos2pi 1e-15 absolute (times r), the product half an ulp:
    |z - z_ref| <= r 1e-15 + 3 ulp(r)"""
    seed = 99
    st = g.DeviceParticleFilterState(g.models.lgssm2(), 16, seed=seed)
    for blk in (0, 3):
        gid = np.arange(4096, dtype=np.float64) + 1000.0
        z0, z1 = st.debug_math(6, gid, np.full(gid.size, float(blk)))
        worst = 0.0
        for i in range(gid.size):
            w = hp.block(seed, int(gid[i]), blk, 0, hp.TAG_UPDATE)
            u1, u2 = hp.u52(w[0], w[1]), hp.u52(w[2], w[3])
            r = hp.M.sqrt(-2 * hp.M.log(hp.mpf(u1)))
            ang = 2 * hp.PI * hp.mpf(u2)
            bound = float(r) * 1e-15 + 3 * math.ulp(float(r))
            for got, want in ((z0[i], r * hp.M.cos(ang)), (z1[i], r * hp.M.sin(ang))):
                err = float(abs(hp.mpf(float(got)) - want))
                worst = max(worst, err / bound)
                assert err <= bound, (blk, i, got, want, err, bound)
        print(f"box-muller block {blk}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------- log_ behind the public API
def test_optimal_resize_never_shows_log_garbage(g, o):
    """gpf_k_resize.hpp's log_((double)opt_a): opt_a >= 1 and opt_B > 0 down to 1 and 2 particles, one dominant weight or all equal"""
    m = g.models.lgssm2()
    y = g.models.simulate(m, 1)[0]
    for n_old, n_new, what, lw in hc.optimal_resize_cases():
        st = g.pf_initialize(m, (), y, n_old, seed=3)
        st.log_weights = lw
        g.pf_resize(st, n_new, "optimal", check=False)
        assert st.n_particles == n_new
        hc.check_no_log_garbage(st.log_weights, lw)
        f = o.OracleFilter(m.model_id, m.params, n_old, 3).initialize(y)
        f.lw = lw.copy()
        f.resize(n_new, "optimal", check=False)
        assert np.array_equal(st.log_weights.view(np.uint64), f.lw.view(np.uint64)), (n_old, n_new, what)


def test_blockwise_resample_with_a_dead_block(g, o):
    """gpf_k_block.hpp's log_((double)cnt): cnt is the block's particle count, never the count of live weights"""
    m = g.models.lgssm2()
    y = g.models.simulate(m, 1)[0]
    st = g.pf_initialize(m, (), y, 64, seed=3)
    lw = st.log_weights
    lw[16:32] = -np.inf
    st.log_weights = lw
    g.pf_resample_blocks(st, 16, "multinomial", check=False)
    out = st.log_weights
    assert (out[16:32] == -np.inf).all()
    for a in (0, 32, 48):
        assert np.isfinite(out[a:a + 16]).all() and (out[a:a + 16] == out[a]).all()
        assert abs(out[a] - (hc.lse(lw[a:a + 16]) - math.log(16))) < 1e-12
    ess, lml = g.block_stats(st, 16)                      # the dead block: the documented -Inf / NaN, never a finite number of hundreds of nats
    assert not np.isfinite(lml[1]) and np.isfinite(np.delete(lml, 1)).all()
    assert np.isnan(ess[1]) or 0.0 <= ess[1] <= 16.0
