"""pf_introduce! (reference src/resize.jl:351-421, test/resize.jl:256-339) -- include/gpf.h gpf_introduce.  CPU: the test-side
specification (coalesce_spec.py) against the reference's own assertions; GPU: the device against it bit for bit, and the filter
continuing from the enlarged state."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coalesce_spec import bits, introduce_expected, set_state   # noqa: E402


def _line_hist(T, slope=0.0):
    import gpf_amd as g
    return np.array([g.models.line_obs(t, slope) for t in range(1, T + 1)]) if T else np.array([g.models.line_obs(0, 0.0)])


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_spec_introduce_default_proposal(g, o):
    """test/resize.jl:256-266: introduce 50 into 50 -> 100 particles, every slope in [-2, 2]; with nothing observed the weights are 0"""
    m = g.models.line_model()
    for T in (0, 10):
        hist = _line_hist(T)
        f = o.OracleFilter(m.model_id, m.params, 50, 3).initialize(hist[0])
        for e in range(1, hist.shape[0]):
            f.update(hist[e])
        rows, lw, par, lml = introduce_expected(o, f, 50, hist)
        set_state(f, rows, lw, par, lml, epoch_step=1)
        assert f.n == 100 and rows.shape == (100, f.W)
        assert np.all((-2 <= rows[:, 0]) & (rows[:, 0] <= 2)) and np.all(rows[:, 0] == np.round(rows[:, 0]))
        assert np.array_equal(par[50:], np.zeros(50)) and np.array_equal(par[:50], np.arange(1, 51))
        if T == 0:
            assert np.all(np.abs(lw) < 1e-12)                        # all(w ≈ 0), test/resize.jl:261


def test_spec_introduce_fixed_proposal(g, o):
    """test/resize.jl:286-293: slope ~ uniform_discrete(0, 0) proposed -> every slope 0, every weight log(1/5)"""
    m = g.models.line_model()
    hist = _line_hist(0)
    f = o.OracleFilter(m.model_id, m.params, 50, 3).initialize(hist[0], proposal=True)
    rows, lw, par, lml = introduce_expected(o, f, 50, hist, proposal=True)
    assert np.all(rows[:, 0] == 0.0)
    np.testing.assert_allclose(lw, math.log(1 / 5), rtol=0, atol=1e-12)


def test_spec_introduce_folds_the_log_ml_estimate(g, o):
    """resize.jl:366-369: the running estimate moves into the old weights; log_ml_estimate of the old particles is unchanged"""
    m = g.models.lgssm2()
    ys = g.models.simulate(m, 4)
    f = o.OracleFilter(m.model_id, m.params, 64, 2).initialize(ys[0])
    f.resample("multinomial"); f.update(ys[1])
    assert f.lml_est != 0.0
    rows, lw, par, lml = introduce_expected(o, f, 10, ys[:2])
    assert lml == 0.0 and np.array_equal(lw[:64], f.lw + f.lml_est)


def test_introduce_argument_forms_raise_before_the_device(g):
    class Fake:
        model = g.models.lgssm2(); _params = np.ascontiguousarray(model.params, np.float64); _L = None; _h = None
    with pytest.raises(g.ErrorException, match="own model"):
        g.pf_introduce(Fake(), g.models.sv1(), (1,), [[0.0]], 5)
    with pytest.raises(g.ErrorException, match="native proposals"):
        g.pf_introduce(Fake(), [[0.0, 0.0]], object(), (), 5)
    with pytest.raises(TypeError):
        g.pf_introduce(Fake(), 5)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _assert_same(g, st, f):
    assert st.n_particles == f.n
    assert np.array_equal(bits(st.traces), bits(f.rows))
    assert np.array_equal(bits(st.log_weights), bits(f.lw))
    assert np.array_equal(st.parents, f.parents)
    assert g.get_lml_est(st) == f.log_ml_estimate()


def _pair(g, o, model, N, seed=4, keep_prev=False, ys=None, T=3, proposal=None):
    ys = g.models.simulate(model, T + 2) if ys is None else ys
    st = g.pf_initialize(model, (1,), ys[0], N, seed=seed, keep_prev=keep_prev)
    f = o.OracleFilter(model.model_id, model.params, N, seed, keep_prev=keep_prev).initialize(ys[0])
    g.pf_resample(st, "multinomial", check=False); f.resample("multinomial", check=False)      # log_ml_est != 0
    g.pf_update(st, (2,), (None,), ys[1]); f.update(ys[1])
    return st, f, ys


def _introduce_both(g, o, st, f, n_add, hist, proposal=None, model_form=False):
    rows, lw, par, lml = introduce_expected(o, f, n_add, hist, proposal=proposal is not None)
    if model_form and proposal is not None:
        g.pf_introduce(st, st.model, (1,), hist, proposal, (), n_add)
    elif model_form:
        g.pf_introduce(st, st.model, (1,), hist, n_add)
    elif proposal is not None:
        g.pf_introduce(st, hist, proposal, (), n_add)
    else:
        g.pf_introduce(st, hist, n_add)
    set_state(f, rows, lw, par, lml, epoch_step=1)
    _assert_same(g, st, f)


def _continue(g, st, f, y):
    g.pf_update(st, (9,), (None,), y); f.update(y)
    g.pf_resample(st, "multinomial", check=False); f.resample("multinomial", check=False)
    if st.keep_prev:                                                 # (a move of x_t needs x_{t-1} in the row)
        g.pf_rejuvenate(st, g.mh, (), 1, method="move"); f.rejuvenate("move", 1)
    _assert_same(g, st, f)


_MODELS = ["lgssm2", "bearings4", "sv1", "object_motion", "line_model"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _MODELS)
@pytest.mark.parametrize("T", [1, 2, 10])
def test_hip_introduce_models(g, o, name, T):
    m = getattr(g.models, name)()
    ys = g.models.simulate(m, 12)
    st, f, _ = _pair(g, o, m, 300, ys=ys, keep_prev=(T == 10))
    _introduce_both(g, o, st, f, 200, ys[:T], model_form=(T == 2))
    _continue(g, st, f, ys[T])


@pytest.mark.gpu
def test_hip_introduce_keep_prev_and_checkpoint(g, o):
    m = g.models.bearings4()
    st, f, ys = _pair(g, o, m, 256, keep_prev=True, T=6)
    _introduce_both(g, o, st, f, 100, ys[:4])
    blob = st.checkpoint()
    st2 = g.DeviceParticleFilterState(m, f.n, seed=st.seed, keep_prev=True)
    st2.restore(blob)
    f2 = set_state(type(f)(f.model, f.params, f.n, f.seed, keep_prev=True), f.rows.copy(), f.lw.copy(), f.parents.copy(), f.lml_est)
    f2.epoch, f2.has_prev, f2.last_obs = f.epoch, f.has_prev, f.last_obs
    _continue(g, st, f, ys[4])
    _continue(g, st2, f2, ys[4])


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3])
def test_hip_introduce_locally_optimal(g, o, T):
    m = g.models.lgssm2()
    st, f, ys = _pair(g, o, m, 500)
    _introduce_both(g, o, st, f, 300, ys[:T], proposal=g.locally_optimal, model_form=(T == 3))
    _continue(g, st, f, ys[T])


@pytest.mark.gpu
@pytest.mark.parametrize("T", [0, 1, 10])
def test_hip_introduce_line_fixed(g, o, T):
    """test/resize.jl:286-339 on the device"""
    m = g.models.line_model()
    hist = _line_hist(T)
    st = g.pf_initialize(m, (T,), hist[0], 50, seed=6)
    f = o.OracleFilter(m.model_id, m.params, 50, 6).initialize(hist[0])
    for e in range(1, hist.shape[0]):
        g.pf_update(st, (e + 1,), (None,), hist[e]); f.update(hist[e])
    _introduce_both(g, o, st, f, 50, hist, proposal=g.line_fixed)
    assert st.n_particles == 100 and np.all(st.traces[50:, 1] == 0.0)                # outlier == false
    if T == 0:
        assert np.all(st.traces[50:, 0] == 0.0)
        np.testing.assert_allclose(st.log_weights[50:], math.log(1 / 5), rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_hip_introduce_twice_draws_new_streams(g, o):
    m = g.models.lgssm2()
    st, f, ys = _pair(g, o, m, 200)
    _introduce_both(g, o, st, f, 100, ys[:2])
    first = st.traces[200:].copy()
    _introduce_both(g, o, st, f, 100, ys[:2])
    assert st.n_particles == 400 and not np.array_equal(first, st.traces[300:])
    _continue(g, st, f, ys[2])


@pytest.mark.gpu
def test_hip_introduce_million(g, o):
    m = g.models.lgssm2()
    st, f, ys = _pair(g, o, m, 1000)
    _introduce_both(g, o, st, f, 10 ** 6, ys[:3])


@pytest.mark.gpu
def test_hip_introduce_refusals(g, o):
    import ctypes
    m = g.models.lgssm2()
    st, f, ys = _pair(g, o, m, 256)
    v = st[0:64]
    ob = np.ascontiguousarray(ys[:2])
    pd = ob.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    L = st._L
    assert L.gpf_introduce(v._h, pd, 2, 2, 10, 0) == g._lib.ERR_STATE                               # a view
    assert L.gpf_introduce(st._h, pd, 3, 2, 10, 0) == g._lib.ERR_INVALID_ARGUMENT                   # wrong data vector length
    assert L.gpf_introduce(st._h, pd, 2, 0, 10, 0) == g._lib.ERR_INVALID_ARGUMENT                   # no step
    assert L.gpf_introduce(st._h, pd, 2, 2, 0, 0) == g._lib.ERR_INVALID_ARGUMENT                    # no particle
    assert L.gpf_introduce(st._h, pd, 2, 2, 10, 2) == g._lib.ERR_INVALID_ARGUMENT                   # line_fixed on the LG-SSM
    _ = v.log_weights
    with pytest.raises(g.ErrorException, match="own model"):
        g.pf_introduce(st, g.models.lgssm2(rho=0.5), (1,), ys[:2], 10)
    _introduce_both(g, o, st, f, 10, ys[:2])                                                       # the handle is usable
    with pytest.raises(g.ErrorException):
        _ = v.log_weights                                                                          # the view is stale
    h = g.pf_initialize(m, (1,), ys[0], 128, seed=3, history=4)
    assert L.gpf_introduce(h._h, pd, 2, 2, 10, 0) == g._lib.ERR_STATE                              # a trajectory store
    assert h.n_particles == 128 and np.isfinite(g.get_lml_est(h))
