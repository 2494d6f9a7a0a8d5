"""pf_coalesce! (reference src/resize.jl:309-334, test/resize.jl:226-254) -- include/gpf.h gpf_coalesce.  CPU: the test-side
specification (coalesce_spec.py) against the reference's own assertions, the bindings; GPU: the device against that specification
bit for bit, and the filter continuing from the coalesced state."""
import math
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coalesce_spec import bits, coalesce_expected, set_state   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lse(v):
    m = np.max(v)
    return m + math.log(np.sum(np.exp(v - m)))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_spec_line_model_by_choices(g, o):
    """test/resize.jl:228-239: line_model at step 1 coalesces by choices to <= 5 groups, new == old[parents], log-ML kept (atol 1e-6).
    The outlier is constrained (false) through the strata + fixed-proposal form; a second filter with random outliers is coalesced
    by its slope column."""
    m = g.models.line_model()
    for strata, cols in (((-2., -1., 0., 1., 2.), (0, 1)), (None, (0,))):
        f = o.OracleFilter(m.model_id, m.params, 100, 5)
        f.initialize(g.models.line_obs(1, 0.0), proposal=strata is not None, strata=strata)
        old_rows, old_lml = f.rows.copy(), f.log_ml_estimate()
        rows, lw, par = coalesce_expected(o, f.rows, f.lw, cols)
        set_state(f, rows, lw, par, f.lml_est)
        assert f.n == np.unique(old_rows[:, list(cols)], axis=0).shape[0] <= 5
        assert np.array_equal(f.rows, old_rows[f.parents - 1])
        assert np.all(np.diff(f.parents) > 0)
        assert abs(f.log_ml_estimate() - old_lml) <= 1e-6


def test_spec_replicated_strata_by_identity(g, o):
    """test/resize.jl:241-253: 5 slope strata, pf_replicate!(20), coalesce by identity -> exactly 5, log-ML kept"""
    m = g.models.line_model()
    f = o.OracleFilter(m.model_id, m.params, 5, 9).initialize(g.models.line_obs(1, 0.0), strata=(-2., -1., 0., 1., 2.))
    f.replicate(20)
    old_rows, old_lml = f.rows.copy(), f.log_ml_estimate()
    old_lw = f.lw.copy()
    rows, lw, par = coalesce_expected(o, f.rows, f.lw, range(f.d))
    set_state(f, rows, lw, par, f.lml_est)
    assert f.n == 5 and np.array_equal(f.parents, np.arange(1, 101, 20))
    assert np.array_equal(f.rows, old_rows[f.parents - 1])
    assert abs(f.log_ml_estimate() - old_lml) <= 1e-6
    np.testing.assert_allclose(f.lw, old_lw[f.parents - 1], rtol=0, atol=1e-12)      # log(20 w) + log(5 / 100) = log w


def test_spec_all_distinct_and_neginf(g, o):
    """all rows distinct: bit for bit unchanged; a group of -Inf weights stays -Inf; far below exp's underflow the sum is still exact"""
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((64, 2)); lw = rng.standard_normal(64)
    r2, w2, p2 = coalesce_expected(o, rows, lw, (0, 1))
    assert np.array_equal(bits(r2), bits(rows)) and np.array_equal(bits(w2), bits(lw)) and np.array_equal(p2, np.arange(1, 65))
    rows = np.repeat(np.array([[1.0, 2.0], [3.0, 4.0]]), 3, axis=0)
    lw = np.array([-np.inf, -np.inf, -np.inf, -800.0, -800.0, -801.0])
    r2, w2, p2 = coalesce_expected(o, rows, lw, (0, 1))
    assert np.array_equal(p2, [1, 4]) and w2[0] == -np.inf
    assert abs(w2[1] - (-800.0 + math.log(2 + math.exp(-1.0)) + math.log(2 / 6))) < 1e-9
    with pytest.raises(ValueError):
        coalesce_expected(o, rows, np.where(np.arange(6) == 2, np.nan, 0.0), (0, 1))


def test_coalesce_entry_points_exported(g):
    import ctypes
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, "gpf_coalesce") and hasattr(L, "gpf_introduce")
    names = [s[0] for s in g._lib.SYMBOLS]
    assert "gpf_coalesce" in names and "gpf_introduce" in names
    assert callable(g.pf_coalesce) and callable(g.pf_introduce)


def test_julia_glue_defines_coalesce_and_introduce():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"^import GenParticleFilters:.*\bpf_coalesce!.*\bpf_introduce!", jl, re.M)
    body = re.search(r"^function pf_coalesce!\(s::DeviceParticleFilterState.*?^end", jl, re.S | re.M).group(0)
    assert "ccall((:gpf_coalesce, libgpf)" in body and "_refresh!(s)" in body
    assert re.search(r"^pf_introduce!\(s::DeviceParticleFilterState", jl, re.M)
    body = re.search(r"^function _introduce!\(.*?^end", jl, re.S | re.M).group(0)
    assert "ccall((:gpf_introduce, libgpf)" in body and "_refresh!(s)" in body


def test_coalesce_by_closure_raises_before_the_device(g):
    """a Python callable or a past-step address has no native form: ErrorException, and no call reaches the library"""
    fake = types.SimpleNamespace(dim=2, _L=None, _h=None)            # any library call would fail with AttributeError
    for by in (lambda tr: tr[0], (3, 0), [(3, 0)], 2, -1, "slope", ()):
        with pytest.raises(g.ErrorException, match="native coalescing accepts"):
            g.pf_coalesce(fake, by=by)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _pair(g, o, model, N, seed=7, keep_prev=False, T=2, resample=True):
    """the same filter on the device and in the oracle: initialise, T - 1 updates, a multinomial resample"""
    ys = g.models.simulate(model, T + 3)
    st = g.pf_initialize(model, (1,), ys[0], N, seed=seed, keep_prev=keep_prev)
    f = o.OracleFilter(model.model_id, model.params, N, seed, keep_prev=keep_prev).initialize(ys[0])
    for t in range(1, T):
        g.pf_update(st, (t + 1,), (None,), ys[t]); f.update(ys[t])
    if resample:
        g.pf_resample(st, "multinomial", check=False); f.resample("multinomial", check=False)
        g.pf_update(st, (T + 1,), (None,), ys[T]); f.update(ys[T])   # (weights after the gather: not all equal)
        g.pf_resample(st, "multinomial", check=False); f.resample("multinomial", check=False)
    return st, f, ys


def _assert_same(g, st, f):
    assert st.n_particles == f.n
    assert np.array_equal(bits(st.traces), bits(f.rows))
    assert np.array_equal(bits(st.log_weights), bits(f.lw))
    assert np.array_equal(st.parents, f.parents)
    assert g.get_lml_est(st) == f.log_ml_estimate()


def _coalesce_both(g, o, st, f, by=None, cols=None):
    rows, lw, par = coalesce_expected(o, f.rows, f.lw, cols if cols is not None else range(2 * f.d if f.keep_prev else f.d))
    g.pf_coalesce(st, by=by)
    set_state(f, rows, lw, par, f.lml_est)
    _assert_same(g, st, f)


def _continue(g, st, f, ys):
    """update + resample + rejuvenate continue bit for bit"""
    g.pf_update(st, (9,), (None,), ys[-1]); f.update(ys[-1])
    g.pf_resample(st, "multinomial", check=False); f.resample("multinomial", check=False)
    if st.keep_prev:                                                 # (a move of x_t needs x_{t-1} in the row)
        g.pf_rejuvenate(st, g.mh, (), 1, method="move"); f.rejuvenate("move", 1)
    _assert_same(g, st, f)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, 5000, pytest.param(10 ** 6, marks=pytest.mark.gpu_soak)])
def test_hip_coalesce_lgssm_after_resample(g, o, N):
    st, f, ys = _pair(g, o, g.models.lgssm2(), N)
    n_old = f.n
    _coalesce_both(g, o, st, f)
    assert 1 <= f.n < n_old
    blob = st.checkpoint()                                           # checkpoint of the coalesced state restores into a fresh handle
    st2 = g.DeviceParticleFilterState(st.model, f.n, seed=st.seed)
    st2.restore(blob)
    f2 = set_state(type(f)(f.model, f.params, f.n, f.seed), f.rows.copy(), f.lw.copy(), f.parents.copy(), f.lml_est)
    f2.epoch, f2.has_prev, f2.last_obs = f.epoch, f.has_prev, f.last_obs
    _continue(g, st, f, ys)
    _continue(g, st2, f2, ys)


@pytest.mark.gpu
def test_hip_coalesce_keep_prev(g, o):
    st, f, ys = _pair(g, o, g.models.lgssm2(), 3000, keep_prev=True)
    _coalesce_both(g, o, st, f)
    _continue(g, st, f, ys)


@pytest.mark.gpu
def test_hip_coalesce_sv1_padding_column(g, o):
    """sv1 rows are (x, pad): the padding column is never part of the key.  The pad is made DISTINCT in every row first (the kernels
    write 0 there; gpf_set_rows stores whatever it is given): a pad that leaked into the key would leave every row its own group."""
    st, f, ys = _pair(g, o, g.models.sv1(), 4000)
    assert st.row_width == 2
    rows = f.rows.copy()
    rows[:, 1] = np.arange(1, rows.shape[0] + 1, dtype=np.float64)
    st.traces = rows; f.rows = rows.copy()
    n_old = f.n
    _coalesce_both(g, o, st, f, cols=(0,))
    assert f.n < n_old
    _continue(g, st, f, ys)


@pytest.mark.gpu
def test_hip_coalesce_wide_rows_keep_prev(g, o):
    """W = 8 (bearings4 with keep_prev: x_t and x_{t-1}, no padding): every one of the eight columns is part of the key"""
    st, f, ys = _pair(g, o, g.models.bearings4(), 3000, keep_prev=True)
    assert st.row_width == 8
    n_old = f.n
    _coalesce_both(g, o, st, f)
    assert f.n < n_old
    _continue(g, st, f, ys)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [pytest.param(20000), pytest.param(10 ** 6, marks=pytest.mark.gpu_soak)])
def test_hip_coalesce_object_motion_by_moving(g, o, N):
    """two groups: the contention worst case"""
    m = g.models.object_motion()
    st, f, ys = _pair(g, o, m, N, resample=False)
    col = [c for c in range(2) if np.unique(f.rows[:, c]).size <= 2][0]           # `moving`
    _coalesce_both(g, o, st, f, by=col, cols=(col,))
    assert f.n == 2
    _continue(g, st, f, ys)


@pytest.mark.gpu
def test_hip_coalesce_line_model(g, o):
    """test/resize.jl:228-253 on the device: by choices at step 1, and by identity after replicate"""
    m = g.models.line_model()
    st = g.pf_initialize(m, (1,), g.models.line_obs(1, 0.0), [{"slope": v} for v in (-2, -1, 0, 1, 2)], g.line_fixed, ([1],), 100, seed=5)
    f = o.OracleFilter(m.model_id, m.params, 100, 5).initialize(g.models.line_obs(1, 0.0), proposal=True, strata=(-2., -1., 0., 1., 2.))
    _coalesce_both(g, o, st, f, by="get_choices")
    assert f.n == 5
    st = g.pf_initialize(m, (1,), g.models.line_obs(1, 0.0), [{"slope": v} for v in (-2, -1, 0, 1, 2)], 5, seed=9)
    f = o.OracleFilter(m.model_id, m.params, 5, 9).initialize(g.models.line_obs(1, 0.0), strata=(-2., -1., 0., 1., 2.))
    g.pf_replicate(st, 20); f.replicate(20)
    _coalesce_both(g, o, st, f, by="identity")
    assert f.n == 5
    ys = np.array([g.models.line_obs(t, 1.0) for t in range(2, 4)])
    _continue(g, st, f, ys)


@pytest.mark.gpu
def test_hip_coalesce_all_distinct_unchanged(g, o):
    st, f, ys = _pair(g, o, g.models.lgssm2(), 4096, resample=False)
    rows, lw = st.traces, st.log_weights
    g.pf_coalesce(st)
    assert st.n_particles == 4096 and np.array_equal(bits(st.traces), bits(rows)) and np.array_equal(bits(st.log_weights), bits(lw))
    assert np.array_equal(st.parents, np.arange(1, 4097))
    assert g.get_lml_est(st) == f.log_ml_estimate()


@pytest.mark.gpu
@pytest.mark.parametrize("keys", ["mod5", "distinct"])
def test_hip_coalesce_two_tiles_per_scan_thread(g, o, keys):
    """n = 2048 * 256 + 1 = 524 289: 257 tiles of 2048, so the single workgroup of k_coal_scan gives a thread two tiles (its `per > 1`
    branch, otherwise reached only by the soak case at 10^6).  Five groups, every one spread over every tile, and all rows distinct (no group
    crosses a tile); against the specification bit for bit."""
    n = 2048 * 256 + 1
    m = g.models.lgssm2()
    st, f, ys = _pair(g, o, m, n, resample=False)
    if keys == "mod5":
        rows = f.rows.copy()
        rows[:, :] = (np.arange(n) % 5)[:, None]
        st.traces = rows; f.rows = rows.copy()
    _coalesce_both(g, o, st, f)
    assert f.n == (5 if keys == "mod5" else n)
    st.close()


@pytest.mark.gpu
def test_hip_coalesce_neginf_group_and_nan(g, o):
    m = g.models.lgssm2()
    st, f, ys = _pair(g, o, m, 1000)
    lw = f.lw.copy()
    first = f.rows[0]
    same = np.all(f.rows == first, axis=1)
    lw[same] = -np.inf                                               # the group of particle 0: all -Inf
    st.log_weights = lw; f.lw = lw.copy()
    _coalesce_both(g, o, st, f)
    assert f.lw[0] == -np.inf
    before = (st.traces, st.log_weights, st.parents, g.get_lml_est(st))
    bad = st.log_weights; bad[3] = np.nan
    st.log_weights = bad
    v = st[0:10]
    L = st._L
    import ctypes
    n = ctypes.c_int64(-1)
    assert L.gpf_coalesce(st._h, 0, ctypes.byref(n)) == g._lib.ERR_INVALID_WEIGHTS
    assert st.n_particles == before[0].shape[0]
    assert np.array_equal(bits(st.traces), bits(before[0])) and np.array_equal(st.parents, before[2])
    assert np.array_equal(bits(st.log_weights), bits(bad))
    assert np.array_equal(bits(v.log_weights), bits(bad[:10]))                # the refused call left the views valid


@pytest.mark.gpu
def test_hip_coalesce_refusals(g, o):
    import ctypes
    m = g.models.lgssm2()
    st, f, ys = _pair(g, o, m, 512)
    v = st[0:100]
    n = ctypes.c_int64(0)
    assert st._L.gpf_coalesce(v._h, 0, ctypes.byref(n)) == g._lib.ERR_STATE                     # a view
    assert st._L.gpf_coalesce(st._h, 1 << 2, ctypes.byref(n)) == g._lib.ERR_INVALID_ARGUMENT      # a column beyond the state
    _ = v.log_weights                                                                           # the view still works ...
    with pytest.raises(g.ErrorException, match="past-step"):
        g.pf_coalesce(st, by=[(1, 0)])
    _coalesce_both(g, o, st, f)                                                                 # the handle is usable
    with pytest.raises(g.ErrorException):                                                       # ... and is stale afterwards
        _ = v.log_weights
    h = g.pf_initialize(m, (1,), ys[0], 256, seed=3, history=4)
    assert h._L.gpf_coalesce(h._h, 0, ctypes.byref(n)) == g._lib.ERR_STATE                      # a trajectory store
    assert h.n_particles == 256 and np.isfinite(g.get_lml_est(h))
