"""Resampling across blocks (gpf.h gpf_resample_across_blocks) without a device: the exported symbols and the Python surface, the spec of
tests/across_blocks_spec.py against mpmath (mass conservation, every block's estimate = M afterwards, within the bound derived there), its
exact properties, and the rehearsal of the known-answer test of tests/test_gpu_across_blocks.py."""
import ctypes

import numpy as np
import pytest

import across_blocks_spec as xs
import block_params_spec as bp


def test_symbols_exported_and_in_the_ctypes_table(g):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    pd, pi32, pi64 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    want = {
        "gpf_resample_across_blocks": [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, pi32, pi32, pd],
        "gpf_block_ancestors": [ctypes.c_void_p, pi64],
        "gpf_get_block_params": [ctypes.c_void_p, pd, ctypes.c_int32, ctypes.c_int64],
    }
    for name, args in want.items():
        assert hasattr(L, name), name
        assert table[name][1] is ctypes.c_int and table[name][2] == args, name
    for name in ("pf_resample_across_blocks", "block_ancestors", "get_block_params"):
        assert callable(getattr(g, name)), name
    assert L.gpf_abi_version() == 1                                   # additive: the ABI version stays


def _state(o, g, N, bs, seed=11, T=4, model="lgssm2"):
    m = g.models.by_name(model)
    return xs.uneven_oracle(o, m, xs.block_data(g.models, m, N // bs, T), N, bs, seed)


@pytest.mark.parametrize("N,bs,method", [(1200, 100, "multinomial"), (777, 7, "residual"), (4098, 2049, "stratified"), (37, 1, "multinomial")])
def test_mass_conservation_and_block_estimates_against_mpmath(o, g, N, bs, method):
    """logsumexp over the whole filter is the same before and after a fired call, and every block's estimate afterwards is M -- both in mpmath
    on the spec's Float64 outputs, within across_blocks_spec.property_bound (derived there from the ulps of the delta additions and the
    fixed-point scale K; not fitted)"""
    f = _state(o, g, N, bs)
    lw0 = f.lw.copy()
    T0 = xs.mp_logsumexp(lw0)
    plan = xs.resample_across_blocks(o, f, bs, method)
    assert plan.resampled
    bound = xs.property_bound(plan.L, plan.M, plan.delta, lw0, f.lw, bs, f.lml_est)
    assert 0 < bound < 1e-9                                           # (the fixed-point terms dominate: bs 2^-K and a few ulps of |lw|)
    T1 = xs.mp_logsumexp(f.lw)
    print(f"mass: |after - before| = {float(abs(T1 - T0)):.3e}, bound {bound:.3e}")
    assert abs(T1 - T0) <= bound
    B = N // bs
    logbs = xs.mp_logsumexp(np.zeros(bs))                             # log bs in mpmath
    worst = max(abs(f.lml_est + xs.mp_logsumexp(f.lw[b * bs:(b + 1) * bs]) - logbs - plan.M) for b in range(B))
    print(f"block estimates: worst |estimate - M| = {float(worst):.3e}, bound {bound:.3e}")
    assert worst <= bound
    # ... and the estimates the spec itself reports afterwards: its own evaluation error on the new weights on top
    L1 = xs.block_logweights(f, bs)
    assert np.max(np.abs(L1 - plan.M)) <= bound + xs.lam_of(f.lw, L1, bs, f.lml_est)


def test_copy_is_whole_blocks_and_counts_sum(o, g):
    N, bs = 1200, 100
    f = _state(o, g, N, bs)
    rows0, lw0, e0 = f.rows.copy(), f.lw.copy(), f.epoch
    plan = xs.resample_across_blocks(o, f, bs, "residual")
    B = N // bs
    A = plan.A
    assert A.shape == (B,) and A.min() >= 0 and A.max() < B and np.bincount(A, minlength=B).sum() == B
    assert f.epoch == e0 + 1
    for b in range(B):
        a = A[b]
        assert np.array_equal(f.rows[b * bs:(b + 1) * bs], rows0[a * bs:(a + 1) * bs])
        assert np.array_equal(f.lw[b * bs:(b + 1) * bs], lw0[a * bs:(a + 1) * bs] + (plan.M - plan.L[a]))
        assert np.array_equal(f.parents[b * bs:(b + 1) * bs], a * bs + np.arange(bs) + 1)
    # residual resampling: a block with weight w has at least floor(B w) copies
    w = np.exp(plan.L - plan.L.max()); w /= w.sum()
    assert np.all(np.bincount(A, minlength=B) >= np.floor(B * w * (1 - 1e-9)))


def test_gate_at_the_boundary(o, g):
    """equal block weights: the ESS is exactly B; `ess < ess_frac * B` fires for no ess_frac <= 1"""
    m = g.models.lgssm2()
    N, bs = 600, 100
    f = o.OracleFilter(m.model_id, m.params, N, 3)                    # log-weights 0
    L = xs.block_logweights(f, bs)
    assert np.all(L == L[0])
    for frac, fires in ((1.0, False), (0.5, False), (np.nextafter(1.0, 2.0), True), (None, True), (-1.0, True), (float("nan"), True)):
        h = o.OracleFilter(m.model_id, m.params, N, 3)
        plan = xs.resample_across_blocks(o, h, bs, "multinomial", ess_frac=frac)
        assert plan.ess == N // bs and plan.resampled is fires, frac
        assert h.epoch == 1
        if not fires:
            assert plan.A is None and np.array_equal(h.lw, np.zeros(N)) and np.array_equal(h.parents, np.arange(1, N + 1))
        else:
            assert np.array_equal(h.lw, np.zeros(N))                  # M = L: delta = 0


@pytest.mark.parametrize("method", xs.METHODS)
def test_one_block_is_the_identity(o, g, method):
    f = _state(o, g, 100, 100)
    rows0, lw0 = f.rows.copy(), f.lw.copy()
    plan = xs.resample_across_blocks(o, f, 100, method)
    assert plan.resampled and np.array_equal(plan.A, [0]) and plan.M == plan.L[0] and plan.delta[0] == 0.0
    assert np.array_equal(f.rows, rows0) and np.array_equal(f.lw, lw0) and np.array_equal(f.parents, np.arange(1, 101))


def test_invalid_block_weights(o, g):
    N, bs = 400, 100
    for bad in (np.nan, np.inf):
        f = _state(o, g, N, bs)
        f.lw[150] = bad
        rows0, lw0, e0 = f.rows.copy(), f.lw.copy(), f.epoch
        for check in (True, "warn", False):
            with pytest.raises(o.OracleError):
                xs.resample_across_blocks(o, f, bs, "multinomial", check=check)
        assert f.epoch == e0 and np.array_equal(f.rows, rows0) and np.array_equal(f.lw, lw0, equal_nan=True)
    # all -Inf: refused under check = True, else the uniform fallback -- ancestors from uniform block weights, every delta 0
    f = _state(o, g, N, bs)
    f.lw[:] = -np.inf
    with pytest.raises(o.OracleError):
        xs.resample_across_blocks(o, f, bs, "stratified", check=True)
    assert f.epoch == _state(o, g, N, bs).epoch
    plan = xs.resample_across_blocks(o, f, bs, "stratified", check="warn")
    assert plan.invalid and plan.resampled and np.all(plan.delta == 0.0) and np.isnan(plan.ess)
    assert np.array_equal(plan.A, np.arange(N // bs))                 # stratified over uniform weights: one copy each
    assert np.all(f.lw == -np.inf)
    # ... and a gated call does not fire on a NaN ESS
    assert not xs.resample_across_blocks(o, f, bs, "stratified", ess_frac=0.5, check=False).resampled
    # one -Inf block among finite ones is no error: it has no offspring
    f = _state(o, g, N, bs)
    f.lw[100:200] = -np.inf
    plan = xs.resample_across_blocks(o, f, bs, "residual", check=True)
    assert not plan.invalid and 1 not in plan.A


def test_refusals(o, g):
    f = _state(o, g, 400, 100)
    for bs in (0, 3, 150):
        with pytest.raises(o.OracleError):
            xs.resample_across_blocks(o, f, bs)
    with pytest.raises(o.OracleError):
        xs.resample_across_blocks(o, f, 100, "multinomial_sorted")


def test_known_answer_rehearsal_on_the_oracle(o, g):
    """an adaptive theta grid: the whole filter's log_ml_estimate after block-wise steps with an outer resample every step estimates the grid
    evidence log mean_k exp(kalman_loglik(theta_k)); the data-generating theta holds the plurality of the blocks at the end.  The device
    reproduces these numbers bit for bit, so the band and the seed are fixed here."""
    est, assign, ref, ms, ys, plans = xs.xka_oracle(o, g.models)
    ev = xs.xka_evidence(ms, ys, g.models)
    fired = sum(p.resampled for p in plans)
    counts = np.bincount(assign, minlength=len(ms))
    print(f"estimate - evidence = {est - ev:+.4f}, outer resamples fired {fired} / {len(plans)}, blocks per theta {counts}")
    assert -xs.XKA_TOL_BELOW < est - ev < xs.XKA_TOL_ABOVE
    assert 0 < fired < len(plans)                                     # both branches of the gate are exercised
    assert bp.KA_GRID[int(np.argmax(counts))] == bp.KA_TRUE
    # the composed oracle of the rehearsal agrees with the plain one on a state without per-block parameters
    for p in plans:
        if p.resampled:
            assert np.bincount(p.A, minlength=p.B).sum() == p.B
