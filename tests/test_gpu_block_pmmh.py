"""The particle-marginal MH move per block in one launch: gpf_pmmh_blocks / pf_pmmh_blocks (gpf_k_block_pmmh.hpp) against the loop of existing calls it
stands for -- a twin handle made by pf_initialize_blocks(seed=seed, params=proposed) and run by pf_run_blocks, block_stats for its estimates, the accept
rule on the host and the existing setters for the expected state.  Every comparison is np.array_equal.  The expected state is a second copy of the state
that never saw the call: that both continue identically holds only if the call left the state's epoch and seed alone."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_block_conditional import block_obs, model_of

pytestmark = pytest.mark.gpu

INF = float("inf")
# both sides of each team-shape boundary of team_dispatch (128 | 129: 2 | 8 particles per lane; 512 | 513: a wave | the workgroup), the smallest and the
# largest block; up to 128 particles the proposal filter lives in LDS, above in the call's scratch.  n = 3 bs + 7: a short last block
SIZES = [7, 128, 129, 512, 513, 2048]
SEED, TWIN_SEED = 23, 1009


def eq(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def the_loop(g, m, n, bs, ys, prop, thr, method, keep_mass, ess_frac=0.5, sort_particles=True, shared=False, state_params=None, spoil=None, relative=False):
    """(state after pf_pmmh_blocks, its result, expected state, expected parents, accepted, Lp, twin, per-block shift): the issue's loop, written out"""
    B = (n + bs - 1) // bs
    y0 = np.broadcast_to(ys[0], (B,) + ys[0].shape) if shared else ys[:, 0]
    sp = state_params if state_params is not None else [m] * B
    st, ex = (g.pf_initialize_blocks(m, (1,), y0, n, bs, seed=SEED, params=sp) for _ in range(2))
    if spoil is not None:
        for s in (st, ex):
            lw = s.log_weights; lw[spoil] = np.nan; s.log_weights = lw
    twin = g.pf_initialize_blocks(m, (), y0, n, bs, seed=TWIN_SEED, params=prop)
    T = ys.shape[0] if shared else ys.shape[1]
    if T > 1:
        try:
            g.pf_run_blocks(twin, ys[1:] if shared else ys[:, 1:], bs, method, ess_frac=ess_frac, sort_particles=sort_particles)
        except g.ErrorException:
            pass
    Lp, Ls = g.block_stats(twin, bs)[1], g.block_stats(st, bs)[1]
    if relative:
        thr = Lp + thr
    with np.errstate(invalid="ignore"):
        acc = Lp > thr
        if keep_mass:
            acc &= np.isfinite(Ls)                                            # (a state block with invalid weights is never replaced)
        shift = Ls - Lp if keep_mass else np.zeros(B)
    sel = np.repeat(acc, bs)[:n]
    rows, lw, par = ex.traces, ex.log_weights, ex.parents
    rows[sel] = twin.traces[sel]
    lw[sel] = (twin.log_weights + np.repeat(shift, bs)[:n])[sel] if keep_mass else twin.log_weights[sel]
    par[sel] = twin.parents[sel]
    ex.traces, ex.log_weights = rows, lw
    p = g.get_block_params(ex); p[acc] = g.get_block_params(twin)[acc]
    g.set_block_params(ex, p, bs)
    r = g.pf_pmmh_blocks(st, ys, prop, thr, bs, method, seed=TWIN_SEED, ess_frac=ess_frac, sort_particles=sort_particles, keep_mass=keep_mass)
    return st, r, ex, par, acc, Lp, twin, shift


def check(g, st, r, ex, par, acc, Lp, bs, y_next=None):
    assert eq(r.accepted, acc) and eq(r.lml, Lp) and r.accepted.dtype == bool
    assert eq(st.traces, ex.traces) and eq(st.log_weights, ex.log_weights) and eq(st.parents, par)
    assert eq(g.get_block_params(st), g.get_block_params(ex)) and eq(g.block_stats(st, bs), g.block_stats(ex, bs))
    if y_next is not None:                                                    # one further step on both: every block resamples, so parents agree as well
        for s in (st, ex):
            g.pf_run_blocks(s, y_next, bs, "multinomial", ess_frac=None)
        assert eq(st.traces, ex.traces) and eq(st.log_weights, ex.log_weights) and eq(st.parents, ex.parents)


def proposals(g, B, k=0):
    return [g.models.lgssm2(rho=(0.9, 0.95, 0.99)[(b + k) % 3], sr=(0.3, 0.5, 0.8, 0.4)[(b + k) % 4]) for b in range(B)]


# ----------------------------------------------------------------------------- 1. the main grid
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("keep_mass", [False, True])
@pytest.mark.parametrize("method", ["multinomial", "residual", "stratified"])
@pytest.mark.parametrize("bs", SIZES)
def test_lockstep_with_the_loop(g, bs, method, keep_mass, T):
    n, B, m = 3 * bs + 7, 4, g.models.lgssm2()
    ys = np.ascontiguousarray(block_obs(g, m, B, T + 1))
    # thresholds on the twin's own estimates: blocks 0 and 2 accept, 1 and 3 do not
    st, r, ex, par, acc, Lp, twin, shift = the_loop(g, m, n, bs, ys[:, :T], proposals(g, B, 1), np.array([-1.0, 1.0, -1.0, 1.0]), method, keep_mass,
                                                    state_params=proposals(g, B), relative=True)
    assert eq(acc, [True, False, True, False])
    check(g, st, r, ex, par, acc, Lp, bs, ys[:, T:])
    for s in (st, ex, twin):
        s.close()


def test_the_mass_shift_in_extended_precision(g):
    n, bs, B, m = 3 * 129 + 7, 129, 4, g.models.lgssm2()
    ys = np.ascontiguousarray(block_obs(g, m, B, 3))
    st, r, ex, par, acc, Lp, twin, shift = the_loop(g, m, n, bs, ys, proposals(g, B, 1), np.full(B, -INF), "residual", True)
    assert acc.all()
    L = np.longdouble
    Ls = g.block_stats(g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, params=[m] * B), bs)[1]
    want = L(twin.log_weights) + np.repeat(L(Ls) - L(r.lml), bs)[:n]
    got = st.log_weights
    assert eq(r.accepted, L(r.lml) > L(np.full(B, -INF)))
    assert np.all(np.abs(L(got) - want) <= np.spacing(np.abs(got)))            # one ulp of the double result


# ----------------------------------------------------------------------------- 2. other models, series forms, options
@pytest.mark.parametrize("name,bs,method", [("bearings4", 65, "residual"), ("sv1", 130, "stratified"), ("object_motion", 600, "multinomial"),
                                            ("line_model", 100, "multinomial"), ("bearings4", 513, "stratified")])
def test_other_models(g, name, bs, method):
    n, B = 3 * bs + 7, 4
    if name == "line_model":
        m = g.models.line_model()
        ys = np.stack([[g.models.line_obs(t + 1, float(s)) for t in range(4)] for s in (-2, 0, 1, 2)])
    else:
        m = model_of(g, name)
        ys = np.ascontiguousarray(block_obs(g, m, B, 4))
    thr = np.array([-INF, INF, -INF, INF])
    st, r, ex, par, acc, Lp, *_ = the_loop(g, m, n, bs, ys[:, :3], [m] * B, thr, method, True)
    assert eq(acc, [True, False, True, False])
    check(g, st, r, ex, par, acc, Lp, bs, ys[:, 3:])


@pytest.mark.parametrize("bs,method,ess_frac,sort_particles", [(100, "residual", 0.5, True), (300, "multinomial", None, True), (100, "stratified", 0.5, False),
                                                               (600, "stratified", None, False)])
def test_shared_series_and_options(g, bs, method, ess_frac, sort_particles):
    n, B, m = 3 * bs + 7, 4, g.models.lgssm2()
    y = np.ascontiguousarray(g.models.simulate(m, 4))
    thr = np.array([-INF, INF, -INF, -INF])
    kw = dict(ess_frac=ess_frac, sort_particles=sort_particles)
    st, r, ex, par, acc, Lp, *_ = the_loop(g, m, n, bs, y, proposals(g, B), thr, method, True, shared=True, **kw)
    check(g, st, r, ex, par, acc, Lp, bs)
    tiled = np.ascontiguousarray(np.broadcast_to(y, (B,) + y.shape))          # a per-block copy of the series: the same call
    st2, r2, *_ = the_loop(g, m, n, bs, tiled, proposals(g, B), thr, method, True, **kw)
    assert eq(r.lml, r2.lml) and eq(st.traces, st2.traces) and eq(st.log_weights, st2.log_weights) and eq(st.parents, st2.parents)


# ----------------------------------------------------------------------------- 3. threshold extremes, invalid weights
@pytest.mark.parametrize("keep_mass", [False, True])
@pytest.mark.parametrize("bs", [100, 300])
def test_threshold_extremes(g, bs, keep_mass):
    n, B, m = 3 * bs + 7, 4, g.models.lgssm2()
    ys = np.ascontiguousarray(block_obs(g, m, B, 3))
    st, r, ex, par, acc, Lp, twin, shift = the_loop(g, m, n, bs, ys, proposals(g, B), np.full(B, -INF), "multinomial", keep_mass)
    assert acc.all() and eq(st.traces, twin.traces) and eq(st.parents, twin.parents)
    assert eq(st.log_weights, twin.log_weights + np.repeat(shift, bs)[:n] if keep_mass else twin.log_weights)
    check(g, st, r, ex, par, acc, Lp, bs)
    before = (st.traces, st.log_weights, st.parents, g.get_block_params(st))
    r = g.pf_pmmh_blocks(st, ys, proposals(g, B, 2), np.full(B, INF), bs, seed=5, keep_mass=keep_mass)
    assert not r.accepted.any() and np.isfinite(r.lml).all()
    assert all(eq(x, y) for x, y in zip(before, (st.traces, st.log_weights, st.parents, g.get_block_params(st))))


@pytest.mark.parametrize("bs", [100, 300])
def test_invalid_weights_are_no_error(g, bs):
    n, B, m = 3 * bs + 7, 4, g.models.line_model()
    ys = np.stack([[g.models.line_obs(t + 1, float(s)) for t in range(3)] for s in (-2, 0, 1, 2)])
    ys[1, 2, 0] = 1e200                                                       # no particle of block 1 supports it: z^2 overflows, all weights -Inf
    st, r, ex, par, acc, Lp, *_ = the_loop(g, m, n, bs, ys, [m] * B, np.full(B, -INF), "multinomial", False)
    assert eq(acc, [True, False, True, True]) and not np.isfinite(Lp[1])
    check(g, st, r, ex, par, acc, Lp, bs)
    ys[1, 2, 0] = ys[0, 2, 0]
    st, r, ex, par, acc, Lp, *_ = the_loop(g, m, n, bs, ys, [m] * B, np.full(B, -INF), "multinomial", True, spoil=2 * bs + 1)
    assert eq(acc, [True, True, False, True])                                 # block 2 of the state holds a NaN weight: kept as it is
    check(g, st, r, ex, par, acc, Lp, bs)


# ----------------------------------------------------------------------------- 4. refusals: the state unchanged
def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.parametrize("case,status", [("n_steps_0", 1), ("n_steps_4098", 1), ("method", 3), ("n_obs", 1), ("block_size", 1), ("other_block_size", 1),
                                         ("params_null", 1), ("thr_null", 1), ("n_params", 1), ("n_blocks", 1), ("params_nan", 1), ("thr_nan", 1),
                                         ("obs_inf", 1), ("no_params", 6), ("keep_prev", 6), ("view", 6)])
def test_refusals_leave_the_state_alone(g, case, status):
    n, bs, B, m = 307, 100, 4, g.models.lgssm2()
    ys = np.ascontiguousarray(block_obs(g, m, B, 3))
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, params=None if case == "no_params" else [m] * B, keep_prev=case == "keep_prev")
    rows = g.block_params_rows(m, [m] * B, n, bs)
    thr = np.zeros(B)
    a = dict(obs=ys, n_obs=2, n_steps=3, bs=bs, params=pd(rows), n_params=rows.shape[1], thr=pd(thr), n_blocks=B, method=0)
    if case == "n_steps_0": a["n_steps"] = 0
    if case == "n_steps_4098": a["n_steps"] = 4098
    if case == "method": a["method"] = 7
    if case == "n_obs": a["n_obs"] = 1
    if case == "block_size": a["bs"] = 0
    if case == "other_block_size": a["bs"] = 50
    if case == "params_null": a["params"] = None
    if case == "thr_null": a["thr"] = None
    if case == "n_params": a["n_params"] = 25
    if case == "n_blocks": a["n_blocks"] = B + 1
    if case == "params_nan": rows[2, 1] = np.nan
    if case == "thr_nan": thr[3] = np.nan
    if case == "obs_inf": a["obs"] = ys.copy(); a["obs"][1, 2, 0] = INF
    h = st[0:100] if case == "view" else st
    before = st.checkpoint().tobytes()
    acc, lml = np.zeros(B, np.int32), np.zeros(B)
    got = st._L.gpf_pmmh_blocks(h._h, pd(a["obs"]), a["n_obs"], a["n_steps"], 0, a["bs"], a["params"], a["n_params"], a["thr"], a["n_blocks"], 77,
                                a["method"], 1, 0.5, 1, acc.ctypes.data_as(C.POINTER(C.c_int32)), pd(lml))
    assert got == status and st._L.gpf_last_error(h._h)
    assert st.checkpoint().tobytes() == before
