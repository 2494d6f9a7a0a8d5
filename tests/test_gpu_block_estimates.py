"""Per-block posterior estimates in one launch: gpf_block_moments / gpf_block_proportion (gpf_k_block.hpp) -- the batched form of the
reference's `for b in blocks; mean(state[b], addr); var(state[b], addr); proportionmap(state[b], addr); end` (src/statistics.jl:13-14,
48-50, 91-101 on ParticleFilterSubStates, src/view.jl:35-48).  Every value must EQUAL (as a double, NaN-aware; the sign of a zero is not part of
the claim) the oracle's o_wsum over the block's rows with the block's own weight summary (tests/test_block_estimates_host.py pins that reference to
the summation tree of DESIGN.md §3.5), and the device's own mean / var / proportionmap on a view of the block."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def make(g, o, model_name, N, seed=11, keep_prev=False, T=6):
    m = g.models.by_name(model_name); ys = g.models.simulate(m, T)
    st = g.pf_initialize(m, (1,), ys[0], N, seed=seed, keep_prev=keep_prev)
    f = o.OracleFilter(m.model_id, m.params, N, seed, keep_prev=keep_prev).initialize(ys[0])
    return m, ys, st, f


def same_state(st, f):
    return np.array_equal(st.traces, f.rows) and np.array_equal(st.log_weights, f.lw, equal_nan=True) and np.array_equal(st.parents, f.parents)


def eq(a, b):
    """equality of doubles, NaN == NaN"""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def oracle_value(o, f, a, b, col, pw, c=0.0):
    """mean (pw 1), var term sum around c (pw 2) or proportion of value c (pw 3) of the sub-state f[a:b]; NaN for NaN / +Inf weights"""
    v = f[a:b]
    s = v.summary()
    if s.bad:
        return float("nan")
    return o.lib().o_wsum(s.q, s.S, np.ascontiguousarray(v.rows), f.W, col, v.n, pw, float(c))


def oracle_moments(o, f, nb):
    B = (f.n + nb - 1) // nb
    mu, s2 = np.empty((B, f.W)), np.empty((B, f.W))
    for k, a in enumerate(range(0, f.n, nb)):
        b = min(a + nb, f.n)
        for c in range(f.W):
            mu[k, c] = oracle_value(o, f, a, b, c, 1)
            s2[k, c] = oracle_value(o, f, a, b, c, 2, mu[k, c])
    return mu, s2


def oracle_proportions(o, f, nb, col, values):
    B = (f.n + nb - 1) // nb
    out = np.empty((B, len(values)))
    for k, a in enumerate(range(0, f.n, nb)):
        for j, v in enumerate(values):
            out[k, j] = oracle_value(o, f, a, min(a + nb, f.n), col, 3, v)
    return out


def run_steps(g, o, st, f, ys, nb, steps=3, method="multinomial"):
    """a few update / block-resample steps, then one more update: the weights differ inside every block"""
    for t in range(1, steps + 1):
        g.pf_update(st, (t + 1,), (None,), ys[t]); f.update(ys[t])
        g.pf_resample_blocks(st, nb, method, check=False)
        from oracle import oracle
        oracle.resample_blocks(f, nb, method, check=False)
    g.pf_update(st, (steps + 2,), (None,), ys[steps + 1]); f.update(ys[steps + 1])
    assert same_state(st, f)


# 1. the three team shapes and their edges (<= 128: a wave, 2 per lane; <= 512: a wave, 8 per lane; else a workgroup), ragged last blocks
@pytest.mark.parametrize("N,nb", [(100, 100), (1000, 100), (4096, 2048), (5000, 2048), (777, 64), (37, 1), (2500, 1000), (300, 7),
                                  (3000, 300), (2100, 512), (1000, 129), (640, 128), (1539, 513), (11, 2)])
def test_moments_equal_the_oracle_per_block(g, o, N, nb):
    m, ys, st, f = make(g, o, "lgssm2", N)
    run_steps(g, o, st, f, ys, nb)
    mu, s2 = g.block_moments(st, nb)
    rmu, rs2 = oracle_moments(o, f, nb)
    assert mu.shape == s2.shape == ((N + nb - 1) // nb, st.row_width)
    assert eq(mu, rmu), (N, nb, "mean")
    assert eq(s2, rs2), (N, nb, "var")
    # the one-output forms and the column forms are the same numbers
    assert eq(g.block_mean(st, nb), mu) and eq(g.block_var(st, nb), s2)
    for c in range(st.row_width):
        assert eq(g.block_mean(st, nb, c), mu[:, c]) and eq(g.block_var(st, nb, c), s2[:, c])
    assert same_state(st, f)
    st.close()


# 2. row widths 2, 4 and 8: every column, the x_{t-1} columns of keep_prev included
@pytest.mark.parametrize("model_name,keep_prev", [("bearings4", True), ("sv1", True), ("bearings4", False), ("object_motion", False)])
@pytest.mark.parametrize("nb", [100, 300, 1000])
def test_moments_other_row_widths(g, o, model_name, keep_prev, nb):
    m, ys, st, f = make(g, o, model_name, 3 * nb + nb // 2, keep_prev=keep_prev)
    run_steps(g, o, st, f, ys, nb, method="residual")
    mu, s2 = g.block_moments(st, nb)
    rmu, rs2 = oracle_moments(o, f, nb)
    assert mu.shape[1] == f.W
    assert eq(mu, rmu), (model_name, keep_prev, nb, "mean")
    assert eq(s2, rs2), (model_name, keep_prev, nb, "var")
    st.close()


# 3. against the device's own views, a sample of blocks; nb > 2048 is the library's loop over view handles
@pytest.mark.parametrize("N,nb", [(1000, 100), (3000, 300), (5000, 2048), (10_000, 4096), (5000, 2049)])
def test_equal_the_device_views(g, o, N, nb):
    m, ys, st, f = make(g, o, "object_motion", N)
    for t in range(1, 4):
        g.pf_update(st, (t + 1,), (None,), ys[t]); f.update(ys[t])
    mu, s2 = g.block_moments(st, nb)
    vals, pr = g.block_proportionmap(st, nb, 0)
    B = (N + nb - 1) // nb
    rmu, rs2 = oracle_moments(o, f, nb)
    assert eq(mu, rmu) and eq(s2, rs2)                                       # (also the loop path equals the oracle)
    for k in sorted({0, B // 2, B - 1}):
        a, b = k * nb, min((k + 1) * nb, N)
        v = st[a:b]
        for c in range(st.row_width):
            assert mu[k, c] == g.mean(v, c) and s2[k, c] == g.var(v, c), (N, nb, k, c)
        pm = g.proportionmap(v, 0)
        for j, x in enumerate(vals):
            assert pr[k, j] == pm.get(float(x), 0.0), (N, nb, k, x)
        v.close()
    st.close()


# 4. proportions of a discrete column
def line_filters(g, o, N, seed=5, T=4):
    m = g.models.line_model()
    st = g.pf_initialize(m, (0,), g.models.line_obs(0), N, seed=seed)
    f = o.OracleFilter(m.model_id, m.params, N, seed).initialize(g.models.line_obs(0))
    for t in range(1, T):
        g.pf_update(st, (t,), (None,), g.models.line_obs(t, 1.0)); f.update(g.models.line_obs(t, 1.0))
    return m, st, f


@pytest.mark.parametrize("N,nb", [(1030, 100), (2100, 512), (4500, 2048), (600, 7), (300, 1), (301, 2), (700, 128), (1000, 129), (1539, 513)])
@pytest.mark.parametrize("which", ["object_motion.moving", "line_model.outlier", "line_model.slope"])
def test_proportions_equal_the_oracle(g, o, which, N, nb):
    if which == "object_motion.moving":
        m, ys, st, f = make(g, o, "object_motion", N)
        for t in range(1, 4):
            g.pf_update(st, (t + 1,), (None,), ys[t]); f.update(ys[t])
        col = 0
    else:
        m, st, f = line_filters(g, o, N)
        col = 1 if which.endswith("outlier") else 0
    assert same_state(st, f)
    # block 1 is made to hold ONE value only: the other values are absent from it (and present elsewhere), whatever the model drew
    rows = st.traces.copy()
    first = np.unique(rows[:, col])[0]
    rows[nb:2 * nb, col] = first
    st.traces = rows; f.rows = rows.copy()
    vals, pr = g.block_proportionmap(st, nb, col)
    assert vals.size >= 2 and vals[0] == first and np.all(pr[1, 1:] == 0.0)
    assert eq(vals, np.unique(f.rows[:, col])) and pr.shape == ((N + nb - 1) // nb, vals.size)
    assert eq(pr, oracle_proportions(o, f, nb, col, vals)), (which, N, nb)
    assert np.all(np.abs(pr.sum(axis=1) - 1.0) <= 4 * EPS * vals.size), np.abs(pr.sum(axis=1) - 1.0).max()
    # a value that no particle (of any block) holds, next to values that blocks do hold: 0.0 for it, the same numbers for the others
    req = np.ascontiguousarray(np.concatenate([vals[:1], [12345.5], vals[1:]])[:16])
    out = np.empty((pr.shape[0], req.size))
    st._check(st._L.gpf_block_proportion(st._h, nb, col, g.api._pd(req), req.size, g.api._pd(out)))
    assert np.all(out[:, 1] == 0.0) and eq(out[:, 0], pr[:, 0]) and eq(out[:, 2:], pr[:, 1:req.size - 1])
    # ... and wherever a block lacks a value (block 1 by construction; small blocks now and then): 0.0 there, as the oracle says
    held = np.array([[np.any(f.rows[a:a + nb, col] == x) for x in vals] for a in range(0, N, nb)])
    assert not held[1, 1:].any() and np.all(pr[~held] == 0.0)
    st.close()


def test_more_than_16_values_go_in_chunks(g, o):
    """18 distinct values in a column: two calls of 16 and 2; more than max_values raises like proportionmap"""
    N, nb = 900, 100
    m, ys, st, f = make(g, o, "lgssm2", N)
    rows = st.traces.copy()
    rows[:, 1] = (np.arange(N) * 7) % 18
    st.traces = rows; f.rows = rows.copy()
    g.pf_update(st, (2,), (None,), ys[1]); f.update(ys[1])
    rows = st.traces.copy(); rows[:, 1] = (np.arange(N) * 7) % 18
    st.traces = rows; f.rows = rows.copy()
    vals, pr = g.block_proportionmap(st, nb, 1)
    assert vals.size == 18 and eq(pr, oracle_proportions(o, f, nb, 1, vals))
    with pytest.raises(g.ErrorException, match="distinct values"):
        g.block_proportionmap(st, nb, 1, max_values=17)
    st.close()


# 5. adversarial weights per block
def adversarial_weights(nb, rng):
    blocks = [np.zeros(nb), np.where(np.arange(nb) == 17 % nb, 0.0, -800.0), np.full(nb, -np.inf), -700.0 * rng.random(nb),
              np.where(rng.random(nb) < 0.8, -np.inf, -rng.random(nb)), -1e-9 * rng.random(nb), np.full(nb, -3.25),
              -np.arange(nb, dtype=np.float64), np.where(np.arange(nb) % 2 == 0, -0.0, 0.0), -50.0 * rng.random(nb) ** 4]
    nan_block = -rng.random(nb); nan_block[nb // 3] = np.nan
    inf_block = -rng.random(nb); inf_block[nb - 1] = np.inf
    blocks.insert(4, nan_block); blocks.insert(8, inf_block)
    blocks[4 + 1][0] = 0.0                                                   # (the -Inf-heavy block keeps at least one finite weight)
    kinds = ["ok"] * len(blocks)
    kinds[2], kinds[4], kinds[8] = "neginf", "nan", "posinf"
    return np.concatenate(blocks), kinds


@pytest.mark.parametrize("nb", [100, 400, 1000])
def test_adversarial_block_weights(g, o, nb):
    """equal, one dominant, all -Inf (uniform), wide range, -Inf-heavy, ...; a block with a NaN and one with +Inf are NaN, their neighbours are not"""
    lw, kinds = adversarial_weights(nb, np.random.default_rng(5))
    N = lw.size
    m, ys, st, f = make(g, o, "object_motion", N)
    g.pf_update(st, (2,), (None,), ys[1]); f.update(ys[1])
    st.log_weights = lw; f.lw = lw.copy()
    mu, s2 = g.block_moments(st, nb)
    vals, pr = g.block_proportionmap(st, nb, 0)
    rmu, rs2 = oracle_moments(o, f, nb)
    rpr = oracle_proportions(o, f, nb, 0, vals)
    for k, kind in enumerate(kinds):
        if kind in ("nan", "posinf"):
            assert np.isnan(mu[k]).all() and np.isnan(s2[k]).all() and np.isnan(pr[k]).all(), (k, kind)
            continue
        assert eq(mu[k], rmu[k]) and eq(s2[k], rs2[k]) and eq(pr[k], rpr[k]), (k, kind)
        assert np.isfinite(mu[k]).all() and np.isfinite(s2[k]).all() and abs(pr[k].sum() - 1.0) <= 4 * EPS * vals.size, (k, kind)
        if kind == "neginf":                                                 # what the device's own view of the block returns
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                v = st[k * nb:(k + 1) * nb]
                for c in range(st.row_width):
                    assert mu[k, c] == g.mean(v, c) and s2[k, c] == g.var(v, c)
                pm = g.proportionmap(v, 0)
                assert all(pr[k, j] == pm.get(float(x), 0.0) for j, x in enumerate(vals))
                v.close()
    assert eq(st.log_weights, lw)
    st.close()


def test_big_blocks_with_an_invalid_block(g, o):
    """the loop path (blocks beyond 2048 particles): a NaN block is NaN, the others equal the oracle"""
    N, nb = 9000, 4000
    m, ys, st, f = make(g, o, "lgssm2", N)
    g.pf_update(st, (2,), (None,), ys[1]); f.update(ys[1])
    lw = st.log_weights.copy(); lw[nb + 5] = np.nan
    st.log_weights = lw; f.lw = lw.copy()
    mu, s2 = g.block_moments(st, nb)
    rmu, rs2 = oracle_moments(o, f, nb)
    assert np.isnan(mu[1]).all() and np.isnan(s2[1]).all()
    assert eq(mu, rmu) and eq(s2, rs2) and np.isfinite(mu[[0, 2]]).all()
    st.close()


# 6. no side effects: a filter that reads its estimates at every step stays bit-identical to one that never does
def test_no_side_effects(g, o):
    N, nb, T = 3050, 100, 7
    m = g.models.object_motion()
    B = (N + nb - 1) // nb
    base = np.asarray(g.models.simulate(m, T))
    ys = base[None, :, :] + 0.2 * np.random.default_rng(3).standard_normal((B,) + base.shape)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], N, nb, seed=13, keep_prev=True) for _ in range(2))

    def read(x):
        g.block_moments(x, nb); g.block_mean(x, nb, 1); g.block_var(x, nb); g.block_proportionmap(x, nb, 0)

    read(a)
    for t in range(1, T):
        for x in (a, b):
            g.pf_update_blocks(x, (t + 1,), (None,), ys[:, t], nb)
            if x is a:
                read(x)
            g.pf_resample_blocks(x, nb, "residual", ess_frac=0.5, check=False)
            if x is a:
                read(x)
            g.pf_rejuvenate_blocks(x, None, (), 1, method="move" if t % 2 else "reweight", only_resampled=True)
            if x is a:
                read(x)
    assert np.array_equal(a.traces, b.traces) and np.array_equal(a.log_weights, b.log_weights) and np.array_equal(a.parents, b.parents)
    assert np.array_equal(g.block_resampled(a), g.block_resampled(b))
    ea, la = g.block_stats(a, nb); eb, lb = g.block_stats(b, nb)
    assert eq(ea, eb) and eq(la, lb) and g.get_lml_est(a) == g.get_lml_est(b)
    assert eq(g.block_moments(a, nb)[0], g.block_moments(b, nb)[0])
    a.close(); b.close()


# 7. per-block parameters: the estimates of block b equal those of a filter created with block b's parameters
def test_with_block_params(g, o):
    N, nb, T = 1030, 100, 4
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    B = (N + nb - 1) // nb
    assign = (np.arange(B) * np.arange(B) + np.arange(B) // 2) % 3
    base = np.asarray(g.models.simulate(sets[0], T))
    ys = base[None, :, :] + 0.3 * np.random.default_rng(7).standard_normal((B,) + base.shape)
    st = g.pf_initialize_blocks(sets[0], (1,), ys[:, 0], N, nb, seed=13, keep_prev=True, params=[sets[k] for k in assign])
    twins = [g.pf_initialize_blocks(s, (1,), ys[:, 0], N, nb, seed=13, keep_prev=True) for s in sets]
    for t in range(1, T):
        for x in [st] + twins:
            g.pf_update_blocks(x, (t + 1,), (None,), ys[:, t], nb)
            if t < T - 1:
                g.pf_resample_blocks(x, nb, "residual", ess_frac=0.5, check=False)
                g.pf_rejuvenate_blocks(x, None, (), 1, method="move", only_resampled=True)
    mu, s2 = g.block_moments(st, nb)
    vals, pr = g.block_proportionmap(st, nb, 0)
    assert list(vals) == [0.0, 1.0]
    tw = []
    for x in twins:
        tmu, ts2 = g.block_moments(x, nb)
        tpr = np.empty((B, 2))
        x._check(x._L.gpf_block_proportion(x._h, nb, 0, g.api._pd(np.array([0.0, 1.0])), 2, g.api._pd(tpr)))
        tw.append((tmu, ts2, tpr))
    for k in range(B):
        tmu, ts2, tpr = tw[assign[k]]
        assert eq(mu[k], tmu[k]) and eq(s2[k], ts2[k]) and eq(pr[k], tpr[k]), k
    assert len({tuple(tw[j][0][0]) for j in range(3)}) == 3                  # (the parameter sets do give different estimates)
    for x in [st] + twins:
        x.close()


# 8. refused calls leave the state untouched
def test_refusals_leave_the_state_alone(g, o):
    N, nb = 600, 100
    m, ys, st, f = make(g, o, "object_motion", N)
    g.pf_update(st, (2,), (None,), ys[1]); f.update(ys[1])
    L, h, pd = st._L, st._h, g.api._pd
    W = st.row_width
    B = N // nb
    mu, pr, v16 = np.full((B, W), 7.0), np.full((B, 17), 7.0), np.arange(17, dtype=np.float64)
    INV, STATE = g._lib.ERR_INVALID_ARGUMENT, g._lib.ERR_STATE
    assert L.gpf_block_moments(h, nb, None, None) == INV                     # both outputs NULL
    assert L.gpf_block_moments(h, 0, pd(mu), None) == INV                    # block_size < 1
    assert L.gpf_block_proportion(h, nb, -1, pd(v16), 2, pd(pr)) == INV      # a column out of range
    assert L.gpf_block_proportion(h, nb, W, pd(v16), 2, pd(pr)) == INV
    assert L.gpf_block_proportion(h, nb, 0, pd(v16), 0, pd(pr)) == INV       # n_values 0 or 17
    assert L.gpf_block_proportion(h, nb, 0, pd(v16), 17, pd(pr)) == INV
    assert L.gpf_block_proportion(h, nb, 0, None, 2, pd(pr)) == INV
    assert L.gpf_block_proportion(h, nb, 0, pd(v16), 2, None) == INV
    assert L.gpf_block_moments(None, nb, pd(mu), None) == INV
    assert np.all(mu == 7.0) and np.all(pr == 7.0)                           # nothing was written
    with pytest.raises(g.ErrorException):
        g.block_mean(st, nb, W)
    with pytest.raises(g.ErrorException):
        g.block_var(st, nb, -1)
    with pytest.raises(g.ErrorException, match="trajectory store"):
        g.block_mean(st, nb, (2, 0))                                         # a past-step address
    with pytest.raises(g.ErrorException, match="trajectory store"):
        g.block_proportionmap(st, nb, (2, 0))
    view = st[0:200]
    with pytest.raises(g.ErrorException, match="view"):
        g.block_moments(view, nb)
    with pytest.raises(g.ErrorException, match="view"):
        g.block_proportionmap(view, nb, 0)
    shard = g.DeviceParticleFilterState(m, 200, seed=1, n_global=400, gid0=0)
    L.gpf_initialize(shard._h, pd(np.ascontiguousarray(ys[0])), 2)
    assert L.gpf_block_moments(shard._h, nb, pd(mu), None) == STATE and "shard" in L.gpf_last_error(shard._h).decode()
    assert L.gpf_block_proportion(shard._h, nb, 0, pd(v16), 2, pd(pr)) == STATE and "shard" in L.gpf_last_error(shard._h).decode()
    hist = g.pf_initialize(m, (1,), ys[0], 200, seed=1, history=4)
    assert L.gpf_block_moments(hist._h, nb, pd(mu), None) == STATE and "trajectory" in L.gpf_last_error(hist._h).decode()
    assert L.gpf_block_proportion(hist._h, nb, 0, pd(v16), 2, pd(pr)) == STATE and "trajectory" in L.gpf_last_error(hist._h).decode()
    assert np.all(mu == 7.0) and np.all(pr == 7.0)
    # the filter is where the oracle is, and goes on from there exactly as it
    assert same_state(st, f) and g.get_lml_est(st) == f.log_ml_estimate()
    from oracle import oracle
    g.pf_resample_blocks(st, nb, "multinomial", check=False); oracle.resample_blocks(f, nb, "multinomial", check=False)
    g.pf_update(st, (3,), (None,), ys[2]); f.update(ys[2])
    assert same_state(st, f)
    rmu, rs2 = oracle_moments(o, f, nb)
    got = g.block_moments(st, nb)
    assert eq(got[0], rmu) and eq(got[1], rs2)
    for x in (view, shard, hist, st):
        x.close()
