"""The block-wise trajectory store on the device (gpf.h gpf_history_enable_blocks, gpf_block_history_moments, gpf_block_history_proportion): the
reference's `mean(state[b], t => :addr)` for many small filters in one state.

  1. / 2.  the recorded genealogy: after every step history_column(t, c) EQUALS, for every t and c, the answer of the NumPy genealogy of
           tests/block_history_spec.py, which is fed only what a caller can see (rows, state.parents, block_resampled, block_ancestors);
  3.       the per-block queries EQUAL gpf_block_moments / gpf_block_proportion on a store-less twin filter whose rows hold the past values;
  4.       refused calls change nothing;
  5.       the README example per block against the exact smoothed posterior.
Sizes: 1000 particles in blocks of 7 / 100 (a wave, 2 per lane), 300 (a wave, 8 per lane), 999 (the workgroup; the last block is ONE particle);
1200 where resampling across blocks needs congruent blocks."""
import ctypes
import warnings

import numpy as np
import pytest

from block_history_spec import Genealogy

pytestmark = pytest.mark.gpu
T = 6
MODELS = ["sv1", "object_motion", "lgssm2", "bearings4"]                     # d = 1, 2, 2, 4
# The data decide which blocks pass the ESS test.  Every block gets the simulated series plus its own noise, whose scale varies from block to block
# and step to step by a factor of up to 8 either way, so that at ess_frac = 0.7 some blocks resample and some do not; sv1's observations say little
# about its state (a larger base scale makes some of them outliers), bearings4's default bearing noise of 0.005 rad pins the state so hard that
# every block always resamples (a wider one is used).  Checked against the CPU oracle of the same loop: every case below sees both kinds.
NOISE = {"sv1": 2.0, "object_motion": 0.3, "lgssm2": 0.3, "bearings4": 0.3}
SIZES = [7, 100, 300, 999]
EDGES = [("sv1", 1), ("object_motion", 2), ("bearings4", 128), ("lgssm2", 129), ("sv1", 512), ("bearings4", 513), ("object_motion", 2048)]
CYCLE = [("multinomial", True), ("residual", True), ("stratified", True), ("stratified", False), ("multinomial", False)]


def eq(a, b):
    """equality of doubles, NaN == NaN"""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def n_blocks(n, bs):
    return (n + bs - 1) // bs


def model_of(g, name):
    return g.models.bearings4(sb=0.5) if name == "bearings4" else g.models.by_name(name)


def block_obs(g, m, n, bs, steps, seed=7):
    """[n_blocks, steps, n_obs]: every block its own data"""
    base = np.asarray(g.models.simulate(m, steps))
    B = n_blocks(n, bs)
    rng = np.random.default_rng(seed)
    scale = NOISE[m.name] * 8.0 ** rng.uniform(-1, 1, (B, steps, 1))
    return base[None, :, :] + scale * rng.standard_normal((B,) + base.shape)


def latent(st):
    return st.traces[:, :st.dim]


def check_genealogy(st, gen, where):
    gen.set_rows(latent(st))
    for t in range(1, gen.steps + 1):
        for c in range(st.dim):
            assert np.array_equal(st.history_column(t, c), gen.trace(t, c)), (where, t, c)


def history_steps(st):
    k = ctypes.c_int32(-1)
    st._check(st._L.gpf_history_steps(st._h, ctypes.byref(k)))
    return k.value


def run(g, model_name, n, bs, keep_prev=True, seed=11, steps=T, whole_at=3, per_step=None, room=0):
    """the README loop per block, `steps` steps: resample (the methods in turn, ess_frac 0.7), rejuvenate the resampled blocks, update with
    per-block observations; at step whole_at a whole-filter resample on top; the store has room for `room` steps more.  Returns (state, genealogy,
    blocks resampled, blocks not resampled)."""
    m = model_of(g, model_name)
    ys = block_obs(g, m, n, bs, steps)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=seed, keep_prev=keep_prev, history=steps + room)
    gen = Genealogy(n)
    gen.begin_step(latent(st))
    n_res = n_not = 0
    if per_step:
        per_step(st, gen, 0)
    for t in range(1, steps):
        method, sort_particles = CYCLE[(t - 1) % len(CYCLE)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            k = g.pf_resample_blocks(st, bs, method, ess_frac=0.7, sort_particles=sort_particles, check=False)
        mask = g.block_resampled(st)
        assert k == mask.sum()
        n_res += int(mask.sum()); n_not += int((~mask).sum())
        gen.resample("blocks", st.parents, mask, bs)
        if keep_prev:
            g.pf_rejuvenate_blocks(st, None, (), 1, method="move", only_resampled=True)
        if t == whole_at:
            g.pf_resample(st, "multinomial", check=False)
            gen.resample("global", st.parents)
        gen.set_rows(latent(st))
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs)
        gen.begin_step(latent(st))
        if per_step:
            per_step(st, gen, t)
    return st, gen, n_res, n_not


# ----------------------------------------------------------------------------- 1. the genealogy, bitwise
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("model_name", MODELS)
def test_genealogy_of_the_block_loop(g, model_name, bs):
    n = 1000

    def per_step(st, gen, t):
        assert history_steps(st) == gen.steps == t + 1
        check_genealogy(st, gen, (model_name, bs, t))
        if t >= 1:                                                            # x_{t-1} travels with the particle: independent of all bookkeeping
            rows = st.traces
            for c in range(st.dim):
                assert np.array_equal(st.history_column(t, c), rows[:, st.dim + c]), (model_name, bs, t, c, "keep_prev")

    st, gen, n_res, n_not = run(g, model_name, n, bs, per_step=per_step)
    assert n_res > 0 and n_not > 0, (n_res, n_not)                            # both branches of the block compose were exercised
    st.close()


def test_genealogy_without_keep_prev(g):
    st, gen, n_res, n_not = run(g, "lgssm2", 1000, 100, keep_prev=False, per_step=lambda st, gen, t: check_genealogy(st, gen, t))
    assert n_res > 0 and n_not > 0, (n_res, n_not)
    st.close()


# ----------------------------------------------------------------------------- 2. with resampling across blocks (the nested filter)
@pytest.mark.parametrize("bs", [8, 100, 300])
def test_genealogy_with_resampling_across_blocks(g, bs):
    n = 1200
    B = n // bs
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    assign = (np.arange(B) * np.arange(B) + np.arange(B) // 2) % 3
    ys = block_obs(g, sets[0], n, bs, T)
    st = g.pf_initialize_blocks(sets[0], (1,), ys[:, 0], n, bs, seed=13, keep_prev=True, params=[sets[k] for k in assign], history=T)
    gen = Genealogy(n)
    gen.begin_step(latent(st))
    fired = held = n_res = n_not = 0
    for t in range(1, T):
        method, sort_particles = CYCLE[(t - 1) % len(CYCLE)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g.pf_resample_blocks(st, bs, method, ess_frac=0.7, sort_particles=sort_particles, check=False)
        mask = g.block_resampled(st)
        n_res += int(mask.sum()); n_not += int((~mask).sum())
        gen.resample("blocks", st.parents, mask, bs)
        check_genealogy(st, gen, (bs, t, "blocks"))
        before = [st.history_column(s, c) for s in range(1, gen.steps + 1) for c in range(st.dim)]
        # t = 2: a gate that cannot fire (ESS < 0); t = 4: one that must (ESS <= B < 1.5 B); else no gate
        ess_frac = {2: 0.0, 4: 1.5}.get(t)
        A = g.pf_resample_across_blocks(st, bs, ("multinomial", "residual", "stratified")[t % 3], ess_frac=ess_frac, check=False)
        if A is None:
            assert t == 2
            held += 1
            after = [st.history_column(s, c) for s in range(1, gen.steps + 1) for c in range(st.dim)]
            assert all(np.array_equal(x, y) for x, y in zip(before, after))   # a call that does not fire composes nothing
        else:
            assert t != 2 and np.array_equal(A, g.block_ancestors(st))
            fired += 1
            parents = np.repeat(A - 1, bs) * bs + np.tile(np.arange(bs), B) + 1     # block b is a copy of block A[b]
            assert np.array_equal(st.parents, parents)
            gen.resample("global", parents)
        check_genealogy(st, gen, (bs, t, "across"))
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs)
        gen.begin_step(latent(st))
        check_genealogy(st, gen, (bs, t, "update"))
        rows = st.traces
        for c in range(st.dim):
            assert np.array_equal(st.history_column(t, c), rows[:, st.dim + c]), (bs, t, c, "keep_prev")
    assert held == 1 and fired == T - 2 and n_res > 0 and n_not > 0, (held, fired, n_res, n_not)
    st.close()


# ----------------------------------------------------------------------------- 3. the queries, bit for bit
def c_moments(st, bs, step=0):
    """the C entry points: gpf_block_moments (step 0: [B, row_width]) or gpf_block_history_moments ([B, dim])"""
    B = n_blocks(st.n_particles, bs)
    mu, s2 = np.empty((B, st.dim if step else st.row_width)), np.empty((B, st.dim if step else st.row_width))
    pd = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if step:
        st._check(st._L.gpf_block_history_moments(st._h, step, bs, pd(mu), pd(s2)))
    else:
        st._check(st._L.gpf_block_moments(st._h, bs, pd(mu), pd(s2)))
    return mu, s2


def c_proportion(st, bs, col, values, step=0):
    values = np.ascontiguousarray(values, np.float64)
    out = np.empty((n_blocks(st.n_particles, bs), values.size))
    pd = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if step:
        st._check(st._L.gpf_block_history_proportion(st._h, step, bs, col, pd(values), values.size, pd(out)))
    else:
        st._check(st._L.gpf_block_proportion(st._h, bs, col, pd(values), values.size, pd(out)))
    return out


def match_values(column, k):
    """k values to ask for: the smallest k - 1 the column holds and one it does not"""
    u = np.unique(column)
    return np.concatenate([u[:k - 1], [u.max() + 1.0]])


def twin_of(g, st, lw):
    """a store-less filter of the same size and model with the given log-weights; its rows are set per query"""
    tw = g.DeviceParticleFilterState(st.model, st.n_particles, seed=3)
    tw.traces = np.zeros((st.n_particles, tw.row_width))
    tw.log_weights = lw
    return tw


def twin_expectation(st, tw, bs, t):
    """what gpf_block_moments / gpf_block_proportion say about the past values t => . sitting in a filter's rows"""
    rows = np.zeros((st.n_particles, tw.row_width))
    for c in range(st.dim):
        rows[:, c] = st.history_column(t, c)
    tw.traces = rows
    mu, s2 = c_moments(tw, bs)
    props = {}
    for c in range(st.dim):
        for k in (3, 16):
            v = match_values(rows[:, c], k)
            props[c, k] = (v, c_proportion(tw, bs, c, v))
    return mu[:, :st.dim], s2[:, :st.dim], props


def queries_equal_the_twin(g, model_name, n, bs):
    st, gen, _, _ = run(g, model_name, n, bs)
    d, B = st.dim, n_blocks(n, bs)
    # (a) step = T is the current step
    mu_now, s2_now = g.block_moments(st, bs)
    mu_T, s2_T = g.block_moments(st, bs, step=T)
    assert mu_T.shape == s2_T.shape == (B, d)
    assert eq(mu_T, mu_now[:, :d]) and eq(s2_T, s2_now[:, :d])
    for c in range(d):
        v = match_values(st.column(c), 16)
        assert eq(c_proportion(st, bs, c, v, step=T), c_proportion(st, bs, c, v))
    # (b) every step against the twin
    tw = twin_of(g, st, st.log_weights)
    for t in range(1, T + 1):
        rmu, rs2, props = twin_expectation(st, tw, bs, t)
        mu, s2 = g.block_moments(st, bs, step=t)
        assert eq(mu, rmu), (model_name, bs, t, "mean")
        assert eq(s2, rs2), (model_name, bs, t, "var")
        assert eq(c_moments(st, bs, step=t)[0], rmu)
        for c in range(d):
            assert eq(g.block_mean(st, bs, (t, c)), rmu[:, c]) and eq(g.block_var(st, bs, (t, c)), rs2[:, c])
            for k in (3, 16):
                v, want = props[c, k]
                assert eq(c_proportion(st, bs, c, v, step=t), want), (model_name, bs, t, c, k, "proportion")
    assert np.all(np.isfinite(mu))
    tw.close(); st.close()


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("model_name", MODELS)
def test_queries_equal_the_estimates_of_a_twin(g, model_name, bs):
    queries_equal_the_twin(g, model_name, 1000, bs)


# the edges of the three team shapes (<= 128: a wave, 2 per lane; <= 512: a wave, 8 per lane; else the workgroup), five whole blocks and a short one
@pytest.mark.parametrize("model_name,bs", EDGES)
def test_queries_equal_the_estimates_of_a_twin_at_the_team_edges(g, model_name, bs):
    queries_equal_the_twin(g, model_name, 5 * bs + (bs + 1) // 2, bs)


def test_block_proportionmap_of_a_past_choice(g):
    bs = 100
    st, gen, _, _ = run(g, "object_motion", 1000, bs)
    vals_now, pr_now = g.block_proportionmap(st, bs, 0)
    vals_T, pr_T = g.block_proportionmap(st, bs, (T, 0))
    assert eq(vals_T, vals_now) and eq(pr_T, pr_now)
    tw = twin_of(g, st, st.log_weights)
    for t in range(1, T + 1):
        vals, pr = g.block_proportionmap(st, bs, (t, 0))
        assert set(vals) <= {0.0, 1.0} and pr.shape == (10, vals.size)
        rows = np.zeros((1000, tw.row_width)); rows[:, 0] = st.history_column(t, 0)
        tw.traces = rows
        assert eq(pr, c_proportion(tw, bs, 0, vals))
        assert np.abs(pr.sum(axis=1) - 1.0).max() < 1e-12
        p1 = pr[:, list(vals).index(1.0)] if 1.0 in vals else np.zeros(10)
        assert np.abs(g.block_mean(st, bs, (t, 0)) - p1).max() < 1e-12       # the mean of a 0/1 choice
    tw.close(); st.close()


@pytest.mark.parametrize("model_name,bs", [("sv1", 100), ("object_motion", 300), ("bearings4", 999)])
def test_a_block_with_nan_weights_reads_nan(g, model_name, bs):
    st, gen, _, _ = run(g, model_name, 1000, bs)
    lw = st.log_weights
    bad = 0 if bs == 999 else 1
    lw[bad * bs + 3] = np.nan
    st.log_weights = lw
    tw = twin_of(g, st, lw)
    for t in (1, T - 1, T):
        rmu, rs2, props = twin_expectation(st, tw, bs, t)
        mu, s2 = g.block_moments(st, bs, step=t)
        assert np.all(np.isnan(mu[bad])) and np.all(np.isnan(s2[bad]))
        others = np.arange(mu.shape[0]) != bad
        assert np.all(np.isfinite(mu[others])) and np.all(np.isfinite(s2[others]))
        assert eq(mu, rmu) and eq(s2, rs2)
        v, want = props[0, 3]
        got = c_proportion(st, bs, 0, v, step=t)
        assert np.all(np.isnan(got[bad])) and eq(got, want)
    tw.close(); st.close()


def test_queries_change_nothing(g):
    bs = 100
    a, _, _, _ = run(g, "object_motion", 1000, bs, room=1)
    b, _, _, _ = run(g, "object_motion", 1000, bs, room=1)
    for t in range(1, T + 1):
        g.block_moments(a, bs, step=t); g.block_mean(a, bs, (t, 1)); g.block_proportionmap(a, bs, (t, 0))
    assert np.array_equal(a.checkpoint(), b.checkpoint())                      # rows, weights, parents, log-ML estimate, RNG epoch
    nxt = block_obs(g, a.model, 1000, bs, 1, seed=99)[:, 0]
    for x in (a, b):                                                           # ... and the step that follows is the same, its record included
        g.pf_resample_blocks(x, bs, "multinomial", check=False)
        g.pf_rejuvenate_blocks(x, None, (), 1, method="move", only_resampled=True)
        if x is a:
            g.block_moments(a, bs, step=T)                                     # (a query between the resample and the update snapshots the step early)
        g.pf_update_blocks(x, (T + 1,), (None,), nxt, bs)
    assert history_steps(a) == history_steps(b) == T + 1
    assert np.array_equal(a.checkpoint(), b.checkpoint())
    for t in range(1, T + 2):
        for c in range(a.dim):
            assert np.array_equal(a.history_column(t, c), b.history_column(t, c)), (t, c)
        assert eq(g.block_moments(a, bs, step=t)[0], g.block_moments(b, bs, step=t)[0])
    a.close(); b.close()


# ----------------------------------------------------------------------------- 4. refusals
def test_the_plain_store_still_refuses_block_calls(g):
    m = g.models.object_motion()
    ys = g.models.simulate(m, 3)
    st = g.pf_initialize(m, (1,), ys[0], 400, seed=1, keep_prev=True, history=4)
    blob = st.checkpoint()
    obs = np.tile(ys[1], (4, 1))
    for call in (lambda: g.pf_resample_blocks(st, 100, "multinomial", check=False),
                 lambda: g.pf_update_blocks(st, (2,), (None,), obs, 100),
                 lambda: g.block_moments(st, 100),
                 lambda: g.block_proportionmap(st, 100, 0),
                 lambda: g.set_block_params(st, [m] * 4, 100),
                 lambda: g.pf_resample_across_blocks(st, 100, check=False),
                 lambda: g.block_mean(st, 100, (1, 0)),
                 lambda: g.block_moments(st, 100, step=1)):
        with pytest.raises(g.ErrorException, match="trajectory store"):
            call()
    L, pd = st._L, g.api._pd
    mu, pr, v2 = np.full((4, 2), 7.0), np.full((4, 2), 7.0), np.array([0.0, 1.0])
    assert L.gpf_block_history_moments(st._h, 1, 100, pd(mu), None) == g._lib.ERR_STATE and "trajectory store" in L.gpf_last_error(st._h).decode()
    assert L.gpf_block_history_proportion(st._h, 1, 100, 0, pd(v2), 2, pd(pr)) == g._lib.ERR_STATE and "trajectory store" in L.gpf_last_error(st._h).decode()
    assert np.all(mu == 7.0) and np.all(pr == 7.0)
    assert np.array_equal(st.checkpoint(), blob) and history_steps(st) == 1
    st.close()


def test_a_storeless_state_refuses_past_addresses(g):
    m = g.models.object_motion()
    ys = block_obs(g, m, 400, 100, 2)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], 400, 100, seed=1)
    blob = st.checkpoint()
    for call in (lambda: g.block_mean(st, 100, (1, 0)), lambda: g.block_var(st, 100, (1, 0)), lambda: g.block_proportionmap(st, 100, (1, 0)),
                 lambda: g.block_moments(st, 100, step=1)):
        with pytest.raises(g.ErrorException, match="trajectory store"):
            call()
    L, pd = st._L, g.api._pd
    mu, pr, v2 = np.full((4, 2), 7.0), np.full((4, 2), 7.0), np.array([0.0, 1.0])
    assert L.gpf_block_history_moments(st._h, 1, 100, pd(mu), pd(mu)) == g._lib.ERR_STATE and "trajectory store" in L.gpf_last_error(st._h).decode()
    assert L.gpf_block_history_proportion(st._h, 1, 100, 0, pd(v2), 2, pd(pr)) == g._lib.ERR_STATE and "trajectory store" in L.gpf_last_error(st._h).decode()
    assert np.all(mu == 7.0) and np.all(pr == 7.0) and np.array_equal(st.checkpoint(), blob)
    st.close()


def test_bad_arguments_and_big_blocks_change_nothing(g):
    n, bs, steps = 4200, 100, 3
    m = g.models.object_motion()
    ys = block_obs(g, m, n, bs, steps)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=5, keep_prev=True, history=steps)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    g.pf_resample_blocks(st, bs, "residual", check=False)
    L, h, pd = st._L, st._h, g.api._pd
    INV, STATE = g._lib.ERR_INVALID_ARGUMENT, g._lib.ERR_STATE
    B, d = n // bs, st.dim
    mu, s2, pr, v17 = np.full((B, d), 7.0), np.full((B, d), 7.0), np.full((B, 17), 7.0), np.arange(17, dtype=np.float64)
    blob, cols = st.checkpoint(), [st.history_column(t, c) for t in (1, 2) for c in range(d)]
    assert history_steps(st) == 2
    for step in (0, 3, -1):                                                   # T = 2
        assert L.gpf_block_history_moments(h, step, bs, pd(mu), pd(s2)) == INV
        assert L.gpf_block_history_proportion(h, step, bs, 0, pd(v17), 2, pd(pr)) == INV
    for col in (-1, d):
        assert L.gpf_block_history_proportion(h, 1, bs, col, pd(v17), 2, pd(pr)) == INV
    for k in (0, 17):
        assert L.gpf_block_history_proportion(h, 1, bs, 0, pd(v17), k, pd(pr)) == INV
    assert L.gpf_block_history_moments(h, 1, bs, None, None) == INV
    assert L.gpf_block_history_moments(h, 1, 0, pd(mu), None) == INV
    assert L.gpf_block_history_proportion(h, 1, bs, 0, None, 2, pd(pr)) == INV
    assert L.gpf_block_history_proportion(h, 1, bs, 0, pd(v17), 2, None) == INV
    assert L.gpf_block_history_moments(None, 1, bs, pd(mu), None) == INV
    assert L.gpf_block_history_proportion(None, 1, bs, 0, pd(v17), 2, pd(pr)) == INV
    # blocks of more than 2048 particles would need sub-state views
    big = 2100
    i32, i64, dbl = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_double(0.0)
    ess = np.full(2, 7.0)
    for status in (L.gpf_block_history_moments(h, 1, big, pd(mu), None),
                   L.gpf_block_history_proportion(h, 1, big, 0, pd(v17), 2, pd(pr)),
                   L.gpf_block_moments(h, big, pd(mu), None),
                   L.gpf_block_proportion(h, big, 0, pd(v17), 2, pd(pr)),
                   L.gpf_block_stats(h, big, pd(ess), None),
                   L.gpf_resample_blocks(h, 0, big, float("nan"), 1, float("nan"), 0, ctypes.byref(i32), ctypes.byref(i64)),
                   L.gpf_resample_across_blocks(h, 0, big, 1, float("nan"), 0, ctypes.byref(i32), ctypes.byref(i32), ctypes.byref(dbl))):
        assert status == STATE and "trajectory store" in L.gpf_last_error(h).decode()
    assert np.all(mu == 7.0) and np.all(s2 == 7.0) and np.all(pr == 7.0) and np.all(ess == 7.0)
    # views and resizing stay refused on either store
    with pytest.raises(g.ErrorException, match="trajectory store"):
        st[0:100]
    with pytest.raises(g.ErrorException, match="trajectory store"):
        g.pf_resize(st, 100)
    assert np.array_equal(st.checkpoint(), blob) and history_steps(st) == 2
    assert all(np.array_equal(x, st.history_column(t, c)) for x, (t, c) in zip(cols, [(t, c) for t in (1, 2) for c in range(d)]))
    # "one block" asked for as any size >= n is one block of n particles: fine up to 2048
    small = g.pf_initialize_blocks(m, (1,), ys[:1, 0], 1000, 1000, seed=5, history=2)
    one = np.empty((1, d))
    assert L.gpf_block_history_moments(small._h, 1, 2 ** 32, pd(one), None) == g._lib.OK
    assert eq(one, g.block_moments(small, 1000, step=1)[0])
    small.close(); st.close()


def test_bad_observations_leave_the_store_alone(g):
    """a block-wise update or initialisation refused for its observations (NULL, wrong width, wrong number of rows) has not begun a step: the step
    count, every past-step column and the checkpoint are what they were"""
    n, bs = 1000, 100
    m = g.models.object_motion()
    ys = block_obs(g, m, n, bs, 4)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=9, keep_prev=True, history=4)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    g.pf_resample_blocks(st, bs, "residual", ess_frac=0.7, check=False)
    L, h, pd = st._L, st._h, g.api._pd
    INV = g._lib.ERR_INVALID_ARGUMENT
    where = [(t, c) for t in (1, 2) for c in range(st.dim)]
    blob, cols = st.checkpoint(), [st.history_column(t, c) for t, c in where]
    obs = np.ascontiguousarray(ys[:, 2])
    flags = np.zeros(n // bs, np.int32)
    pi = flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    strata = np.array([0.0, 1.0])
    for status in (L.gpf_update_blocks(h, pd(obs), obs.shape[1] + 1, bs), L.gpf_update_blocks(h, pd(obs), obs.shape[1] - 1, bs),
                   L.gpf_update_blocks(h, None, obs.shape[1], bs),
                   L.gpf_update_blocks_proposal(h, pd(obs), obs.shape[1] + 1, bs, pi, 1), L.gpf_update_blocks_proposal(h, None, obs.shape[1], bs, pi, 1),
                   L.gpf_update_blocks_strata(h, pd(obs), obs.shape[1] + 1, bs, pd(strata), 2, 1), L.gpf_update_blocks_strata(h, None, obs.shape[1], bs, pd(strata), 2, 1),
                   L.gpf_initialize_blocks(h, pd(obs), obs.shape[1] + 1, bs), L.gpf_initialize_blocks(h, None, obs.shape[1], bs),
                   L.gpf_initialize_blocks_strata(h, None, obs.shape[1], bs, pd(strata), 2, 0)):
        assert status == INV
        assert history_steps(st) == 2
    with pytest.raises(g.ErrorException):
        g.pf_update_blocks(st, (3,), (None,), ys[:5, 2], bs)                   # 5 rows for 10 blocks
    with pytest.raises(g.ErrorException):
        g.pf_update_blocks(st, (3,), (None,), np.zeros((n // bs, 3)), bs)      # the model takes 2 values per block
    assert history_steps(st) == 2 and np.array_equal(st.checkpoint(), blob)
    assert all(np.array_equal(x, st.history_column(t, c)) for x, (t, c) in zip(cols, where))
    # ... and the filter goes on as one that never saw those calls
    twin = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=9, keep_prev=True, history=4)
    g.pf_update_blocks(twin, (2,), (None,), ys[:, 1], bs)
    g.pf_resample_blocks(twin, bs, "residual", ess_frac=0.7, check=False)
    for x in (st, twin):
        g.pf_update_blocks(x, (3,), (None,), ys[:, 2], bs)
    assert history_steps(st) == 3 and np.array_equal(st.checkpoint(), twin.checkpoint())
    for t in (1, 2, 3):
        for c in range(st.dim):
            assert np.array_equal(st.history_column(t, c), twin.history_column(t, c)), (t, c)
    twin.close(); st.close()


def test_past_step_addresses_are_one_based(g):
    m = g.models.object_motion()
    ys = block_obs(g, m, 400, 100, 2)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], 400, 100, seed=1, history=2)
    for call in (lambda: g.block_moments(st, 100, step=0), lambda: g.block_mean(st, 100, (0, 0)), lambda: g.block_var(st, 100, (0, 0)),
                 lambda: g.block_proportionmap(st, 100, (0, 0)), lambda: g.block_mean(st, 100, (-1, 0))):
        with pytest.raises(g.ErrorException, match="1-based"):
            call()
    assert g.block_moments(st, 100, step=1)[0].shape == (4, st.dim)
    st.close()


def test_a_full_store_refuses_the_update_and_changes_nothing(g):
    n, bs = 1000, 100
    m = g.models.object_motion()
    ys = block_obs(g, m, n, bs, 4)

    def start():
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=9, keep_prev=True, history=2)
        g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
        g.pf_resample_blocks(st, bs, "stratified", ess_frac=0.7, check=False)
        return st

    a, b = start(), start()
    cols = [a.history_column(t, c) for t in (1, 2) for c in range(a.dim)]
    with pytest.raises(g.ErrorException, match="trajectory store full"):
        g.pf_update_blocks(a, (3,), (None,), ys[:, 2], bs)
    assert history_steps(a) == 2 and np.array_equal(a.checkpoint(), b.checkpoint())
    assert all(np.array_equal(x, a.history_column(t, c)) for x, (t, c) in zip(cols, [(t, c) for t in (1, 2) for c in range(a.dim)]))
    for x in (a, b):                                                           # the per-block observations are still those of step 2
        g.pf_rejuvenate_blocks(x, None, (), 2, method="move")
    assert np.array_equal(a.checkpoint(), b.checkpoint())
    a.close(); b.close()


# ----------------------------------------------------------------------------- 5. known answer: the README example in every block
def exact_object_motion(model, ys):
    """enumerate the 2^T `moving` sequences of the README model (y is a random walk with sigma_y = 0.01, integrated out as extra observation
    variance) -> exact smoothed P(moving_t | y_1:T)"""
    import itertools, math
    steps, yobs = ys.shape[0], ys[:, 0]
    p_stay, p_start, sy, sobs = model.params[0], model.params[1], model.info["sy"], model.info["sobs"]
    var = sobs ** 2 + np.arange(1, steps + 1) * sy ** 2
    post, Z = np.zeros(steps), 0.0
    for seq in itertools.product([0, 1], repeat=steps):
        p, prev = 1.0, 0
        for mv in seq:
            pm = p_stay if prev else p_start
            p *= pm if mv else 1.0 - pm
            prev = mv
        y = np.cumsum([mv * ys[t, 1] for t, mv in enumerate(seq)])
        w = p * math.exp(np.sum(-0.5 * (yobs - y) ** 2 / var - 0.5 * np.log(2 * np.pi * var)))
        Z += w
        post += w * np.array(seq)
    return post / Z


def test_readme_example_per_block_against_the_exact_posterior(g):
    """64 independent README filters of 100 particles in one state (residual resampling when ESS < N / 2, mh rejuvenation of the resampled blocks),
    the same data for every block, T = 10: the mean over blocks of mean(state[b], t => :moving) against the exact smoothed posterior.
    The bound is that of tests/test_history.py for 32 independent N = 100 filters; here there are 64."""
    model = g.models.object_motion()
    ys = np.asarray(g.models.simulate(model, 10))
    exact = exact_object_motion(model, ys)
    B, N = 64, 100
    st = g.pf_initialize_blocks(model, (1,), np.tile(ys[0], (B, 1)), B * N, N, seed=1, keep_prev=True, history=10)
    for t in range(1, 10):
        g.pf_resample_blocks(st, N, "residual", ess_frac=0.5)
        g.pf_rejuvenate_blocks(st, None, (), 1, method="move", only_resampled=True)
        g.pf_update_blocks(st, (t + 1,), (None,), np.tile(ys[t], (B, 1)), N)
    est = np.array([g.block_mean(st, N, (t, 0)) for t in range(1, 11)])      # [T, B]
    assert est.shape == (10, B) and np.all((est >= 0.0) & (est <= 1.0 + 1e-12))
    err = np.abs(est.mean(axis=1) - exact)
    print("README example per block: mean over blocks", est.mean(axis=1), "exact", exact, "max error", err.max())
    assert err.max() < 0.08, (est.mean(axis=1), exact)
    s2 = g.block_var(st, N, (5, 0))
    assert np.abs(s2 - est[4] * (1.0 - est[4])).max() < 1e-12               # the variance of a 0/1 choice
    st.close()
