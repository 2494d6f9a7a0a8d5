"""Resampling across blocks on the device (gpf.h gpf_resample_across_blocks) against tests/across_blocks_spec.py -- the expected result
composed from the CPU oracle: rows, log-weights, parents, block ancestors, ESS, the gate's verdict and the next block_stats bit for bit; the
ancestors of a real device filter of B particles; per-block parameters and observations travelling with their block; refusals that change
nothing."""
import warnings

import numpy as np
import pytest

import across_blocks_spec as xs
import block_params_spec as bp

pytestmark = pytest.mark.gpu

SHAPES = [(100, 100), (200, 100), (300, 100), (37, 1), (777, 7), (4096, 64), (8192, 2048), (4098, 2049), (25700, 100), (65792, 256)]
CASES = [("multinomial", True), ("residual", True), ("stratified", True), ("stratified", False)]


def same_state(st, f):
    return np.array_equal(st.traces, f.rows) and np.array_equal(st.log_weights, f.lw) and np.array_equal(st.parents, f.parents)


def make(g, o, model_name, N, bs, keep_prev=True, seed=13, T=4):
    """a device state and its oracle after a block-wise initialisation and T - 1 block-wise updates, every block on its own data"""
    m = g.models.by_name(model_name)
    ys = xs.block_data(g.models, m, N // bs, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, bs, seed=seed, keep_prev=keep_prev)
    for t in range(1, T):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs)
    f = xs.uneven_oracle(o, m, ys, N, bs, seed, keep_prev=keep_prev)
    return m, ys, st, f


def check_call(g, o, st, f, bs, method, sort_particles=True, ess_frac=None, check=False):
    """one call on both sides; everything the call reports and leaves behind must agree"""
    A = g.pf_resample_across_blocks(st, bs, method, ess_frac=ess_frac, sort_particles=sort_particles, check=check)
    plan = xs.resample_across_blocks(o, f, bs, method, ess_frac=ess_frac, sort_particles=sort_particles, check=check)
    assert (A is not None) == plan.resampled
    assert st._across_ess == plan.ess or (np.isnan(st._across_ess) and np.isnan(plan.ess))
    if plan.resampled:
        assert A.dtype == np.int64 and np.array_equal(A, plan.A + 1) and np.array_equal(g.block_ancestors(st), A)
    assert same_state(st, f)
    ess, lml = g.block_stats(st, bs)
    assert np.array_equal(lml, xs.block_logweights(f, bs))
    return plan


@pytest.mark.parametrize("method,sort_particles", CASES)
@pytest.mark.parametrize("N,bs", SHAPES)
def test_device_equals_spec(g, o, N, bs, method, sort_particles):
    m, ys, st, f = make(g, o, "lgssm2", N, bs)
    assert same_state(st, f)
    plan = check_call(g, o, st, f, bs, method, sort_particles)
    assert plan.resampled
    # the state goes on: the next block-wise step reads the copied rows, weights and observations under the advanced epoch
    T = ys.shape[1]
    obs = ys[plan.A, T - 1]
    g.pf_rejuvenate_blocks(st, None, (), 1, method="move"); o.rejuvenate_blocks(f, bs, obs, "move")
    assert same_state(st, f)
    g.pf_update_blocks(st, (T + 1,), (None,), ys[:, 0], bs); o.update_blocks(f, bs, ys[:, 0])
    assert same_state(st, f)
    st.close()


@pytest.mark.parametrize("model_name,keep_prev,width", [("lgssm2", False, 2), ("bearings4", False, 4), ("bearings4", True, 8), ("sv1", True, 2),
                                                        ("object_motion", False, None)])
def test_row_widths(g, o, model_name, keep_prev, width):
    N, bs = 3300, 300
    m, ys, st, f = make(g, o, model_name, N, bs, keep_prev=keep_prev)
    assert width is None or st.row_width == width
    check_call(g, o, st, f, bs, "residual")
    check_call(g, o, st, f, bs, "multinomial")                       # twice in a row: the second call reads what the first one wrote
    st.close()


def test_grid_stride(g, o):
    """the gather's grid is sized by bytes and capped at 2048 workgroups of 16 KB of rows each: 600000 particles of 8 doubles are 2344 chunks, so
    workgroups take a second chunk; the last chunk is partial"""
    N, bs = 600_000, 1000
    m, ys, st, f = make(g, o, "bearings4", N, bs, keep_prev=True, T=2)
    assert st.row_width == 8 and N * 4 > 2048 * 1024 and (N * 4) % 1024 != 0
    check_call(g, o, st, f, bs, "residual")
    st.close()


@pytest.mark.parametrize("method,sort_particles", CASES)
def test_same_ancestors_as_a_device_filter_of_B_particles(g, o, method, sort_particles):
    N, bs, T = 25700, 100, 4
    m, ys, st, f = make(g, o, "lgssm2", N, bs, T=T)
    L = g.block_stats(st, bs)[1]
    A = g.pf_resample_across_blocks(st, bs, method, sort_particles=sort_particles, check=False)
    twin = g.pf_initialize(m, (1,), ys[0, 0], N // bs, seed=13)      # the same number of epoch-advancing calls: initialise + T - 1 updates
    for t in range(1, T):
        g.pf_update(twin, (t + 1,), (None,), ys[0, t])
    twin.log_weights = L
    kw = {"sort_particles": sort_particles} if method == "stratified" else {}
    g.pf_resample(twin, method, check=False, **kw)
    assert np.array_equal(twin.parents, A)
    twin.close(); st.close()


def test_everything_travels(g, o):
    """per-block parameters and observations move with their block: outer resample -> rejuvenate -> update equals the composed oracle with
    assign[A]; get_block_params = the input rows permuted by A; checkpoint -> restore -> set_block_params(get_block_params) continues bit for bit"""
    N, bs, T = 1200, 100, 4
    m = g.models.lgssm2()
    sets = [g.models.lgssm2(rho=0.9, sr=0.3), g.models.lgssm2(rho=0.99, sr=0.8, theta=0.3), g.models.lgssm2(sq=0.3, s0=2.0)]
    B = N // bs
    assign = (np.arange(B) * np.arange(B) + np.arange(B) // 2) % 3
    ys = xs.block_data(g.models, m, B, T + 3)
    rows_in = np.stack([sets[k].params for k in assign])
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, bs, seed=13, keep_prev=True, params=rows_in)
    ref = bp.ParamBlocksOracle(o, m.model_id, [s.params for s in sets], assign, N, bs, 13, keep_prev=True).initialize(ys[:, 0])
    assert np.array_equal(g.get_block_params(st), rows_in)
    perm = np.arange(B)
    for t in range(1, T):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs); ref.update(ys[:, t])
        A = g.pf_resample_across_blocks(st, bs, "residual", check=False)
        plan = xs.resample_across_param_blocks(ref, "residual", check=False)
        assert np.array_equal(A, plan.A + 1) and same_state(st, ref), t
        perm = perm[plan.A]
        assert np.array_equal(g.get_block_params(st), rows_in[perm]) and np.array_equal(ref.assign, assign[perm])
        g.pf_rejuvenate_blocks(st, None, (), 1, method="move" if t % 2 else "reweight")
        ref.rejuvenate(ys[plan.A, t], "move" if t % 2 else "reweight")
        assert same_state(st, ref), ("rejuvenate", t)
        assert np.array_equal(g.block_stats(st, bs)[1], ref.block_lml())
    # a checkpoint does not hold the rows
    blob = st.checkpoint()
    rows_now = g.get_block_params(st)
    st2 = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, bs, seed=13, keep_prev=True)
    st2.restore(blob)
    g.set_block_params(st2, rows_now, bs)
    for t in range(T, T + 3):
        for x in (st, st2):
            g.pf_update_blocks(x, (t + 1,), (None,), ys[:, t], bs)
        ref.update(ys[:, t])
        assert same_state(st, ref) and same_state(st2, ref), t
        As = [g.pf_resample_across_blocks(x, bs, "stratified", ess_frac=0.9, check=False) for x in (st, st2)]
        plan = xs.resample_across_param_blocks(ref, "stratified", ess_frac=0.9, check=False)
        for A in As:
            assert (A is None) == (not plan.resampled) and (A is None or np.array_equal(A, plan.A + 1))
        assert same_state(st, ref) and same_state(st2, ref), t
    assert np.array_equal(g.get_block_params(st), g.get_block_params(st2))
    st.close(); st2.close()


def test_gate_not_fired(g, o):
    N, bs = 1200, 100
    m, ys, st, f = make(g, o, "bearings4", N, bs)
    rows, lw, par = st.traces, st.log_weights, st.parents
    plan = check_call(g, o, st, f, bs, "multinomial", ess_frac=1e-9)
    assert not plan.resampled
    assert np.array_equal(st.traces, rows) and np.array_equal(st.log_weights, lw) and np.array_equal(st.parents, par)
    # the epoch has advanced once: the next block-wise steps match the oracle that advanced its epoch too
    T = ys.shape[1]
    g.pf_rejuvenate_blocks(st, None, (), 1, method="move"); o.rejuvenate_blocks(f, bs, ys[:, T - 1], "move")
    g.pf_update_blocks(st, (T + 1,), (None,), ys[:, 0], bs); o.update_blocks(f, bs, ys[:, 0])
    assert same_state(st, f)
    # equal block weights: ESS exactly B, `<` does not fire at ess_frac = 1
    st2 = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, bs, seed=13)
    st2.log_weights = np.zeros(N)
    assert g.pf_resample_across_blocks(st2, bs, "residual", ess_frac=1.0) is None and st2._across_ess == N // bs
    assert g.pf_resample_across_blocks(st2, bs, "residual", ess_frac=float(np.nextafter(1.0, 2.0))) is not None
    st.close(); st2.close()


def test_invalid_weights(g, o):
    N, bs = 400, 100
    for bad in (np.nan, np.inf):
        m, ys, st, f = make(g, o, "lgssm2", N, bs)
        lw = st.log_weights; lw[150] = bad
        st.log_weights = lw; f.lw[150] = bad
        rows, par = st.traces, st.parents
        for check in (True, "warn", False):
            with pytest.raises(g.ErrorException, match="Invalid weights"):
                g.pf_resample_across_blocks(st, bs, "multinomial", check=check)
        assert np.array_equal(st.traces, rows) and np.array_equal(st.log_weights, lw, equal_nan=True) and np.array_equal(st.parents, par)
        # state AND epoch untouched: repaired weights, then the next step draws from the stream of the unadvanced epoch
        lw[150] = -1.0; st.log_weights = lw; f.lw[150] = -1.0
        T = ys.shape[1]
        g.pf_update_blocks(st, (T + 1,), (None,), ys[:, 0], bs); o.update_blocks(f, bs, ys[:, 0])
        assert same_state(st, f)
        st.close()
    for check in (True, "warn", False):
        m, ys, st, f = make(g, o, "lgssm2", N, bs)
        st.log_weights = np.full(N, -np.inf); f.lw[:] = -np.inf
        if check is True:
            with pytest.raises(g.ErrorException, match="Invalid weights"):
                g.pf_resample_across_blocks(st, bs, "stratified", check=True)
            with pytest.raises(o.OracleError):
                xs.resample_across_blocks(o, f, bs, "stratified", check=True)
        else:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                plan = check_call(g, o, st, f, bs, "stratified", check=check)
            assert plan.resampled and plan.invalid
            assert (sum("Invalid block weights" in str(x.message) for x in w) == 1) == (check == "warn")
        T = ys.shape[1]
        st.log_weights = np.zeros(N); f.lw[:] = 0.0
        g.pf_update_blocks(st, (T + 1,), (None,), ys[:, 0], bs); o.update_blocks(f, bs, ys[:, 0])
        assert same_state(st, f), check
        st.close()


def test_refusals_change_nothing(g, o):
    N, bs = 1200, 100
    m, ys, st, f = make(g, o, "lgssm2", N, bs)
    rows, lw, par = st.traces, st.log_weights, st.parents
    with pytest.raises(g.ErrorException, match="gpf_block_ancestors"):
        g.block_ancestors(st)
    for bad_bs in (0, -5, 7, 500, 1201):                            # < 1; 1200 % bs != 0
        with pytest.raises(g.ErrorException):
            g.pf_resample_across_blocks(st, bad_bs, "multinomial")
    with pytest.raises(g.ErrorException, match="not recognized"):
        g.pf_resample_across_blocks(st, bs, "multinomial_sorted")
    with pytest.raises(g.ErrorException):
        g.pf_resample_across_blocks(st[0:600], bs, "multinomial")
    view = st[0:600]
    assert st._L.gpf_resample_across_blocks(view._h, 0, bs, 1, float("nan"), 0, None, None, None) == g._lib.ERR_STATE
    assert st._L.gpf_resample_across_blocks(st._h, 4, bs, 1, float("nan"), 0, None, None, None) == g._lib.ERR_UNKNOWN_METHOD
    assert st._L.gpf_resample_across_blocks(st._h, 0, 7, 1, float("nan"), 0, None, None, None) == g._lib.ERR_INVALID_ARGUMENT
    with pytest.raises(g.ErrorException):
        g.get_block_params(st)                                       # none are set
    # per-block parameters of another block size
    g.set_block_params(st, [m] * (N // 200), 200)
    with pytest.raises(g.ErrorException, match="per-block parameters"):
        g.pf_resample_across_blocks(st, bs, "multinomial")
    g.set_block_params(st, None)
    assert np.array_equal(st.traces, rows) and np.array_equal(st.log_weights, lw) and np.array_equal(st.parents, par)
    T = ys.shape[1]
    g.pf_update_blocks(st, (T + 1,), (None,), ys[:, 0], bs); o.update_blocks(f, bs, ys[:, 0])
    assert same_state(st, f)                                         # the RNG stream of the unadvanced epoch
    # a filter with a trajectory store
    hs = g.pf_initialize(m, (1,), ys[0, 0], N, seed=1, history=4)
    with pytest.raises(g.ErrorException, match="trajectory store"):
        g.pf_resample_across_blocks(hs, bs, "multinomial")
    hs.close(); st.close()


def test_side_effects(g, o):
    N, bs = 1200, 100
    m, ys, st, f = make(g, o, "lgssm2", N, bs)
    g.pf_resample_blocks(st, bs, "residual", check=False)
    g.pf_rejuvenate_blocks(st, None, (), 1, only_resampled=True)     # fine: the mask is current
    g.pf_resample_blocks(st, bs, "residual", check=False)
    assert g.pf_resample_across_blocks(st, bs, "multinomial", check=False) is not None
    with pytest.raises(g.ErrorException, match="only_resampled"):
        g.pf_rejuvenate_blocks(st, None, (), 1, only_resampled=True)  # the mask is stale: it named blocks of the old layout
    with pytest.raises(g.ErrorException):
        g.block_resampled(st)
    # a resize invalidates the block ancestors
    assert g.block_ancestors(st).size == N // bs
    g.pf_resize(st, 600, "multinomial", check=False)
    with pytest.raises(g.ErrorException, match="gpf_block_ancestors"):
        g.block_ancestors(st)
    st.close()


def test_pending_work_is_materialised_first(g, o):
    """a deferred gather (whole-filter resample) and a lazy move in front of the call"""
    N, bs = 1200, 100
    m = g.models.lgssm2()
    ys = np.asarray(g.models.simulate(m, 4))
    st = g.pf_initialize(m, (1,), ys[0], N, seed=5, keep_prev=True)
    f = o.OracleFilter(m.model_id, m.params, N, 5, keep_prev=True).initialize(ys[0])
    g.pf_update(st, (2,), (None,), ys[1]); f.update(ys[1])
    g.pf_rejuvenate(st, None, (), 1, method="reweight"); f.rejuvenate("reweight", 1)
    check_call(g, o, st, f, bs, "residual")
    g.pf_resample(st, "multinomial", check=False); f.resample("multinomial", check=False)
    check_call(g, o, st, f, bs, "multinomial")                       # all weights 0 after the whole-filter resample: equal block weights
    g.pf_update(st, (3,), (None,), ys[2]); f.update(ys[2])
    assert same_state(st, f) and g.get_lml_est(st) == f.log_ml_estimate()
    st.close()


def test_known_answer(g, o):
    """the adaptive theta grid of tests/test_across_blocks_host.py on the device: equal to the oracle rehearsal bit for bit, hence inside its band"""
    est, assign, ref, ms, ys, plans = xs.xka_oracle(o, g.models)
    B, bs = assign.size, xs.XKA_NB
    N = B * bs
    rows_in = np.stack([m.params for m in ms])[np.arange(B) % len(ms)]
    st = g.pf_initialize_blocks(ms[0], (1,), np.tile(ys[0], (B, 1)), N, bs, seed=xs.XKA_SEED, keep_prev=False, params=rows_in)
    perm = np.arange(B)
    for t in range(1, xs.XKA_T):
        g.pf_update_blocks(st, (t + 1,), (None,), np.tile(ys[t], (B, 1)), bs, proposals=[g.locally_optimal] * B)
        g.pf_resample_blocks(st, bs, "residual", ess_frac=0.5, check=False)
        A = g.pf_resample_across_blocks(st, bs, xs.XKA_METHOD, ess_frac=0.5, check=False)
        assert (A is not None) == plans[t - 1].resampled
        if A is not None:
            assert np.array_equal(A, plans[t - 1].A + 1)
            perm = perm[A - 1]
    assert same_state(st, ref)
    assert np.array_equal(g.get_block_params(st), rows_in[perm]) and np.array_equal(assign, (np.arange(B) % len(ms))[perm])
    got = g.log_ml_estimate(st)
    assert got == est
    ev = xs.xka_evidence(ms, ys, g.models)
    assert -xs.XKA_TOL_BELOW < got - ev < xs.XKA_TOL_ABOVE
    counts = np.bincount(assign, minlength=len(ms))
    assert bp.KA_GRID[int(np.argmax(counts))] == bp.KA_TRUE
    st.close()
