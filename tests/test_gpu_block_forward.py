"""Forward-only smoothing per block on the device (gpf.h gpf_forward_enable_blocks, gpf_block_forward_moments):

  1. all seven outputs bit for bit against the NumPy restatement of tests/block_forward_spec.py, which is fed only with what a caller sees: four models,
     block sizes 1, 2, 7 and 2048, both sides of every edge at which the kernels change shape, the query after every step and after every call of a
     step, keep_prev;
  2. against the store on the same state: the six identities of tests/test_block_forward_host.py with block_smoothed_pair_moments on the device; line_model;
  3. the same bits with and without a store; the query changes nothing, and a close after a query gives the bits of a run without the query;
  4. the ESS gate's unequal weights, per-block parameters, the nested filter, a rejuvenation between resample and update, a -Inf particle, a target on
     its fallback, a NaN block;
  5. every refusal, with state and statistics unchanged afterwards;
  6. what the feature is for: 200 steps without a store, where a store of 8 steps refuses the ninth.

The edges.  k_block_forward gives a WAVE 64 consecutive targets of one block and a workgroup four waves: 64 | 65 is one or two waves per block, 256 | 257
four or five (a block's waves in one workgroup or two).  Its candidates are read through wave-uniform addresses, not through tiles: there is no tile size.
k_block_forward_reduce takes its team shape from team_dispatch: 128 | 129 (2 or 8 particles per lane of a wave) and 512 | 513 (a wave or the workgroup)."""
import ctypes as C

import numpy as np
import pytest

import block_forward_spec as fsp
from test_block_forward_host import LEVELS, assert_inside, gamma, identities, k_fwd
from test_gpu_block_backward import MODELS, SEED, SIZES, T, Dev, quiet
from test_gpu_block_conditional import block_obs, eq, n_of, refused, snapshot, unchanged

pytestmark = pytest.mark.gpu
EDGES = [63, 64, 65, 128, 129, 256, 257, 512, 513]
assert set(SIZES) >= {1, 2, 7, 2048}
NAMES = fsp.Moments._fields[:6]


class Forward:
    """the package with forward=True passed to every pf_initialize_blocks -- and, store=False, without the store Dev asks for"""

    def __init__(self, g, store=True):
        self._g, self._store = g, store

    def __getattr__(self, name):
        return getattr(self._g, name)

    def pf_initialize_blocks(self, *a, **kw):
        if not self._store:
            kw["history"], kw["history_weights"] = 0, False
        return self._g.pf_initialize_blocks(*a, forward=True, **kw)


class FDev(Dev):
    """Dev with the forward mode on.  The restatement runs in lockstep, one close per look: `every`: the query is compared after every update (before
    the step's resamples) and after the last call of every step; `at`: only after the last call of these steps (track: the restatement still closes every step as it ends, so that a long run costs one close per step);
    neither: nothing is compared on the way.
    rejuvenate: pf_rejuvenate_blocks behind the step's resamples (keep_prev).  P: the parameters the restatement uses (default: the model's)."""

    def __init__(self, g, o, name, bs, *, store=True, every=False, at=(), track=False, rejuvenate=False, P=None, after_update=None, **kw):
        self.o, self.has_store, self.every, self.at, self.track, self.rejuvenate, self.P = o, store, every, set(at), track, rejuvenate, P
        self.T_prev, self.T_cur, self.t_cur, self.looks = None, None, 0, 0

        def hook(d, t):
            if after_update is not None:
                after_update(d, t)
            if d.every:
                d.record()
                d.look(("after the update", t))

        super().__init__(Forward(g, store), name, bs, after_update=hook, **kw)
        self.g = g

    def record(self):
        s = self.S.steps
        x = np.stack([self.st.history_column(s, c) for c in range(self.m.dim)], axis=1) if self.has_store else self.st.traces[:, :self.m.dim]
        self.S.end_step(x, self.st.log_weights)

    def end_step(self):                                                      # (Dev calls it after the last call of every step)
        if self.rejuvenate and self.S.steps >= 2:
            self.g.pf_rejuvenate_blocks(self.st, None, (), 1, method="move")
            self.epoch += 1
        self.record()
        if self.every or self.S.steps in self.at:
            self.look(("the step's last call", self.S.steps))
        elif self.track:
            self.statistics()

    def statistics(self):
        """the restatement's T of the current step from its T of the step closed last: kept from the last look of that step, else formed from step 1"""
        S, t = self.S, self.S.steps
        name = "line_model" if self.m.name == "line_model" else self.m.name
        P = self.m.params if self.P is None else self.P
        if t != self.t_cur:
            in_step = t == self.t_cur + 1 and self.T_cur is not None
            self.T_prev = self.T_cur if in_step else fsp.statistics(self.o, name, P, S, t - 1) if t > 1 else None
            self.t_cur = t
        if t == 1:
            self.T_cur = fsp.first(S.x(1))
        else:
            self.T_cur = fsp.close(self.o, name, P, self.T_prev, S.x(t - 1), S.lw[t - 2], S.x(t), S.step_map(t), S.obs[t - 1], S.bs)
        return self.T_cur

    def want(self):
        t = self.S.steps
        return fsp.query(self.o, self.statistics(), self.S.x(t), self.S.lw[t - 1], self.S.bs, t)

    def got(self):
        return self.g.block_forward_moments(self.st, self.bs)

    def look(self, where):
        check(self.got(), self.want(), (self.m.name, self.bs) + where)
        self.looks += 1


def check(a, b, where):
    assert a.n_steps == b.n_steps, (where, a.n_steps, b.n_steps)
    for what, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape, (where, what, x.shape, y.shape)
        assert eq(x, y), (where, what, np.argwhere(~((x == y) | (np.isnan(x) & np.isnan(y))))[:5])


def same(a, b):
    return a.n_steps == b.n_steps and all(eq(x, y) for x, y in zip(a[:6], b[:6]))


# ----------------------------------------------------------------------------- 1. bit for bit against the restatement
CASES = [(name, bs, False) for name in MODELS for bs in (1, 2, 7, 2048)] + [(name, bs, False) for name in ("lgssm2", "bearings4") for bs in EDGES] + \
        [(name, bs, True) for name in MODELS for bs in (7, 513)]


@pytest.mark.parametrize("name,bs,keep_prev", CASES)
def test_all_outputs_are_the_restatement_after_every_step(g, o, name, bs, keep_prev):
    d = FDev(g, o, name, bs, keep_prev=keep_prev, every=bs < 2048, at=range(1, T + 1))
    assert d.looks == (2 * T if bs < 2048 else T)
    r = d.got()
    dim, B = d.m.dim, d.B
    assert r.n_steps == T and r.sum.shape == r.first.shape == (B, dim) and all(x.shape == (B, dim, dim) for x in (r.second, r.cross, r.first2, r.last2))
    for m2 in (r.second, r.first2, r.last2):
        assert np.array_equal(m2, m2.transpose(0, 2, 1))
    assert all(np.all(np.isfinite(x)) for x in r[:6])
    assert eq(r.last2, g.block_smoothed_pair_moments(d.st, bs, steps=T)[1][:, 0])            # the pairwise smoother's second at the last step
    d.close()


def test_the_cross_moment_carries_dependence(g, o):
    """somewhere cross is not sum_s mean_s (x) mean_{s+1}, nor its own transpose (otherwise the tests above could pass on either)"""
    d = FDev(g, o, "lgssm2", 129)
    r = d.got()
    mean = g.block_smoothed_pair_moments(d.st, 129)[0]
    assert np.max(np.abs(r.cross - (mean[:, :-1, :, None] * mean[:, 1:, None, :]).sum(axis=1))) > 1e-4
    assert np.max(np.abs(r.cross - r.cross.transpose(0, 2, 1))) > 1e-4
    d.close()


# ----------------------------------------------------------------------------- 2. against the store on the same state
def device_back(d):
    mean, second, cross, blocks = d.g.block_smoothed_pair_moments(d.st, d.bs, return_blocks=True)
    return mean, second, cross, blocks, d.g.block_smoothed_weights(d.st, d.bs)


@pytest.mark.parametrize("name,bs", [("lgssm2", 7), ("object_motion", 129), ("bearings4", 513), ("sv1", 2048)])
def test_the_six_identities_against_the_pairwise_smoother_on_the_device(g, o, name, bs):
    d = FDev(g, o, name, bs)
    d.record()
    assert_inside(identities(o, name, d.m.params, d.S, got=d.got(), back=device_back(d)), (name, bs, "device"))
    d.close()


def test_line_model_cross_of_the_slopes_is_second_minus_last2(g, o):
    """no pair links two slopes (tests/test_gpu_block_pairs.py), so in exact arithmetic cross[0][0] = sum_{s<T} second_s[0][0] = second[0][0] - last2[0][0].
    All terms are squares: sum|terms| is second[0][0] itself up to its own gamma.  Roundings: K_FWD on either statistic, 2 + LEVELS on last2, the
    difference formed here"""
    bs = 129
    d = FDev(g, o, "line_model", bs, n=8 * bs, at=[T])
    r = d.got()
    k = k_fwd(T, bs)
    second, cross, last2 = r.second[:, 0, 0], r.cross[:, 0, 0], r.last2[:, 0, 0]
    bound = (2 * gamma(k) + gamma(3 + LEVELS)) * second / (1 - gamma(k))
    err = np.abs(cross - (second - last2))
    live = second > 0
    print("line_model, cross[slope][slope] against second - last2: worst error / bound", float((err[live] / bound[live]).max()))
    assert live.any() and np.all(second >= 0) and np.all(err <= bound), (err.max(), bound.min())
    d.record()
    assert_inside(identities(o, "line_model", d.m.params, d.S, got=r, back=device_back(d)), "line_model, device")
    d.close()


# ----------------------------------------------------------------------------- 3. with and without a store; the query changes nothing
@pytest.mark.parametrize("bs", [7, 300])
def test_the_same_bits_with_and_without_a_store(g, o, bs):
    a, b = FDev(g, o, "lgssm2", bs, ess_frac=0.5), FDev(g, o, "lgssm2", bs, ess_frac=0.5, store=False, at=[T])
    assert eq(a.st.traces, b.st.traces) and eq(a.st.log_weights, b.st.log_weights)
    assert same(a.got(), b.got())
    with pytest.raises(g.ErrorException):                                    # (b has no store to smooth over)
        g.block_smoothed_pair_moments(b.st, bs)
    a.close(); b.close()


@pytest.mark.parametrize("store", [True, False])
def test_the_query_changes_nothing_and_the_close_recomputes(g, o, store):
    bs = 129
    a, b = FDev(g, o, "object_motion", bs, store=store, keep_prev=True, every=True), FDev(g, o, "object_motion", bs, store=store, keep_prev=True)
    assert a.looks == 2 * T and b.looks == 0
    before = snapshot(a.st, store)
    r1, r2 = a.got(), a.got()
    assert same(r1, r2) and unchanged(before, snapshot(a.st, store))        # rows, weights, parents, the store's records and (checkpoint) the epoch
    assert same(r1, b.got())                                                 # every close of `a` came after queries, none of `b`
    if not store:                                                            # (one more step, which a store of T steps has no room for)
        ys = block_obs(g, a.m, a.B, T + 1, seed=11)[:, T]
        for d in (a, b):
            g.pf_update_blocks(d.st, (T + 1,), (None,), ys, bs)
        assert same(a.got(), b.got()) and a.got().n_steps == T + 1
    a.close(); b.close()


# ----------------------------------------------------------------------------- 4. special cases
def test_the_ess_gate_leaves_unequal_weights_and_blocks_that_did_not_resample(g, o):
    d = FDev(g, o, "lgssm2", 7, n=40 * 7 + 5, ess_frac=0.5, every=True)
    assert d.n_res > 0 and d.n_not > 0, (d.n_res, d.n_not)
    d.close()


def test_per_block_parameters_are_the_blocks_current_rows(g, o):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    bs = 129
    assign = np.arange((n_of(bs) + bs - 1) // bs) % 3
    P = np.stack([sets[k].params for k in assign])
    d = FDev(g, o, "object_motion", bs, keep_prev=True, params=[sets[k] for k in assign], P=P, every=True)
    r = d.got()
    d.record()
    assert not eq(r.cross, fsp.forward(o, "object_motion", sets[0].params, d.S).cross)       # (the rows matter)
    d.close()


@pytest.mark.parametrize("bs", [8, 300])
def test_the_nested_filter(g, o, bs):
    d = FDev(g, o, "object_motion", bs, n=24 * bs, keep_prev=True, ess_frac=0.8, across=True, at=range(1, T + 1))
    assert d.fired > 0 and d.looks == T
    blocks = g.block_smoothed_pair_moments(d.st, bs, return_blocks=True)[3]
    assert np.any(blocks != blocks[:, -1:])                                  # (some lineage changed its block)
    d.record()
    assert_inside(identities(o, "object_motion", d.m.params, d.S, got=d.got(), back=device_back(d)), ("nested", bs))
    d.close()


@pytest.mark.parametrize("store", [True, False])
def test_a_rejuvenation_between_resample_and_update(g, o, store):
    d = FDev(g, o, "lgssm2", 129, keep_prev=True, rejuvenate=True, store=store, at=range(1, T + 1))
    plain = FDev(g, o, "lgssm2", 129, keep_prev=True, store=store)
    assert d.looks == T and not same(d.got(), plain.got())                   # (the moves are in the statistics)
    d.close(); plain.close()


@pytest.mark.parametrize("bs,B", [(7, 64), (513, 3)])
def test_a_particle_of_weight_zero_is_a_dead_candidate(g, o, bs, B):
    dead = np.arange(bs * B) % bs % 2 == 1                                   # local 1, 3, 5 of every block

    def kill(d, t):
        if t == 2:                                                           # step 2, which no resample follows: the -Inf weights stay in its record
            lw = d.st.log_weights
            lw[dead] = -np.inf
            d.st.log_weights = lw

    d = FDev(g, o, "lgssm2", bs, n=bs * B, resample=False, after_update=kill, every=True)
    assert np.all(np.isneginf(d.S.lw[1][dead])) and np.all(np.isfinite(d.S.lw[1][~dead]))
    assert all(np.all(np.isfinite(x)) for x in d.got()[:6])
    d.close()


@pytest.mark.parametrize("bs,B", [(129, 4), (513, 4)])
def test_a_target_on_its_fallback(g, o, bs, B):
    odd = np.arange(bs * B) % 3 == 0

    def foreign_slope(d, t):
        if t >= T - 1:                                                       # a slope outside uniform_discrete(-2, 2), which no particle of the step before
            rows = d.st.traces                                               # holds, and equal weights, so that the step's resample keeps such particles
            rows[odd, 0] = 7.0 + t
            d.st.traces = rows
            d.st.log_weights = np.zeros(bs * B)

    d = FDev(g, o, "line_model", bs, n=bs * B, after_update=foreign_slope, final_resample=True, every=True)
    assert np.any(d.S.x(T)[:, 0] == 7.0 + T) and np.any(d.S.x(T)[:, 0] < 7.0) and np.any(d.S.x(T - 1)[:, 0] == 6.0 + T)
    r = d.got()
    assert np.any(r.cross[:, 0, 0] != r.second[:, 0, 0] - r.last2[:, 0, 0])                  # (the foreign targets pair two slopes)
    d.close()


@pytest.mark.parametrize("bs", [7, 513])                                      # (n_of: three full blocks and a short fourth)
def test_a_nan_block_reads_nan(g, o, bs):
    a, b = FDev(g, o, "lgssm2", bs), FDev(g, o, "lgssm2", bs)
    lw = b.st.log_weights
    lw[bs + 3] = np.nan
    b.st.log_weights = lw
    ra, rb = a.got(), b.got()
    assert all(np.all(np.isnan(x[1])) for x in rb[:6]) and rb.n_steps == T
    keep = np.arange(a.B) != 1
    assert all(eq(x[keep], y[keep]) for x, y in zip(ra[:6], rb[:6]))
    a.close(); b.close()


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_change_nothing(g, o):
    m = g.models.object_motion()
    bs, n, B = 7, 28, 4
    ys = block_obs(g, m, B, 4)
    E, lib = g.ErrorException, g._lib
    L = lib.load()
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    NAN = float("nan")
    y0 = np.ascontiguousarray(ys[0, 0])
    n_obs = y0.size

    def raw(st, size=bs, out=True):
        return L.gpf_block_forward_moments(st._h, size, P(np.empty(B * 2)) if out else None, None, None, None, None, None, None)

    # the query: the mode is off; nothing is initialised; a NULL handle
    plain = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED)
    refused(g, plain, lambda: g.block_forward_moments(plain, bs), E, store=False)
    assert raw(plain) == lib.ERR_STATE
    plain.close()
    empty = g.DeviceParticleFilterState(m, n, seed=SEED)
    assert L.gpf_forward_enable_blocks(empty._h) == 0 and raw(empty) == lib.ERR_STATE
    empty.close()
    assert L.gpf_forward_enable_blocks(None) == lib.ERR_INVALID_ARGUMENT
    assert L.gpf_block_forward_moments(None, bs, P(np.empty(B * 2)), None, None, None, None, None, None) == lib.ERR_INVALID_ARGUMENT
    # enabling after the initialisation; on a shard
    late = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED)
    assert L.gpf_forward_enable_blocks(late._h) == lib.ERR_STATE
    late.close()
    shard = g.DeviceParticleFilterState(m, n, seed=SEED, n_global=2 * n, gid0=0)
    assert L.gpf_forward_enable_blocks(shard._h) == lib.ERR_STATE
    shard.close()
    # blocks of more than 2048 particles
    with pytest.raises(E, match="2048"):
        g.pf_initialize_blocks(m, (1,), np.tile(ys[0, 0], (2, 1)), 2 * 4096, 4096, seed=SEED, forward=True)

    for store in (True, False):
        kw = dict(history=4, history_weights=True) if store else {}
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=True, forward=True, **kw)
        g.pf_resample_blocks(st, bs, "multinomial", check=False)
        g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
        stats = g.block_forward_moments(st, bs)

        def nothing_changed(call, code=None):
            before = snapshot(st, store)
            if code is None:
                with pytest.raises(E):
                    call()
            else:
                assert call() == code, call
            assert unchanged(before, snapshot(st, store)) and same(stats, g.block_forward_moments(st, bs)), call

        h = st._h
        i32, i64 = C.c_int32(), C.c_int64()
        # the query's own arguments
        nothing_changed(lambda: raw(st, size=0), lib.ERR_INVALID_ARGUMENT)
        nothing_changed(lambda: raw(st, size=13), lib.ERR_INVALID_ARGUMENT)
        nothing_changed(lambda: raw(st, out=False), lib.ERR_INVALID_ARGUMENT)
        nothing_changed(lambda: g.block_forward_moments(st, 13))
        # another clamped block size in a step, a resample, a resample across blocks
        nothing_changed(lambda: g.pf_update_blocks(st, (3,), (None,), ys[:2, 2], 14))
        nothing_changed(lambda: L.gpf_update_blocks(h, P(np.ascontiguousarray(ys[:2, 2])), n_obs, 14), lib.ERR_INVALID_ARGUMENT)
        nothing_changed(lambda: L.gpf_resample_blocks(h, 0, 14, NAN, 0, NAN, 0, None, None), lib.ERR_INVALID_ARGUMENT)
        nothing_changed(lambda: L.gpf_resample_across_blocks(h, 0, 14, 0, NAN, 0, None, None, None), lib.ERR_INVALID_ARGUMENT)
        # a refused block-wise call closes nothing: observations of the wrong shape
        nothing_changed(lambda: g.pf_update_blocks(st, (3,), (None,), ys[:3, 2], bs))
        # the whole-filter calls
        nothing_changed(lambda: L.gpf_initialize(h, P(y0), n_obs), lib.ERR_STATE)
        nothing_changed(lambda: L.gpf_update(h, P(y0), n_obs), lib.ERR_STATE)
        nothing_changed(lambda: g.pf_update(st, (3,), (None,), ys[0, 2]))
        nothing_changed(lambda: L.gpf_step_ess(h, P(y0), n_obs, 0.5, 0, 0, 0, -1, 0, None, None, None), lib.ERR_STATE)
        nothing_changed(lambda: L.gpf_resample(h, 0, NAN, 0, 0, None), lib.ERR_STATE)
        nothing_changed(lambda: g.pf_resample(st, "multinomial", check=False))
        nothing_changed(lambda: L.gpf_resample_local(h, 0, 0, 0, None), lib.ERR_STATE)
        nothing_changed(lambda: L.gpf_resample_with_priorities(h, 0, P(np.zeros(n)), 0, 0, None), lib.ERR_STATE)
        # views, resizing, a checkpoint, a communicator
        nothing_changed(lambda: st[0:7])
        nothing_changed(lambda: L.gpf_resize(h, 2 * n, 0, NAN, 0, None), lib.ERR_STATE)
        nothing_changed(lambda: g.pf_resize(st, 2 * n))
        nothing_changed(lambda: L.gpf_coalesce(h, 0, C.byref(i64)), lib.ERR_STATE)
        nothing_changed(lambda: L.gpf_introduce(h, P(y0), n_obs, 1, 4, 0), lib.ERR_STATE)
        blob = st.checkpoint()                                               # (saved as without the mode ...)
        nothing_changed(lambda: st.restore(blob))                            # (... and not loaded)
        nothing_changed(lambda: L.gpf_comm_create(h, None, 0, 1), lib.ERR_STATE)
        # the state is alive and well: the next step closes step 2
        g.pf_update_blocks(st, (3,), (None,), ys[:, 2], bs)
        assert g.block_forward_moments(st, bs).n_steps == 3
        st.close()
    # a checkpoint of a state with the mode is a checkpoint of one without
    a = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, forward=True)
    b = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED)
    assert bytes(a.checkpoint()) == bytes(b.checkpoint())
    a.close(); b.close()
    # a block size that differs from the per-block parameters'
    sets = [g.models.object_motion(), g.models.object_motion(sy=0.2)]
    bp = g.pf_initialize_blocks(m, (1,), ys[:2, 0], 28, 14, seed=SEED, params=sets, forward=True)
    refused(g, bp, lambda: g.pf_update_blocks(bp, (2,), (None,), ys[:, 1], 7), E, store=False)
    assert g.block_forward_moments(bp, 14).n_steps == 1
    bp.close()


# ----------------------------------------------------------------------------- 6. the point of the feature
def test_two_hundred_steps_without_a_store(g, o):
    """16 blocks of 32 lgssm2 particles, 200 steps, no store: 8 (2 * 14 + 2 + 1) bytes per particle whatever the length.  The restatement runs in lockstep
    (one close per step: 199 x 512 targets in NumPy are this test's seconds) and is compared at steps 50, 100 and 200"""
    steps, bs, B = 200, 32, 16
    d = FDev(g, o, "lgssm2", bs, n=bs * B, steps=steps, ess_frac=0.5, store=False, at=[50, 100, 200], track=True)
    assert d.looks == 3 and d.got().n_steps == steps and d.n_res > 0 and d.n_not > 0
    with pytest.raises(g.ErrorException):
        d.st.history_column(1, 0)                                            # (there is no store)
    d.close()
    # a twin with a store of 8 steps refuses the ninth, whatever the mode
    m = d.m
    st = g.pf_initialize_blocks(m, (1,), d.ys[:, 0], bs * B, bs, seed=SEED, history=8, history_weights=True, forward=True)
    for t in range(1, 8):
        quiet(lambda: g.pf_resample_blocks(st, bs, "multinomial", ess_frac=0.5, check=False))
        g.pf_update_blocks(st, (t + 1,), (None,), d.ys[:, t], bs)
    assert g.block_forward_moments(st, bs).n_steps == 8
    with pytest.raises(g.ErrorException, match="trajectory store full"):
        g.pf_update_blocks(st, (9,), (None,), d.ys[:, 8], bs)
    assert g.block_forward_moments(st, bs).n_steps == 8                       # (the refused step closed nothing)
    st.close()
