"""Ancestor sampling for conditional SMC per block on the device (gpf.h gpf_resample_blocks_ancestor, gpf_block_ancestor_log_weights):

  1. block_ancestor_log_weights is bit for bit the NumPy restatement of Model<M>::logtrans (tests/block_ancestor_spec.py): five models, keep_prev on
     and off, block sizes 7, 129 and 5000, per-block parameters;
  2. lockstep, bit for bit, with AncestorLoop: rows, log-weights, parents, block_resampled, block_stats and history_column at every step over T = 6,
     at the edges of the three team shapes, with and without the ESS gate;
  3. against the conditional call on the same incoming state: only slot 0's row and parent differ, and somewhere they do;
  4. edge weights: -Inf particles are never drawn, a reference no particle can lead to gives a0 = 0, a NaN block is left and reported as before;
  5. ancestor resample, then resampling across blocks, then block_sample_trajectories: the composed genealogy;
  6. refused calls change nothing;
  7. invariance against the exact smoother at T = 8 (tests/test_block_ancestor_host.py runs the same experiment, and its negative control, on the CPU)."""
import ctypes as C
import warnings

import numpy as np
import pytest

import block_ancestor_spec as asp
import block_conditional_spec as cs
from block_history_spec import Genealogy
from block_trajectories_spec import paths
from test_gpu_block_conditional import block_obs, eq, history_steps, model_of, n_of, references, refused, snapshot, unchanged

pytestmark = pytest.mark.gpu
T = 6
MODELS = ["sv1", "object_motion", "lgssm2", "bearings4"]                     # d = 1, 2, 2, 4
SIZES = [1, 2, 7, 128, 129, 512, 513, 2048]                                  # a wave 2 / 8 per lane, the workgroup, and their edges
SEED = 17


def quiet(call):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return call()


# ----------------------------------------------------------------------------- 1. the ancestor log-weights
def line_data(g, B, steps, seed=3):
    """[B, steps, 2] data vectors of line_model: every block its own slope"""
    rng = np.random.default_rng(seed)
    return np.stack([[g.models.line_obs(t + 1, float(s)) for t in range(steps)] for s in rng.integers(-2, 3, B)])


def after_two_steps(g, name, bs, keep_prev, params=None, assign=None):
    """(state after an initialise and two steps, model, data [B, 4, n_obs], reference [B, d] for the step being entered)"""
    m = g.models.line_model() if name == "line_model" else model_of(g, name)
    n = n_of(bs)
    B = (n + bs - 1) // bs
    ys = line_data(g, B, 4) if name == "line_model" else block_obs(g, m, B, 4)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=keep_prev, params=None if params is None else [params[k] for k in assign])
    for t in (1, 2):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs)
    if name == "line_model":                                                 # a slope of the model's support and an outlier flag: some particles hold it, some do not
        ref = np.stack([np.arange(B) % 5 - 2.0, np.arange(B) % 2 * 1.0], axis=1)
    else:
        ref = references(g, m, B, 4)[:, 3]
    return st, m, ys, ref


def state_of(st):
    """everything a call could change: the checkpoint blob (rows, log-weights, parents, epoch, ...) -- without the bytes that pad an odd number of 4-byte
    parents to the blob's 8-byte size, which no one writes -- and the arrays as the package returns them"""
    blob = bytes(st.checkpoint())
    return blob[:len(blob) - 4 * st.n_particles % 8], st.traces, st.log_weights, st.parents, []


@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("bs", [7, 129, 5000])
@pytest.mark.parametrize("name", ["sv1", "lgssm2", "object_motion", "bearings4", "line_model"])
def test_ancestor_log_weights_are_the_restatement(g, name, bs, keep_prev):
    st, m, ys, ref = after_two_steps(g, name, bs, keep_prev)
    before = state_of(st)
    got = g.block_ancestor_log_weights(st, bs, ys[:, 3], ref)
    want = asp.ancestor_log_weights(name, m.params, st.log_weights, st.traces, bs, ys[:, 3], ref, m.dim)
    assert eq(got, want), (name, bs, keep_prev, np.flatnonzero(got != want)[:5])
    assert unchanged(before, state_of(st))                                   # (reads the state, changes nothing: no epoch advance)
    if name == "line_model":
        assert np.isneginf(got).any() and np.isfinite(got).any()
    else:
        assert np.all(np.isfinite(got)) and not eq(got, st.log_weights)
    st.close()


def test_ancestor_log_weights_with_block_params(g):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    bs = 129
    assign = np.arange((n_of(bs) + bs - 1) // bs) % 3
    st, m, ys, ref = after_two_steps(g, "object_motion", bs, True, params=sets, assign=assign)
    got = g.block_ancestor_log_weights(st, bs, ys[:, 3], ref)
    P = np.stack([sets[k].params for k in assign])
    want = asp.ancestor_log_weights("object_motion", P, st.log_weights, st.traces, bs, ys[:, 3], ref, m.dim)
    assert eq(got, want)
    assert not eq(got, asp.ancestor_log_weights("object_motion", sets[0].params, st.log_weights, st.traces, bs, ys[:, 3], ref, m.dim))
    st.close()


# ----------------------------------------------------------------------------- 2. lockstep parity with the restatement
def compare(g, st, L, bs, where, mask=None):
    assert eq(st.traces, L.rows), (where, "rows")
    assert eq(st.log_weights, L.lw), (where, "lw")
    ess, lml = g.block_stats(st, bs)
    ess_o, lml_o = L.block_stats()
    assert eq(ess, ess_o) and eq(lml, lml_o), (where, "block_stats")
    if mask is not None:                                                     # (the parents of a block that did not resample are an earlier call's)
        in_res = np.repeat(mask, bs)[:L.n]
        assert np.array_equal(st.parents[in_res], L.parents[in_res]), (where, "parents")
        assert np.array_equal(st.parents[cs.slot0(L.n, bs)[mask]], L.a0[mask] + 1), (where, "slot 0's parent is its drawn ancestor")
    assert history_steps(st) == L.gen.steps
    for t in range(1, L.gen.steps + 1):
        for c in range(st.dim):
            assert np.array_equal(st.history_column(t, c), L.gen.trace(t, c)), (where, "history", t, c)


def lockstep(g, o, name, bs, keep_prev, ess_frac, params=None, assign=None):
    """returns (blocks that resampled, blocks that did not, resampled blocks whose slot 0 drew another particle)"""
    m = model_of(g, name)
    n = n_of(bs)
    B = (n + bs - 1) // bs
    ys, ref = block_obs(g, m, B, T), references(g, m, B, T)
    sets = None if params is None else [p.params for p in params]
    L = asp.AncestorLoop(o, m, n, bs, SEED, keep_prev, param_sets=sets, assign=assign)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=keep_prev, history=T, reference=ref[:, 0],
                                params=None if params is None else [params[k] for k in assign])
    L.initialize(ys[:, 0], ref[:, 0])
    compare(g, st, L, bs, (name, bs, keep_prev, 0))
    n_res = n_not = n_moved = 0
    for t in range(1, T):
        k = quiet(lambda: g.pf_resample_blocks(st, bs, "multinomial", ess_frac=ess_frac, check=False, conditional=True, reference=ref[:, t], observations=ys[:, t]))
        mask = L.resample(ys[:, t], ref[:, t], ess_frac)
        assert np.array_equal(g.block_resampled(st), mask) and k == mask.sum(), (name, bs, t, "block_resampled")
        n_res += int(mask.sum()); n_not += int((~mask).sum()); n_moved += int((L.a0 != 0).sum())
        compare(g, st, L, bs, (name, bs, keep_prev, t, "resample"), mask=mask)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs, reference=ref[:, t])
        L.update(ys[:, t], ref[:, t])
        compare(g, st, L, bs, (name, bs, keep_prev, t, "update"))
    st.close()
    return n_res, n_not, n_moved


@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_lockstep_with_the_spec(g, o, name, bs, keep_prev):
    n_res, n_not, n_moved = lockstep(g, o, name, bs, keep_prev, 0.5)
    if bs == 1:
        assert n_res == 0                                                    # (one particle: its ESS is 1, never below half a particle)
    n_res, n_not, n_moved = lockstep(g, o, name, bs, keep_prev, None)
    assert n_not == 0 and n_res > 0
    if bs == 1:
        assert n_moved == 0                                                  # a block of one particle: a0 = 0
    elif bs >= 7:
        assert n_moved > 0


def test_lockstep_gate_sees_both_kinds(g, o):
    n_res, n_not, n_moved = lockstep(g, o, "lgssm2", 7, True, 0.5)
    assert n_res > 0 and n_not > 0 and n_moved > 0, (n_res, n_not, n_moved)


def test_lockstep_with_block_params(g, o):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    bs = 129
    B = (n_of(bs) + bs - 1) // bs
    n_res, _, n_moved = lockstep(g, o, "object_motion", bs, True, 0.7, params=sets, assign=np.arange(B) % 3)
    assert n_res > 0 and n_moved > 0


# ----------------------------------------------------------------------------- 3. against the conditional call
@pytest.mark.parametrize("name,bs,keep_prev", [("lgssm2", 7, False), ("bearings4", 129, True), ("object_motion", 2048, True)])
def test_only_slot_0_differs_from_the_conditional_call(g, name, bs, keep_prev):
    m = model_of(g, name)
    n = 16 * bs
    B = n // bs
    ys, ref = block_obs(g, m, B, 3), references(g, m, B, 3)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=keep_prev, history=3, reference=ref[:, 0]) for _ in range(2))
    for st in (a, b):
        g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs, reference=ref[:, 1])
    rows_in = a.traces
    assert eq(rows_in, b.traces) and eq(a.log_weights, b.log_weights)
    ka = quiet(lambda: g.pf_resample_blocks(a, bs, "multinomial", ess_frac=0.9, check=False, conditional=True))
    kb = quiet(lambda: g.pf_resample_blocks(b, bs, "multinomial", ess_frac=0.9, check=False, conditional=True, reference=ref[:, 2], observations=ys[:, 2]))
    mask = g.block_resampled(a)
    assert ka == kb and np.array_equal(mask, g.block_resampled(b)) and mask.any()
    b0 = cs.slot0(n, bs)
    others = np.ones(n, bool); others[b0[mask]] = False
    assert eq(a.traces[others], b.traces[others]) and eq(a.log_weights, b.log_weights)
    in_res = np.repeat(mask, bs) & others
    assert np.array_equal(a.parents[in_res], b.parents[in_res])
    a0 = b.parents[b0[mask]] - 1
    assert np.all(a.parents[b0[mask]] == 1) and np.all((a0 >= 0) & (a0 < bs)) and np.any(a0 != 0)
    assert eq(b.traces[b0[mask]], rows_in[b0[mask] + a0]) and eq(a.traces[b0[mask]], rows_in[b0[mask]])
    ea, la = g.block_stats(a, bs); eb, lb = g.block_stats(b, bs)
    assert eq(ea, eb) and eq(la, lb)
    # the same epoch, the same streams afterwards; the filter's per-block observations are still the previous step's
    for st in (a, b):
        g.pf_update_blocks(st, (3,), (None,), ys[:, 2], bs, reference=ref[:, 2])
    assert eq(a.traces[others], b.traces[others]) and eq(a.log_weights[others], b.log_weights[others])
    a.close(); b.close()


def test_a_rejuvenation_before_the_update_sees_the_previous_observation(g):
    """the ancestor call stages its data vectors apart from the filter's per-block observations"""
    m = g.models.lgssm2()
    bs, B = 7, 32
    ys, ref = block_obs(g, m, B, 3), references(g, m, B, 3)
    a, b = (g.pf_initialize_blocks(m, (1,), ys[:, 0], bs * B, bs, seed=SEED, keep_prev=True, reference=ref[:, 0]) for _ in range(2))
    for st in (a, b):
        g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs, reference=ref[:, 1])
    g.block_ancestor_log_weights(b, bs, 100.0 + ys[:, 2], ref[:, 2])
    quiet(lambda: g.pf_resample_blocks(a, bs, "multinomial", check=False, conditional=True))
    quiet(lambda: g.pf_resample_blocks(b, bs, "multinomial", check=False, conditional=True, reference=ref[:, 2], observations=100.0 + ys[:, 2]))
    for st in (a, b):
        g.pf_rejuvenate_blocks(st)
    others = np.ones(bs * B, bool); others[cs.slot0(bs * B, bs)] = False
    assert eq(a.traces[others], b.traces[others]) and eq(a.log_weights[others], b.log_weights[others])
    a.close(); b.close()


# ----------------------------------------------------------------------------- 4. edge weights
def test_particles_of_weight_zero_are_never_drawn(g):
    m = g.models.lgssm2()
    bs, B = 7, 512
    n = bs * B
    ys, ref = block_obs(g, m, B, 2), references(g, m, B, 2)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, reference=ref[:, 0])
    lw = st.log_weights
    dead = np.zeros(n, bool)
    dead[np.arange(n) % bs % 2 == 1] = True                                  # local 1, 3, 5 of every block
    dead[: 8 * bs : bs] = True                                               # ... and slot 0 of the first eight
    lw[dead] = -np.inf
    st.log_weights = lw
    assert quiet(lambda: g.pf_resample_blocks(st, bs, "multinomial", check=False, conditional=True, reference=ref[:, 1], observations=ys[:, 1])) == B
    a0 = st.parents[cs.slot0(n, bs)] - 1
    assert not dead[cs.slot0(n, bs) + a0].any() and np.any(a0 != 0) and np.all(a0[:8] != 0)
    assert not dead[(np.arange(n) // bs) * bs + st.parents - 1].any()
    st.close()


def test_a_reference_no_particle_leads_to_keeps_its_predecessor(g):
    m = g.models.line_model()
    bs, B = 129, 4
    n = bs * B
    ys = line_data(g, B, 2)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED)
    ref = np.tile([7.0, 0.0], (B, 1))                                        # a slope outside uniform_discrete(-2, 2)
    ref[1] = [st.traces[bs + 5, 0], 1.0]                                     # ... except block 1: the slope of its particle 5
    lwa = g.block_ancestor_log_weights(st, bs, ys[:, 1], ref)
    assert np.all(np.isneginf(lwa[:bs])) and np.all(np.isneginf(lwa[2 * bs:])) and np.isfinite(lwa[bs + 5])
    rows_in = st.traces
    assert quiet(lambda: g.pf_resample_blocks(st, bs, "multinomial", check=False, conditional=True, reference=ref, observations=ys[:, 1])) == B
    par = st.parents[cs.slot0(n, bs)]
    assert par[0] == par[2] == par[3] == 1
    assert rows_in[bs + par[1] - 1, 0] == ref[1, 0]                          # block 1: an ancestor that holds the reference's slope
    st.close()


def test_a_nan_block_is_left_and_reported_as_by_the_conditional_call(g):
    m = g.models.lgssm2()
    bs, B = 7, 6
    n = bs * B
    ys, ref = block_obs(g, m, B, 2), references(g, m, B, 2)
    res = {}
    for mode in ("conditional", "ancestor"):
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, reference=ref[:, 0])
        lw = st.log_weights
        lw[bs + 3] = np.nan
        st.log_weights = lw
        rows_in = st.traces
        kw = dict(reference=ref[:, 1], observations=ys[:, 1]) if mode == "ancestor" else {}
        with pytest.raises(g.ErrorException) as e:
            g.pf_resample_blocks(st, bs, "multinomial", check=False, conditional=True, **kw)
        mask = np.zeros(B, np.int32)                                             # (the library's own mask: the call ran, whatever it returned)
        assert st._L.gpf_block_resampled(st._h, mask.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        assert not mask[1] and mask.sum() == B - 1
        assert eq(st.traces[bs:2 * bs], rows_in[bs:2 * bs]) and eq(st.log_weights[bs:2 * bs], lw[bs:2 * bs])
        res[mode] = (str(e.value), mask, st.log_weights, st.parents, st.traces)
        st.close()
    c, a = res["conditional"], res["ancestor"]
    assert c[0] == a[0] and "NaN" in a[0] and np.array_equal(c[1], a[1]) and eq(c[2], a[2])
    others = np.ones(n, bool); others[cs.slot0(n, bs)] = False
    assert eq(c[4][others], a[4][others]) and np.array_equal(c[3][others], a[3][others])


# ----------------------------------------------------------------------------- 5. composition with the outer level and the trajectory draw
@pytest.mark.parametrize("bs", [8, 300])
def test_ancestor_resample_then_across_blocks_then_trajectories(g, bs):
    m = g.models.lgssm2()
    n = 24 * bs
    B = n // bs
    ys, ref = block_obs(g, m, B, T), references(g, m, B, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=True, history=T, reference=ref[:, 0])
    gen = Genealogy(n)
    gen.begin_step(st.traces[:, :m.dim])
    fired = moved = 0
    for t in range(1, T):
        quiet(lambda: g.pf_resample_blocks(st, bs, "multinomial", ess_frac=0.8, check=False, conditional=True, reference=ref[:, t], observations=ys[:, t]))
        mask = g.block_resampled(st)
        par = st.parents
        moved += int((par[cs.slot0(n, bs)[mask]] != 1).sum())
        gen.resample("blocks", par, mask, bs)
        A = g.pf_resample_across_blocks(st, bs, "multinomial", ess_frac=None, check=False)
        if A is not None:
            fired += 1
            gen.resample("global", st.parents)
        gen.set_rows(st.traces[:, :m.dim])
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs, reference=ref[:, t])
        gen.begin_step(st.traces[:, :m.dim])
        for s in range(1, gen.steps + 1):
            for c in range(m.dim):
                assert np.array_equal(st.history_column(s, c), gen.trace(s, c)), (bs, t, s, c)
    assert fired > 0 and moved > 0
    traj, idx = g.block_sample_trajectories(st, bs, 3, return_indices=True)
    assert np.all((idx >= 1) & (idx <= bs))
    assert eq(traj, paths(gen, idx, bs, 1, gen.steps, m.dim))
    st.close()


# ----------------------------------------------------------------------------- 6. refusals change nothing
def test_refusals_change_nothing(g):
    m = g.models.object_motion()
    bs, n, B = 7, 26, 4
    ys, ref = block_obs(g, m, B, 3), references(g, m, B, 3)
    E = g.ErrorException
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=True, history=3, reference=ref[:, 0])
    res = lambda *a, **kw: g.pf_resample_blocks(st, bs, *a, check=False, conditional=True, **{**dict(reference=ref[:, 1], observations=ys[:, 1]), **kw})
    lwa = lambda **kw: g.block_ancestor_log_weights(st, bs, **{**dict(reference=ref[:, 1], observations=ys[:, 1]), **kw})
    refused(g, st, lambda: res("residual"), ValueError)
    refused(g, st, lambda: res("stratified"), ValueError)
    bad = ref[:, 1].copy()
    for v in (np.nan, np.inf, -np.inf):
        bad[B - 1, m.dim - 1] = v
        refused(g, st, lambda: res("multinomial", reference=bad), E)
        refused(g, st, lambda: lwa(reference=bad), E)
    for call in (lambda **kw: res("multinomial", **kw), lwa):
        refused(g, st, lambda: call(reference=np.zeros((B, m.dim + 1))), E)          # n_ref
        refused(g, st, lambda: call(reference=np.zeros((B + 1, m.dim))), E)          # rows
        refused(g, st, lambda: call(observations=np.zeros((B, 3))), E)               # n_obs
        refused(g, st, lambda: call(observations=np.zeros((B + 1, 2))), E)
    # the library's own refusals, behind the Python checks: status codes of the conditional call
    o_, r_ = np.ascontiguousarray(ys[:, 1]), np.ascontiguousarray(ref[:, 1])
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    raw = lambda method, size, ob=o_, n_obs=2, rf=r_, n_ref=2: st._L.gpf_resample_blocks_ancestor(st._h, method, size, float("nan"), 0, None if ob is None else P(ob), n_obs,
                                                                                                     None if rf is None else P(rf), n_ref, None, None)
    cond = lambda method, size: st._L.gpf_resample_blocks_conditional(st._h, method, size, float("nan"), 0, None, None)
    for method, size in ((1, bs), (2, bs), (7, bs), (0, 0)):
        before = snapshot(st)
        code = raw(method, size)
        assert code != 0 and code == cond(method, size) and unchanged(before, snapshot(st))
    for kw in (dict(ob=None), dict(rf=None), dict(n_obs=1), dict(n_ref=3)):
        before = snapshot(st)
        assert raw(0, bs, **kw) == g._lib.ERR_INVALID_ARGUMENT and unchanged(before, snapshot(st)), kw
    out = np.empty(n)
    before = snapshot(st)
    assert st._L.gpf_block_ancestor_log_weights(st._h, bs, P(o_), 2, P(r_), 2, None) == g._lib.ERR_INVALID_ARGUMENT
    assert st._L.gpf_block_ancestor_log_weights(st._h, bs, None, 2, P(r_), 2, P(out)) == g._lib.ERR_INVALID_ARGUMENT
    assert st._L.gpf_block_ancestor_log_weights(st._h, 0, P(o_), 2, P(r_), 2, P(out)) == g._lib.ERR_INVALID_ARGUMENT and unchanged(before, snapshot(st))
    assert quiet(lambda: res("multinomial")) == B                                    # (the state is alive and well)
    st.close()
    # a block size that differs from the per-block parameters'
    sets = [g.models.object_motion(), g.models.object_motion(sy=0.2)]
    bp = g.pf_initialize_blocks(m, (1,), ys[:2, 0], 28, 14, seed=SEED, keep_prev=True, params=sets)
    ys4 = np.tile(ys[0, 1], (4, 1)); ref4 = np.tile(ref[0, 1], (4, 1))
    refused(g, bp, lambda: g.pf_resample_blocks(bp, 7, "multinomial", check=False, conditional=True, reference=ref4, observations=ys4), E, store=False)
    bp.close()
    # blocks of 2049 particles; a view; a filter with a whole-filter store
    big = g.pf_initialize_blocks(m, (1,), np.tile(ys[0, 0], (2, 1)), 2 * 2049, 2049, seed=SEED, keep_prev=True, reference=ref[:2, 0])
    y2, r2 = np.tile(ys[0, 1], (2, 1)), ref[:2, 1]
    refused(g, big, lambda: g.pf_resample_blocks(big, 2049, "multinomial", check=False, conditional=True, reference=r2, observations=y2), E, store=False)
    assert np.all(np.isfinite(g.block_ancestor_log_weights(big, 2049, y2, r2)))      # (per particle: any block size)
    view = big[0:14]
    refused(g, big, lambda: g.pf_resample_blocks(view, 7, "multinomial", check=False, conditional=True, reference=r2, observations=y2), E, store=False)
    refused(g, big, lambda: g.block_ancestor_log_weights(view, 7, y2, r2), E, store=False)
    before = snapshot(big, False)
    y2c, r2c = np.ascontiguousarray(y2), np.ascontiguousarray(r2)
    assert view._L.gpf_resample_blocks_ancestor(view._h, 0, 7, float("nan"), 0, P(y2c), 2, P(r2c), 2, None, None) == g._lib.ERR_STATE
    assert view._L.gpf_block_ancestor_log_weights(view._h, 7, P(y2c), 2, P(r2c), 2, P(np.empty(14))) == g._lib.ERR_STATE and unchanged(before, snapshot(big, False))
    big.close()
    whole = g.pf_initialize(m, (1,), ys[0, 0], n, seed=SEED, keep_prev=True, history=3)
    refused(g, whole, lambda: g.pf_resample_blocks(whole, bs, "multinomial", check=False, conditional=True, reference=ref[:, 1], observations=ys[:, 1]), E, store=False)
    refused(g, whole, lambda: g.block_ancestor_log_weights(whole, bs, ys[:, 1], ref[:, 1]), E, store=False)
    whole.close()


# ----------------------------------------------------------------------------- 7. invariance against the exact smoother
def device_steps(g):
    m = g.models.lgssm2()
    n, bs = cs.INV_B * cs.INV_N, cs.INV_N
    box = {}

    def initialize(obs, ref):
        box["st"] = g.pf_initialize_blocks(m, (1,), obs, n, bs, seed=cs.INV_SEED, history=asp.INV_T, reference=ref)

    def resample(obs, ref):
        assert g.pf_resample_blocks(box["st"], bs, "multinomial", check=False, conditional=True, reference=ref, observations=obs) == cs.INV_B

    def update(obs, ref):
        g.pf_update_blocks(box["st"], (), (), obs, bs, reference=ref)

    def sample():
        traj = g.block_sample_trajectories(box["st"], bs, 1)
        box["st"].close()
        return traj

    return initialize, resample, update, sample


def test_invariance_against_the_exact_smoother(g):
    """lgssm2 defaults, T = 8, B = 4096 blocks of N = 8, reference paths drawn in NumPy from the exact p(x_1:8 | y_1:8): pinned initialise, then
    (ancestor resample, pinned update) x 7, then one trajectory per block.  Ancestor sampling leaves the smoothing law invariant, so the output paths
    are exact draws: every mean within 5 sqrt(Sigma_tt / B) of the smoothed mean, every sample variance within 5 sqrt(2 / B) relative of Sigma_tt.
    tests/test_block_ancestor_host.py shows on the CPU that a wrong ancestor density (logtrans = 0) fails these bounds."""
    zm, zv, renewed = asp.invariance_run(device_steps(g), g.models)
    print("ancestor sampling: mean z", np.round(zm, 2).tolist(), "variance z", np.round(zv, 2).tolist(), "x_1 renewed", renewed)
    assert np.all(zm <= cs.INV_SIGMAS) and np.all(zv <= cs.INV_SIGMAS), (zm, zv)
