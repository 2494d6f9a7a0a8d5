"""Conditional SMC for block-wise filters on the device (gpf.h gpf_initialize_blocks_ref, gpf_update_blocks_ref, gpf_resample_blocks_conditional):

  1. lockstep parity, bit for bit, with the restatement of tests/block_conditional_spec.py (the CPU oracle's own block loops with slot 0 patched): rows,
     log-weights, parents, block_stats, block_resampled and history_column at every past step, over T = 6 steps, once with the ESS gate and once resampling
     every step, at the block sizes where the kernels change shape and a short last block;
  2. everything but slot 0 of a pinned update equals the plain update, bit for bit;
  3. the nested filter: conditional resample, then resampling across blocks, in one step -- the store's genealogy against tests/block_history_spec.py;
  4. refused calls change nothing (state, weights, epoch -- through the checkpoint blob -- and the store);
  5. invariance against the exact smoother: the drawn paths of the conditional loop are exact draws of p(x_1:4 | y_1:4), those of the plain filter at the
     same shape are not.  tests/test_block_conditional_host.py runs the same experiment on the CPU restatement (the evidence for seed, shapes and bounds)."""
import ctypes
import warnings

import numpy as np
import pytest

import block_conditional_spec as cs
from block_history_spec import Genealogy

pytestmark = pytest.mark.gpu
T = 6
MODELS = ["sv1", "object_motion", "lgssm2", "bearings4"]                     # d = 1, 2, 2, 4
SIZES = [1, 2, 7, 128, 129, 512, 513, 2048]                                  # a wave 2 / 8 per lane, the workgroup, and their edges
NOISE = {"sv1": 2.0, "object_motion": 0.3, "lgssm2": 0.3, "bearings4": 0.3}
SEED = 17


def eq(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def n_of(bs):
    return 3 * bs + 5                                                        # three full blocks and five particles more: a short last block for bs > 5


def model_of(g, name):
    return g.models.bearings4(sb=0.5) if name == "bearings4" else g.models.by_name(name)


def block_obs(g, m, B, steps, seed=7):
    """[B, steps, n_obs]: every block its own data, the noise scale varying from block to block (some blocks pass the ESS test, some do not)"""
    base = np.asarray(g.models.simulate(m, steps))
    rng = np.random.default_rng(seed)
    scale = NOISE[m.name] * 8.0 ** rng.uniform(-1, 1, (B, steps, 1))
    return base[None, :, :] + scale * rng.standard_normal((B,) + base.shape)


def references(g, m, B, steps, seed=5):
    """[B, steps, d]: valid latent values -- a simulated path of the model's own filter shape plus noise on the continuous columns; the discrete latent
    of object_motion (column 0, `moving`) is 0 or 1"""
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((B, steps, m.dim))
    if m.name == "object_motion":
        ref[..., 0] = rng.integers(0, 2, (B, steps))
    if m.name == "bearings4":
        ref += np.array([1.0, 1.0, 0.0, 0.0])                                 # (away from the origin of the bearing)
    return ref


def history_steps(st):
    k = ctypes.c_int32(-1)
    st._check(st._L.gpf_history_steps(st._h, ctypes.byref(k)))
    return k.value


def compare(g, st, L, bs, where, parents_mask=None):
    assert eq(st.traces, L.rows), (where, "rows")
    assert eq(st.log_weights, L.lw), (where, "lw")
    ess, lml = g.block_stats(st, bs)
    ess_o, lml_o = L.block_stats()
    assert eq(ess, ess_o) and eq(lml, lml_o), (where, "block_stats")
    if parents_mask is not None:                                             # (the parents of a block that did not resample are an earlier call's)
        in_res = np.repeat(parents_mask, bs)[:L.n]
        assert np.array_equal(st.parents[in_res], L.parents[in_res]), (where, "parents")
        b0 = cs.slot0(L.n, bs)[parents_mask]
        assert np.all(st.parents[b0] == 1), (where, "slot 0 keeps itself")
    assert history_steps(st) == L.gen.steps
    for t in range(1, L.gen.steps + 1):
        for c in range(st.dim):
            assert np.array_equal(st.history_column(t, c), L.gen.trace(t, c)), (where, "history", t, c)


def lockstep(g, o, name, bs, keep_prev, ess_frac, params=None, assign=None):
    m = model_of(g, name)
    n = n_of(bs)
    B = (n + bs - 1) // bs
    ys, ref = block_obs(g, m, B, T), references(g, m, B, T)
    sets = None if params is None else [p.params for p in params]
    L = cs.ConditionalLoop(o, m, n, bs, SEED, keep_prev, param_sets=sets, assign=assign)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=keep_prev, history=T, reference=ref[:, 0],
                                params=None if params is None else [params[k] for k in assign])
    L.initialize(ys[:, 0], ref[:, 0])
    compare(g, st, L, bs, (name, bs, keep_prev, 0))
    n_res = n_not = 0
    for t in range(1, T):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            k = g.pf_resample_blocks(st, bs, "multinomial", ess_frac=ess_frac, check=False, conditional=True)
        mask = L.resample(ess_frac, conditional=True)
        assert np.array_equal(g.block_resampled(st), mask) and k == mask.sum(), (name, bs, t, "block_resampled")
        n_res += int(mask.sum()); n_not += int((~mask).sum())
        compare(g, st, L, bs, (name, bs, keep_prev, t, "resample"), parents_mask=mask)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs, reference=ref[:, t])
        L.update(ys[:, t], ref[:, t])
        compare(g, st, L, bs, (name, bs, keep_prev, t, "update"))
        assert eq(st.traces[cs.slot0(n, bs), :m.dim], ref[:, t])             # the pinned value, as given
    st.close()
    return n_res, n_not


# ----------------------------------------------------------------------------- 1. lockstep parity with the restatement
@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_lockstep_with_the_spec(g, o, name, bs, keep_prev):
    n_res, n_not = lockstep(g, o, name, bs, keep_prev, 0.5)
    if bs == 1:
        assert n_res == 0                                                    # (one particle: its ESS is 1, never below half a particle)
    n_res, n_not = lockstep(g, o, name, bs, keep_prev, None)
    assert n_not == 0 and n_res > 0


def test_lockstep_gate_sees_both_kinds(g, o):
    n_res, n_not = lockstep(g, o, "lgssm2", 7, True, 0.5)
    assert n_res > 0 and n_not > 0, (n_res, n_not)


def test_lockstep_with_block_params(g, o):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    bs = 129
    B = (n_of(bs) + bs - 1) // bs
    n_res, _ = lockstep(g, o, "object_motion", bs, True, 0.7, params=sets, assign=np.arange(B) % 3)
    assert n_res > 0


# ----------------------------------------------------------------------------- 2. everything but slot 0
@pytest.mark.parametrize("name,bs,keep_prev", [("lgssm2", 7, False), ("bearings4", 129, True), ("object_motion", 2048, True), ("sv1", 5000, True)])
def test_everything_but_slot_0_is_the_plain_update(g, name, bs, keep_prev):
    """two filters of one seed on the same incoming state: the pinned update and the plain one differ in slot 0 only (bearings4 with keep_prev: rows of
    8 doubles, the kernel's staged wide-row path; 5000: beyond the block resampler's 2048, these kernels are per particle)"""
    m = model_of(g, name)
    n = n_of(bs)
    B = (n + bs - 1) // bs
    ys, ref = block_obs(g, m, B, 2), references(g, m, B, 2)
    a = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=keep_prev)
    b = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=keep_prev)
    assert eq(a.traces, b.traces) and eq(a.log_weights, b.log_weights)
    rows_in = a.traces
    g.pf_update_blocks(a, (2,), (None,), ys[:, 1], bs)
    g.pf_update_blocks(b, (2,), (None,), ys[:, 1], bs, reference=ref[:, 1])
    b0 = cs.slot0(n, bs)
    others = np.ones(n, bool); others[b0] = False
    ra, rb = a.traces, b.traces
    assert eq(ra[others], rb[others]) and eq(a.log_weights[others], b.log_weights[others])
    assert eq(rb[b0, :m.dim], ref[:, 1])
    if keep_prev:
        assert eq(rb[b0, m.dim:2 * m.dim], rows_in[b0, :m.dim])
    assert np.all(rb[b0, (2 if keep_prev else 1) * m.dim:] == 0.0)
    assert not eq(a.log_weights[b0], b.log_weights[b0]) and np.all(np.isfinite(b.log_weights[b0]))
    # the next plain call on both: the same epoch, the same streams
    g.pf_update_blocks(a, (3,), (None,), ys[:, 1], bs)
    g.pf_update_blocks(b, (3,), (None,), ys[:, 1], bs)
    assert eq(a.traces[others], b.traces[others]) and eq(a.log_weights[others], b.log_weights[others])
    a.close(); b.close()


# ----------------------------------------------------------------------------- 3. the nested filter
@pytest.mark.parametrize("bs", [8, 300])
def test_conditional_resample_then_across_blocks(g, bs):
    m = g.models.lgssm2()
    n = 24 * bs
    B = n // bs
    ys, ref = block_obs(g, m, B, T), references(g, m, B, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=True, history=T, reference=ref[:, 0])
    gen = Genealogy(n)
    gen.begin_step(st.traces[:, :m.dim])
    fired = 0
    for t in range(1, T):
        kept = st.traces[cs.slot0(n, bs)]
        g.pf_resample_blocks(st, bs, "multinomial", ess_frac=0.8, check=False, conditional=True)
        mask = g.block_resampled(st)
        par = st.parents
        assert np.all(par[cs.slot0(n, bs)[mask]] == 1)
        assert eq(st.traces[cs.slot0(n, bs)], kept)                          # slot 0 of every block is where it was, resampled or not
        gen.resample("blocks", par, mask, bs)
        A = g.pf_resample_across_blocks(st, bs, "multinomial", ess_frac=None, check=False)
        if A is not None:
            fired += 1
            gen.resample("global", st.parents)
            assert eq(st.traces[cs.slot0(n, bs)], kept[A - 1])               # whole blocks were copied: the retained particles travel with them
        gen.set_rows(st.traces[:, :m.dim])
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs, reference=ref[:, t])
        gen.begin_step(st.traces[:, :m.dim])
        for s in range(1, gen.steps + 1):
            for c in range(m.dim):
                assert np.array_equal(st.history_column(s, c), gen.trace(s, c)), (bs, t, s, c)
    assert fired > 0
    st.close()


# ----------------------------------------------------------------------------- 4. refusals change nothing
def snapshot(st, store=True):
    hist = []
    if store:
        hist = [history_steps(st)] + [st.history_column(t, c) for t in range(1, history_steps(st) + 1) for c in range(st.dim)]
    return bytes(st.checkpoint()), st.traces, st.log_weights, st.parents, hist


def unchanged(a, b):
    return a[0] == b[0] and eq(a[1], b[1]) and eq(a[2], b[2]) and np.array_equal(a[3], b[3]) and len(a[4]) == len(b[4]) and all(eq(x, y) for x, y in zip(a[4], b[4]))


def refused(g, st, call, exc, store=True):
    before = snapshot(st, store)
    with pytest.raises(exc):
        call()
    assert unchanged(before, snapshot(st, store)), call


def test_refusals_change_nothing(g):
    m = g.models.object_motion()
    bs, n = 7, 26
    B = 4
    ys, ref = block_obs(g, m, B, 4), references(g, m, B, 4)
    E = g.ErrorException
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=True, history=2, reference=ref[:, 0])
    upd = lambda **kw: g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs, **kw)
    bad = ref[:, 1].copy()
    refused(g, st, lambda: upd(reference=np.zeros((B + 1, m.dim))), E)       # rows
    refused(g, st, lambda: upd(reference=np.zeros((B, m.dim + 1))), E)       # columns: the library's own check
    refused(g, st, lambda: upd(reference=np.zeros(B * m.dim)), E)
    for v in (np.nan, np.inf, -np.inf):
        bad[B - 1, m.dim - 1] = v
        refused(g, st, lambda: upd(reference=bad), E)
    refused(g, st, lambda: upd(reference=ref[:, 1], strata=[0.0, 1.0]), ValueError)
    refused(g, st, lambda: upd(proposals=[None] * B, reference=ref[:, 1]), ValueError)
    res = lambda *a, **kw: g.pf_resample_blocks(st, bs, *a, check=False, conditional=True, **kw)
    refused(g, st, lambda: res("residual"), ValueError)
    refused(g, st, lambda: res("stratified"), ValueError)
    refused(g, st, lambda: res("multinomial", priority_fn=g.Tempering(0.5)), ValueError)
    # the library's own refusals, behind the Python checks
    raw = lambda method, size: st._L.gpf_resample_blocks_conditional(st._h, method, size, float("nan"), 0, None, None)
    for method in (1, 2, 7):
        before = snapshot(st)
        assert raw(method, bs) != 0 and unchanged(before, snapshot(st))
    assert "not a valid conditional scheme" in (raw(1, bs), st._L.gpf_last_error(st._h).decode())[1]
    before = snapshot(st)
    assert raw(0, 0) != 0 and unchanged(before, snapshot(st))
    # a full store on a pinned update: the store holds 2 steps
    upd(reference=ref[:, 1])
    refused(g, st, lambda: g.pf_update_blocks(st, (3,), (None,), ys[:, 2], bs, reference=ref[:, 2]), E)
    assert g.pf_resample_blocks(st, bs, "multinomial", check=False, conditional=True) == B    # (the state is alive and well)
    st.close()
    # blocks of 2049 particles; a view; a filter with a whole-filter store
    big = g.pf_initialize_blocks(m, (1,), np.tile(ys[0, 0], (2, 1)), 2 * 2049, 2049, seed=SEED, keep_prev=True, reference=ref[:2, 0])
    refused(g, big, lambda: g.pf_resample_blocks(big, 2049, "multinomial", check=False, conditional=True), E, store=False)
    g.pf_update_blocks(big, (2,), (None,), np.tile(ys[0, 1], (2, 1)), 2049, reference=ref[:2, 1])              # (the step takes any block size)
    view = big[0:14]
    refused(g, big, lambda: g.pf_resample_blocks(view, 7, "multinomial", check=False, conditional=True), E, store=False)
    refused(g, big, lambda: g.pf_update_blocks(view, (3,), (None,), ys[:2, 2], 7, reference=ref[:2, 2]), E, store=False)
    before = snapshot(big, False)
    assert view._L.gpf_resample_blocks_conditional(view._h, 0, 7, float("nan"), 0, None, None) != 0 and unchanged(before, snapshot(big, False))
    big.close()
    whole = g.pf_initialize(m, (1,), ys[0, 0], n, seed=SEED, keep_prev=True, history=3)
    refused(g, whole, lambda: g.pf_update_blocks(whole, (2,), (None,), ys[:, 1], bs, reference=ref[:, 1]), E, store=False)
    refused(g, whole, lambda: g.pf_resample_blocks(whole, bs, "multinomial", check=False, conditional=True), E, store=False)
    whole.close()


# ----------------------------------------------------------------------------- 5. invariance against the exact smoother
def device_steps(g, conditional):
    m = g.models.lgssm2()
    n, bs = cs.INV_B * cs.INV_N, cs.INV_N
    box = {}

    def initialize(obs, ref):
        box["st"] = g.pf_initialize_blocks(m, (1,), obs, n, bs, seed=cs.INV_SEED, history=cs.INV_T, reference=ref)

    def resample():
        assert g.pf_resample_blocks(box["st"], bs, "multinomial", check=False, conditional=conditional) == cs.INV_B

    def update(obs, ref):
        g.pf_update_blocks(box["st"], (), (), obs, bs, reference=ref)

    def sample():
        traj = g.block_sample_trajectories(box["st"], bs, 1)
        box["st"].close()
        return traj

    return initialize, resample, update, sample


def test_invariance_against_the_exact_smoother(g):
    """lgssm2, T = 4, B = 4096 blocks of N = 8 on one observation sequence, reference paths drawn in NumPy from the exact p(x_1:4 | y_1:4): pinned
    init, then per step a conditional multinomial resample of every block and a pinned update, then block_sample_trajectories(n_samples = 1).  The
    kernel leaves the smoothing law invariant, so the output paths are exact draws: for every t and coordinate the mean over blocks is within
    5 sqrt(Sigma_tt / B) of the smoothed mean and the sample variance within 5 sqrt(2 / B) relative of Sigma_tt (the Gaussian sampling error of a
    variance).  The plain filter at the same shape fails the variance bound at t = 1: path degeneracy at N = 8 (N used: 8)."""
    zm, zv = cs.invariance_run(device_steps(g, True), g.models, True)
    print("conditional: mean z", np.round(zm, 2).tolist(), "variance z", np.round(zv, 2).tolist())
    assert np.all(zm <= cs.INV_SIGMAS) and np.all(zv <= cs.INV_SIGMAS), (zm, zv)
    zm_p, zv_p = cs.invariance_run(device_steps(g, False), g.models, False)
    print("plain: mean z", np.round(zm_p, 2).tolist(), "variance z", np.round(zv_p, 2).tolist())
    assert np.all(zv_p[0] > cs.INV_SIGMAS), zv_p
