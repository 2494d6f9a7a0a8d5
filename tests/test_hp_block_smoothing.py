"""Ancestor sampling, backward simulation and marginal smoothing per block against their DEFINITIONS -- the CPU rehearsal of
tests/test_gpu_hp_block_smoothing.py.  The NumPy restatements (tests/block_ancestor_spec.py, block_backward_spec.py, block_smooth_spec.py) run on
the CPU oracle's filter and their outputs go through the three checks of tests/hp_checks.py (check_ancestor, check_backward, check_smooth), whose
reference is tests/hp_weights.py: the transition densities of the Gen programs in mpmath (hp_reference.Ref.logtrans, natural parameters only), the
inverse CDF at the exact uniform, FFBSm's recursion in E arithmetic.  Here the reference, its derived bounds and its undecidable counts are
validated without a GPU; the device tests drive the same functions.

Negative controls: every control runs a restatement with ONE mistake of meaning -- the kind the bit-for-bit device tests cannot see, because the
kernel and its twin would share it -- and must produce violations where the unmutated run of the same case produces none.

Shapes: the three team shapes of the block-wise kernels at their smallest edge sizes, three full blocks and a short one of five particles; blocks
0, 1 and the short one are checked.  The mpmath reference costs about 0.2 ms per (target, candidate) pair, so the wide cases are thinned by blocks and
steps (BLOCKS, LO below), never by block size."""
import copy

import numpy as np
import pytest

import block_ancestor_spec as asp
import block_backward_spec as bsp
import block_smooth_spec as ssp
import hp_checks as hc
import hp_reference as hp
from test_gpu_block_conditional import block_obs, n_of, references

SEED, SIZES = 17, [7, 129, 513]
MODELS = ["sv1", "object_motion", "lgssm2", "bearings4"]
T_SMOOTH = T_ANC = 3
T_BACK, K_DRAWS = 4, 8
KEEP = 24                                                                    # survivors of the thinned last step at 513


def blocks_of(bs):
    return [0, 1, (n_of(bs) + bs - 1) // bs - 1]                             # the first, the second and the short last block


def back_blocks(name, bs):
    """at 513 a transition costs 8 x 513 pairs per block: the second block is checked for object_motion only"""
    return [b for b in blocks_of(bs) if not (bs == 513 and b == 1 and name != "object_motion")]


def smooth_lo(bs):
    """the lowest step checked per block: at 129 the second block stops at T - 1 (a step of 129 x 129 pairs is 3 s of mpmath); at 513 every block does
    -- below it the weights are dense again and a step costs 513 x 513 pairs"""
    B = (n_of(bs) + bs - 1) // bs
    return {7: {}, 129: {1: T_SMOOTH - 1}, 513: {b: T_SMOOTH - 1 for b in range(B)}}[bs]


def line_data(g, B, steps, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([[g.models.line_obs(t + 1, float(s)) for t in range(steps)] for s in rng.integers(-2, 3, B)])


def case_obs(g, m, B, T):
    if m.name == "line_model":
        return line_data(g, B, T)
    ys = block_obs(g, m, B, T)
    return hc.moving_obs(ys) if m.name == "object_motion" else ys


def param_sets(g):
    return [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]


def survivors(cnt):
    """about KEEP particles of a block of `cnt`: the first and the last index, several waves, and two targets of one reduction round (0 and 1)"""
    if cnt <= KEEP:
        return np.arange(cnt)
    return np.unique(np.concatenate([[0, 1, cnt - 1], np.linspace(2, cnt - 2, KEEP - 3).astype(np.int64)]))


def thin_mask(n, bs):
    keep = np.zeros(n, bool)
    for b0 in range(0, n, bs):
        keep[b0 + survivors(min(bs, n - b0))] = True
    return keep


def kill(n, bs):
    """(particles whose weight becomes -Inf, particles whose weight becomes -800: certainly flushed by exp_) for the dead-past-particle cases: at 7
    the odd locals, at 513 all but the survivors of thin_mask; local 2 of every block is the flushed one"""
    dead = np.arange(n) % bs % 2 == 1 if bs == 7 else ~thin_mask(n, bs)
    flushed = np.arange(n) % bs == 2
    return dead, flushed & ~dead


def store_loop(g, o, name, bs, T, sets=None, thin=False, ess_frac=None, resample=True, kill_at=None):
    """(model, StoreLoop after T steps, parameters for the restatements, one Ref per block).  kill_at: the step after whose update kill() applies"""
    m = hc.case_model(g, name)
    n = n_of(bs)
    B = (n + bs - 1) // bs
    ys = case_obs(g, m, B, T)
    assign = None if sets is None else np.arange(B) % len(sets)
    L = bsp.StoreLoop(o, m, n, bs, SEED, param_sets=None if sets is None else [s.params for s in sets], assign=assign)
    L.initialize(ys[:, 0])
    for t in range(1, T):
        if kill_at == t:
            dead, flushed = kill(n, bs)
            for f in L.L.f:
                f.lw[dead], f.lw[flushed] = -np.inf, -800.0
            L._end()
        if resample:
            L.resample(ess_frac)
        L.update(ys[:, t])
    if thin:                                                                 # all but about KEEP current weights of every block: -Inf
        for f in L.L.f:
            f.lw[~thin_mask(n, bs)] = -np.inf
        L._end()
    P = m.params if sets is None else np.stack([sets[k].params for k in assign])
    refs = [hp.Ref(m if sets is None else sets[assign[b]]) for b in range(B)]
    return m, L, P, refs


def run_backward(o, name, L, P, refs, blocks, store=None, **kw):
    """violations of the restatement's indices (store: what the restatement reads; the check always reads the true one)"""
    _, idx = bsp.backward(o, name, P, L.store if store is None else store, L.seed, L.epoch, K_DRAWS, **kw)
    v = hc.Violations()
    left = hc.check_backward(v, refs, L.store, blocks, L.seed, L.epoch, idx, f"backward {name} {L.store.bs}")
    return v, left, idx


def run_smooth(o, name, L, P, refs, blocks, lo=None, store=None, **kw):
    out = ssp.smooth(o, name, P, L.store if store is None else store, **kw)
    v = hc.Violations()
    fell = hc.check_smooth(v, refs, L.store, blocks, *out, f"smooth {name} {L.store.bs}", lo=lo)
    return v, fell, out


def shifted(store, what):
    """the Store a restatement reads with one mistake: "obs" -- step s + 1 is given the observation rows of step s; "lw" -- snapshot s is given the
    recorded weights of snapshot s + 1 (the current weights of step T stay)"""
    S = copy.copy(store)
    if what == "obs":
        S.obs = [store.obs[0]] + store.obs[:-1]
    else:
        S.lw = store.lw[1:] + [store.lw[-1]]
    return S


def swapped(P, i, j):
    P = np.array(P, np.float64)
    P[..., [i, j]] = P[..., [j, i]]
    return P


# ----------------------------------------------------------------------------- backward simulation
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_backward_simulation_follows_the_definition(g, o, name, bs):
    m, L, P, refs = store_loop(g, o, name, bs, T_BACK)
    blocks = back_blocks(name, bs)
    v, left, idx = run_backward(o, name, L, P, refs, blocks)
    if name == "object_motion":
        hc.moving_inputs(L.store, blocks, held={b: L.store.x(T_BACK)[idx[b, :, -1] - 1, 0] for b in blocks} if bs > 7 else None)
    v.finish(f"backward {name} {bs}")


def test_backward_simulation_of_the_line_model_is_exact(g, o):
    """logtrans is 0 or -Inf: the draw is among the candidates of the held slope, never another"""
    m, L, P, refs = store_loop(g, o, "line_model", 129, T_BACK)
    v, left, idx = run_backward(o, "line_model", L, P, refs, blocks_of(129))
    v.finish("backward line_model")
    x = [L.store.x(s)[idx[:, :, s - 1] - 1, 0] for s in range(1, T_BACK + 1)]
    assert all(np.array_equal(x[0][b], x[s][b]) for s in range(T_BACK) for b in blocks_of(129)) and len(np.unique(L.store.x(1)[:129, 0])) > 1


def test_backward_simulation_with_block_parameters(g, o):
    m, L, P, refs = store_loop(g, o, "object_motion", 129, T_BACK, sets=param_sets(g))
    v, left, _ = run_backward(o, "object_motion", L, P, refs, blocks_of(129))
    hc.moving_inputs(L.store, blocks_of(129))
    v.finish("backward block parameters")
    v, _, _ = run_backward(o, "object_motion", L, np.roll(P, 1, axis=0), refs, blocks_of(129))          # control: another block's parameter row
    print("control, another block's parameter row: backward", len(v.bad))
    assert v.bad


# ----------------------------------------------------------------------------- marginal smoothing
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", ["object_motion", "lgssm2"])
def test_smoothing_follows_the_definition(g, o, name, bs):
    m, L, P, refs = store_loop(g, o, name, bs, T_SMOOTH, thin=bs == 513)
    blocks = blocks_of(bs)
    if name == "object_motion":
        hc.moving_inputs(L.store, blocks)
    v, fell, _ = run_smooth(o, name, L, P, refs, blocks, lo=smooth_lo(bs))
    v.finish(f"smooth {name} {bs}")


@pytest.mark.parametrize("name", ["sv1", "bearings4"])
def test_smoothing_of_the_other_models(g, o, name):
    m, L, P, refs = store_loop(g, o, name, 7, T_SMOOTH, ess_frac=0.5)          # (the ESS gate leaves unequal recorded weights in some blocks)
    v, fell, _ = run_smooth(o, name, L, P, refs, blocks_of(7))
    v.finish(f"smooth {name} 7")


DEAD = [("lgssm2", 7), ("object_motion", 513)]


def dead_blocks(bs):
    return blocks_of(bs) if bs == 7 else [0, blocks_of(bs)[-1]]              # (at 513 a block costs 2 x 24 x 513 pairs)


@pytest.mark.parametrize("name,bs", DEAD)
def test_smoothing_with_dead_and_flushed_past_particles(g, o, name, bs):
    """no resample; after step 2 some weights become -Inf and one per block -800 (kill): they stay in the record of steps 2 and 3.  A -Inf or flushed
    candidate has W = 0 exactly at step 2; every block is followed down to step 1 -- at 513 through the workgroup team's two transitions with 24
    targets of weight each"""
    m, L, P, refs = store_loop(g, o, name, bs, T_SMOOTH, resample=False, kill_at=2)
    dead, flushed = kill(L.store.n, bs)
    assert np.isneginf(L.store.lw[1][dead]).all() and np.all(L.store.lw[1][flushed] == -800.0) and np.isfinite(L.store.lw[1][~dead]).all()
    v, _, out = run_smooth(o, name, L, P, refs, dead_blocks(bs))
    v.finish(f"smooth {name} {bs} with dead particles")
    W2 = out[2][:, 1].reshape(-1)[:L.store.n] if L.store.n % bs == 0 else np.concatenate([out[2][b, 1, :min(bs, L.store.n - b * bs)] for b in range(L.store.B)])
    assert np.all(W2[dead | flushed] == 0.0)


def test_smoothing_fallback_hands_the_weight_to_the_recorded_parent(g, o):
    """line_model, whose -Inf transitions leave candidates of weight exactly 0; a slope no candidate holds hands its weight to the recorded parent"""
    m, L, P, refs = store_loop(g, o, "line_model", 129, T_SMOOTH)
    S = L.store
    S.gen.rows[-1][::3, 0] = 7.0                                             # step T: a foreign slope on every third particle
    v, fell, out = run_smooth(o, "line_model", L, P, refs, blocks_of(129))
    assert fell > 0
    v.finish("smooth fallback")


def test_a_nan_block_reads_nan_and_index_0(g, o):
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T_BACK)
    for f in L.L.f:
        f.lw[7 + 3] = np.nan
    L._end()
    v, _, idx = run_backward(o, "lgssm2", L, P, refs, blocks_of(7))
    assert np.all(idx[1] == 0) and np.all(idx[0] > 0)
    v.finish("backward, a NaN block")
    v, _, out = run_smooth(o, "lgssm2", L, P, refs, blocks_of(7))
    assert np.isnan(out[0][1]).all() and np.all(out[3][1] == 0) and np.isfinite(out[0][0]).all()
    v.finish("smooth, a NaN block")


def test_smoothing_with_block_parameters(g, o):
    m, L, P, refs = store_loop(g, o, "object_motion", 7, T_SMOOTH, sets=param_sets(g))
    v, _, _ = run_smooth(o, "object_motion", L, P, refs, blocks_of(7))
    v.finish("smooth block parameters")
    v, _, _ = run_smooth(o, "object_motion", L, np.roll(P, 1, axis=0), refs, blocks_of(7))
    print("control, another block's parameter row: smooth", len(v.bad))
    assert v.bad


# ----------------------------------------------------------------------------- ancestor sampling
def ancestor_data(g, m, B):
    """(observations [B, T_ANC, n_obs], references [B, T_ANC, d]); line_model: a slope of the support and an outlier flag, held by some particles"""
    if m.name == "line_model":
        return line_data(g, B, T_ANC), np.tile(np.stack([np.arange(B) % 5 - 2.0, np.arange(B) % 2 * 1.0], axis=1)[:, None], (1, T_ANC, 1))
    ref = references(g, m, B, T_ANC)
    return case_obs(g, m, B, T_ANC), hc.moving_references(ref) if m.name == "object_motion" else ref


def ancestor_case(g, o, name, bs, keep_prev, sets=None, density=True, mistake=None):
    """(violations of logtrans, violations of a_0, undecidable draws, a_0 that moved) of pinned initialise -> (ancestor resample -> pinned update)* over
    T_ANC steps.  `mistake(P, obs_rows[t - 1], obs_rows[t])` -> (P, obs) the restatement of the ancestor weights is given instead of the true ones."""
    m = hc.case_model(g, name)
    n = n_of(bs)
    B = (n + bs - 1) // bs
    ys, ref = ancestor_data(g, m, B)
    assign = None if sets is None else np.arange(B) % len(sets)
    L = asp.AncestorLoop(o, m, n, bs, SEED, keep_prev, param_sets=None if sets is None else [s.params for s in sets], assign=assign)
    P = m.params if sets is None else np.stack([sets[k].params for k in assign])
    refs = [hp.Ref(m if sets is None else sets[assign[b]]) for b in range(B)]
    blocks, vl, va, left, moved, calls = blocks_of(bs), hc.Violations(), hc.Violations(), 0, 0, []
    L.initialize(ys[:, 0], ref[:, 0])
    for t in range(1, T_ANC):                                                # the filter first: what every call saw and returned
        rows0, lw0, epoch = L.rows.copy(), L.lw.copy(), L.epoch
        Pm, om = (P, ys[:, t]) if mistake is None else mistake(P, ys[:, t - 1], ys[:, t])
        got = asp.ancestor_log_weights(name, Pm, np.zeros(n), rows0, bs, om, ref[:, t], m.dim)
        mask = L.resample(ys[:, t], ref[:, t], None, density=density)
        calls.append((rows0, lw0, epoch, got, mask.copy(), np.array(L.parents), L.a0.copy()))
        L.update(ys[:, t], ref[:, t])
    if name == "object_motion":
        hc.moving_ancestor_inputs(bs, blocks, [(c[0], ref[:, t], ys[:, t]) for t, c in zip(range(1, T_ANC), calls)], f"ancestor {name} {bs}")
    for t, (rows0, lw0, epoch, got, mask, parents, a0) in zip(range(1, T_ANC), calls):
        assert mask[blocks].all(), (name, bs, t, "a checked block did not resample")
        hc.check_logtrans(vl, refs, bs, blocks, rows0, ref[:, t], ys[:, t], got, f"logtrans {name} {bs}")
        und = hc.check_ancestor(va, refs, bs, blocks, rows0, lw0, ref[:, t], ys[:, t], SEED, epoch, mask, parents, f"ancestor {name} {bs}")
        assert sorted(und) == blocks
        left, moved = left + sum(und.values()), moved + int((a0[blocks] != 0).sum())
    return vl, va, left, moved


@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS + ["line_model"])
def test_ancestor_weights_and_draws_follow_the_definition(g, o, name, bs, keep_prev):
    vl, va, left, moved = ancestor_case(g, o, name, bs, keep_prev)
    print(f"ancestor {name} {bs}: a_0 != 0 in {moved} of {3 * (T_ANC - 1)} draws")
    vl.finish(f"logtrans {name} {bs}")
    va.finish(f"ancestor {name} {bs}")
    assert moved > 0 or (name == "line_model" and bs == 7)                   # (seven particles: the reference's slope is rarely another one's)


def test_ancestor_sampling_with_block_parameters(g, o):
    vl, va, left, moved = ancestor_case(g, o, "object_motion", 129, True, sets=param_sets(g))
    vl.finish("logtrans block parameters")
    va.finish("ancestor block parameters")
    assert moved > 0


# ----------------------------------------------------------------------------- the negative controls
CONTROLS = [("no transition density", "lgssm2", dict(trans=False), None), ("the observation row of step s", "object_motion", {}, "obs"),
            ("the recorded weights of snapshot s + 1", "lgssm2", {}, "lw"), ("sp and sv exchanged", "bearings4", {}, (8, 9)),
            ("log p(moving|still) and log(1 - p(moving|moving)) exchanged", "object_motion", {}, (7, 6))]
OPS = [("backward", 129), ("smooth", 7)]
# the exchanged Bernoulli terms move weight between candidates of different `moving` at the same position; under sy = 0.01 a held particle's candidates
# of weight all sit at one position and are copies of one particle, so no backward DRAW changes (0 of 72 here): that control runs on the smoothing
# weights and on the ancestor weights below
GRID = [(c, op) for c in CONTROLS for op in OPS if not (c[3] == (7, 6) and op[0] == "backward")]


@pytest.mark.parametrize("control,shape", GRID, ids=[f"{c[0]}-{op[0]}" for c, op in GRID])
def test_a_mistake_of_meaning_is_seen(g, o, control, shape):
    """backward simulation at 129 (blocks of seven hold so many copies of one particle that most wrong densities draw the same index), smoothing at 7"""
    (what, name, kw, mistake), (op, bs) = control, shape
    run = run_backward if op == "backward" else run_smooth
    m, L, P, refs = store_loop(g, o, name, bs, T_BACK if op == "backward" else T_SMOOTH, ess_frac=0.5 if mistake == "lw" else None)
    blocks = blocks_of(bs)
    assert not run(o, name, L, P, refs, blocks)[0].bad                       # the unmutated twin
    if isinstance(mistake, str):
        kw = dict(kw, store=shifted(L.store, mistake))
    elif mistake is not None:
        P = swapped(P, *mistake)
    bad = len(run(o, name, L, P, refs, blocks, **kw)[0].bad)
    print(f"control, {what}: {op} {bad} violations")
    assert bad > 0, (what, op)


def test_every_target_on_its_fallback_is_seen_by_smoothing(g, o):
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T_SMOOTH)
    assert not run_smooth(o, "lgssm2", L, P, refs, blocks_of(7))[0].bad
    v, _, _ = run_smooth(o, "lgssm2", L, P, refs, blocks_of(7), fallback=True)
    print("control, fallback=True: smooth", len(v.bad))
    assert v.bad


ANC_CONTROLS = [("the observation row of step s", "object_motion", lambda P, prev, cur: (P, prev)),
                ("sp and sv exchanged", "bearings4", lambda P, prev, cur: (swapped(P, 8, 9), cur)),
                ("log p(moving|still) and log(1 - p(moving|moving)) exchanged", "object_motion", lambda P, prev, cur: (swapped(P, 7, 6), cur))]


@pytest.mark.parametrize("what,name,mistake", ANC_CONTROLS, ids=[c[0] for c in ANC_CONTROLS])
def test_a_mistake_of_meaning_is_seen_in_the_ancestor_weights(g, o, what, name, mistake):
    assert not ancestor_case(g, o, name, 7, True)[0].bad
    vl = ancestor_case(g, o, name, 7, True, mistake=mistake)[0]
    print(f"control, {what}: logtrans {len(vl.bad)} violations")
    assert vl.bad


def test_another_blocks_parameter_row_is_seen_in_the_ancestor_weights(g, o):
    assert not ancestor_case(g, o, "object_motion", 7, True, sets=param_sets(g))[0].bad
    vl = ancestor_case(g, o, "object_motion", 7, True, sets=param_sets(g), mistake=lambda P, prev, cur: (np.roll(P, 1, axis=0), cur))[0]
    print("control, another block's parameter row: logtrans", len(vl.bad))
    assert vl.bad


def test_an_ancestor_drawn_without_the_density_is_seen(g, o):
    """density=False: a_0 in proportion to w alone"""
    bad = 0
    for bs in (7, 129):
        assert not ancestor_case(g, o, "lgssm2", bs, False)[1].bad
        bad += len(ancestor_case(g, o, "lgssm2", bs, False, density=False)[1].bad)
    print("control, density=False: ancestor", bad)
    assert bad > 0
