"""Pairwise smoothing per block (gpf.h gpf_block_smooth_pairs) against its DEFINITION -- the CPU rehearsal of
tests/test_gpu_hp_block_pairs.py.  The NumPy restatement (tests/block_pairs_spec.py) runs on the CPU oracle's filter (store_loop of
tests/test_hp_block_smoothing.py, whose shapes, thinning and helpers these are) and its outputs go through hp_checks.check_pairs: the walk of
check_smooth (hp_checks.reference_walk), hw.smooth_step's pair sums A_i[c] = sum_j W_{s+1}^j p_ij x_{s+1}^j[c] in mpmath with E bounds, hw.second and
hw.cross.  The bit-for-bit device test cannot see a mistake the kernel shares with its twin -- the wrong observation row when a lineage changes
block, an exchanged parameter, A accumulated for the wrong pair, the roles of s and s + 1 exchanged --; this can, and the Monte-Carlo band of the law
experiment is orders of magnitude wider than these bounds.

Negative controls: each is ONE mistake of meaning, on the restatement's outputs or in what the restatement reads, and must produce violations where the
unmutated run of the same case (checked against the same reference walk) produces none.  All of them are visible at these shapes.

Shapes: blocks of 7, 129 and 513 particles, three full blocks and a short one of five -- the sizes at which a reduction round of 2 or 4 targets ends
ragged and a lane or a wave is partly beyond the block; T = 3; thinned by blocks and steps (smooth_lo, thin), never by block size.

The skip rule (a target of smoothing weight exactly 0 is skipped entirely).  For finite rows it changes no bit (asserted below), so it is tested where
it matters: a target of weight exactly 0 with a non-finite row in a block that stays valid.  That is reachable without any new API at the LAST step: a
particle whose current weight is -Inf has W_T = q / S = 0 exactly, only NaN / +Inf current weights make a block NaN, and its row can be overwritten with
+Inf in one column before the step is recorded.  Then the step's own mean and second entries of that column are NaN by the statements (0 * Inf, as the
marginal smoother's mean), and everything that depends on the skip -- the pair (T - 1, T) and all lower steps -- must be finite and within bound: with
`0 * Inf` added to A instead, cross_{T-1} is NaN in that column (the control skip=False).  The last step is taken because nothing else happens to the
row there: no later update propagates it, and no walk has it among its candidates, where it would enter logtrans."""
import copy

import numpy as np
import pytest

import across_blocks_spec as xs
import block_backward_spec as bsp
import block_pairs_spec as psp
import block_smooth_spec as ssp
import hp_checks as hc
import hp_reference as hp
from test_gpu_block_conditional import block_obs
from test_hp_block_smoothing import (CONTROLS, DEAD, SEED, SIZES, T_SMOOTH, blocks_of, dead_blocks, kill, param_sets, shifted, smooth_lo,
                                     store_loop, swapped)

T = T_SMOOTH
NESTED_BS, NESTED_B = 8, 24


def reference(L, refs, blocks, lo=None, stop=1):
    """the reference walk of a case, computed once for every check of it"""
    return hc.reference_walk(refs, L.store, blocks, lo, stop=stop, pairs=True)


def run_pairs(o, name, L, P, refs, blocks, lo=None, steps=None, store=None, walk=None, mutate=None, control=False, **kw):
    """(violations, fallbacks, outputs) of the restatement (store: what it reads; the check always reads the true one; mutate: a mistake applied to
    its outputs; control: the run carries a mistake on purpose and its printed ratios say so)"""
    wlo, whi = (1, L.store.steps) if steps is None else steps
    out = psp.pairs(o, name, P, L.store if store is None else store, wlo, whi, **kw)
    if mutate is not None:
        out = mutate(*out)
    v = hc.Violations()
    fell = hc.check_pairs(v, refs, L.store, blocks, *out, ("MISTAKEN ON PURPOSE, " if control else "") + f"pairs {name} {L.store.bs}", lo=lo, steps=steps, walk=walk)
    return v, fell, out


def seen(what, o, name, L, P, refs, blocks, lo=None, **mistake):
    """a control: the unmutated run is clean, the mutated one is not, against one reference walk; prints and returns its count"""
    walk = reference(L, refs, blocks, lo)
    assert not run_pairs(o, name, L, P, refs, blocks, lo=lo, walk=walk)[0].bad, (what, "the unmutated twin")
    bad = len(run_pairs(o, name, L, mistake.pop("wrong_P", P), refs, blocks, lo=lo, walk=walk, control=True, **mistake)[0].bad)
    print(f"control, {what}: pairs {name} {L.store.bs} {bad} violations")
    assert bad > 0, what
    return bad


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", ["object_motion", "lgssm2"])
def test_pairs_follow_the_definition(g, o, name, bs):
    m, L, P, refs = store_loop(g, o, name, bs, T, thin=bs == 513)
    blocks = blocks_of(bs)
    if name == "object_motion":
        hc.moving_inputs(L.store, blocks)
    v, _, out = run_pairs(o, name, L, P, refs, blocks, lo=smooth_lo(bs))
    v.finish(f"pairs {name} {bs}")
    assert np.all(np.isfinite(out[2]))


@pytest.mark.parametrize("name", ["sv1", "bearings4"])
def test_pairs_of_the_other_models(g, o, name):
    m, L, P, refs = store_loop(g, o, name, 7, T, ess_frac=0.5)                 # (the ESS gate leaves unequal recorded weights in some blocks)
    run_pairs(o, name, L, P, refs, blocks_of(7))[0].finish(f"pairs {name} 7")


BEARINGS_WIDE = dict(blocks=[0], lo={0: T - 1})                              # about 24 x 513 pairs of mpmath


def test_pairs_of_four_columns_on_the_workgroup_team(g, o):
    """bearings4 at 513, the only D = 4 instantiation (two entries per tree) on the team that carries the most state: the last step thinned to KEEP
    survivors, one block, the top transition only"""
    m, L, P, refs = store_loop(g, o, "bearings4", 513, T, thin=True)
    run_pairs(o, "bearings4", L, P, refs, **BEARINGS_WIDE)[0].finish("pairs bearings4 513")


@pytest.mark.parametrize("name,bs", DEAD)
def test_pairs_with_dead_and_flushed_past_particles(g, o, name, bs):
    """the case of the marginal smoother: no resample; after step 2 some weights become -Inf and one per block -800.  They are candidates of weight
    exactly 0 in the walk from 3 to 2 and targets the walk from 2 to 1 skips"""
    m, L, P, refs = store_loop(g, o, name, bs, T, resample=False, kill_at=2)
    dead, flushed = kill(L.store.n, bs)
    assert np.isneginf(L.store.lw[1][dead]).all() and np.all(L.store.lw[1][flushed] == -800.0)
    v, _, out = run_pairs(o, name, L, P, refs, dead_blocks(bs))
    v.finish(f"pairs {name} {bs} with dead particles")
    assert np.all(np.isfinite(out[2][dead_blocks(bs)]))


def test_pairs_fallback_hands_the_pair_to_the_recorded_parent(g, o):
    """line_model with a foreign slope on every third particle of step T: t = W_j for the recorded parent alone"""
    m, L, P, refs = store_loop(g, o, "line_model", 129, T)
    L.store.gen.rows[-1][::3, 0] = 7.0
    v, fell, _ = run_pairs(o, "line_model", L, P, refs, blocks_of(129))
    assert fell > 0
    v.finish("pairs fallback")


def test_pairs_with_block_parameters(g, o):
    m, L, P, refs = store_loop(g, o, "object_motion", 7, T, sets=param_sets(g))
    blocks = blocks_of(7)
    run_pairs(o, "object_motion", L, P, refs, blocks)[0].finish("pairs block parameters")
    seen("another block's parameter row", o, "object_motion", L, P, refs, blocks, wrong_P=np.roll(P, 1, axis=0))


def test_a_nan_block_reads_nan_and_lineage_0(g, o):
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T)
    for f in L.L.f:
        f.lw[7 + 3] = np.nan
    L._end()
    v, _, out = run_pairs(o, "lgssm2", L, P, refs, blocks_of(7))
    assert all(np.isnan(x[1]).all() for x in out[:3]) and np.all(out[3][1] == 0) and np.isfinite(out[2][0]).all()
    v.finish("pairs, a NaN block")


WINDOW = (1, 2)


def test_a_windowed_call_is_walked_from_the_last_step(g, o):
    """steps = (1, 2) of T = 3: two steps and the one pair (1, 2), under the smoothing weights that the walk from step 3 leaves"""
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T)
    v, _, out = run_pairs(o, "lgssm2", L, P, refs, blocks_of(7), steps=WINDOW)
    assert out[0].shape[1] == 2 and out[2].shape[1] == 1
    v.finish("pairs, steps (1, 2)")
    walk = hc.reference_walk(refs, L.store, blocks_of(7), pairs=True)          # the control: the window taken for the whole call -- steps 2 and 3
    whole = psp.pairs(o, "lgssm2", P, L.store)
    v = hc.Violations()
    hc.check_pairs(v, refs, L.store, blocks_of(7), whole[0][:, 1:], whole[1][:, 1:], whole[2][:, 1:], whole[3][:, 1:], "MISTAKEN ON PURPOSE, pairs, the wrong window", steps=WINDOW, walk=walk)
    print("control, steps (2, 3) returned for (1, 2): pairs", len(v.bad))
    assert v.bad


# ----------------------------------------------------------------------------- the nested filter
def nested_loop(g, o, steps=T):
    """block resample (ESS gate 0.8), then resampling across blocks, every step: 24 blocks of 8 object_motion particles with keep_prev, the case of
    tests/test_gpu_hp_block_smoothing.py's backward simulation.  Returns store_loop's tuple and how often the across-block call fired"""
    m = hc.case_model(g, "object_motion")
    bs, B = NESTED_BS, NESTED_B
    ys = nested_obs(g, m, steps)
    L = bsp.StoreLoop(o, m, B * bs, bs, SEED, keep_prev=True)
    L.initialize(ys[:, 0])
    fired = 0
    for t in range(1, steps):
        L.resample(0.8)
        plan = xs.resample_across_blocks(o, L.L.f[0], bs, "multinomial", ess_frac=None, check=False)
        if plan.resampled:
            fired += 1
            L.store.resample_across(L.L.f[0].parents, plan.A + 1)
            L._end()
        L.update(ys[:, t])
    return m, L, m.params, [hp.Ref(m)] * B, fired


def nested_obs(g, m, steps=T):
    return hc.moving_obs(block_obs(g, m, NESTED_B, steps))


def candidates_rows(store):
    """the Store a restatement reads with the wrong block's observation row: step s is given the row of the CANDIDATES' block (the block of the
    recorded parents) in place of the targets' -- the same row unless the lineage changed its block"""
    S = copy.copy(store)
    S.obs = list(store.obs)
    for s in range(2, store.steps + 1):
        born = store.step_map(s)[np.arange(store.B) * store.bs] // store.bs
        S.obs[s - 1] = store.obs[s - 1][born]
    return S


def check_nested(blocks_out, store):
    """some lineage changed its block, and the rows of the two blocks differ there"""
    moved = [(b, s) for b in range(store.B) for s in range(1, store.steps) if blocks_out[b, s - 1] != blocks_out[b, s]]
    assert moved and any(not np.array_equal(store.obs[s][blocks_out[b, s] - 1], store.obs[s][blocks_out[b, s - 1] - 1]) for b, s in moved)
    return len(moved)


def test_both_smoothers_in_the_nested_filter(g, o):
    """the targets' block c, the candidates' block cp and the observation row of block c differ only here; every block is checked (a transition costs
    8 x 8 pairs), by check_smooth and check_pairs over ONE reference walk"""
    m, L, P, refs, fired = nested_loop(g, o)
    blocks = list(range(NESTED_B))
    assert fired > 0
    hc.moving_inputs(L.store, blocks, travelling=True, label="nested")
    walk = reference(L, refs, blocks)
    v, _, out = run_pairs(o, "object_motion", L, P, refs, blocks, walk=walk)
    v.finish("pairs nested")
    print("nested: (block, step) where the lineage changed its block:", check_nested(out[3], L.store))
    sm = ssp.smooth(o, "object_motion", P, L.store)
    v = hc.Violations()
    hc.check_smooth(v, refs, L.store, blocks, *sm, "smooth nested", walk=walk)
    v.finish("smooth nested")
    assert np.array_equal(sm[3], out[3])
    wrong = candidates_rows(L.store)
    bad = len(run_pairs(o, "object_motion", L, P, refs, blocks, walk=walk, store=wrong, control=True)[0].bad)
    v = hc.Violations()
    hc.check_smooth(v, refs, L.store, blocks, *ssp.smooth(o, "object_motion", P, wrong), "MISTAKEN ON PURPOSE, smooth nested, the candidates' row", walk=walk)
    print(f"control, the candidates' block's observation row: pairs {bad}, smooth {len(v.bad)} violations")
    assert bad > 0 and v.bad


# ----------------------------------------------------------------------------- the skip rule
SKIP = {0: (2, 1), 1: (0, 0)}                                                # block -> (local index of the particle, the column that becomes +Inf)


def skip_mask(n, bs):
    """(particles whose current weight becomes -Inf, the same as [n, d] mask of the entries that become +Inf) -- d = 2"""
    dead, inf = np.zeros(n, bool), np.zeros((n, 2), bool)
    for b, (i, col) in SKIP.items():
        dead[b * bs + i], inf[b * bs + i, col] = True, True
    return dead, inf


def check_skip(out, blocks):
    """what the rule is for: the pair below the particle's step and every lower step are finite; its own step reads NaN in its column only"""
    mean, second, cross = out[:3]
    assert np.all(np.isfinite(cross[blocks])) and np.all(np.isfinite(mean[blocks, :-1])) and np.all(np.isfinite(second[blocks, :-1]))
    for b, (_, col) in SKIP.items():
        assert np.isnan(mean[b, -1, col]) and np.isfinite(mean[b, -1, 1 - col]) and np.isfinite(second[b, -1, 1 - col, 1 - col])


def test_a_target_of_weight_zero_with_an_infinite_row_is_skipped(g, o):
    """the module docstring: lgssm2 at 7, one particle of blocks 0 and 1 with current weight -Inf and +Inf in one column of its last row"""
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T)
    dead, inf = skip_mask(L.store.n, 7)
    for f in L.L.f:
        f.lw[dead] = -np.inf
        f.rows[:, :2][inf] = np.inf
    L._end()
    assert np.isinf(L.store.x(T)[inf]).all() and np.isneginf(L.store.lw[-1][dead]).all()
    v, _, out = run_pairs(o, "lgssm2", L, P, refs, blocks_of(7))
    check_skip(out, blocks_of(7))
    v.finish("pairs, a skipped target with an infinite row")
    # the control: the restatement without the rule; and, for finite rows, that the rule changes no bit -- which is why only this case tests it
    seen("a target of weight 0 is not skipped", o, "lgssm2", L, P, refs, blocks_of(7), skip=False)
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T, resample=False, kill_at=2)
    assert all(np.array_equal(a, b) for a, b in zip(psp.pairs(o, "lgssm2", P, L.store), psp.pairs(o, "lgssm2", P, L.store, skip=False)))


# ----------------------------------------------------------------------------- the negative controls
def transposed(mean, second, cross, blocks):
    return mean, second, cross.transpose(0, 1, 3, 2), blocks


def independent(mean, second, cross, blocks):
    return mean, second, mean[:, :-1, :, None] * mean[:, 1:, None, :], blocks


def pair_below(mean, second, cross, blocks):
    """the pair (s - 1, s) stored at s"""
    return mean, second, np.concatenate([cross[:, :1], cross[:, :-1]], axis=1), blocks


def centred(mean, second, cross, blocks):
    return mean, second - mean[..., :, None] * mean[..., None, :], cross, blocks


OUTPUT_CONTROLS = [("cross transposed", "lgssm2", transposed), ("cross transposed", "bearings4", transposed),
                   ("mean_s (x) mean_{s+1} in place of cross", "lgssm2", independent), ("the pair (s - 1, s) stored at s", "lgssm2", pair_below),
                   ("second centred on the mean", "lgssm2", centred)]


@pytest.mark.parametrize("what,name,mutate", OUTPUT_CONTROLS, ids=[f"{c[0]}-{c[1]}" for c in OUTPUT_CONTROLS])
def test_a_wrong_output_is_seen(g, o, what, name, mutate):
    m, L, P, refs = store_loop(g, o, name, 7, T)
    seen(what, o, name, L, P, refs, blocks_of(7), mutate=mutate)


@pytest.mark.parametrize("control", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_a_mistake_of_meaning_is_seen(g, o, control):
    """the store and parameter mistakes of tests/test_hp_block_smoothing.py through check_pairs, at 7"""
    what, name, kw, mistake = control
    m, L, P, refs = store_loop(g, o, name, 7, T, ess_frac=0.5 if mistake == "lw" else None)
    kw = dict(kw)
    if isinstance(mistake, str):
        kw["store"] = shifted(L.store, mistake)
    elif mistake is not None:
        kw["wrong_P"] = swapped(P, *mistake)
    seen(what, o, name, L, P, refs, blocks_of(7), **kw)


def test_every_target_on_its_fallback_is_seen(g, o):
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T)
    seen("fallback=True", o, "lgssm2", L, P, refs, blocks_of(7), fallback=True)
