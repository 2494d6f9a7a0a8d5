"""Forward-only smoothing per block (gpf.h gpf_block_forward_moments) against its DEFINITION -- the CPU rehearsal of
tests/test_gpu_hp_block_forward.py.  The NumPy restatement (tests/block_forward_spec.py) runs on the CPU oracle's filter (store_loop of
tests/test_hp_block_smoothing.py, whose models, data and helpers these are) and its outputs go through hp_forward.check_forward: the mpmath values of the
pairwise reference walked BACKWARDS over the whole store, summed over the steps, with the Float64 bound of every entry derived by E propagation through the
forward statements.  The bit-for-bit device test cannot see a mistake the kernel shares with its twin -- the wrong observation row when a lineage changes
block, an exchanged parameter, cross transposed, the increment formed with the recorded parent's row --; this can.

Shapes: blocks of 7 (three full ones and a short one of five), T = 3, every block and every step: the forward form has no window, a close reads every
target of the step, so the cases stay at the size where a whole run is a second of mpmath; the nested filter at 24 blocks of 8.  Nothing is thinned or
skipped.  Negative controls: each is ONE mistake of meaning and must produce violations where the unmutated run of the same case produces none."""
import numpy as np
import pytest

import across_blocks_spec as xs
import block_forward_spec as fsp
import hp_checks as hc
import hp_forward as hf
import hp_reference as hp
from test_hp_block_pairs import NESTED_B, NESTED_BS, nested_obs
from test_hp_block_smoothing import SEED, T_SMOOTH, kill, param_sets, store_loop

T = T_SMOOTH


def all_blocks(S):
    return list(range(S.B))


def run(o, name, L, P, refs, label, mutate=None, control=False, **kw):
    out = fsp.forward(o, name, P, L.store, **kw)
    if mutate is not None:
        out = mutate(out)
    v = hc.Violations()
    hf.check_forward(v, refs, L.store, all_blocks(L.store), out, ("MISTAKEN ON PURPOSE, " if control else "") + label)
    return v, out


@pytest.mark.parametrize("name", ["lgssm2", "object_motion", "sv1", "bearings4"])
@pytest.mark.parametrize("ess", [None, 0.5])
def test_forward_moments_follow_the_definition(g, o, name, ess):
    m, L, P, refs = store_loop(g, o, name, 7, T, ess_frac=ess)               # (the ESS gate leaves unequal recorded weights in some blocks)
    if name == "object_motion":
        hc.moving_inputs(L.store, all_blocks(L.store))
    v, out = run(o, name, L, P, refs, f"forward {name} 7 ess {ess}")
    v.finish(f"forward {name} 7")
    assert all(np.all(np.isfinite(x)) for x in out[:6])


def test_forward_with_dead_and_flushed_past_particles(g, o):
    """no resample; after step 2 some weights become -Inf and one per block -800: candidates with q = 0 in the close of step 3"""
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T, resample=False, kill_at=2)
    dead, flushed = kill(L.store.n, 7)
    assert np.isneginf(L.store.lw[1][dead]).all() and np.all(L.store.lw[1][flushed] == -800.0)
    run(o, "lgssm2", L, P, refs, "forward lgssm2 7 with dead particles")[0].finish("forward, dead particles")


def test_forward_fallback_takes_the_recorded_parent(g, o):
    """line_model with a foreign slope on every third particle of steps 2 and 3: the close of step 2 and the query's forming of step 3 fall back"""
    m, L, P, refs = store_loop(g, o, "line_model", 7, T)
    L.store.gen.rows[1][::3, 0] = 7.0
    L.store.gen.rows[2][::3, 0] = 8.0
    run(o, "line_model", L, P, refs, "forward fallback")[0].finish("forward fallback")


def test_forward_with_block_parameters(g, o):
    m, L, P, refs = store_loop(g, o, "object_motion", 7, T, sets=param_sets(g))
    run(o, "object_motion", L, P, refs, "forward block parameters")[0].finish("forward block parameters")
    bad = len(run(o, "object_motion", L, np.roll(P, 1, axis=0), refs, "forward block parameters", control=True)[0].bad)
    print("control, another block's parameter row:", bad, "violations")
    assert bad > 0


def test_a_nan_block_reads_nan(g, o):
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T)
    for f in L.L.f:
        f.lw[7 + 3] = np.nan
    L._end()
    v, out = run(o, "lgssm2", L, P, refs, "forward, a NaN block")
    assert all(np.isnan(x[1]).all() for x in out[:6]) and all(np.isfinite(x[0]).all() for x in out[:6])
    v.finish("forward, a NaN block")


def nested(g, o):
    m = hc.case_model(g, "object_motion")
    ys = nested_obs(g, m)
    n, bs = NESTED_B * NESTED_BS, NESTED_BS
    import block_backward_spec as bsp
    L = bsp.StoreLoop(o, m, n, bs, SEED, keep_prev=True)
    L.initialize(ys[:, 0])
    fired = 0
    for t in range(1, T):
        L.resample(0.8)
        f = L.L.f[0]
        plan = xs.resample_across_blocks(o, f, bs, "multinomial", check=False)
        if plan.resampled:
            fired += 1
            L.store.resample_across(f.parents, plan.A + 1)
            L._end()
        L.update(ys[:, t])
    return m, L, fired


def test_forward_in_the_nested_filter(g, o):
    """block resample, then resampling across blocks, every step: the targets' block, the candidates' block and the observation row differ only here"""
    m, L, fired = nested(g, o)
    assert fired > 0
    blocks = all_blocks(L.store)
    hc.moving_inputs(L.store, blocks, travelling=True, label="nested")
    refs = [hp.Ref(m)] * L.store.B
    run(o, "object_motion", L, m.params, refs, "forward nested")[0].finish("forward nested")


# ----------------------------------------------------------------------------- negative controls
@pytest.mark.parametrize("what", ["cross transposed", "the recorded parent's row for xbar", "no transition density", "second for last2", "sum without step 1"])
def test_one_mistake_of_meaning_is_seen(g, o, what):
    m, L, P, refs = store_loop(g, o, "lgssm2", 7, T, ess_frac=0.5)
    assert not run(o, "lgssm2", L, P, refs, "forward lgssm2 7")[0].bad
    kw, mutate = {}, None
    if what == "cross transposed":
        mutate = lambda r: r._replace(cross=r.cross.transpose(0, 2, 1))
    elif what == "the recorded parent's row for xbar":
        kw = dict(parent_x=True)
    elif what == "no transition density":
        kw = dict(trans=False)
    elif what == "second for last2":
        mutate = lambda r: r._replace(last2=r.second)
    else:
        mutate = lambda r: r._replace(sum=r.sum - r.first)
    bad = len(run(o, "lgssm2", L, P, refs, "forward lgssm2 7", mutate=mutate, control=True, **kw)[0].bad)
    print(f"control, {what}: {bad} violations")
    assert bad > 0, what
