"""Ancestor sampling, backward simulation and marginal smoothing per block on the device against their DEFINITIONS: the checks of tests/hp_checks.py
(check_logtrans, check_ancestor, check_backward, check_smooth) over the mpmath reference of tests/hp_weights.py, fed with what a caller sees -- the
Store of tests/block_backward_spec.py filled by the Dev helper, the seed, the epoch and the device's outputs.  tests/test_hp_block_smoothing.py is the
CPU rehearsal: the same checks on the NumPy restatements, the negative controls, and the evidence for shapes, seeds and thinning.  The bit-for-bit
tests (test_gpu_block_ancestor.py, test_gpu_block_backward.py, test_gpu_block_smooth.py) cannot see a mistake the kernel shares with its twin; these
can.  Every tolerance is a derived E bound; an undecidable draw (within the reference's own quantisation bound of a CDF boundary) is not compared and at
most hp_checks.MAX_UNDECIDABLE per (block, step) are allowed -- the checks assert it, on the reference's own verdicts alone."""
import warnings

import numpy as np
import pytest

import hp_checks as hc
import hp_reference as hp
import test_hp_block_smoothing as cpu
from test_gpu_block_backward import Dev
from test_gpu_block_conditional import n_of, references

pytestmark = pytest.mark.gpu
SEED, SIZES, MODELS = cpu.SEED, cpu.SIZES, cpu.MODELS
T_BACK, T_SMOOTH, T_ANC, K_DRAWS = cpu.T_BACK, cpu.T_SMOOTH, cpu.T_ANC, cpu.K_DRAWS


def dev(g, name, bs, steps, sets=None, **kw):
    """(Dev, one Ref per block): the models, data and shapes of the CPU rehearsal"""
    m = hc.case_model(g, name)
    n = kw.pop("n", n_of(bs))
    B = (n + bs - 1) // bs
    assign = None if sets is None else np.arange(B) % len(sets)
    d = Dev(g, name, bs, n=n, steps=steps, seed=SEED, model=m, ys=kw.pop("ys", None) if "ys" in kw else cpu.case_obs(g, m, B, steps),
            params=None if sets is None else [sets[k] for k in assign], **kw)
    return d, [hp.Ref(m if sets is None else sets[assign[b]]) for b in range(B)]


# ----------------------------------------------------------------------------- ancestor sampling
def ancestor_case(g, name, bs, keep_prev, sets=None):
    m = hc.case_model(g, name)
    n = n_of(bs)
    B = (n + bs - 1) // bs
    ys, ref = cpu.ancestor_data(g, m, B)
    assign = None if sets is None else np.arange(B) % len(sets)
    refs = [hp.Ref(m if sets is None else sets[assign[b]]) for b in range(B)]
    blocks, vl, va, moved, epoch, calls = cpu.blocks_of(bs), hc.Violations(), hc.Violations(), 0, 1, []
    label = f"ancestor {name} {bs}"
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=keep_prev, reference=ref[:, 0], params=None if sets is None else [sets[k] for k in assign])
    for t in range(1, T_ANC):                                                # the filter first: what every call saw and returned
        rows0, lw0 = st.traces, st.log_weights
        st.log_weights = np.zeros(n)                                         # with log_weights = 0 the ancestor weights are logtrans itself
        got = g.block_ancestor_log_weights(st, bs, ys[:, t], ref[:, t])
        st.log_weights = lw0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g.pf_resample_blocks(st, bs, "multinomial", check=False, conditional=True, reference=ref[:, t], observations=ys[:, t])
        calls.append((rows0, lw0, epoch, got, g.block_resampled(st), st.parents))
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs, reference=ref[:, t])
        epoch += 2
    st.close()
    if name == "object_motion":
        hc.moving_ancestor_inputs(bs, blocks, [(c[0], ref[:, t], ys[:, t]) for t, c in zip(range(1, T_ANC), calls)], label)
    for t, (rows0, lw0, E, got, mask, parents) in zip(range(1, T_ANC), calls):
        assert mask[blocks].all(), (label, t, "a checked block did not resample")
        hc.check_logtrans(vl, refs, bs, blocks, rows0, ref[:, t], ys[:, t], got, f"logtrans {name} {bs}")
        und = hc.check_ancestor(va, refs, bs, blocks, rows0, lw0, ref[:, t], ys[:, t], SEED, E, mask, parents, label)
        assert sorted(und) == blocks
        moved += int((parents[[b * bs for b in blocks]] != 1).sum())
    vl.finish(f"logtrans {name} {bs}")
    va.finish(label)
    return moved


@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS + ["line_model"])
def test_ancestor_weights_and_draws_follow_the_definition(g, name, bs, keep_prev):
    moved = ancestor_case(g, name, bs, keep_prev)
    assert moved > 0 or (name == "line_model" and bs == 7)


def test_ancestor_sampling_with_block_parameters(g):
    assert ancestor_case(g, "object_motion", 129, True, sets=cpu.param_sets(g)) > 0


# ----------------------------------------------------------------------------- backward simulation
def backward_case(g, name, bs, blocks, label, sets=None, travelling=False, held=True, **kw):
    d, refs = dev(g, name, bs, T_BACK, sets=sets, **kw)
    traj, idx, E = d.draw(K_DRAWS)
    if name == "object_motion":
        hc.moving_inputs(d.S, blocks, held={b: d.S.x(T_BACK)[idx[b, :, -1] - 1, 0] for b in blocks} if bs > 7 and held else None, travelling=travelling, label=label)
    v = hc.Violations()
    left = hc.check_backward(v, refs, d.S, blocks, SEED, E, idx, label)
    for b in blocks:                                                         # the paths are the rows of the indices
        for s in range(1, T_BACK + 1):
            assert np.array_equal(traj[b, :, s - 1], d.S.x(s)[idx[b, :, s - 1] - 1]), (label, b, s)
    v.finish(label)
    return d, idx


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_backward_simulation_follows_the_definition(g, name, bs):
    backward_case(g, name, bs, cpu.back_blocks(name, bs), f"backward {name} {bs}")[0].close()


def test_backward_simulation_of_the_line_model_is_exact(g):
    d, idx = backward_case(g, "line_model", 129, cpu.blocks_of(129), "backward line_model")
    x = [d.S.x(s)[idx[:, :, s - 1] - 1, 0] for s in range(1, T_BACK + 1)]
    assert all(np.array_equal(x[0], x[s]) for s in range(T_BACK)) and len(np.unique(d.S.x(1)[:129, 0])) > 1
    d.close()


def test_backward_simulation_with_block_parameters(g):
    backward_case(g, "object_motion", 129, cpu.blocks_of(129), "backward block parameters", sets=cpu.param_sets(g), keep_prev=True, held=False)[0].close()


def test_backward_simulation_in_the_nested_filter(g):
    """block resample, then resampling across blocks, every step, shared parameters: the candidates are the lineage's block and the observation rows
    move with their blocks"""
    bs, B = 8, 24
    m = hc.case_model(g, "object_motion")
    d, idx = backward_case(g, "object_motion", bs, list(range(B)), "backward nested", n=B * bs, keep_prev=True, ess_frac=0.8, across=True,
                           ys=hc.moving_obs(cpu.block_obs(g, m, B, T_BACK)), travelling=True)   # (every block: a transition costs 8 x 8 pairs)
    assert d.fired > 0
    p = idx - 1
    assert any(np.any(d.S.step_map(s)[p[:, :, s - 1]] // bs != p[:, :, s - 1] // bs) for s in range(2, T_BACK + 1))     # (some lineage changed its block)
    d.close()


# ----------------------------------------------------------------------------- marginal smoothing
def got(d):
    return d.g.block_smoothed_moments(d.st, d.bs, return_weights=True, return_blocks=True)


def smooth_case(g, name, bs, label, lo=None, sets=None, blocks=None, **kw):
    d, refs = dev(g, name, bs, T_SMOOTH, sets=sets, **kw)
    blocks = cpu.blocks_of(bs) if blocks is None else blocks
    if name == "object_motion":
        hc.moving_inputs(d.S, blocks, label=label)
    v = hc.Violations()
    fell = hc.check_smooth(v, refs, d.S, blocks, *got(d), label, lo=lo)
    v.finish(label)
    return d, fell


def thin(d, t):
    """Dev's after_update hook: at the last step all but about KEEP current weights of every block become -Inf"""
    if t == T_SMOOTH:
        lw = d.st.log_weights
        lw[~cpu.thin_mask(d.n, d.bs)] = -np.inf
        d.st.log_weights = lw


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", ["object_motion", "lgssm2"])
def test_smoothing_follows_the_definition(g, name, bs):
    d, _ = smooth_case(g, name, bs, f"smooth {name} {bs}", lo=cpu.smooth_lo(bs), after_update=thin if bs == 513 else None)
    if bs == 513:
        assert np.isneginf(d.S.lw[-1]).sum() == d.n - cpu.thin_mask(d.n, bs).sum()
    d.close()


@pytest.mark.parametrize("name", ["sv1", "bearings4"])
def test_smoothing_of_the_other_models(g, name):
    smooth_case(g, name, 7, f"smooth {name} 7", ess_frac=0.5)[0].close()


@pytest.mark.parametrize("name,bs", cpu.DEAD)
def test_smoothing_with_dead_and_flushed_past_particles(g, name, bs):
    """the case of the CPU rehearsal: no resample; after step 2 some weights become -Inf and one per block -800 (cpu.kill)"""
    def kill(d, t):
        if t == 2:                                                           # step 2, which no resample follows: the weights stay in its record
            dead, flushed = cpu.kill(d.n, bs)
            lw = d.st.log_weights
            lw[dead], lw[flushed] = -np.inf, -800.0
            d.st.log_weights = lw

    d, _ = smooth_case(g, name, bs, f"smooth {name} {bs} with dead particles", blocks=cpu.dead_blocks(bs), resample=False, after_update=kill)
    dead, flushed = cpu.kill(d.n, bs)
    assert np.isneginf(d.S.lw[1][dead]).all() and np.all(d.S.lw[1][flushed] == -800.0)
    W = got(d)[2]
    W2 = np.concatenate([W[b, 1, :min(bs, d.n - b * bs)] for b in range(d.B)])
    assert np.all(W2[dead | flushed] == 0.0)
    d.close()


def test_smoothing_fallback_hands_the_weight_to_the_recorded_parent(g):
    """line_model with a foreign slope on every third particle of step T (the case of tests/test_gpu_block_smooth.py): all its ancestor weights are -Inf"""
    bs, B = 129, 4

    def foreign_slope(d, t):
        if t == T_SMOOTH:
            rows = d.st.traces
            rows[np.arange(bs * B) % 3 == 0, 0] = 7.0
            d.st.traces = rows
            d.st.log_weights = np.zeros(bs * B)

    d, fell = smooth_case(g, "line_model", bs, "smooth fallback", n=bs * B, after_update=foreign_slope, final_resample=True)
    assert fell > 0
    d.close()


def test_a_nan_block_reads_nan_and_index_0(g):
    d, refs = dev(g, "lgssm2", 7, T_BACK)
    lw = d.st.log_weights
    lw[7 + 3] = np.nan
    d.st.log_weights = lw
    d.S.lw[-1] = lw.copy()
    blocks, v = cpu.blocks_of(7), hc.Violations()
    _, idx, E = d.draw(K_DRAWS)
    hc.check_backward(v, refs, d.S, blocks, SEED, E, idx, "backward, a NaN block")
    out = got(d)
    hc.check_smooth(v, refs, d.S, blocks, *out, "smooth, a NaN block")
    assert np.all(idx[1] == 0) and np.all(idx[0] > 0) and np.isnan(out[0][1]).all() and np.isfinite(out[0][0]).all()
    v.finish("a NaN block")
    d.close()


def test_smoothing_with_block_parameters(g):
    smooth_case(g, "object_motion", 7, "smooth block parameters", sets=cpu.param_sets(g), keep_prev=True)[0].close()
