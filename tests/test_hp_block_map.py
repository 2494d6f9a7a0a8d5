"""The most probable path per block against its definition, the CPU rehearsal: the checks of tests/hp_map.py -- the same dynamic programme in mpmath from
the models of tests/hp_reference.py, every tolerance a derived E bound -- on the NumPy restatement (tests/block_map_spec.py) over the CPU oracle's
filters, all five models, up to blocks of 64 at T = 3; the new model members logprior and transrest pinned per value against the full Gen densities; and
the negative controls of the restatement rejected.  tests/test_gpu_hp_block_map.py sends the device's outputs through the same checks.

Of the five controls, four are rejected here.  The fifth -- the largest j on ties -- changes no total: both paths are maximisers under ANY arithmetic,
so no check on scores can tell them apart; it is rejected by the bit-for-bit tests (tests/test_block_map_host.py, tests/test_gpu_block_map.py)."""
import numpy as np
import pytest

import block_map_spec as msp
import hp_checks as hc
import hp_map as hm
import hp_reference as hp
from test_block_map_host import cpu_loop

MODELS = ["lgssm2", "sv1", "bearings4", "object_motion", "line_model"]
SHAPES = [(7, 4), (64, 3)]                                                   # (block size, steps)


def checked_blocks(bs, B):
    return [0, B - 1]                                                        # a full block and the short last one


def run_case(g, o, name, bs, T, n=None, **kw):
    n = 2 * bs + 5 if n is None else n                                       # two full blocks and a short one
    m, S, P, ev = cpu_loop(g, o, name, n, bs, T, **kw)
    sets = kw.get("sets")
    refs = [hp.Ref(m if sets is None else sets[kw["assign"][b]]) for b in range(S.B)]
    return m, S, P, refs, ev


# ----------------------------------------------------------------------------- the new model members, value by value
def points(name, rng, k=24):
    x = rng.standard_normal((k, {"lgssm2": 2, "sv1": 1, "bearings4": 4, "object_motion": 2, "line_model": 2}[name])) * 3.0
    if name == "object_motion":
        x[:, 0] = rng.integers(0, 2, k)
    if name == "line_model":
        x[:, 0], x[:, 1] = rng.integers(-2, 3, k), rng.integers(0, 2, k)
    return x


@pytest.mark.parametrize("name", MODELS)
def test_logprior_is_the_initial_law_without_its_constants(g, name):
    m = hc.case_model(g, name)
    ref, rng, v = hp.Ref(m), np.random.default_rng(5), hc.Violations()
    x = points(name, rng)
    for obs in ([0.3, 0.8], [-1.2, 0.0]):                                    # (line_model: a step with an outlier choice, and model args (0,))
        got = msp.logprior(name, m.params, x, np.array(obs))
        for i in range(len(x)):
            v.value(f"{name} logprior obs {obs}", i, got[i], hm.logprior(ref, [float(c) for c in x[i]], obs))
    v.finish(f"{name} logprior")


@pytest.mark.parametrize("name", MODELS)
def test_transrest_is_what_logtrans_leaves_out_that_depends_on_x(g, name):
    m = hc.case_model(g, name)
    ref, rng = hp.Ref(m), np.random.default_rng(6)
    x, xp = points(name, rng), points(name, rng)
    if name == "line_model":
        v = hc.Violations()
        for obs in ([0.3, 2.0], [0.0, 0.0]):
            got = msp.transrest(name, m.params, x, np.array(obs))
            for i in range(len(x)):
                want = hm.transrest(ref, [float(c) for c in x[i]], obs)
                v.value(f"transrest obs {obs}", i, got[i], want)
                assert abs(hm.x_free_rest(ref, [float(c) for c in x[i]], [float(c) for c in x[i]], obs) - want.v) < hp.mpf(2) ** -120
        v.finish("line_model transrest")
        assert len(set(got.tolist())) == 1 and len(set(msp.transrest(name, m.params, x, np.array([0.3, 2.0])).tolist())) == 2
    else:                                                                    # the full density minus logtrans is a constant: nothing is left for transrest
        assert msp.transrest(name, m.params, x, np.array([0.3, 0.8])) is None and hm.transrest(ref, list(x[0]), [0.3, 0.8]) is None
        for i in range(len(x)):
            rest = hm.x_free_rest(ref, [float(c) for c in xp[i]], [float(c) for c in x[i]], [0.3, 0.8])
            assert abs(rest) < hp.mpf(2) ** -100, (name, i, rest)


# ----------------------------------------------------------------------------- the restatement through the checks
@pytest.mark.parametrize("bs,T", SHAPES)
@pytest.mark.parametrize("name", MODELS)
def test_the_restatement_returns_a_maximiser_and_its_total(g, o, name, bs, T):
    m, S, P, refs, _ = run_case(g, o, name, bs, T)
    worst = hm.check_map(refs, S, checked_blocks(bs, S.B), *msp.map_paths(o, name, P, S), f"map {name} {bs}")
    print(f"map {name} {bs} x {T}: worst |logp - S| / bound", round(worst, 3))


def test_the_nested_filter(g, o):
    m, S, P, refs, (_, fired) = run_case(g, o, "lgssm2", 7, 4, n=6 * 7, ess_frac=0.8, across=True)
    assert fired > 0
    got = msp.map_paths(o, "lgssm2", P, S)
    assert np.any((got[1] - 1) // 7 != np.arange(S.B)[:, None])
    hm.check_map(refs, S, list(range(S.B)), *got, "map nested")


def test_per_block_parameters(g, o):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    m, S, P, refs, _ = run_case(g, o, "object_motion", 7, 4, sets=sets, assign=np.arange(3) % 3)
    hm.check_map(refs, S, list(range(S.B)), *msp.map_paths(o, "object_motion", P, S), "map block parameters")


# ----------------------------------------------------------------------------- the negative controls
@pytest.mark.parametrize("key,name", [("node", "lgssm2"), ("obs_next", "object_motion"), ("rest", "line_model"), ("ptr_trace", "lgssm2"), ("ptr_trace", "sv1")])
def test_a_control_is_rejected(g, o, key, name):
    m, S, P, refs, _ = run_case(g, o, name, 7, 4)
    blocks = list(range(S.B))
    hm.check_map(refs, S, blocks, *msp.map_paths(o, name, P, S), f"{name}, no mistake")
    with pytest.raises(AssertionError, match="not a maximiser|logp is not the returned path's total"):
        hm.check_map(refs, S, blocks, *msp.map_paths(o, name, P, S, **{key: False}), f"{name} with {key}=False")
