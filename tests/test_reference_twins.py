"""Pin of the oracle to the reference's own arithmetic, for boxes that have Julia + Gen (SURVEY.md §8c "what travels"):
julia/reference_twins.jl evaluates log p(y_t | x_t) with Gen on @gen twins of the five native models at the latent values
of tests/golden/twin_inputs.txt and writes tests/golden/ref_twin_weights.txt.  When that file is present the oracle must
agree with Gen at rtol 1e-12 (Julia's libm vs the oracle's own exp/log/atan2); while it is absent -- the build image and
the GPU boxes have no Julia -- the comparison is SKIPPED and parity stays "unpinned" for random streams AND for Gen's
per-particle semantics.  The inputs themselves are checked against the oracle on every run, so the fixture cannot rot."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "twin_inputs.txt")
REF = os.path.join(HERE, "golden", "ref_twin_weights.txt")


def read_inputs():
    rows = []
    for ln in open(INPUTS):
        f = ln.split()
        nobs = int(f[2]); obs = np.array(f[3:3 + nobs], float); d = int(f[3 + nobs])
        prev = np.array(f[4 + nobs:4 + nobs + d], float); cur = np.array(f[4 + nobs + d:4 + nobs + 2 * d], float)
        rows.append((f[0], int(f[1]), obs, prev, cur, float(f[4 + nobs + 2 * d])))
    return rows


def oracle_loglik(g, o, name, obs, prev, cur):
    m = g.models.by_name(name)
    W = m.row_width(True)
    row = np.zeros((1, W)); row[0, :m.dim] = cur; row[0, m.dim:2 * m.dim] = prev
    out = np.empty(1)
    o.lib().o_loglik_rows(m.model_id, np.ascontiguousarray(m.params), row, W, 1, np.ascontiguousarray(obs), out)
    return out[0]


def test_twin_inputs_are_the_oracles(g, o):
    rows = read_inputs()
    assert {r[0] for r in rows} == {"lgssm2", "bearings4", "sv1", "object_motion", "line_model"}
    for name, t, obs, prev, cur, ll in rows:
        assert oracle_loglik(g, o, name, obs, prev, cur) == ll


def test_twin_inputs_agree_with_the_mpmath_reference(g):
    """the fixture's one independent witness while Gen's answers are absent: every log p(y_t | x_t) a Julia box would score equals the density of
    the model DEFINITION in mpmath (tests/hp_reference.py, natural parameters only), within the bound derived for that value"""
    import hp_reference as hp
    rows = read_inputs()
    refs = {name: hp.Ref(g.models.by_name(name)) for name in {r[0] for r in rows}}
    tols = []
    for name, t, obs, prev, cur, ll in rows:
        want = refs[name].loglik(list(cur), list(obs))
        d, tol = hp.differs(ll, want)
        assert d <= tol, (name, t, ll, want)
        tols.append(hp.rel_tol(want))
    assert np.median(tols) < 1e-12


def test_twins_script_names_every_model():
    src = open(os.path.join(os.path.dirname(HERE), "julia", "reference_twins.jl")).read()
    for fn in ("lgssm2_step", "bearings4_step", "sv1_step", "object_motion_step", "line_step_twin", "project(trace, ysel)", "pf_resample!"):
        assert fn in src


@pytest.mark.skipif(not os.path.exists(REF), reason="tests/golden/ref_twin_weights.txt absent: no Julia/Gen box has run julia/reference_twins.jl yet")
def test_oracle_matches_gen(g, o):
    rows = read_inputs()
    ref = [ln.split() for ln in open(REF)]
    assert len(ref) == len(rows)
    for (name, t, obs, prev, cur, ll), r in zip(rows, ref):
        assert r[0] == name and int(r[1]) == t
        np.testing.assert_allclose(ll, float(r[2]), rtol=1e-12, atol=1e-12, err_msg=f"{name} step {t}")
