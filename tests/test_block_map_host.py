"""The most probable path per block (gpf.h gpf_block_map_path), the parts that need no GPU: the entry point exists in every layer (header, library,
ctypes table, package, Julia glue); and the NumPy restatement -- tests/block_map_spec.py -- against the enumeration of ALL bs^T sequences of a block
on the CPU oracle's filters: logp is the maximum of the right-nested totals bit for bit (rounded addition is monotone), the returned path's own total is
logp bit for bit, and where the maximiser is bitwise unique the path IS the maximiser.  The nested filter, per-block parameters, ESS-gated steps, a short
last block, T = 1, an all -Inf continuation and an undefined lineage; every negative-control switch of the restatement changes logp or the path
somewhere."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import across_blocks_spec as xs
import block_backward_spec as bsp
import block_map_spec as msp
from test_gpu_block_conditional import block_obs, model_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = ["gpf_handle", "int64_t", "int32_t", "int32_t", "double*", "int64_t*", "double*"]


def header():
    return open(os.path.join(ROOT, "include", "gpf.h")).read()


# ----------------------------------------------------------------------------- the entry point in every layer
def test_header_declares_the_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"gpf_status\s+gpf_block_map_path\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "gpf_block_map_path is not declared in include/gpf.h"
    params = [re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", a.strip()).replace(" ", "") for a in m.group(1).split(",")]
    assert params == PROTO


def test_header_states_the_definition():
    txt = header()
    end = txt.index("gpf_status gpf_block_map_path(gpf_handle")
    doc = txt[txt.rindex("/*", 0, end):end]
    assert "Godsill, Doucet & West 2001" in doc
    for piece in ("c_T = b", "logp NaN", "transrest", "v_T^j = n_T^j", "ASCENDING j", "if (val > best) { best = val; ptr = j; }", "a NaN never wins",
                  "the smallest j wins a tie", "logprior(P_b, x_1^i, obs_1[c_1])", "the smallest i attaining the maximum", "p_{s+1} = ptr_s[p_s]",
                  "NOT a normalised log density", "right-nested", "the epoch does not advance"):
        assert piece in doc, piece
    for refusal in ("GPF_ERR_STATE", "GPF_ERR_INVALID_ARGUMENT", "whole-filter call", "2048", "all outputs NULL", "per-block parameters", "2^31"):
        assert refusal in doc, refusal


def test_library_exports_the_entry_point(g):
    L = ctypes.CDLL(g._lib.LIB_PATH)
    assert hasattr(L, "gpf_block_map_path"), "gpf_block_map_path is not exported by the built library"
    assert L.gpf_abi_version() == 1                                                          # additive: the ABI version stays


def test_ctypes_table(g):
    C = ctypes
    pd = C.POINTER(C.c_double)
    table = {s[0]: s for s in g._lib.SYMBOLS}
    assert table["gpf_block_map_path"][1:] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, pd, C.POINTER(C.c_int64), pd])


def test_package_exports_and_argument_checks(g):
    assert list(inspect.signature(g.block_map_trajectories).parameters) == ["state", "block_size", "steps", "return_indices", "return_log_density"]

    class NoStore:
        history_blocks = True
    with pytest.raises(g.ErrorException, match="history_weights=True"):                      # the message names the keyword
        g.block_map_trajectories(NoStore(), 4)


def test_julia_glue_calls_the_entry_point():
    jl = open(os.path.join(ROOT, "julia", "GenParticleFiltersAMD.jl")).read()
    assert re.search(r"ccall\(\(:gpf_block_map_path, libgpf\), Cint, \(Ptr\{Cvoid\}, Int64, Cint, Cint, Ptr\{Cdouble\}, Ptr\{Int64\}, Ptr\{Cdouble\}\)", jl)
    assert re.search(r"^function block_map_trajectories\(s::DeviceParticleFilterState, block_size::Int", jl, re.M)


# ----------------------------------------------------------------------------- the oracle's filters
def line_data(g, B, steps, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([[g.models.line_obs(t + 1, float(s)) for t in range(steps)] for s in rng.integers(-2, 3, B)])


def cpu_loop(g, o, name, n, bs, T, seed=17, ess_frac=None, sets=None, assign=None, across=False):
    """initialise -> (resample blocks [-> resample across blocks] -> update)* on the CPU oracle, recorded into a Store: (model, store, P, events)"""
    m = g.models.line_model() if name == "line_model" else model_of(g, name)
    B = (n + bs - 1) // bs
    ys = line_data(g, B, T) if name == "line_model" else block_obs(g, m, B, T)
    L = bsp.StoreLoop(o, m, n, bs, seed, param_sets=None if sets is None else [s.params for s in sets], assign=assign)
    L.initialize(ys[:, 0])
    kept = fired = 0
    for t in range(1, T):
        kept += int((~L.resample(ess_frac)).sum())
        if across:
            f = L.L.f[0]
            plan = xs.resample_across_blocks(o, f, bs, "multinomial", check=False)
            if plan.resampled:
                fired += 1
                L.store.resample_across(f.parents, plan.A + 1)
                L._end()
        L.update(ys[:, t])
    P = m.params if sets is None else np.stack([sets[k].params for k in assign])
    return m, L.store, P, (kept, fired)


def check_block(o, name, P, S, b, got, unique):
    """the three properties for final block b; got = map_paths' outputs for all steps.  Returns whether the maximiser was bitwise unique"""
    path, idx, logp = got
    tot = msp.brute_force(o, name, P, S, b)
    m, arg = msp.maximum(tot)
    assert (np.isnan(m) and np.isnan(logp[b])) or logp[b] == m, (name, b, logp[b], m)                    # bit for bit
    if not np.isfinite(m):
        return False
    p = msp.local_path(S, idx[b])
    assert tot[p] == logp[b], (name, b, "the returned path's own total")
    for s in range(1, S.steps + 1):
        assert np.array_equal(path[b, s - 1], S.x(s)[idx[b, s - 1] - 1])
    assert p in arg
    rows = lambda q: [S.x(s)[S.bs * ((idx[b, s - 1] - 1) // S.bs) + q[s - 1]].tobytes() for s in range(1, S.steps + 1)]
    if unique == "index":
        assert len(arg) == 1, (name, b, "the maximiser is not unique for this seed", arg)
    elif unique:                                                             # (the copies a resample made of one particle are one point of the grid)
        assert all(rows(q) == rows(arg[0]) for q in arg), (name, b, "the maximiser is not unique for this seed", arg)
    return len(arg) == 1


CASES = [(name, bs, T) for name in ("lgssm2", "sv1", "bearings4", "object_motion") for bs in (3, 4) for T in (4, 5)]


@pytest.mark.parametrize("resample", [True, False])
@pytest.mark.parametrize("name,bs,T", CASES)
def test_logp_is_the_brute_force_maximum_and_the_path_its_unique_maximiser(g, o, name, bs, T, resample):
    """resample=True: every block resamples at every step, so the snapshots below T hold copies of one particle, and the maximiser is unique as a sequence
    of latent VALUES -- every index sequence that attains the maximum has the same rows bit for bit, the returned one among them.  resample=False (an ESS
    gate that never fires: identity maps): no copies, and the maximiser is unique as an index sequence.  Seed 17 throughout: unique in every case"""
    n = 2 * bs + (bs - 1)                                                      # two full blocks and a short last one
    m, S, P, (kept, _) = cpu_loop(g, o, name, n, bs, T, ess_frac=None if resample else 0.0)
    assert kept == (0 if resample else (T - 1) * S.B)
    got = msp.map_paths(o, name, P, S)
    assert np.all(np.isfinite(got[2])) and np.all(got[1] >= 1)
    for b in range(S.B):
        check_block(o, name, P, S, b, got, unique=True if resample else "index")
    sub = msp.map_paths(o, name, P, S, 2, 3)                                   # the range selects what is written, not what is maximised
    assert np.array_equal(sub[0], got[0][:, 1:3]) and np.array_equal(sub[1], got[1][:, 1:3]) and np.array_equal(sub[2], got[2])


@pytest.mark.parametrize("bs,T", [(3, 4), (4, 5)])
def test_line_model_where_exact_ties_are_the_rule(g, o, bs, T):
    m, S, P, _ = cpu_loop(g, o, "line_model", 3 * bs, bs, T)
    got = msp.map_paths(o, "line_model", P, S)
    ties = sum(not check_block(o, "line_model", P, S, b, got, unique=False) for b in range(S.B))
    assert ties > 0
    for b in range(S.B):                                                      # one slope along the whole path
        assert np.all(got[0][b, :, 0] == got[0][b, 0, 0])


def test_the_nested_filter(g, o):
    bs, T = 3, 4
    m, S, P, (_, fired) = cpu_loop(g, o, "lgssm2", 6 * bs, bs, T, ess_frac=0.8, across=True)
    assert fired > 0
    got = msp.map_paths(o, "lgssm2", P, S)
    blocks = (got[1] - 1) // bs
    assert np.array_equal(blocks[:, -1], np.arange(S.B)) and np.any(blocks != blocks[:, -1:])             # (some lineage changed its block)
    for b in range(S.B):
        check_block(o, "lgssm2", P, S, b, got, unique=True)


def test_per_block_parameters(g, o):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    bs, T = 4, 4
    assign = np.arange(3) % 3
    m, S, P, _ = cpu_loop(g, o, "object_motion", 3 * bs, bs, T, sets=sets, assign=assign)
    got = msp.map_paths(o, "object_motion", P, S)
    for b in range(S.B):
        check_block(o, "object_motion", P, S, b, got, unique=True)
    other = msp.map_paths(o, "object_motion", sets[0].params, S)
    assert np.array_equal(other[2][0], got[2][0]) and not np.array_equal(other[2][1:], got[2][1:])      # (the rows matter)


def test_ess_gated_steps_with_identity_maps(g, o):
    bs, T = 4, 5
    m, S, P, (kept, _) = cpu_loop(g, o, "lgssm2", 5 * bs + 3, bs, T, ess_frac=0.5)
    assert kept > 0                                                          # (blocks that did not resample: the step's map is the identity there)
    got = msp.map_paths(o, "lgssm2", P, S)
    for b in range(S.B):
        check_block(o, "lgssm2", P, S, b, got, unique=True)


def test_one_step_is_the_arg_max_of_prior_plus_likelihood(g, o):
    for name in ("lgssm2", "line_model"):
        m, S, P, _ = cpu_loop(g, o, name, 11, 4, 1)
        path, idx, logp = msp.map_paths(o, name, P, S)
        for b in range(S.B):
            x = S.x(1)[b * 4:min(b * 4 + 4, 11)]
            tot = msp.logprior(name, P, x, S.obs[0][b]) + msp.loglik(o, name, P, x, S.obs[0][b])    # (no transrest at step 1)
            assert logp[b] == tot.max() and idx[b, 0] == b * 4 + int(np.argmax(tot)) + 1 and np.array_equal(path[b, 0], x[int(np.argmax(tot))])


def hand_store(x_steps, obs, resample=None):
    """one block of four line_model particles; resample: {step: 1-based parents}"""
    S = bsp.Store(4, 4, 2)
    for s, x in enumerate(x_steps, 1):
        S.begin_step(np.array([obs[s - 1]]))
        if resample and s in resample:
            S.resample_blocks(np.array(resample[s]), np.array([True]))
        S.end_step(np.array(x, np.float64), np.zeros(4))
    return S


def test_an_all_minus_inf_continuation(g, o):
    """line_model: a slope no child holds has best = -Inf (ptr 0) and can never be on the path; where NO candidate's slope goes on, every total is -Inf:
    logp = -Inf, NaN paths, indices 0"""
    m = g.models.line_model()
    obs = [g.models.line_obs(1, 1.0), g.models.line_obs(2, 1.0)]
    x1 = [[1.0, 0.0], [2.0, 0.0], [1.0, 1.0], [-1.0, 0.0]]
    S = hand_store([x1, [[1.0, 0.0], [1.0, 1.0], [7.0, 0.0], [1.0, 0.0]]], obs)
    G = msp.grid(o, "line_model", m.params, S, {2: S.step_map(2)}, 0)
    tot, ptrs = msp.recursion(G)
    assert np.all(np.isneginf(tot[[1, 3]])) and np.all(np.isfinite(tot[[0, 2]])) and np.all(ptrs[0][[1, 3]] == 0)
    got = msp.map_paths(o, "line_model", m.params, S)
    check_block(o, "line_model", m.params, S, 0, got, unique=False)
    assert np.all(got[0][0, :, 0] == 1.0) and np.isfinite(got[2][0])
    dead = hand_store([x1, [[7.0, 0.0], [7.0, 1.0], [5.0, 0.0], [0.0, 0.0]]], obs)
    path, idx, logp = msp.map_paths(o, "line_model", m.params, dead)
    assert np.isneginf(logp[0]) and np.all(np.isnan(path)) and np.all(idx == 0)
    assert np.isneginf(msp.maximum(msp.brute_force(o, "line_model", m.params, dead, 0))[0])


def test_an_undefined_lineage_reads_nan_everywhere(g, o):
    """two blocks of two; step 2 ends with a resample that takes block 0's particles from both blocks: block 0 has no lineage (NaN, 0, NaN at EVERY
    step -- step 2 too, which the smoothers would still answer), block 1 is unaffected"""
    m = g.models.lgssm2()
    S = bsp.Store(4, 2, 2)
    rng = np.random.default_rng(1)
    S.begin_step(rng.standard_normal((2, 2))); S.end_step(rng.standard_normal((4, 2)), np.zeros(4))
    S.begin_step(rng.standard_normal((2, 2))); S.resample_global(np.array([1, 3, 4, 3])); S.end_step(rng.standard_normal((4, 2)), np.zeros(4))
    assert msp.lineage(S, {2: S.step_map(2)}, 0) is None and msp.lineage(S, {2: S.step_map(2)}, 1) == [1, 1]
    path, idx, logp = msp.map_paths(o, "lgssm2", m.params, S)
    assert np.all(np.isnan(path[0])) and np.all(idx[0] == 0) and np.isnan(logp[0]) and msp.brute_force(o, "lgssm2", m.params, S, 0) is None
    check_block(o, "lgssm2", m.params, S, 1, (path, idx, logp), unique=True)


# ----------------------------------------------------------------------------- the negative controls
def test_every_control_switch_changes_logp_or_the_path(g, o):
    """the five mistakes of tests/block_map_spec.py, each on a listed case: what the tests above pin is not indifferent to them"""
    lg = cpu_loop(g, o, "lgssm2", 11, 4, 4)
    om = cpu_loop(g, o, "object_motion", 11, 4, 4)
    lm = cpu_loop(g, o, "line_model", 12, 4, 5)
    changed = {}
    for key, (name, (m, S, P, _)) in (("node", ("lgssm2", lg)), ("obs_next", ("object_motion", om)), ("rest", ("line_model", lm)),
                                      ("first_tie", ("line_model", lm)), ("ptr_trace", ("lgssm2", lg))):
        right, wrong = msp.map_paths(o, name, P, S), msp.map_paths(o, name, P, S, **{key: False})
        changed[key] = (not np.array_equal(right[2], wrong[2]), not np.array_equal(right[1], wrong[1]))
        if key in ("node", "obs_next", "rest"):                                # the totals change: brute force under the switch has another maximum
            assert any(msp.maximum(msp.brute_force(o, name, P, S, b, **{key: False}))[0] != right[2][b] for b in range(S.B)), key
        else:                                                                  # the totals stand: logp is the same, the path is another
            assert changed[key] == (False, True), (key, changed[key])
            if key == "ptr_trace":                                             # ... and no longer attains logp
                tot = [msp.brute_force(o, name, P, S, b) for b in range(S.B)]
                assert any(tot[b][msp.local_path(S, wrong[1][b])] != right[2][b] for b in range(S.B))
    print("controls (logp changed, path changed):", changed)
    assert all(a or b for a, b in changed.values()), changed
