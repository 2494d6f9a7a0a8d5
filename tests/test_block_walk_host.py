"""The random walks over the block-wise calls (tests/block_walk_spec.py), the parts that need no GPU:

  1. the rehearsal: every committed seed's plan runs through the model alone -- the device's answers are replaced by the model's own, and the Store is
     fed from the model.  The composition of the spec pieces is coherent: the Store's genealogy gives the trace the model's rows and parents give, the
     ancestral and backward restatements return indices inside their blocks, and the run reaches its last op;
  2. coverage: conditions on the GENERATOR over the committed seeds, those that depend on the data ("fired", both kinds of block at the ESS gate)
     verified in the model runs.  The table is printed;
  3. the smallest law check: a two-step sv1 store of four particles whose second step holds a conditional resample -- the backward draws follow the
     closed form, so the Store reads a conditional step's parents correctly (tests/test_block_backward_host.py has the store without a resample)."""
import numpy as np
import pytest

import block_backward_spec as bsp
import block_conditional_spec as cs
import block_walk_spec as ws
from block_ancestor_spec import logtrans
from block_history_spec import Genealogy

MIN_PER_KIND, MIN_PER_SITUATION = 8, 2


@pytest.fixture(scope="module")
def runs(g, o):
    """(setup, ops, the finished model-only walk) of every committed seed"""
    out = []
    for seed in ws.SEEDS:
        setup, ops = ws.plan(seed)
        out.append((setup, ops, ws.Walk(g, o, setup, ops, device=False).run()))
    return out


# ----------------------------------------------------------------------------- 1. the rehearsal
def test_plans_are_deterministic():
    for seed in ws.SEEDS[:4]:
        assert repr(ws.plan(seed)) == repr(ws.plan(seed))
    assert repr(ws.plan(ws.SEEDS[0])) != repr(ws.plan(ws.SEEDS[1]))


def test_every_run_reaches_its_last_op(runs):
    for setup, ops, w in runs:
        assert len(w.log) == len(ops) >= ws.N_OPS, setup
        assert setup["n"] <= 4 * 2048


def test_the_store_and_the_model_tell_one_genealogy(g, o):
    """the walk again, with a second Genealogy kept from the model's rows and parents alone (as ConditionalLoop keeps its own): after every op the
    Store's trace of every step equals it"""
    for seed in ws.SEEDS:
        setup, ops = ws.plan(seed)
        if setup["store"] == "none":
            continue
        w = ws.Walk(g, o, setup, ops, device=False)
        gen = Genealogy(setup["n"])
        d = w.d

        changed = w.changed                                                  # (the walker's own hook: called after every accepted state-changing op)

        def hook():
            changed()
            op = w.ops[w.i] if w.i >= 0 else dict(op="initialize")
            M = w.model
            if op["op"] in ("initialize", "update"):
                gen.begin_step(M.rows[:, :d])
            elif op["op"] == "resample":
                gen.resample("blocks", np.array(M.parents), M.mask.copy(), setup["bs"])
            elif op["op"] == "across":
                gen.resample("global", np.array(M.parents))
            gen.set_rows(M.rows[:, :d])
            w.end_step()
            assert gen.steps == w.S.steps
            for t in range(1, gen.steps + 1):
                for c in range(d):
                    assert np.array_equal(w.S.gen.trace(t, c), gen.trace(t, c), equal_nan=True), (seed, w.i, op, t, c)

        w.changed = hook
        w.run()


def test_draws_stay_inside_their_blocks(runs):
    """Walk.get_sample / get_backward assert it for every draw (Walk._range_ok); here: every run with a store made such draws"""
    for setup, ops, w in runs:
        if setup["store"] == "none":
            continue
        drew = [e for e in w.log if e["kind"] in ("get_sample", "get_backward") and e["out"].startswith("ok")]
        assert len(drew) >= 1, setup


# ----------------------------------------------------------------------------- 2. coverage
def test_coverage_of_the_committed_seeds(runs):
    kinds, refusals, situations = {}, {}, dict.fromkeys(ws.SITUATIONS, 0)
    for setup, ops, w in runs:
        for e in w.log:
            kinds[e["kind"]] = kinds.get(e["kind"], 0) + 1
            if e["out"].startswith("refused"):
                refusals[e["out"]] = refusals.get(e["out"], 0) + 1
        for k, v in ws.situations(setup, w.log).items():
            situations[k] += v
    setups = [s for s, _, _ in runs]
    axes = {"block sizes": sorted({s["bs"] for s in setups}), "profiles": sorted({s["profile"] for s in setups}),
            "keep_prev": sorted({s["keep_prev"] for s in setups}), "models": sorted({s["model"] for s in setups}),
            "stores": sorted({s["store"] for s in setups}), "burst seeds": [s["seed"] for s in setups if s["mode"] == "burst"],
            "short store": [s["seed"] for s, ops, _ in runs if s["cap"] == sum(op["op"] == "update" for op in ops)]}
    print("\nblock walk coverage over seeds", ws.SEEDS)
    for k in sorted(kinds):
        print(f"  op {k:22s} {kinds[k]:4d}")
    for k in sorted(refusals):
        print(f"  {k:25s} {refusals[k]:4d}")
    for k, v in axes.items():
        print(f"  {k:25s} {v}")
    for k in ws.SITUATIONS:
        print(f"  {situations[k]:4d}  {k}")
    all_kinds = ["update", "update_ref", "resample_plain", "resample_cond", "resample_anc", "across", "rejuvenate", "poke", "refused"] + ["get_" + x for x in ws.GETTERS]
    for k in all_kinds:
        assert kinds.get(k, 0) >= MIN_PER_KIND, (k, kinds.get(k, 0))
    for what in ws.REFUSALS:
        assert refusals.get("refused " + what, 0) >= 2, what
    for what, least in (("refused store_full", 1), ("refused congruent", 2), ("refused mask", 2), ("refused no_store", 2)):
        assert refusals.get(what, 0) >= least, what
    assert axes["block sizes"] == ws.SIZES and axes["profiles"] == ["A", "B"] and axes["keep_prev"] == [False, True] and len(axes["models"]) >= 4
    assert axes["stores"] == ["full", "none", "plain"] and len(axes["short store"]) == 1
    assert 3 * len(axes["burst seeds"]) >= len(ws.SEEDS)
    for k in ws.SITUATIONS:
        assert situations[k] >= MIN_PER_SITUATION, (k, situations[k])
    for setup, ops, w in runs:                                               # every burst run has a staging burst of five or more
        if setup["mode"] == "burst":
            assert ws.situations(setup, w.log)["staging burst of five or more"] >= 1, setup
            assert all(len(run) >= 5 for run in ws.bursts(w.log)[:-1]), setup
    fired = sum(e["out"] == "ok fired" for _, _, w in runs for e in w.log)
    held = sum(e["out"] == "ok held" for _, _, w in runs for e in w.log)
    print(f"  across-block calls: {fired} fired, {held} held")
    assert fired >= 2 and held >= 1


def test_a_nan_is_the_last_state_change_only(runs):
    some = 0
    for setup, ops, w in runs:
        nan = [i for i, op in enumerate(ops) if op["op"] == "poke" and op["what"] == "nan"]
        some += len(nan)
        for i in nan:
            assert all(op["op"] == "get" and op["what"] in ("sample", "backward") for op in ops[i + 1:]), setup
    assert some >= 2


# ----------------------------------------------------------------------------- 3. the smallest law check
def test_draw_frequencies_after_a_conditional_resample_match_the_exact_kernel(g, o):
    """one block of four sv1 particles, two steps, unequal weights at step 1; step 2 is updated and then resampled by the conditional step
    (block_conditional_spec.conditional_resample on an oracle filter that holds the hand-built rows and weights): slot 0 keeps itself, the weights become
    equal.  P(i2, i1) = (1 / 4) w1[i1] f(x2[i2] | x1[i1]) / sum_k w1[k] f(x2[i2] | x1[k]) over the FINAL order of step 2.  2^16 draws of the restatement
    against these sixteen probabilities: Pearson's chi-square has 15 degrees of freedom, mean 15 and standard deviation sqrt(30); the bound is 5 of these
    units above the mean, as in tests/test_block_backward_host.py."""
    m = g.models.by_name("sv1")
    x1, x2 = np.array([[-0.6], [-0.1], [0.3], [0.9]]), np.array([[-0.4], [0.0], [0.2], [0.7]])
    lw1, lw2 = np.log([0.1, 0.2, 0.3, 0.4]), np.log([0.4, 0.3, 0.2, 0.1])
    f = o.OracleFilter(m.model_id, m.params, 4, 11)
    f.rows[:, :1] = x2
    f.lw[:] = lw2
    f.epoch = 2
    mask = cs.conditional_resample(o, f, 4)
    assert mask.all() and f.parents[0] == 1 and f.rows[0, 0] == x2[0, 0] and len(set(f.parents.tolist())) > 1
    S = bsp.Store(4, 4, 1)
    S.begin_step(np.zeros((1, 1))); S.end_step(x1, lw1)
    S.begin_step(np.zeros((1, 1))); S.resample_blocks(f.parents.copy(), mask); S.end_step(f.rows[:, :1], f.lw)
    assert np.array_equal(S.step_map(2), f.parents - 1) and np.array_equal(S.x(2)[:, 0], x2[f.parents - 1, 0])
    ns = 1 << 16
    traj, idx = bsp.backward(o, "sv1", m.params, S, seed=11, epoch=f.epoch, n_samples=ns)
    dens = np.exp(np.stack([logtrans("sv1", m.params, x1, S.x(2)[i], np.zeros(1)) for i in range(4)]))     # [i2, i1]
    back = np.exp(lw1)[None, :] * dens
    prob = 0.25 * back / back.sum(axis=1, keepdims=True)
    assert abs(prob.sum() - 1.0) < 1e-12
    got = np.zeros((4, 4))
    np.add.at(got, (idx[0, :, 1] - 1, idx[0, :, 0] - 1), 1)
    chi2 = float(((got - ns * prob) ** 2 / (ns * prob)).sum())
    print("chi-square of 2^16 draws over 16 cells, after a conditional resample:", round(chi2, 2))
    assert chi2 <= 15 + 5 * np.sqrt(30), chi2
    assert np.array_equal(traj[0, :, 0, 0], x1[idx[0, :, 0] - 1, 0]) and np.array_equal(traj[0, :, 1, 0], S.x(2)[idx[0, :, 1] - 1, 0])
    # the recorded parent is what a draw falls back to: with logtrans = -Inf everywhere the walk is the ancestral one
    S2 = bsp.Store(4, 4, 2)
    lm = g.models.line_model()
    S2.begin_step(np.zeros((1, 2))); S2.end_step(np.array([[1.0, 0.0]] * 4), np.zeros(4))
    S2.begin_step(np.zeros((1, 2))); S2.resample_blocks(f.parents.copy(), mask); S2.end_step(np.array([[7.0, 0.0]] * 4), np.zeros(4))
    _, idx2 = bsp.backward(o, "line_model", lm.params, S2, seed=11, epoch=0, n_samples=64)
    assert np.array_equal(idx2[0, :, 0], f.parents[idx2[0, :, 1] - 1])
