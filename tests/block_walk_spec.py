"""Random walks over the block-wise calls, in lockstep with the restatements the per-feature tests already use.

  plan(seed)   -> (setup, ops): deterministic, no GPU, no oracle.  The setup fixes model, keep_prev, block size (the edges of the three team shapes), n
                  (3 bs + 5: a short last block, or 4 bs: congruent blocks), the profile, the store ("full": history + history_weights, "plain": history
                  only, "none") with its capacity, and the mode.  About 30 ops.  Everything that depends on the number of recorded steps (step ranges, a
                  past step) is kept as a fraction in [0, 1) and resolved against the step count of the moment.
  Walk         runs a plan on a model of the state machine and, with device=True, on the device in lockstep.
                 profile A  one parameter vector: an OracleFilter stepped by oracle.initialize_blocks / update_blocks / resample_blocks / rejuvenate_blocks,
                            block_conditional_spec.pinned_* / conditional_resample, block_ancestor_spec.ancestor_resample and
                            across_blocks_spec.resample_across_blocks;
                 profile B  three parameter sets of object_motion, block b starts with set b % 3: block_params_spec.ParamBlocksOracle with
                            across_blocks_spec.resample_across_param_blocks.  Plain updates, plain resamples, rejuvenation, resampling across blocks and
                            every getter; NO conditional or ancestor resamples and no pinned updates: their restatement with parameters is
                            ConditionalLoop's one-filter-per-set composition, which cannot move a block from one filter to another, so those pairs stay
                            with tests/test_gpu_block_conditional.py and tests/test_gpu_block_ancestor.py.
               A block_backward_spec.Store is fed only with what the device returns (state.parents, block_resampled, the block ancestors, history_column
               of the current step and state.log_weights at the end of every step) and answers the store getters; the model's rows are the second,
               independent check.
               mode "checked": rows, log-weights, parents, block_resampled, block_stats and every history column are compared after every op.
               mode "burst":   state-changing ops come in runs of 5 to 8 with NO read-back between them -- block resamples go through the C entry points
                               with NULL outputs, which do not wait for the stream -- and everything is compared at the flush before the next getter; the
                               Store's inputs of those steps come from the model, which the flush then shows equal to the device.
  device_only  the same plan on the device alone, read back after every op or not at all (tests/test_gpu_block_walk.py test_burst_equals_checked).
  situations   how often the ordered situations the walk is for occur in one run, from the log of its model-only run (tests/test_block_walk_host.py asserts
               them over the committed seeds).  The generator places each of them once per run where the setup allows it; the rest is chance.

What the model knows beyond the arrays: the mask of the last block resample is gone after an update or an across-block call that fired (gpf.h), so
`block_resampled` and `only_resampled` rejuvenation are refused then; a refused call changes nothing; rejuvenation uses the per-block observations of the
last update, permuted by every across-block call that fired since.

Helper module, no tests."""
import ctypes as C
import os

import numpy as np

import across_blocks_spec as xs
import block_ancestor_spec as asp
import block_backward_spec as bsp
import block_conditional_spec as cs
import block_params_spec as bp
from block_trajectories_spec import draw_indices, paths
from test_gpu_block_conditional import block_obs, eq, model_of, references, snapshot, unchanged

SIZES = [1, 2, 7, 128, 129, 512, 513, 2048]                                  # a wave 2 / 8 per lane, the workgroup, and their edges
N_SEEDS = int(os.environ.get("GPF_BLOCKWALK_SEEDS", "16"))                   # GPF_BLOCKWALK_SEEDS=300 for a longer hunt
OFFSET = int(os.environ.get("GPF_BLOCKWALK_OFFSET", "0"))                    # ... GPF_BLOCKWALK_OFFSET=100000 for other sequences
SEEDS = [OFFSET + k for k in range(N_SEEDS)]
METHODS = ["multinomial", "residual", "stratified"]
GETTERS = ["stats", "resampled", "ancestors", "moments", "moments_past", "columns", "anc_lw", "sample", "backward"]
STORE_GETTERS = {"moments_past": "plain", "columns": "plain", "sample": "plain", "backward": "full"}   # the least store each needs
REFUSALS = ["size", "steps", "cond_residual", "no_weights"]
N_OPS = 30


# ----------------------------------------------------------------------------- the generator
def plan(seed):
    seed = int(seed)
    rng = np.random.default_rng([seed, 0x77A1C])
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    bs = SIZES[seed % 8]
    profile = "B" if seed % 3 == 2 else "A"
    mode = "burst" if seed % 5 in (1, 3) else "checked"
    store = "none" if seed % 16 == 9 else "plain" if seed % 8 == 6 else "full"
    keep_prev = seed % 4 != 0
    if profile == "B":
        name, n, pinned = "object_motion", (6 if bs <= 129 else 4) * bs, False
    else:
        name = "line_model" if seed % 8 == 4 else pick(["lgssm2", "bearings4", "sv1", "object_motion"])   # (line_model: no keep_prev, no rejuvenation)
        n = 3 * bs + 5 if rng.random() < 0.5 else 4 * bs
        pinned = bool(rng.random() < 0.5)
    ops, dead = [], [False]                                                  # dead: some block may hold nothing but -Inf weights
    can_rej = keep_prev                                                      # (gpf_rejuvenate_blocks needs x_{t-1} in the row)

    def frac():
        return float(rng.random())

    def steps():
        r = rng.random()
        return ("all",) if r < 0.6 else ("last",) if r < 0.7 else ("range", frac(), frac())

    def resample():
        ess = pick([None, 0.5, 0.8])
        r = rng.random()
        if profile == "B":
            return dict(op="resample", kind="plain", method=pick(METHODS), ess_frac=ess, sort=True, alpha=None)
        if r < 0.45:                                                         # (a tempered resample of an all -Inf block would leave NaN weights: -Inf - -Inf)
            alpha = pick([None, 0.5, 2.0])
            return dict(op="resample", kind="plain", method=pick(METHODS), ess_frac=ess, sort=bool(rng.random() < 0.5), alpha=None if dead[0] else alpha)
        return dict(op="resample", kind="cond" if r < 0.70 else "anc", ess_frac=ess)

    def update():
        return dict(op="update", ref=bool(profile == "A" and rng.random() < 0.5))

    def rejuvenate(only=None):
        return dict(op="rejuvenate", method=pick(["move", "reweight"]), n_iters=int(rng.integers(1, 3)), only=bool(rng.random() < 0.5) if only is None else only)

    def across():
        return dict(op="across", method=pick(METHODS), ess_frac=pick([None, None, 0.8] if profile == "B" else [None, 0.5, 0.9]), sort=bool(rng.random() < 0.5))

    def refused():
        if store != "full" and rng.random() < 0.7:                           # (a backward draw on a store without the weights mode)
            return dict(op="refused", what="no_weights")
        return dict(op="refused", what=pick(REFUSALS[:3]))

    def poke():
        what = "block" if rng.random() < 0.4 else "particle"
        dead[0] = dead[0] or what == "block" or bs <= 2
        return dict(op="poke", what=what, u=frac(), v=frac())

    def state_op(prev, prev2, staging):
        if staging:
            r = rng.random()
            if r < 0.8:
                return update()
            if profile == "A" and r < 0.9:
                return dict(op="resample", kind="anc", ess_frac=pick([None, 0.8]))
            return rejuvenate() if can_rej else resample()
        was = prev["op"] if prev else None
        if can_rej and was == "resample" and prev["kind"] != "plain" and rng.random() < 0.55:
            prev["ess_frac"] = pick([0.5, 0.8])                              # (gated: where some block stays, the mask matters to the rejuvenation)
            return rejuvenate(True)
        if can_rej and was == "across" and rng.random() < 0.6:
            return rejuvenate(True)
        if can_rej and was == "refused" and prev2 and prev2["op"] == "resample" and rng.random() < 0.8:
            return rejuvenate(True)
        if can_rej and was == "resample" and rng.random() < 0.35:
            return rejuvenate(None if rng.random() < 0.3 else True)
        if was == "resample" and rng.random() < 0.25:
            return refused()
        r = rng.random()
        for p, make in ((0.32, update), (0.30, resample), (0.20 if profile == "B" else 0.10, across), (0.08 if can_rej else 0.0, rejuvenate),
                        (0.08, poke), (1.0, refused)):
            if r < p:
                return make()
            r -= p

    def getter():
        w = np.array([2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 3.0, 4.0])
        what = GETTERS[int(rng.choice(len(GETTERS), p=w / w.sum()))]
        op = dict(op="get", what=what)
        if what == "moments_past":
            op["u"] = frac()
        if what in ("sample", "backward"):
            op.update(k=pick([1, 3]), steps=steps())
        return op

    def state_run(length, staging=False, lead=()):
        for k in range(length):
            prev, prev2 = (ops[-1] if ops else None), (ops[-2] if len(ops) > 1 else None)
            ops.append(lead[k] if k < len(lead) else state_op(prev, prev2, staging))

    if mode == "burst":                                                      # the staging burst: five or more updates / ancestor resamples back to back
        state_run(int(rng.integers(7, 9)), staging=True)
        for _ in range(int(rng.integers(1, 3))):
            ops.append(getter())
    # situations the walk must meet, each once per run where the setup allows it, at the head of a run of state-changing ops chosen at random
    motifs = []
    if can_rej and n % bs == 0:                                              # a block resample, an across-block call whose gate cannot fire (ESS < 0), then
        motifs.append(lambda: (update(), dict(resample(), ess_frac=pick([0.5, 0.8])), dict(across(), ess_frac=0.0), rejuvenate(True)))   # the mask is still there
    if n % bs != 0:                                                          # a short last block: the across-block call is refused, the mask stays
        motifs.append(lambda: (update(), dict(resample(), ess_frac=pick([0.5, 0.8])), across()) + ((rejuvenate(True),) if can_rej else ()))
    if can_rej and profile == "A":
        motifs.append(lambda: (update(), dict(op="resample", kind="cond", ess_frac=pick([0.5, 0.8])), rejuvenate(True)))
    if profile == "A":
        motifs.append(lambda: (dict(op="resample", kind="plain", method=pick(METHODS[1:]), ess_frac=pick([None, 0.8]), sort=False, alpha=None),))
        motifs.append(lambda: (dict(op="resample", kind="plain", method=pick(METHODS), ess_frac=None, sort=True, alpha=None if dead[0] else pick([0.5, 2.0])),))
    if store != "full":
        motifs.append(lambda: (dict(op="refused", what="no_weights"),))
    while len(ops) < N_OPS:
        lead = ()
        if ops and ops[-1]["op"] == "get" and ops[-1]["what"] in ("sample", "backward") and rng.random() < 0.8:
            lead = (update(), resample())                                    # (further filtering after a draw that cost epochs)
        elif motifs and rng.random() < 0.75:
            lead = motifs.pop(int(rng.integers(len(motifs))))()
        state_run(max(len(lead), int(rng.integers(5, 9) if mode == "burst" else rng.integers(1, 5))), lead=lead)
        for _ in range(int(rng.integers(1, 4))):
            ops.append(getter())
    if rng.random() < 0.5:                                                   # one NaN, as the last state-changing op only
        ops.append(dict(op="poke", what="nan", u=frac(), v=frac()))
    ops.append(dict(op="get", what="sample", k=3, steps=("all",)))
    ops.append(dict(op="get", what="backward", k=3, steps=("all",)))
    n_updates = sum(op["op"] == "update" for op in ops)
    short = seed % 16 == 5 and store != "none"                               # one seed: the last update finds the store full
    setup = dict(seed=seed, model=name, keep_prev=keep_prev, bs=bs, n=n, profile=profile, store=store, cap=n_updates + (0 if short else 1),
                 mode=mode, pinned=pinned, filter_seed=17 + seed, n_data=n_updates + 2)
    return setup, ops


def kind_of(op):
    if op["op"] == "resample":
        return "resample_" + op["kind"]
    if op["op"] == "get":
        return "get_" + op["what"]
    if op["op"] == "update":
        return "update_ref" if op["ref"] else "update"
    return op["op"]


# ----------------------------------------------------------------------------- data and parameter sets
def model_for(g, setup):
    return g.models.line_model() if setup["model"] == "line_model" else model_of(g, setup["model"])


def param_sets(g):
    return [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]


class Data:
    """ys [B, n_data, n_obs] and refs [B, n_data, d]: every block its own data and reference values, fixed by the plan's seed"""

    def __init__(self, g, setup):
        m, B, steps = model_for(g, setup), n_blocks(setup), setup["n_data"]
        if setup["model"] == "line_model":                                   # (data vector (y_t, x_t = t); a slope of the support and an outlier flag)
            slope = np.random.default_rng(setup["seed"]).integers(-2, 3, B)
            self.ys = np.stack([[g.models.line_obs(t + 1, float(s)) for t in range(steps)] for s in slope])
            bt = np.arange(B)[:, None] + np.arange(steps)[None, :]
            self.refs = np.stack([bt % 5 - 2.0, bt % 2 * 1.0], axis=2)
        else:
            self.ys = block_obs(g, m, B, steps, seed=7 + setup["seed"])
            self.refs = references(g, m, B, steps, seed=5 + setup["seed"])


def n_blocks(setup):
    return (setup["n"] + setup["bs"] - 1) // setup["bs"]


# ----------------------------------------------------------------------------- the model of the state machine
class Refused(Exception):
    pass


class ModelA:
    """one parameter vector: an OracleFilter and the spec functions that step it"""

    def __init__(self, g, o, setup):
        self.o, self.m, self.bs, self.n = o, model_for(g, setup), setup["bs"], setup["n"]
        self.keep_prev = setup["keep_prev"]
        self.f = o.OracleFilter(self.m.model_id, self.m.params, self.n, setup["filter_seed"], keep_prev=self.keep_prev)
        self.obs = self.mask = self.A = None

    rows = property(lambda self: self.f.rows)
    lw = property(lambda self: self.f.lw)
    parents = property(lambda self: self.f.parents)
    epoch = property(lambda self: self.f.epoch)
    P = property(lambda self: self.m.params)

    def bump(self, k):
        self.f.epoch += int(k)

    def blocks(self):
        return [(a, min(a + self.bs, self.n)) for a in range(0, self.n, self.bs)]

    def initialize(self, obs, ref):
        cs.pinned_initialize(self.o, self.f, self.bs, obs, ref) if ref is not None else self.o.initialize_blocks(self.f, self.bs, obs)
        self.obs, self.mask = np.array(obs), None

    def update(self, obs, ref):
        cs.pinned_update(self.o, self.f, self.bs, obs, ref) if ref is not None else self.o.update_blocks(self.f, self.bs, obs)
        self.obs, self.mask = np.array(obs), None

    def resample(self, op, obs_next, ref_next):
        if op["kind"] == "plain":
            mask = self.o.resample_blocks(self.f, self.bs, op["method"], ess_frac=op["ess_frac"], sort_particles=op["sort"], check=False, priority_alpha=op["alpha"])
        elif op["kind"] == "cond":
            mask = cs.conditional_resample(self.o, self.f, self.bs, op["ess_frac"])
        else:
            mask, _ = asp.ancestor_resample(self.o, self.f, self.bs, obs_next, ref_next, op["ess_frac"])
        self.mask = np.asarray(mask, bool)
        return self.mask

    def across(self, op):
        if self.n % self.bs != 0:
            raise Refused("blocks must be congruent")
        plan = xs.resample_across_blocks(self.o, self.f, self.bs, op["method"], ess_frac=op["ess_frac"], sort_particles=op["sort"], check=False)
        return self._moved(plan)

    def _moved(self, plan):
        if plan.resampled:
            self.obs, self.mask, self.A = self.obs[plan.A], None, plan.A + 1
        return plan.A + 1 if plan.resampled else None

    def rejuvenate(self, op):
        if not self.keep_prev or (op["only"] and self.mask is None):
            raise Refused("rejuvenate")
        self.o.rejuvenate_blocks(self.f, self.bs, self.obs, op["method"], mask=self.mask if op["only"] else None, n_iters=op["n_iters"])

    def poke(self, idx, value):
        self.f.lw[idx] = value

    def stats(self):
        v = [self.f[a:b] for a, b in self.o.blocks_of(self.f, self.bs)]
        return np.array([x.effective_sample_size() for x in v]), np.array([x.log_ml_estimate() for x in v])


class ModelB(ModelA):
    """per-block parameters: block_params_spec.ParamBlocksOracle"""

    def __init__(self, g, o, setup):
        self.o, self.m, self.bs, self.n = o, model_for(g, setup), setup["bs"], setup["n"]
        self.keep_prev = setup["keep_prev"]
        self.sets = [s.params for s in param_sets(g)]
        B = n_blocks(setup)
        self.ref = bp.ParamBlocksOracle(o, self.m.model_id, self.sets, np.arange(B) % 3, self.n, self.bs, setup["filter_seed"], keep_prev=self.keep_prev)
        self.obs = self.mask = self.A = None

    rows = property(lambda self: self.ref.rows)
    lw = property(lambda self: self.ref.lw)
    parents = property(lambda self: self.ref.parents)
    epoch = property(lambda self: self.ref.f[0].epoch)
    P = property(lambda self: np.stack([self.sets[k] for k in self.ref.assign]))

    def bump(self, k):
        for f in self.ref.f:
            f.epoch += int(k)

    def initialize(self, obs, ref):
        assert ref is None
        self.ref.initialize(obs)
        self.obs, self.mask = np.array(obs), None

    def update(self, obs, ref):
        assert ref is None
        self.ref.update(obs)
        self.obs, self.mask = np.array(obs), None

    def resample(self, op, obs_next, ref_next):
        assert op["kind"] == "plain" and op["alpha"] is None and op["sort"]
        self.mask = np.asarray(self.ref.resample(op["method"], op["ess_frac"]), bool)
        return self.mask

    def across(self, op):
        return self._moved(xs.resample_across_param_blocks(self.ref, op["method"], ess_frac=op["ess_frac"], sort_particles=op["sort"], check=False))

    def rejuvenate(self, op):
        if not self.keep_prev or (op["only"] and self.mask is None):
            raise Refused("rejuvenate")
        self.ref.rejuvenate(self.obs, op["method"], mask=self.mask if op["only"] else None, n_iters=op["n_iters"])

    def poke(self, idx, value):
        for f in self.ref.f:                                                 # (every filter holds the block; only its owner's copy is read)
            f.lw[idx] = value

    def stats(self):
        return self.ref.block_ess(), self.ref.block_lml()


# ----------------------------------------------------------------------------- the device side of one op
class Device:
    """the calls of one op on a device state.  raw=True: block resamples through the C entry points with NULL outputs (no wait for the stream)"""

    def __init__(self, g, setup, data, raw):
        self.g, self.bs, self.raw, self.B = g, setup["bs"], raw, n_blocks(setup)
        m = model_for(g, setup)
        sets = param_sets(g)
        self.st = g.pf_initialize_blocks(m, (1,), data.ys[:, 0], setup["n"], self.bs, seed=setup["filter_seed"], keep_prev=setup["keep_prev"],
                                         history=setup["cap"] if setup["store"] != "none" else 0, history_weights=setup["store"] == "full",
                                         params=[sets[b % 3] for b in range(self.B)] if setup["profile"] == "B" else None,
                                         reference=data.refs[:, 0] if setup["pinned"] else None)

    def update(self, obs, ref):
        self.g.pf_update_blocks(self.st, (), (), obs, self.bs, reference=ref)

    def resample(self, op, obs_next, ref_next):
        """the number of blocks that resampled, or None (raw)"""
        g, st = self.g, self.st
        ess = float("nan") if op["ess_frac"] is None else float(op["ess_frac"])
        if not self.raw:
            if op["kind"] == "plain":
                return g.pf_resample_blocks(st, self.bs, op["method"], ess_frac=op["ess_frac"], sort_particles=op["sort"], check=False,
                                            priority_fn=None if op["alpha"] is None else g.Tempering(op["alpha"]))
            kw = dict(reference=ref_next, observations=obs_next) if op["kind"] == "anc" else {}
            return g.pf_resample_blocks(st, self.bs, "multinomial", ess_frac=op["ess_frac"], check=False, conditional=True, **kw)
        if op["kind"] == "plain":
            code = st._L.gpf_resample_blocks(st._h, g.api.RESAMPLE_METHODS[op["method"]], self.bs, float("nan") if op["alpha"] is None else float(op["alpha"]),
                                             int(op["sort"]), ess, 0, None, None)
        elif op["kind"] == "cond":
            code = st._L.gpf_resample_blocks_conditional(st._h, 0, self.bs, ess, 0, None, None)
        else:
            ob, rf = np.ascontiguousarray(obs_next, np.float64), np.ascontiguousarray(ref_next, np.float64)
            code = st._L.gpf_resample_blocks_ancestor(st._h, 0, self.bs, ess, 0, g.api._pd(ob), ob.shape[1], g.api._pd(rf), rf.shape[1], None, None)
        st._check(code)
        st._n_blocks_last = self.B                                           # (what pf_resample_blocks notes for block_resampled)
        return None

    def across(self, op, bs=None):
        return self.g.pf_resample_across_blocks(self.st, self.bs if bs is None else bs, op["method"], ess_frac=op["ess_frac"], sort_particles=op["sort"], check=False)

    def rejuvenate(self, op):
        self.g.pf_rejuvenate_blocks(self.st, None, (), op["n_iters"], method=op["method"], only_resampled=op["only"])

    def refused_call(self, what, T):
        """(the call of a documented refusal, the exception it raises, the C call behind the package's own check or None)"""
        g, st, bs = self.g, self.st, self.bs
        if what == "size":                                                   # bs + 1: no whole number of blocks, not the observations' size, not the parameters'
            return (lambda: g.pf_resample_across_blocks(st, bs + 1, check=False)), g.ErrorException, None
        if what == "steps":
            return (lambda: g.block_sample_trajectories(st, bs, 1, steps=(1, T + 1))), g.ErrorException, None
        if what == "cond_residual":
            return ((lambda: g.pf_resample_blocks(st, bs, "residual", check=False, conditional=True)), ValueError,
                    lambda: st._L.gpf_resample_blocks_conditional(st._h, 1, bs, float("nan"), 0, None, None))
        buf = np.empty(self.B * st.dim)
        return ((lambda: g.block_backward_trajectories(st, bs)), g.ErrorException,
                lambda: st._L.gpf_block_backward_sample(st._h, bs, 1, 1, 1, g.api._pd(buf), None))

    def close(self):
        self.st.close()


def resolve_steps(spec, T):
    if spec[0] == "all":
        return 1, T
    if spec[0] == "last":
        return T, T
    a, b = sorted((1 + int(spec[1] * T), 1 + int(spec[2] * T)))
    return a, b


def poke_index(op, setup):
    bs, n = setup["bs"], setup["n"]
    b = int(op["u"] * n_blocks(setup))
    lo, hi = b * bs, min((b + 1) * bs, n)
    return np.arange(lo, hi) if op["what"] == "block" else np.array([lo + int(op["v"] * (hi - lo))])


def trimmed(snap, n):
    """test_gpu_block_conditional.snapshot without the bytes that pad an odd number of 4-byte parents to the blob's 8-byte size, which no one writes"""
    blob = snap[0]
    return (blob[:len(blob) - (4 * n) % 8],) + tuple(snap[1:])


# ----------------------------------------------------------------------------- the walker
class Walk:
    def __init__(self, g, o, setup, ops, device=True):
        self.g, self.o, self.setup, self.ops = g, o, setup, ops
        self.bs, self.n, self.B = setup["bs"], setup["n"], n_blocks(setup)
        self.m = model_for(g, setup)
        self.d = self.m.dim
        self.data = Data(g, setup)
        self.model = (ModelB if setup["profile"] == "B" else ModelA)(g, o, setup)
        self.S = bsp.Store(self.n, self.bs, self.d) if setup["store"] != "none" else None
        self.checked = setup["mode"] == "checked"
        self.dev = Device(g, setup, self.data, raw=not self.checked) if device else None
        self.twin = None
        self.T, self.log, self.dirty, self.par_expect, self.i, self.nan_poked = 0, [], False, None, -1, False

    # -- plumbing
    def need(self, ok, *what):
        if not ok:
            lo = max(0, self.i - 7)
            raise AssertionError(f"block walk seed {self.setup['seed']}: {what} at op {self.i}\n  setup {self.setup}\n  last ops " +
                                 "".join(f"\n    {k}: {self.ops[k]} -> {self.log[k]['out'] if k < len(self.log) else '?'}" for k in range(lo, self.i + 1)))

    def close(self):
        if self.dev:
            self.dev.close()
        if self.twin is not None:
            self.twin.close()

    def has(self, level):
        return self.setup["store"] == "full" or (level == "plain" and self.setup["store"] == "plain")

    def end_step(self):
        """the current step's record in the Store: its latent columns and log-weights as they stand"""
        if self.S is None:
            return
        if self.dev and self.checked:
            st = self.dev.st
            self.S.end_step(np.stack([st.history_column(self.S.steps, c) for c in range(self.d)], axis=1), st.log_weights)
        else:
            self.S.end_step(self.model.rows[:, :self.d], self.model.lw)

    def flush(self):
        """the device equals the model: rows, log-weights, block_stats, the parents and mask of the last resample, every history column"""
        if not self.dirty:
            return
        self.dirty = False
        if not self.dev:
            self.end_step()
            return
        g, st, M = self.g, self.dev.st, self.model
        rows, lw = st.traces, st.log_weights
        self.need(eq(rows, M.rows), "rows", np.argwhere(~((rows == M.rows) | np.isnan(M.rows)))[:4].tolist())
        self.need(eq(lw, M.lw), "log_weights", np.flatnonzero(~((lw == M.lw) | np.isnan(M.lw)))[:4].tolist())
        self.check_stats()
        if M.mask is not None:
            self.need(np.array_equal(g.block_resampled(st), M.mask), "block_resampled")
        if self.par_expect is not None:
            sel = np.repeat(self.par_expect[1], self.bs)[:self.n] if self.par_expect[0] == "blocks" else np.ones(self.n, bool)
            self.need(np.array_equal(st.parents[sel], M.parents[sel]), "parents", self.par_expect[0])
        if self.setup["profile"] == "B":
            self.need(np.array_equal(g.get_block_params(st), M.P), "block parameters")
        self.end_step()
        self.check_columns()

    def check_stats(self):
        ess, lml = self.g.block_stats(self.dev.st, self.bs)
        ess_m, lml_m = self.model.stats()
        lw = self.model.lw
        ok = np.array([not np.isnan(lw[a:b]).any() for a, b in self.model.blocks()])
        self.need(eq(ess[ok], ess_m[ok]) and eq(lml[ok], lml_m[ok]), "block_stats", ess, ess_m, lml, lml_m)
        self.need(np.all(np.isnan(ess[~ok])), "block_stats of a NaN block")

    def check_columns(self):
        if self.S is None or not self.dev:
            return
        st = self.dev.st
        k = C.c_int32(-1)
        st._check(st._L.gpf_history_steps(st._h, C.byref(k)))
        self.need(k.value == self.S.steps, "history_steps", k.value, self.S.steps)
        for t in range(1, self.S.steps + 1):
            for c in range(self.d):
                self.need(np.array_equal(st.history_column(t, c), self.S.gen.trace(t, c), equal_nan=True), "history_column", t, c)

    def refused(self, call, exc, raw=None):
        """a refused call raises and changes nothing (checked mode: test_gpu_block_conditional.snapshot / unchanged around it)"""
        if not self.dev:
            return
        st = self.dev.st
        before = trimmed(snapshot(st, self.S is not None), self.n) if self.checked else None
        try:
            call()
        except exc:
            pass
        else:
            self.need(False, "the call was not refused")
        if raw is not None:
            self.need(raw() != 0, "the library did not refuse the call")
        if self.checked:
            self.need(unchanged(before, trimmed(snapshot(st, self.S is not None), self.n)), "a refused call changed the state")

    def changed(self):
        self.need(self.nan_poked or not np.isnan(self.model.lw).any(), "a NaN weight before the last poke")
        self.dirty = True
        if self.checked:
            self.flush()

    # -- the run
    def run(self):
        setup, data = self.setup, self.data
        ref = data.refs[:, 0] if setup["pinned"] else None
        self.model.initialize(data.ys[:, 0], ref)
        if self.S is not None:
            self.S.begin_step(data.ys[:, 0])
        self.T = 1
        self.changed()
        for i, op in enumerate(self.ops):
            self.i = i
            out = getattr(self, "op_" + op["op"])(op)
            self.log.append(dict(op=op, out=out, T=self.T, kind=kind_of(op)))
        self.flush()
        return self

    def op_update(self, op):
        t = self.T                                                           # (0-based index of the step being entered)
        obs, ref = self.data.ys[:, t], self.data.refs[:, t] if op["ref"] else None
        self.end_step()                                                      # the step that ends, in its final order
        if self.S is not None and self.S.steps >= self.setup["cap"]:
            self.refused(lambda: self.dev.update(obs, ref), self.g.ErrorException)
            return "refused store_full"
        self.model.update(obs, ref)
        if self.dev:
            self.dev.update(obs, ref)
        if self.S is not None:
            self.S.begin_step(obs)
        self.T += 1
        self.changed()
        return "ok"

    def op_resample(self, op):
        obs, ref = self.data.ys[:, self.T], self.data.refs[:, self.T]        # the step being entered: what the next update uses
        mask = self.model.resample(op, obs, ref).copy()
        if self.dev:
            k = self.dev.resample(op, obs, ref)
            self.need(k is None or k == mask.sum(), "the number of blocks that resampled", k, int(mask.sum()))
        if self.S is not None:
            if self.dev and self.checked:
                got = self.g.block_resampled(self.dev.st)
                self.need(np.array_equal(got, mask), "block_resampled", got, mask)
                self.S.resample_blocks(self.dev.st.parents, got)
            else:
                self.S.resample_blocks(self.model.parents.copy(), mask)
        self.par_expect = ("blocks", mask)
        self.changed()
        return f"ok {int(mask.sum())}/{self.B}"

    def op_across(self, op):
        try:
            A = self.model.across(op)
        except Refused:
            self.refused(lambda: self.dev.across(op), self.g.ErrorException)
            return "refused congruent"
        if self.dev:
            got = self.dev.across(op)
            self.need((got is None) == (A is None) and (A is None or np.array_equal(got, A)), "block ancestors", got, A)
        if A is None:
            return "ok held"
        if self.S is not None:
            self.S.resample_across(self.dev.st.parents if self.dev and self.checked else self.model.parents.copy(), A)
        self.par_expect = ("global",)
        self.changed()
        return "ok fired"

    def op_rejuvenate(self, op):
        try:
            self.model.rejuvenate(op)
        except Refused:
            self.refused(lambda: self.dev.rejuvenate(op), self.g.ErrorException)
            return "refused mask"
        if self.dev:
            self.dev.rejuvenate(op)
        self.changed()
        return "ok"

    def op_poke(self, op):
        idx, value = poke_index(op, self.setup), np.nan if op["what"] == "nan" else -np.inf
        self.nan_poked = self.nan_poked or op["what"] == "nan"
        self.model.poke(idx, value)
        if self.dev:
            if self.checked:
                lw = self.dev.st.log_weights
                lw[idx] = value
            else:
                lw = self.model.lw
            self.dev.st.log_weights = lw
        self.changed()
        return "ok"

    def op_refused(self, op):
        what = op["what"]
        if self.dev:
            self.refused(*self.dev.refused_call(what, self.T))
        return "refused " + what

    # -- getters: checked at once
    def op_get(self, op):
        self.flush()
        what = op["what"]
        level = STORE_GETTERS.get(what)
        if level is not None and not self.has(level):                        # the store getters of a run without (that kind of) store are refusals
            if self.dev:
                st, g, bs = self.dev.st, self.g, self.bs
                call = {"moments_past": lambda: g.block_moments(st, bs, step=1), "columns": lambda: st.history_column(1, 0),
                        "sample": lambda: g.block_sample_trajectories(st, bs, 1), "backward": lambda: g.block_backward_trajectories(st, bs, 1)}[what]
                self.refused(call, g.ErrorException)
            return "refused no_store"
        return getattr(self, "get_" + what)(op)

    def get_stats(self, op):
        if self.dev:
            self.check_stats()
        return "ok"

    def get_resampled(self, op):
        if self.model.mask is None:
            self.refused(lambda: self.g.block_resampled(self.dev.st), self.g.ErrorException)
            return "refused mask"
        if self.dev:
            self.need(np.array_equal(self.g.block_resampled(self.dev.st), self.model.mask), "block_resampled")
        return "ok"

    def get_ancestors(self, op):
        if self.model.A is None:
            self.refused(lambda: self.g.block_ancestors(self.dev.st), self.g.ErrorException)
            return "refused none"
        if self.dev:
            self.need(np.array_equal(self.g.block_ancestors(self.dev.st), self.model.A), "block_ancestors")
        return "ok"

    def _twin(self):
        if self.twin is None:
            self.twin = self.g.DeviceParticleFilterState(self.m, self.n, seed=3, keep_prev=self.setup["keep_prev"])
        return self.twin

    def _twin_moments(self, rows):
        """gpf_block_moments of a store-less twin filter that holds `rows` and the model's log-weights (tests/test_gpu_block_history.py)"""
        from test_gpu_block_history import c_moments
        tw = self._twin()
        tw.traces = rows
        tw.log_weights = self.model.lw
        return c_moments(tw, self.bs)

    def get_moments(self, op):
        if self.dev:
            mu, s2 = self.g.block_moments(self.dev.st, self.bs)
            wmu, ws2 = self._twin_moments(self.model.rows)
            self.need(eq(mu, wmu) and eq(s2, ws2), "block_moments")
        return "ok"

    def get_moments_past(self, op):
        t = 1 + int(op["u"] * self.T)
        self.end_step()
        if self.dev:
            rows = np.zeros((self.n, self.dev.st.row_width))
            for c in range(self.d):
                rows[:, c] = self.S.gen.trace(t, c)
            mu, s2 = self.g.block_moments(self.dev.st, self.bs, step=t)
            wmu, ws2 = self._twin_moments(rows)
            self.need(eq(mu, wmu[:, :self.d]) and eq(s2, ws2[:, :self.d]), "block_moments of step", t)
        return f"ok t={t}"

    def get_columns(self, op):
        self.end_step()
        self.check_columns()
        return "ok"

    def get_anc_lw(self, op):
        obs, ref = self.data.ys[:, self.T], self.data.refs[:, self.T]
        want = asp.ancestor_log_weights(self.m.name, self.model.P, self.model.lw, self.model.rows, self.bs, obs, ref, self.d)
        if self.dev:
            self.need(eq(self.g.block_ancestor_log_weights(self.dev.st, self.bs, obs, ref), want), "block_ancestor_log_weights")
        return "ok"

    def _range_ok(self, idx, local, at_T=True):
        """drawn indices (1-based): the particle of step T lies inside the drawing block, those of earlier steps (backward: global) inside the filter;
        0 only for a block whose weights hold a NaN"""
        lw = self.model.lw
        for b, (lo, hi) in enumerate(self.model.blocks()):
            if np.isnan(lw[lo:hi]).any():
                self.need(np.all(idx[b] == 0), "a NaN block draws index 0", b)
                continue
            off = 0 if local else lo
            last = idx[b] if local else idx[b][:, -1]
            self.need(np.all((idx[b] >= 1) & (idx[b] <= self.n)), "drawn indices outside the filter", b)
            if at_T:
                self.need(np.all((last >= off + 1) & (last <= off + hi - lo)), "the drawn particle of step T is outside its block", b)

    def get_sample(self, op):
        lo, hi = resolve_steps(op["steps"], self.T)
        self.end_step()
        M, k = self.model, op["k"]
        self.need(self.S.steps == self.T, "the Store's step count", self.S.steps, self.T)
        idx = draw_indices(self.o, M.lw, self.setup["filter_seed"], M.epoch, self.bs, k)
        self._range_ok(idx, True)
        want = paths(self.S.gen, idx, self.bs, lo, hi, self.d)
        if self.dev:
            traj, got = self.g.block_sample_trajectories(self.dev.st, self.bs, k, steps=(lo, hi), return_indices=True)
            self.need(np.array_equal(got, idx), "block_sample_trajectories: indices", np.argwhere(got != idx)[:4].tolist())
            self.need(eq(traj, want), "block_sample_trajectories: paths")
        M.bump(1)
        return f"ok {lo}..{hi}"

    def get_backward(self, op):
        lo, hi = resolve_steps(op["steps"], self.T)
        self.end_step()
        M, k = self.model, op["k"]
        P = M.P
        if self.dev and self.setup["profile"] == "B":                        # the drawing block's CURRENT rows, as read at the time of the draw
            P = self.g.get_block_params(self.dev.st)
            self.need(np.array_equal(P, M.P), "block parameters at the draw")
        want, widx = bsp.backward(self.o, self.m.name, P, self.S, self.setup["filter_seed"], M.epoch, k, lo, hi)
        self._range_ok(widx, False, at_T=hi == self.T)
        if self.dev:
            traj, idx = self.g.block_backward_trajectories(self.dev.st, self.bs, k, steps=(lo, hi), return_indices=True)
            self.need(np.array_equal(idx, widx), "block_backward_trajectories: indices", np.argwhere(idx != widx)[:4].tolist())
            self.need(eq(traj, want), "block_backward_trajectories: paths")
        M.bump(self.T - lo + 1)
        return f"ok {lo}..{hi}"


def walk(g, o, seed, device=True):
    setup, ops = plan(seed)
    w = Walk(g, o, setup, ops, device=device)
    try:
        return w.run()
    finally:
        w.close()


# ----------------------------------------------------------------------------- the device alone: read back after every op, or never
def device_only(g, seed, readback):
    """the plan of `seed` on the device alone, without its pokes (a poke reads the weights back).  readback=True: rows, log-weights, parents, block_stats
    and every history column are read after every op, as the checked walk does; False: nothing is read before the end.  The draws, which cost epochs, are
    issued either way; the other getters only with readback.  Returns (which ops were refused, the final rows, log-weights, parents, history columns and
    the two path draws)."""
    setup, ops = plan(seed)
    data = Data(g, setup)
    dev = Device(g, setup, data, raw=not readback)
    st, bs, T, refused = dev.st, setup["bs"], 1, []
    store, full = setup["store"] != "none", setup["store"] == "full"

    def columns():
        k = C.c_int32(0)
        st._check(st._L.gpf_history_steps(st._h, C.byref(k)))
        return [st.history_column(t, c) for t in range(1, k.value + 1) for c in range(st.dim)] if store else []

    try:
        for i, op in enumerate(ops):
            what = op["op"]
            try:
                if what == "update":
                    dev.update(data.ys[:, T], data.refs[:, T] if op["ref"] else None)
                    T += 1
                elif what == "resample":
                    dev.resample(op, data.ys[:, T], data.refs[:, T])
                elif what == "across":
                    dev.across(op)
                elif what == "rejuvenate":
                    dev.rejuvenate(op)
                elif what == "get" and op["what"] == "sample":
                    g.block_sample_trajectories(st, bs, op["k"], steps=resolve_steps(op["steps"], T))
                elif what == "get" and op["what"] == "backward":
                    g.block_backward_trajectories(st, bs, op["k"], steps=resolve_steps(op["steps"], T))
                elif what == "get" and readback:
                    if op["what"] == "moments":
                        g.block_moments(st, bs)
                    elif op["what"] == "moments_past":
                        g.block_moments(st, bs, step=1 + int(op["u"] * T))
                    elif op["what"] == "anc_lw":
                        g.block_ancestor_log_weights(st, bs, data.ys[:, T], data.refs[:, T])
            except g.ErrorException:
                refused.append(i)
            if readback:
                st.traces, st.log_weights, st.parents, g.block_stats(st, bs), columns()
        out = [st.traces, st.log_weights, st.parents] + columns()
        if store:
            out += list(g.block_sample_trajectories(st, bs, 3, return_indices=True))
        if full:
            out += list(g.block_backward_trajectories(st, bs, 3, return_indices=True))
        return refused, out
    finally:
        dev.close()


# ----------------------------------------------------------------------------- what the plans contain
SITUATIONS = ["backward over a conditional resample", "backward over an ancestor resample", "backward over residual/stratified, sort_particles off",
              "backward over a tempered resample", "backward over a rejuvenation after the step's resample", "backward over an across-block call that fired, profile B",
              "only_resampled directly after a conditional resample", "only_resampled directly after an ancestor resample",
              "only_resampled directly after an across-block resample", "only_resampled directly after a refused call",
              "update and resample after an ancestral draw", "update and resample after a backward draw", "staging burst of five or more",
              "ESS gate with both kinds of block", "only_resampled after a conditional resample that left some block alone",
              "only_resampled after an across-block call that held, the mask kept"]


def bursts(log):
    """the maximal runs of ops between two getters"""
    run, out = [], []
    for e in log:
        if e["op"]["op"] == "get":
            if run:
                out.append(run)
            run = []
        else:
            run.append(e)
    return out + ([run] if run else [])


def situations(setup, log):
    """how often each ordered situation occurs in one model run"""
    cnt = dict.fromkeys(SITUATIONS, 0)
    tags, resampled_in_step = {}, {}
    ok = lambda e: e["out"].startswith("ok")
    for i, e in enumerate(log):
        op, T = e["op"], e["T"]
        if not ok(e):
            continue
        tag = tags.setdefault(T, set())
        if op["op"] == "resample" and not e["out"].startswith("ok 0/"):
            resampled_in_step[T] = True
            if op["kind"] == "cond":
                tag.add("cond")
            elif op["kind"] == "anc":
                tag.add("anc")
            else:
                if op["method"] != "multinomial" and not op["sort"]:
                    tag.add("nosort")
                if op["alpha"] is not None:
                    tag.add("tempered")
            mixed = e["out"].split()[1].split("/")
            if op["ess_frac"] is not None and 0 < int(mixed[0]) < int(mixed[1]):
                cnt["ESS gate with both kinds of block"] += 1
        if op["op"] == "update":
            resampled_in_step.pop(T, None)                                   # (T is already the new step: nothing resampled in it yet)
        if op["op"] == "rejuvenate" and resampled_in_step.get(T):
            tag.add("rejuv")
        if op["op"] == "across" and e["out"] == "ok fired":
            tag.add("across")
        if op["op"] == "get" and op["what"] == "backward":
            lo, _ = (int(x) for x in e["out"].split()[1].split(".."))
            walked = set().union(*[tags.get(s, set()) for s in range(lo + 1, T + 1)]) if T > lo else set()
            for name, key in zip(SITUATIONS[:5], ("cond", "anc", "nosort", "tempered", "rejuv")):
                cnt[name] += key in walked
            cnt[SITUATIONS[5]] += "across" in walked and setup["profile"] == "B"
        if op["op"] == "rejuvenate" and op["only"] and i > 0:
            prev = log[i - 1]
            if prev["kind"] == "resample_cond" and ok(prev):
                cnt[SITUATIONS[6]] += 1
                done = prev["out"].split()[1].split("/")
                cnt[SITUATIONS[14]] += int(done[0]) < int(done[1])
            if prev["out"] == "ok held":
                cnt[SITUATIONS[15]] += 1
            if prev["kind"] == "resample_anc" and ok(prev):
                cnt[SITUATIONS[7]] += 1
            if prev["out"].startswith("refused"):
                cnt[SITUATIONS[9]] += 1
        if op["op"] == "get" and op["what"] in ("sample", "backward"):
            later = log[i + 1:]
            upd = next((j for j, x in enumerate(later) if x["op"]["op"] == "update" and ok(x)), None)
            if upd is not None and any(x["op"]["op"] == "resample" and ok(x) for x in later[upd + 1:]):
                cnt[SITUATIONS[10 if op["what"] == "sample" else 11]] += 1
    for i, e in enumerate(log):                                              # (the rejuvenation after a call that fired is itself refused: the mask is gone)
        if e["op"]["op"] == "rejuvenate" and e["op"]["only"] and i > 0 and log[i - 1]["op"]["op"] == "across" and ok(log[i - 1]):
            cnt[SITUATIONS[8]] += 1
    if setup["mode"] == "burst":
        cnt[SITUATIONS[12]] += sum(sum(ok(e) and (e["op"]["op"] == "update" or e["kind"] == "resample_anc") for e in run) >= 5 for run in bursts(log))
    return cnt
