"""Backward simulation per block on the device (gpf.h gpf_history_enable_blocks_weights, gpf_block_backward_sample):

  1. paths and indices bit for bit against the NumPy restatement of tests/block_backward_spec.py, which is fed only with what a caller sees (history_column
     and log_weights read back after every step's last call, parents, block_resampled, block ancestors, observations, parameters): four models, keep_prev on
     and off, the edges of the three team shapes, a short last block, n_samples 1 and 3, a sub-range of steps, and the epochs the calls cost;
  2. line_model: a drawn path has one slope; step T is block_sample_trajectories' draw; the ESS gate's unequal weights; per-block parameters;
  3. the nested filter: block resample, then resampling across blocks, every step -- the candidates are the lineage's block;
  4. edge weights: a -Inf particle of a past step is never drawn, a held particle no candidate leads to takes its recorded parent, a NaN block at step T;
  5. refused calls change nothing; a state without history_weights runs every block-wise call as it did;
  6. what the feature is for: more distinct x_1 than the ancestral draw; and the law against the exact smoother (the CPU rehearsal:
     tests/test_block_backward_host.py)."""
import ctypes as C
import warnings

import numpy as np
import pytest

import block_backward_spec as bsp
import block_conditional_spec as cs
from block_trajectories_spec import draw_indices
from test_gpu_block_conditional import block_obs, eq, model_of, n_of, refused, snapshot, unchanged

pytestmark = pytest.mark.gpu
T = 4
MODELS = ["sv1", "object_motion", "lgssm2", "bearings4"]                     # d = 1, 2, 2, 4
SIZES = [1, 2, 7, 128, 129, 512, 513, 2048]                                  # a wave 2 / 8 per lane, the workgroup, and their edges
SEED = 17


def quiet(call):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return call()


def line_data(g, B, steps, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([[g.models.line_obs(t + 1, float(s)) for t in range(steps)] for s in rng.integers(-2, 3, B)])


class Dev:
    """initialise -> (resample blocks [-> resample across blocks] -> update)* on the device with the weights mode of the store, and the Store of the
    restatement filled from what the state returns.  `epoch`: the epoch-advancing calls so far = the epoch the next call runs under."""

    def __init__(self, g, name, bs, *, n=None, keep_prev=False, steps=T, ess_frac=None, across=False, params=None, weights=True, seed=SEED, ys=None,
                 resample=True, after_update=None, final_resample=False, model=None):
        self.g, self.bs = g, bs
        self.m = m = model if model is not None else g.models.line_model() if name == "line_model" else model_of(g, name)
        self.n = n = n_of(bs) if n is None else n
        self.B = B = (n + bs - 1) // bs
        if ys is None:
            ys = line_data(g, B, steps) if name == "line_model" else block_obs(g, m, B, steps)
        self.ys = ys
        self.st = st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=seed, keep_prev=keep_prev, history=steps, history_weights=weights, params=params)
        self.epoch, self.seed = 1, seed
        self.S = bsp.Store(n, bs, m.dim)
        self.S.begin_step(ys[:, 0])
        self.n_res = self.n_not = self.fired = 0
        for t in range(1, steps):
            if after_update is not None:
                after_update(self, t)
            if resample:
                quiet(lambda: g.pf_resample_blocks(st, bs, "multinomial", ess_frac=ess_frac, check=False))
                self.epoch += 1
                mask = g.block_resampled(st)
                self.n_res += int(mask.sum()); self.n_not += int((~mask).sum())
                self.S.resample_blocks(st.parents, mask)
            if across:
                A = g.pf_resample_across_blocks(st, bs, "multinomial", ess_frac=None, check=False)
                self.epoch += 1
                if A is not None:
                    self.fired += 1
                    self.S.resample_across(st.parents, A)
            self.end_step()
            g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs)
            self.epoch += 1
            self.S.begin_step(ys[:, t])
        if after_update is not None:
            after_update(self, steps)
        if final_resample:                                                   # (a resample of the last step: its recorded parents are not the identity)
            quiet(lambda: g.pf_resample_blocks(st, bs, "multinomial", check=False))
            self.epoch += 1
            self.S.resample_blocks(st.parents, g.block_resampled(st))
        self.end_step()

    def end_step(self):
        s = self.S.steps
        self.S.end_step(np.stack([self.st.history_column(s, c) for c in range(self.m.dim)], axis=1), self.st.log_weights)

    def draw(self, k, steps=None):
        """(paths, indices, the epoch the call ran under)"""
        traj, idx = self.g.block_backward_trajectories(self.st, self.bs, k, steps=steps, return_indices=True)
        E = self.epoch
        lo = 1 if steps is None else (steps[0] if isinstance(steps, tuple) else steps)
        self.epoch += self.S.steps - lo + 1
        return traj, idx, E

    def want(self, o, k, E, lo=1, hi=None, P=None):
        name = "line_model" if self.m.name == "line_model" else self.m.name
        return bsp.backward(o, name, self.m.params if P is None else P, self.S, self.seed, E, k, lo, hi)

    def close(self):
        self.st.close()


def check(got, want, where):
    assert eq(got[0], want[0]), (where, "paths")
    assert np.array_equal(got[1], want[1]), (where, "indices", np.argwhere(got[1] != want[1])[:5])


# ----------------------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("keep_prev", [False, True])
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_paths_and_indices_are_the_restatement(g, o, name, bs, keep_prev):
    d = Dev(g, name, bs, keep_prev=keep_prev)
    before = (d.st.traces, d.st.log_weights, d.st.parents, [d.st.history_column(t, c) for t in range(1, T + 1) for c in range(d.m.dim)])
    traj, idx, E = d.draw(1)
    check((traj, idx), d.want(o, 1, E), (name, bs, keep_prev, 1))
    assert traj.shape == (d.B, 1, T, d.m.dim) and idx.shape == (d.B, 1, T) and np.all((idx >= 1) & (idx <= d.n))
    traj, idx, E3 = d.draw(3, steps=(2, 3))                                  # a sub-range: walked from T, written for steps 2 and 3
    assert E3 == E + T
    check((traj, idx), d.want(o, 3, E3, 2, 3), (name, bs, keep_prev, 3))
    _, idx, E1 = d.draw(2, steps=T)                                          # ... which cost T - 2 + 1 epochs; step T alone is the categorical draw
    assert E1 == E3 + T - 1
    blocks = np.arange(d.B)[:, None] * bs
    assert np.array_equal(idx[:, :, 0], blocks + draw_indices(o, d.st.log_weights, SEED, E1, bs, 2))
    after = (d.st.traces, d.st.log_weights, d.st.parents, [d.st.history_column(t, c) for t in range(1, T + 1) for c in range(d.m.dim)])
    assert eq(before[0], after[0]) and eq(before[1], after[1]) and np.array_equal(before[2], after[2]) and all(eq(x, y) for x, y in zip(before[3], after[3]))
    d.close()


def test_backward_draws_leave_the_recorded_genealogy(g, o):
    """somewhere the drawn particle of a past step is not the recorded parent (otherwise the tests above compare ancestral paths)"""
    d = Dev(g, "lgssm2", 129)
    _, idx, _ = d.draw(3)
    moved = 0
    for s in range(T, 1, -1):
        moved += int((d.S.step_map(s)[idx[:, :, s - 1] - 1] != idx[:, :, s - 2] - 1).sum())
    assert moved > 0
    d.close()


# ----------------------------------------------------------------------------- 2. single properties
def test_line_model_paths_have_one_slope(g, o):
    d = Dev(g, "line_model", 129, n=8 * 129)
    traj, idx, E = d.draw(3)
    check((traj, idx), d.want(o, 3, E), "line_model")
    assert np.all(traj[..., 0] == traj[..., :1, 0])                          # logtrans is 0 / -Inf: the slope persists along every drawn path
    assert len(np.unique(traj[..., 0])) > 1
    d.close()


@pytest.mark.parametrize("bs", [7, 513])
def test_step_T_is_the_draw_of_block_sample_trajectories(g, bs):
    a, b = Dev(g, "bearings4", bs), Dev(g, "bearings4", bs)
    _, idx, _ = a.draw(3)
    _, local = g.block_sample_trajectories(b.st, bs, 3, return_indices=True)
    assert np.array_equal(idx[:, :, -1], np.arange(a.B)[:, None] * bs + local)
    a.close(); b.close()


def test_the_ess_gate_leaves_unequal_weights_in_the_store(g, o):
    d = Dev(g, "lgssm2", 7, n=40 * 7 + 5, ess_frac=0.5)
    assert d.n_res > 0 and d.n_not > 0, (d.n_res, d.n_not)
    past = d.S.lw[1].reshape(-1)[: 40 * 7].reshape(40, 7)
    assert np.any(past.max(axis=1) != past.min(axis=1)) and np.any(past.max(axis=1) == past.min(axis=1))   # both kinds of block at step 2
    traj, idx, E = d.draw(3)
    check((traj, idx), d.want(o, 3, E), "ess gate")
    d.close()


def test_per_block_parameters_are_the_drawing_blocks(g, o):
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    bs = 129
    assign = np.arange((n_of(bs) + bs - 1) // bs) % 3
    d = Dev(g, "object_motion", bs, keep_prev=True, params=[sets[k] for k in assign])
    traj, idx, E = d.draw(3)
    P = np.stack([sets[k].params for k in assign])
    check((traj, idx), d.want(o, 3, E, P=P), "block params")
    assert not np.array_equal(idx, d.want(o, 3, E, P=sets[0].params)[1])     # (the rows matter)
    d.close()


# ----------------------------------------------------------------------------- 3. the nested filter
@pytest.mark.parametrize("bs", [8, 300])
def test_nested_filter_walks_the_lineages_blocks(g, o, bs):
    d = Dev(g, "object_motion", bs, n=24 * bs, keep_prev=True, ess_frac=0.8, across=True)
    assert d.fired > 0
    traj, idx, E = d.draw(3)
    check((traj, idx), d.want(o, 3, E), ("nested", bs))
    p = idx - 1
    assert np.array_equal(p[:, :, -1] // bs, np.repeat(np.arange(d.B)[:, None], 3, axis=1))
    elsewhere = 0
    for s in range(T, 1, -1):                                                # the block of step s - 1 is the recorded parent's
        born = d.S.step_map(s)[p[:, :, s - 1]] // bs
        assert np.array_equal(p[:, :, s - 2] // bs, born), s
        elsewhere += int((born != p[:, :, s - 1] // bs).sum())
    assert elsewhere > 0                                                     # (some lineage changed its block)
    d.close()


# ----------------------------------------------------------------------------- 4. edge weights
def test_a_particle_of_weight_zero_at_a_past_step_is_never_drawn(g, o):
    bs, B = 7, 64
    dead = np.arange(bs * B) % bs % 2 == 1                                   # local 1, 3, 5 of every block

    def kill(d, t):
        if t == 2:                                                           # step 2, which no resample follows: the -Inf weights stay in its record
            lw = d.st.log_weights
            lw[dead] = -np.inf
            d.st.log_weights = lw

    d = Dev(g, "lgssm2", bs, n=bs * B, resample=False, after_update=kill)
    assert np.all(np.isneginf(d.S.lw[1][dead])) and np.all(np.isfinite(d.S.lw[1][~dead]))
    traj, idx, E = d.draw(3)
    check((traj, idx), d.want(o, 3, E), "dead particles")
    assert not dead[idx[:, :, 1] - 1].any()
    assert np.any(idx[:, :, 1] != idx[:, :, 2])                              # (no resample: the recorded parent is the particle itself; the draw moved)
    d.close()


def test_a_held_particle_no_candidate_leads_to_takes_its_recorded_parent(g, o):
    bs, B = 129, 4
    odd = np.arange(bs * B) % 3 == 0

    def foreign_slope(d, t):
        if t == T:                                                           # the last step: a slope outside uniform_discrete(-2, 2), which no particle of step
            rows = d.st.traces                                               # T - 1 holds, and equal weights, so that the step's resample keeps such particles
            rows[odd, 0] = 7.0
            d.st.traces = rows
            d.st.log_weights = np.zeros(bs * B)

    d = Dev(g, "line_model", bs, n=bs * B, after_update=foreign_slope, final_resample=True)
    traj, idx, E = d.draw(5)
    check((traj, idx), d.want(o, 5, E), "fallback")
    held = traj[:, :, T - 1, 0] == 7.0
    assert held.any() and (~held).any()
    parent = d.S.step_map(T)[idx[:, :, T - 1] - 1]
    assert np.any(parent != idx[:, :, T - 1] - 1)
    assert np.array_equal((idx[:, :, T - 2] - 1)[held], parent[held])        # all ancestor weights -Inf: the ancestral step
    assert np.all(traj[:, :, T - 2, 0][held] != 7.0) and np.all(traj[:, :, T - 2, 0][~held] == traj[:, :, T - 1, 0][~held])
    d.close()


def test_a_nan_block_gets_index_0_and_nan_paths(g):
    bs = 7
    a, b = Dev(g, "lgssm2", bs), Dev(g, "lgssm2", bs)
    lw = b.st.log_weights
    lw[bs + 3] = np.nan
    b.st.log_weights = lw
    ta, ia, _ = a.draw(3)
    tb, ib, _ = b.draw(3)
    assert np.all(ib[1] == 0) and np.all(np.isnan(tb[1]))
    keep = np.arange(a.B) != 1
    assert eq(ta[keep], tb[keep]) and np.array_equal(ia[keep], ib[keep])
    a.close(); b.close()


# ----------------------------------------------------------------------------- 5. refusals; the plain store is what it was
def test_refusals_change_nothing(g):
    m = g.models.object_motion()
    bs, n, B = 7, 26, 4
    ys = block_obs(g, m, B, 3)
    E = g.ErrorException
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    raw = lambda st, size=bs, k=1, lo=1, hi=2, out=True: st._L.gpf_block_backward_sample(st._h, size, k, lo, hi, P(np.empty(B * 4 * 3 * 2)) if out else None, None)

    def raw_refused(st, code, store=True, **kw):
        before = snapshot(st, store)
        assert raw(st, **kw) == code and unchanged(before, snapshot(st, store)), kw

    # no store; a store without the weights mode
    plain = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED)
    refused(g, plain, lambda: g.block_backward_trajectories(plain, bs), E, store=False)
    raw_refused(plain, g._lib.ERR_STATE, store=False)
    plain.close()
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, history=3)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    with pytest.raises(E, match="history_weights=True"):
        g.block_backward_trajectories(st, bs)
    raw_refused(st, g._lib.ERR_STATE)
    st.close()
    # the weights mode: bad steps, n_samples = 0, a NULL output, a bad block size
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, history=3, history_weights=True)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    for steps in ((0, 2), (2, 1), (1, 3), 3):
        refused(g, st, lambda: g.block_backward_trajectories(st, bs, 1, steps=steps), E)
    refused(g, st, lambda: g.block_backward_trajectories(st, bs, 0), E)
    for kw in (dict(lo=0), dict(lo=2, hi=1), dict(hi=3), dict(k=0), dict(out=False), dict(size=0)):
        raw_refused(st, g._lib.ERR_INVALID_ARGUMENT, **kw)
    raw_refused(st, g._lib.ERR_INVALID_ARGUMENT, size=13)                    # (not the size the walked step was entered with)
    assert g.block_backward_trajectories(st, bs, 2).shape == (B, 2, 2, 2)    # (the state is alive and well)
    # a whole-filter update in the walked range: step 3 has no per-block observation rows
    g.pf_update(st, (3,), (None,), ys[0, 2])
    refused(g, st, lambda: g.block_backward_trajectories(st, bs, 1), E)
    raw_refused(st, g._lib.ERR_STATE, hi=3)
    assert g.block_backward_trajectories(st, bs, 1, steps=3).shape == (B, 1, 1, 2)   # (step 3 alone walks nothing)
    st.close()
    # blocks of 4096 particles
    big = g.pf_initialize_blocks(m, (1,), np.tile(ys[0, 0], (2, 1)), 2 * 4096, 4096, seed=SEED, history=2, history_weights=True)
    refused(g, big, lambda: g.block_backward_trajectories(big, 4096), E)
    before = snapshot(big)
    assert big._L.gpf_block_backward_sample(big._h, 4096, 1, 1, 1, P(np.empty(4)), None) == g._lib.ERR_STATE and unchanged(before, snapshot(big))
    big.close()
    # a block size that differs from the per-block parameters'
    sets = [g.models.object_motion(), g.models.object_motion(sy=0.2)]
    bp = g.pf_initialize_blocks(m, (1,), ys[:2, 0], 28, 14, seed=SEED, history=2, history_weights=True, params=sets)
    refused(g, bp, lambda: g.block_backward_trajectories(bp, 7), E)
    bp.close()


def test_a_state_without_history_weights_is_what_it_was(g):
    """the same sweep of the block-wise calls with and without the keyword: rows, weights, parents, the store's columns and the ancestral draws are equal"""
    m = g.models.object_motion()
    bs, B = 8, 12
    n = bs * B
    ys = block_obs(g, m, B, T)
    out = []
    for weights in (False, True):
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=SEED, keep_prev=True, history=T, history_weights=weights)
        seen = []
        for t in range(1, T):
            quiet(lambda: g.pf_resample_blocks(st, bs, ("multinomial", "residual", "stratified")[t % 3], ess_frac=0.8, check=False))
            seen.append(g.block_resampled(st))
            g.pf_rejuvenate_blocks(st, None, (), 1, method="move", only_resampled=True)
            A = g.pf_resample_across_blocks(st, bs, "multinomial", ess_frac=None, check=False)
            seen.append(np.zeros(0) if A is None else A)
            seen += list(g.block_stats(st, bs)) + list(g.block_moments(st, bs)) + list(g.block_moments(st, bs, step=t))
            g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], bs)
            seen += [st.traces, st.log_weights, st.parents]
        seen += [st.history_column(t, c) for t in range(1, T + 1) for c in range(m.dim)]
        seen += list(g.block_sample_trajectories(st, bs, 3, return_indices=True))
        seen.append(g.get_lml_est(st))
        out.append(seen)
        st.close()
    assert len(out[0]) == len(out[1]) and all(eq(x, y) for x, y in zip(*out))


# ----------------------------------------------------------------------------- 6. what the feature is for
def test_backward_draws_are_more_diverse_at_step_1(g):
    """lgssm2, T = 32, 256 blocks of 16 particles, multinomial every step, 16 draws per block: the genealogy of every block has coalesced -- the ancestral
    draws share one x_1 per block (256 distinct values in all) -- while the backward draws do not (the CPU restatement of this seeded experiment, run under
    the epoch the filter ends at: 372)"""
    Tl, B, N, k = 32, 256, 16, 16
    d = Dev(g, "lgssm2", N, n=B * N, steps=Tl)
    anc = g.block_sample_trajectories(d.st, N, k, steps=1)
    d.epoch += 1
    back, _, _ = d.draw(k)
    count = lambda x1: sum(len(np.unique(x1[b], axis=0)) for b in range(B))
    n_anc, n_back = count(anc[:, :, 0]), count(back[:, :, 0])
    print("distinct x_1 over", B, "blocks x", k, "draws: ancestral", n_anc, "backward", n_back)
    assert n_back > n_anc
    d.close()


def test_backward_draws_follow_the_exact_smoother(g):
    """lgssm2 defaults, T = 8, 1024 blocks of LAW_N particles, multinomial every step, one backward path per block, pooled over the blocks: every
    smoothed mean within 5 standard errors of the exact one, every variance within 5 sqrt(2 / B) relative.  FFBSi is consistent, not unbiased, so the
    block size matters: block_backward_spec.LAW_N is the smallest of 64, 128, 256 at which the CPU restatement of this seeded experiment stays inside
    the bound (its worst unit there: 4.19; 13.3 at 128, 28.2 at 64) -- fixed from the restatement, not from the device."""
    m, ys, mu, Sigma = bsp.law_setup(g.models)
    N = bsp.LAW_N
    d = Dev(g, "lgssm2", N, n=bsp.LAW_B * N, steps=bsp.LAW_T, seed=bsp.LAW_SEED, ys=np.tile(ys[None], (bsp.LAW_B, 1, 1)))
    traj = g.block_backward_trajectories(d.st, N, 1)
    d.close()
    zm, zv = bsp.law_units(traj[:, 0], mu, Sigma)
    print("backward simulation: mean z", np.round(zm, 2).tolist(), "variance z", np.round(zv, 2).tolist())
    assert np.all(zm <= cs.INV_SIGMAS) and np.all(zv <= cs.INV_SIGMAS), (zm, zv)
