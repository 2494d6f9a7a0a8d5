"""Whole trajectories per block on the device (gpf.h gpf_block_sample_trajectories): the reference's
`for b in blocks; sample_unweighted_traces(state[b], k); end` on persistent traces, in one launch.

  1.  the indices EQUAL tests/block_trajectories_spec.py (log-weights, seed, epoch, sizes -> indices), and the call leaves the state as it was;
  2.  the paths EQUAL history_column along the drawn particle's ancestry and the NumPy genealogy fed only with what a caller sees;
  3.  one block of the whole filter draws what sample_unweighted_traces draws;
  4.  the nested filter: ancestors in other blocks;
  5.  the call costs exactly one RNG epoch;
  6.  NaN, all -Inf and one-particle weights;
  7.  the draws of different blocks are independent and follow the weights;
  8.  refused calls change nothing.
Sizes: 1000 particles in blocks of 7 / 100 (a wave, 2 per lane; 7: the last block has 6), 300 (a wave, 8 per lane), 999 (the workgroup; the last block is
ONE particle); n_samples 1, 70 (more than a wave's lanes), 300 (more than the workgroup's threads); 1200 where resampling across blocks needs
congruent blocks."""
import ctypes
import warnings

import numpy as np
import pytest

import block_trajectories_spec as spec
from block_history_spec import Genealogy

pytestmark = pytest.mark.gpu
T = 6
# the data, resampler cycle and noise scales of tests/test_gpu_block_history.py: at ess_frac = 0.7 some blocks resample and some do not
NOISE = {"sv1": 2.0, "object_motion": 0.3, "lgssm2": 0.3, "bearings4": 0.3}
CYCLE = [("multinomial", True), ("residual", True), ("stratified", True), ("stratified", False), ("multinomial", False)]
CASES = [("sv1", 7), ("object_motion", 100), ("bearings4", 300), ("object_motion", 999)]      # d = 1, 2, 4; every team shape
EDGES = [("sv1", 1), ("object_motion", 2), ("bearings4", 128), ("object_motion", 129), ("sv1", 512), ("bearings4", 513), ("object_motion", 2048)]
DRAWS = [1, 70, 300]
I64 = ctypes.POINTER(ctypes.c_int64)


def eq(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def n_blocks(n, bs):
    return (n + bs - 1) // bs


def model_of(g, name):
    return g.models.bearings4(sb=0.5) if name == "bearings4" else g.models.by_name(name)


def block_obs(g, m, n, bs, steps, seed=7):
    base = np.asarray(g.models.simulate(m, steps))
    rng = np.random.default_rng(seed)
    scale = NOISE[m.name] * 8.0 ** rng.uniform(-1, 1, (n_blocks(n, bs), steps, 1))
    return base[None, :, :] + scale * rng.standard_normal((n_blocks(n, bs),) + base.shape)


def latent(st):
    return st.traces[:, :st.dim]


class Loop:
    """the README loop per block with a block-wise store: the state, its genealogy as a caller sees it, and the number of epoch-advancing calls made
    so far (initialisation, every update, resample, rejuvenation and sampling call is one epoch) -- the epoch the NEXT call runs under"""

    def __init__(self, g, model_name, n, bs, seed=11, steps=T, whole_at=3, room=0, params=None):
        self.g, self.n, self.bs, self.seed = g, n, bs, seed
        self.m = model_of(g, model_name) if params is None else params[0]
        self.ys = block_obs(g, self.m, n, bs, steps + room)
        self.st = g.pf_initialize_blocks(self.m, (1,), self.ys[:, 0], n, bs, seed=seed, keep_prev=True, history=steps + room, params=params)
        self.epoch = 1
        self.gen = Genealogy(n)
        self.gen.begin_step(latent(self.st))
        self.n_res = self.n_not = 0
        for t in range(1, steps):
            self.step(t, whole=(t == whole_at))

    def resample_blocks(self, t):
        method, sort_particles = CYCLE[(t - 1) % len(CYCLE)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.g.pf_resample_blocks(self.st, self.bs, method, ess_frac=0.7, sort_particles=sort_particles, check=False)
        self.epoch += 1
        mask = self.g.block_resampled(self.st)
        self.n_res += int(mask.sum()); self.n_not += int((~mask).sum())
        self.gen.resample("blocks", self.st.parents, mask, self.bs)

    def update(self, t):
        self.gen.set_rows(latent(self.st))
        self.g.pf_update_blocks(self.st, (t + 1,), (None,), self.ys[:, t], self.bs)
        self.epoch += 1
        self.gen.begin_step(latent(self.st))

    def step(self, t, whole=False):
        self.resample_blocks(t)
        self.g.pf_rejuvenate_blocks(self.st, None, (), 1, method="move", only_resampled=True)
        self.epoch += 1
        if whole:
            self.g.pf_resample(self.st, "multinomial", check=False)
            self.epoch += 1
            self.gen.resample("global", self.st.parents)
        self.update(t)

    def draw(self, k, steps=None, bs=None):
        """(paths, indices, the epoch the call ran under)"""
        traj, idx = self.g.block_sample_trajectories(self.st, self.bs if bs is None else bs, k, steps=steps, return_indices=True)
        self.epoch += 1
        return traj, idx, self.epoch - 1

    def expected_indices(self, o, k, epoch, bs=None):
        return spec.draw_indices(o, self.st.log_weights, self.seed, epoch, self.bs if bs is None else bs, k)

    def close(self):
        self.st.close()


def snapshot(g, st):
    return st.traces, st.log_weights, st.parents, g.get_lml_est(st)


def same_state(a, b):
    return eq(a[0], b[0]) and eq(a[1], b[1]) and np.array_equal(a[2], b[2]) and eq(a[3], b[3])


def raw_call(st, bs, k, lo, hi, traj, idx):
    pd = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    pi = lambda a: None if a is None else a.ctypes.data_as(I64)
    return st._L.gpf_block_sample_trajectories(st._h, bs, k, lo, hi, pd(traj), pi(idx))


# ----------------------------------------------------------------------------- 1. indices, bit for bit
@pytest.mark.parametrize("model_name,bs", CASES)
def test_indices_equal_the_spec(g, o, model_name, bs):
    L = Loop(g, model_name, 1000, bs)
    assert L.n_res > 0 and L.n_not > 0, (L.n_res, L.n_not)
    B = n_blocks(1000, bs)
    cnt = np.minimum(bs, 1000 - np.arange(B) * bs)
    for k in DRAWS:
        before = snapshot(g, L.st)
        want = L.expected_indices(o, k, L.epoch)
        traj, idx, _ = L.draw(k)
        assert idx.shape == (B, k) and idx.dtype == np.int64 and traj.shape == (B, k, T, L.st.dim)
        assert np.array_equal(idx, want), (model_name, bs, k, np.argwhere(idx != want)[:4])
        assert np.all(idx >= 1) and np.all(idx <= cnt[:, None])
        assert same_state(before, snapshot(g, L.st)), (model_name, bs, k)
    if k > 1 and bs > 1:
        assert len(np.unique(idx[0])) > 1                                      # (not one particle over and over)
    L.close()


# ----------------------------------------------------------------------------- 2. paths, bit for bit
def paths_follow_the_genealogy(g, o, model_name, n, bs):
    L = Loop(g, model_name, n, bs)
    st, d, B = L.st, L.st.dim, n_blocks(n, bs)
    L.gen.set_rows(latent(st))
    cols = {(s, c): st.history_column(s, c) for s in range(1, T + 1) for c in range(d)}
    base = (np.arange(B) * bs)[:, None]
    for k, steps, (lo, hi) in [(DRAWS[0], None, (1, T)), (DRAWS[1], 3, (3, 3)), (DRAWS[2], (2, T - 1), (2, T - 1)), (DRAWS[1], None, (1, T))]:
        traj, idx, E = L.draw(k, steps)
        assert traj.shape == (B, k, hi - lo + 1, d)
        assert np.array_equal(idx, L.expected_indices(o, k, E))
        part = base + idx - 1
        for s in range(lo, hi + 1):
            for c in range(d):
                assert np.array_equal(traj[:, :, s - lo, c], cols[s, c][part]), (model_name, bs, k, s, c)
        assert np.array_equal(traj, spec.paths(L.gen, idx, bs, lo, hi, d)), (model_name, bs, k, steps)
    # either output alone
    k = 70
    want = L.expected_indices(o, k, L.epoch)
    only_idx = np.full((B, k), -7, np.int64)
    assert raw_call(st, bs, k, 2, 4, None, only_idx) == g._lib.OK
    assert np.array_equal(only_idx, want)
    L.epoch += 1
    want = L.expected_indices(o, k, L.epoch)
    only_traj = np.full((B, k, 3, d), -7.0)
    assert raw_call(st, bs, k, 2, 4, only_traj, None) == g._lib.OK
    L.epoch += 1
    assert np.array_equal(only_traj, spec.paths(L.gen, want, bs, 2, 4, d))
    L.close()


@pytest.mark.parametrize("model_name,bs", CASES)
def test_paths_follow_the_genealogy(g, o, model_name, bs):
    paths_follow_the_genealogy(g, o, model_name, 1000, bs)


# the edges of the three team shapes (<= 128: a wave, 2 per lane; <= 512: a wave, 8 per lane; else the workgroup), five whole blocks and a short one
@pytest.mark.parametrize("model_name,bs", EDGES)
def test_paths_follow_the_genealogy_at_the_team_edges(g, o, model_name, bs):
    paths_follow_the_genealogy(g, o, model_name, 5 * bs + (bs + 1) // 2, bs)


# ----------------------------------------------------------------------------- 3. one block equals the whole-filter call
def test_one_block_equals_sample_unweighted_traces(g, o):
    a, b = Loop(g, "object_motion", 1000, 1000), Loop(g, "object_motion", 1000, 1000)
    assert np.array_equal(a.st.checkpoint(), b.st.checkpoint())
    traj, idx, E = a.draw(65)
    rows, ridx = g.sample_unweighted_traces(b.st, 65, return_indices=True)
    assert idx.shape == (1, 65) and np.array_equal(idx[0], ridx)
    assert np.array_equal(traj[0, :, T - 1, :], rows[:, :a.st.dim])
    assert np.array_equal(idx, a.expected_indices(o, 65, E))
    # "one block" asked for as any size >= n
    _, idx2, E2 = a.draw(65, bs=2 ** 40)
    assert E2 == E + 1 and np.array_equal(idx2, a.expected_indices(o, 65, E2, bs=1000))
    a.close(); b.close()


# ----------------------------------------------------------------------------- 4. the nested filter: ancestors in other blocks
@pytest.mark.parametrize("bs", [8, 300])
def test_paths_of_a_nested_filter(g, o, bs):
    n = 1200
    B = n // bs
    sets = [g.models.object_motion(), g.models.object_motion(p_stay=0.95, p_start=0.05, sobs=0.5), g.models.object_motion(sy=0.2)]
    assign = (np.arange(B) * np.arange(B) + np.arange(B) // 2) % 3
    L = Loop(g, "object_motion", n, bs, seed=13, steps=1, room=T - 1, params=[sets[k] for k in assign])
    st, gen = L.st, L.gen
    fired = held = 0
    for t in range(1, T):
        L.resample_blocks(t)
        # t = 2: a gate that cannot fire (ESS < 0); t = 4: one that must (ESS <= B < 1.5 B); else no gate
        A = g.pf_resample_across_blocks(st, bs, ("multinomial", "residual", "stratified")[t % 3], ess_frac={2: 0.0, 4: 1.5}.get(t), check=False)
        L.epoch += 1
        if A is None:
            held += 1
        else:
            fired += 1
            gen.resample("global", st.parents)
        L.update(t)
    assert held == 1 and fired == T - 2 and L.n_res > 0 and L.n_not > 0, (held, fired, L.n_res, L.n_not)
    gen.set_rows(latent(st))
    moved = (gen.index(1) // bs != np.arange(n) // bs).mean()
    assert moved > 0.0, moved                                                 # step-1 ancestors sit in other blocks
    for k, steps, (lo, hi) in [(70, None, (1, T)), (1, (2, T - 1), (2, T - 1)), (300, 1, (1, 1))]:
        traj, idx, E = L.draw(k, steps)
        assert np.array_equal(idx, L.expected_indices(o, k, E)), (bs, k)
        assert np.array_equal(traj, spec.paths(gen, idx, bs, lo, hi, st.dim)), (bs, k, steps)
        part = (np.arange(B) * bs)[:, None] + idx - 1
        for c in range(st.dim):
            assert np.array_equal(traj[:, :, 0, c], st.history_column(lo, c)[part])
    L.close()


# ----------------------------------------------------------------------------- 5. the epoch
def test_the_call_costs_one_epoch(g, o):
    bs = 100
    a, b = Loop(g, "object_motion", 1000, bs, room=1), Loop(g, "object_motion", 1000, bs, room=1)
    E = a.epoch
    _, idx1 = g.block_sample_trajectories(a.st, bs, 70, return_indices=True)
    g.sample_unweighted_traces(b.st, 1)                                        # advances the epoch once and changes nothing
    assert np.array_equal(a.st.checkpoint(), b.st.checkpoint())
    _, idx2 = g.block_sample_trajectories(a.st, bs, 70, return_indices=True)   # a second call draws from the next epoch
    g.sample_unweighted_traces(b.st, 1)
    assert np.array_equal(idx1, a.expected_indices(o, 70, E)) and np.array_equal(idx2, a.expected_indices(o, 70, E + 1))
    assert not np.array_equal(idx1, idx2)
    for x in (a, b):                                                           # the next block-wise README step, its record included
        x.epoch = E + 2
        x.step(T)
    assert np.array_equal(a.st.checkpoint(), b.st.checkpoint())
    for t in range(1, T + 2):
        for c in range(a.st.dim):
            assert np.array_equal(a.st.history_column(t, c), b.st.history_column(t, c)), (t, c)
    _, idx3, E3 = a.draw(70)
    assert np.array_equal(idx3, a.expected_indices(o, 70, E3))                 # (the count of epochs still holds after the step)
    a.close(); b.close()


# ----------------------------------------------------------------------------- 6. weights at the edges
@pytest.mark.parametrize("model_name,bs", [("sv1", 100), ("bearings4", 300), ("object_motion", 999)])
def test_weights_at_the_edges(g, o, model_name, bs):
    L = Loop(g, model_name, 1000, bs)
    st, d, B = L.st, L.st.dim, n_blocks(1000, bs)
    lw = st.log_weights
    bad, neg, one = (0, 1, 2) if B > 2 else (0, None, 1)                      # (999: two blocks, the second of ONE particle -- all its weight on it)
    lw[bad * bs + 3] = np.nan
    if neg is not None:
        lw[neg * bs:(neg + 1) * bs] = -np.inf
    hit = min(one * bs + 5, 999)
    lw[one * bs:(one + 1) * bs] = -np.inf
    lw[hit] = -3.25
    st.log_weights = lw
    L.gen.set_rows(latent(st))
    for k in (1, 70):
        traj, idx, E = L.draw(k)
        assert np.all(idx[bad] == 0) and np.all(np.isnan(traj[bad]))
        others = np.arange(B) != bad
        assert np.all(idx[others] >= 1) and np.all(np.isfinite(traj[others]))
        assert np.array_equal(idx, L.expected_indices(o, k, E))
        assert eq(traj, spec.paths(L.gen, idx, bs, 1, T, d))
        assert np.all(idx[one] == hit - one * bs + 1)
        if neg is not None and k > 1:
            assert len(np.unique(idx[neg])) > 10                              # the uniform fallback spreads over the block
    lw[bad * bs + 3] = np.inf                                                  # +Inf is refused like NaN
    st.log_weights = lw
    traj, idx, E = L.draw(3)
    assert np.all(idx[bad] == 0) and np.all(np.isnan(traj[bad])) and np.array_equal(idx, L.expected_indices(o, 3, E))
    L.close()


# ----------------------------------------------------------------------------- 7. distribution across blocks
# 2000 blocks with the same seven weights, one draw each: the counts c_i of the drawn cells are Binomial(2000, p_i), so
# |c_i - 2000 p_i| <= 5 sqrt(2000 p_i (1 - p_i)) fails with probability < 6e-7 per cell for independent draws.  Every 2000 p_i >= 50 (the normal
# range of the binomial).  The seed was checked against the bound with the spec helper on the CPU before the test ever ran on a device.
P7 = np.array([0.05, 0.10, 0.15, 0.20, 0.25, 0.15, 0.10])
SEED7 = 2024


def bound7(idx):
    p = np.exp(np.log(P7)) / np.exp(np.log(P7)).sum()
    counts = np.bincount(idx.ravel() - 1, minlength=7)
    assert counts.sum() == 2000 and np.all(2000 * p >= 50)
    dev = np.abs(counts - 2000 * p)
    lim = 5 * np.sqrt(2000 * p * (1 - p))
    print("counts", counts, "deviation", dev, "bound", lim)
    return np.all(dev <= lim)


def test_draws_of_different_blocks_are_independent(g, o):
    n, bs = 14000, 7
    m = g.models.object_motion()
    ys = np.tile(np.asarray(g.models.simulate(m, 1))[0], (2000, 1))
    st = g.pf_initialize_blocks(m, (1,), ys, n, bs, seed=SEED7, history=1)
    lw = np.tile(np.log(P7), 2000)
    st.log_weights = lw
    want = spec.draw_indices(o, lw, SEED7, 1, bs, 1)
    assert bound7(want)                                                        # the spec at this seed, on the CPU
    traj, idx = g.block_sample_trajectories(st, bs, 1, return_indices=True)
    assert idx.shape == (2000, 1) and len(np.unique(idx)) == 7                 # (a slot numbering that forgets the block draws ONE cell 2000 times)
    assert bound7(idx)
    assert np.array_equal(idx, want)
    assert np.array_equal(traj[:, 0, 0, :], latent(st)[np.arange(2000) * bs + idx[:, 0] - 1])
    st.close()


# ----------------------------------------------------------------------------- 8. refusals change nothing
def test_refusals_change_nothing(g, o):
    n, bs, steps = 4200, 100, 3
    m = g.models.object_motion()
    ys = block_obs(g, m, n, bs, steps)
    INV, STATE, OK = g._lib.ERR_INVALID_ARGUMENT, g._lib.ERR_STATE, g._lib.OK
    B, k = n // bs, 5
    # without a block-wise store: a store-less block-wise state and a plain-store state
    plain = g.pf_initialize(m, (1,), ys[0, 0], 400, seed=1, keep_prev=True, history=4)
    bare = g.pf_initialize_blocks(m, (1,), ys[:4, 0], 400, 100, seed=1)
    for st in (plain, bare):
        blob = st.checkpoint()
        traj, idx = np.full((4, k, 1, 2), 7.0), np.full((4, k), 7, np.int64)
        assert raw_call(st, 100, k, 1, 1, traj, idx) == STATE and "trajectory store" in st._L.gpf_last_error(st._h).decode()
        with pytest.raises(g.ErrorException, match="trajectory store"):
            g.block_sample_trajectories(st, 100, k)
        assert np.all(traj == 7.0) and np.all(idx == 7) and np.array_equal(st.checkpoint(), blob)
        st.close()
    # bad arguments on a state with the store; T = 2
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n, bs, seed=5, keep_prev=True, history=steps)
    g.pf_update_blocks(st, (2,), (None,), ys[:, 1], bs)
    g.pf_resample_blocks(st, bs, "residual", check=False)
    epoch = 3
    traj, idx = np.full((B, k, 2, st.dim), 7.0), np.full((B, k), 7, np.int64)
    blob, cols = st.checkpoint(), [st.history_column(t, c) for t in (1, 2) for c in range(st.dim)]
    for lo, hi in [(0, 1), (0, 0), (1, 3), (3, 3), (2, 1), (-1, 2)]:
        assert raw_call(st, bs, k, lo, hi, traj, idx) == INV, (lo, hi)
    assert raw_call(st, bs, 0, 1, 2, traj, idx) == INV
    assert raw_call(st, bs, -3, 1, 2, traj, idx) == INV
    assert raw_call(st, bs, k, 1, 2, None, None) == INV
    assert raw_call(st, 0, k, 1, 2, traj, idx) == INV
    assert raw_call(st, bs, 2 ** 31 - 1, 1, 2, None, idx) == INV              # n_blocks * n_samples >= 2^31
    assert raw_call(st, bs, 2 ** 24, 1, 2, traj, None) == INV                 # 42 * 2^24 < 2^31 draws, but x 2 steps x 2 columns >= 2^31 cells
    assert st._L.gpf_block_sample_trajectories(None, bs, k, 1, 2, traj.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), idx.ctypes.data_as(I64)) == INV
    assert raw_call(st, 2100, k, 1, 2, traj, idx) == STATE and "trajectory store" in st._L.gpf_last_error(st._h).decode()
    for call in (lambda: g.block_sample_trajectories(st, bs, k, steps=0), lambda: g.block_sample_trajectories(st, bs, k, steps=(0, 2))):
        with pytest.raises(g.ErrorException, match="1-based"):
            call()
    for call in (lambda: g.block_sample_trajectories(st, bs, k, steps=3), lambda: g.block_sample_trajectories(st, bs, 0),
                 lambda: g.block_sample_trajectories(st, bs, k, steps=(2, 1)), lambda: g.block_sample_trajectories(st, 2100, k)):
        with pytest.raises(g.ErrorException):
            call()
    assert np.all(traj == 7.0) and np.all(idx == 7)
    assert np.array_equal(st.checkpoint(), blob)
    assert all(np.array_equal(x, st.history_column(t, c)) for x, (t, c) in zip(cols, [(t, c) for t in (1, 2) for c in range(st.dim)]))
    # the next accepted call runs under the epoch the refused ones left alone
    got_traj, got = g.block_sample_trajectories(st, bs, k, return_indices=True)
    assert np.array_equal(got, spec.draw_indices(o, st.log_weights, 5, epoch, bs, k))
    assert got_traj.shape == (B, k, 2, st.dim) and np.all(np.isfinite(got_traj))
    st.close()
