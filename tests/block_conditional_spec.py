"""Conditional SMC for block-wise filters (gpf.h gpf_initialize_blocks_ref, gpf_update_blocks_ref, gpf_resample_blocks_conditional), restated on the
CPU oracle: the oracle's own block loops (oracle.initialize_blocks / update_blocks / resample_blocks) run as they are, and slot 0 of every block --
particle b * nb -- is patched afterwards.

  pinned step            the incoming lw[b0] and row of slot 0 are remembered, the plain oracle step runs, then slot 0's row becomes
                         [ref[b] | incoming latent (keep_prev) | 0 ...] and its log-weight lw_before + loglik(P, ref[b], obs[b]) (initialise: the loglik)
  conditional resample   the plain multinomial block resample runs; in the blocks that resampled slot 0's row is restored from the pre-call slot 0
                         and its parent set to local 1 (1-based).  The new weights are the plain call's.

Everything else -- the other particles, the epoch, the masks -- is the plain oracle's.  The functions continue from the patched state, so a loop of them
runs in lockstep with the device over many steps.  `ConditionalLoop` also keeps the genealogy (tests/block_history_spec.py) the device's trajectory
store must reproduce, and `smoother` / `invariance_run` are the exact-smoother experiment of the tests.

Helper module, no tests."""
import numpy as np

from block_history_spec import Genealogy
from block_trajectories_spec import draw_indices, paths


def slot0(n, nb):
    return np.arange(0, n, nb, dtype=np.int64)


def loglik_rows(o, f, rows, obs_rows):
    """loglik(P, rows[k], obs_rows[k]) for every k, by the oracle's model definition"""
    out = np.zeros(len(rows))
    one = np.zeros(1)
    for k in range(len(rows)):
        o.lib().o_loglik_rows(f.model, f.params, np.ascontiguousarray(rows[k], np.float64), f.W, 1, np.ascontiguousarray(obs_rows[k], np.float64), one)
        out[k] = one[0]
    return out


def _pinned_rows(f, ref, incoming=None):
    ref = np.asarray(ref, np.float64)
    new = np.zeros((ref.shape[0], f.W))
    new[:, :f.d] = ref
    if incoming is not None and f.keep_prev:
        new[:, f.d:2 * f.d] = incoming[:, :f.d]
    return new


def pinned_initialize(o, f, nb, obs_rows, ref):
    b0 = slot0(f.n, nb)
    o.initialize_blocks(f, nb, obs_rows)
    new = _pinned_rows(f, ref)
    f.rows[b0] = new
    f.lw[b0] = loglik_rows(o, f, new, obs_rows)
    return f


def pinned_update(o, f, nb, obs_rows, ref):
    b0 = slot0(f.n, nb)
    lw_before, incoming = f.lw[b0].copy(), f.rows[b0].copy()
    o.update_blocks(f, nb, obs_rows)
    new = _pinned_rows(f, ref, incoming)
    f.rows[b0] = new
    f.lw[b0] = lw_before + loglik_rows(o, f, new, obs_rows)
    return f


def conditional_resample(o, f, nb, ess_frac=None):
    """returns the mask of the blocks that resampled"""
    b0 = slot0(f.n, nb)
    kept = f.rows[b0].copy()
    mask = np.asarray(o.resample_blocks(f, nb, "multinomial", ess_frac=ess_frac, check=False), bool)
    f.rows[b0[mask]] = kept[mask]
    f.parents[b0[mask]] = 1
    return mask


class ConditionalLoop:
    """pinned init -> (conditional resample -> pinned update)* on one or several oracle filters.  `param_sets` / `assign`: per-block parameters (block b
    uses param_sets[assign[b]]): one oracle filter per set runs the whole loop and block b of the composed state is block b of filter assign[b] (blocks
    never interact; tests/block_params_spec.py)."""

    def __init__(self, o, model, n, nb, seed, keep_prev, param_sets=None, assign=None):
        self.o, self.n, self.nb, self.d = o, int(n), int(nb), model.dim
        self.B = (self.n + self.nb - 1) // self.nb
        sets = [model.params] if param_sets is None else param_sets
        self.assign = np.zeros(self.B, np.int64) if assign is None else np.asarray(assign, np.int64)
        self.f = [o.OracleFilter(model.model_id, np.asarray(p, np.float64), self.n, seed, keep_prev=keep_prev) for p in sets]
        self.gen = Genealogy(self.n)
        self.mask = None

    def _compose(self, attr):
        if len(self.f) == 1:
            return getattr(self.f[0], attr)
        parts = [getattr(self.f[self.assign[b]], attr)[b * self.nb:min((b + 1) * self.nb, self.n)] for b in range(self.B)]
        return np.concatenate(parts)

    rows = property(lambda self: self._compose("rows"))
    lw = property(lambda self: self._compose("lw"))
    parents = property(lambda self: self._compose("parents"))
    epoch = property(lambda self: self.f[0].epoch)

    def initialize(self, obs_rows, ref=None):
        for f in self.f:
            pinned_initialize(self.o, f, self.nb, obs_rows, ref) if ref is not None else self.o.initialize_blocks(f, self.nb, obs_rows)
        self.gen.begin_step(self.rows[:, :self.d])

    def update(self, obs_rows, ref=None):
        for f in self.f:
            pinned_update(self.o, f, self.nb, obs_rows, ref) if ref is not None else self.o.update_blocks(f, self.nb, obs_rows)
        self.gen.begin_step(self.rows[:, :self.d])

    def resample(self, ess_frac=None, conditional=True):
        masks = []
        for f in self.f:
            masks.append(conditional_resample(self.o, f, self.nb, ess_frac) if conditional else
                         np.asarray(self.o.resample_blocks(f, self.nb, "multinomial", ess_frac=ess_frac, check=False), bool))
        self.mask = np.array([masks[self.assign[b]][b] for b in range(self.B)])
        self.gen.resample("blocks", np.array(self.parents), self.mask.copy(), self.nb)     # (copies: the oracle rewrites its parents in place)
        self.gen.set_rows(self.rows[:, :self.d])
        return self.mask

    def block_stats(self):
        ess, lml = np.zeros(self.B), np.zeros(self.B)
        for b in range(self.B):
            v = self.f[self.assign[b]][b * self.nb:min((b + 1) * self.nb, self.n)]
            ess[b], lml[b] = v.effective_sample_size(), v.log_ml_estimate()
        return ess, lml

    def sample_trajectories(self, n_samples=1):
        """block_sample_trajectories (tests/block_trajectories_spec.py) at the loop's epoch, which then advances"""
        idx = draw_indices(self.o, self.lw, self.f[0].seed, self.epoch, self.nb, n_samples)
        self.gen.set_rows(self.rows[:, :self.d])
        for f in self.f:
            f.epoch += 1
        return paths(self.gen, idx, self.nb, 1, self.gen.steps, self.d)


# ----------------------------------------------------------------------------- the exact smoother of lgssm2 and the invariance experiment
INV_T, INV_B, INV_N, INV_SEED, INV_DATA_SEED, INV_REF_SEED = 4, 4096, 8, 23, 5, 99
INV_SIGMAS = 5.0


def smoother(model, ys):
    """(mu [T, 2], Sigma [2T, 2T]) of p(x_1:T | y_1:T): x_1 ~ N(0, s0^2 I), x_t+1 = A x_t + N(0, sq^2 I), y_t = x_t + N(0, sr^2 I), from the joint precision"""
    A, sq, sr, s0 = model.info["A"], model.info["sq"], model.info["sr"], model.info["s0"]
    T = len(ys)
    J, h, I = np.zeros((2 * T, 2 * T)), np.zeros(2 * T), np.eye(2)
    J[0:2, 0:2] += I / s0 ** 2
    for t in range(T):
        s = slice(2 * t, 2 * t + 2)
        J[s, s] += I / sr ** 2
        h[s] += np.asarray(ys[t]) / sr ** 2
        if t + 1 < T:
            s1 = slice(2 * t + 2, 2 * t + 4)
            J[s, s] += A.T @ A / sq ** 2
            J[s1, s1] += I / sq ** 2
            J[s, s1] += -A.T / sq ** 2
            J[s1, s] += -A / sq ** 2
    Sigma = np.linalg.inv(J)
    return (Sigma @ h).reshape(T, 2), Sigma


def invariance_setup(models):
    """(model, ys [T, 2], reference paths [B, T, 2] drawn from the exact smoother, mu, Sigma)"""
    m = models.lgssm2()
    ys = np.asarray(models.simulate(m, INV_T, seed=INV_DATA_SEED))
    mu, Sigma = smoother(m, ys)
    rng = np.random.default_rng(INV_REF_SEED)
    ref = rng.multivariate_normal(mu.ravel(), Sigma, size=INV_B).reshape(INV_B, INV_T, 2)
    return m, ys, ref, mu, Sigma


def invariance_bounds(traj, mu, Sigma, B):
    """per (t, coordinate): (|mean - mu| / sqrt(Sigma_tt / B), |var / Sigma_tt - 1| / sqrt(2 / B)) -- both must be <= INV_SIGMAS for exact draws"""
    x = np.asarray(traj).reshape(B, -1)
    sd = np.sqrt(np.diag(Sigma))
    zm = np.abs(x.mean(axis=0) - mu.ravel()) / (sd / np.sqrt(B))
    zv = np.abs(x.var(axis=0, ddof=1) / sd ** 2 - 1.0) / np.sqrt(2.0 / B)
    return zm.reshape(mu.shape), zv.reshape(mu.shape)


def invariance_run(step, models, conditional):
    """the experiment on any backend: step = (initialize(obs, ref), resample(), update(obs, ref), sample()) callables; ref is None for the plain filter"""
    m, ys, ref, mu, Sigma = invariance_setup(models)
    initialize, resample, update, sample = step
    obs = lambda t: np.tile(ys[t], (INV_B, 1))
    initialize(obs(0), ref[:, 0] if conditional else None)
    for t in range(1, INV_T):
        resample()
        update(obs(t), ref[:, t] if conditional else None)
    traj = np.asarray(sample()).reshape(INV_B, INV_T, 2)
    return invariance_bounds(traj, mu, Sigma, INV_B)
