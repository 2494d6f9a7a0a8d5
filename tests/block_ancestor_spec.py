"""Ancestor sampling for conditional SMC per block (gpf.h gpf_resample_blocks_ancestor, gpf_block_ancestor_log_weights; Lindsten, Jordan & Schoen 2014,
"Particle Gibbs with ancestor sampling", JMLR 15), restated on the CPU:

  logtrans               Model<M>::logtrans of csrc/gpf_models.hpp in NumPy float64, one operation per rounding, in the header's order: log f(x | xp) minus
                         the terms that do not depend on xp
  ancestor_log_weights   lwa_i = lw_i + logtrans(P_b, row_i[0..d), ref_b, obs_b), b = i // nb
  ancestor_resample      the conditional resample of tests/block_conditional_spec.py runs as it is; in every block that resampled, slot 0 is patched
                         afterwards: s = WeightSummary(lwa of the block), a0 = upper_bound(s.cdf, slot 0's own multinomial target of the call's epoch
                         scaled by s.S) -- 0 where the flags of lwa are bad or all -Inf -- and slot 0's row becomes the pre-call row a0, its parent a0 + 1

`AncestorLoop` runs pinned init -> (ancestor resample -> pinned update)* in lockstep with the device, genealogy included; `invariance_run` is the
exact-smoother experiment at T = 8 (the existing T = 4 cannot tell a wrong ancestor density from a right one).

Helper module, no tests."""
import numpy as np

import block_conditional_spec as cs

NAMES = {1: "lgssm2", 2: "bearings4", 3: "sv1", 4: "object_motion", 5: "line_model"}


def logtrans(name, P, xp, x, obs):
    """xp: [n, d] (or [d]) previous latents, x: [d] the next value, obs: the data vector of the step being entered -> [n]"""
    P, x, obs = np.asarray(P, np.float64), np.asarray(x, np.float64), np.asarray(obs, np.float64)
    xp = np.atleast_2d(np.asarray(xp, np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        if name == "lgssm2":
            t0 = P[0] * xp[:, 0] + P[1] * xp[:, 1]
            t1 = P[2] * xp[:, 0] + P[3] * xp[:, 1]
            a0 = (x[0] - t0) * P[12]
            a1 = (x[1] - t1) * P[12]
            return -0.5 * (a0 * a0 + a1 * a1)
        if name == "sv1":
            mean = P[0] + P[1] * (xp[:, 0] - P[0])
            z = (x[0] - mean) / P[2]
            return -0.5 * (z * z)
        if name == "bearings4":
            z0 = (x[0] - (xp[:, 0] + xp[:, 2])) / P[8]
            z1 = (x[1] - (xp[:, 1] + xp[:, 3])) / P[8]
            z2 = (x[2] - xp[:, 2]) / P[9]
            z3 = (x[3] - xp[:, 3]) / P[9]
            return -0.5 * ((z0 * z0 + z1 * z1) + (z2 * z2 + z3 * z3))
        if name == "object_motion":
            mv, pm = x[0] != 0, xp[:, 0] != 0
            lp = np.where(pm, P[5] if mv else P[6], P[7] if mv else P[8])
            vel = obs[1] if mv else 0.0
            z = (x[1] - (xp[:, 1] + vel)) / P[2]
            return lp + (-0.5 * (z * z))
        if name == "line_model":
            return np.where(xp[:, 0] == x[0], 0.0, -np.inf)
    raise ValueError(name)


def ancestor_log_weights(name, P, lw, rows, nb, obs, ref, d):
    """P: the filter's parameter vector, or [n_blocks, n_params] rows (per-block parameters)"""
    lw, rows, P = np.asarray(lw, np.float64), np.asarray(rows, np.float64), np.asarray(P, np.float64)
    out = np.empty(lw.size)
    with np.errstate(invalid="ignore"):
        for b, lo in enumerate(range(0, lw.size, nb)):
            hi = min(lo + nb, lw.size)
            out[lo:hi] = lw[lo:hi] + logtrans(name, P[b] if P.ndim == 2 else P, rows[lo:hi, :d], ref[b], obs[b])
    return out


def ancestor_resample(o, f, nb, obs, ref, ess_frac=None, density=True):
    """returns (mask of the blocks that resampled, a0 per block -- 0 where the block did not resample).  density=False: the ancestor of slot 0 is drawn
    in proportion to w alone (logtrans = 0) -- NOT a valid kernel, the negative control of the invariance experiment"""
    rows_in = f.rows.copy()
    lwa = ancestor_log_weights(NAMES[f.model], f.params, f.lw, f.rows, nb, obs, ref, f.d) if density else f.lw.copy()
    epoch = f.epoch
    mask = cs.conditional_resample(o, f, nb, ess_frac)
    a0 = np.zeros(mask.size, np.int64)
    for b in np.flatnonzero(mask):
        lo, hi = b * nb, min((b + 1) * nb, f.n)
        s = o.WeightSummary(np.ascontiguousarray(lwa[lo:hi]), hi - lo)
        if not (s.bad or s.uniform):
            a0[b] = int(o.upper_bound(s.cdf, o.targets_multinomial(f.seed, epoch, lo, 1, s.S))[0])
        f.rows[lo] = rows_in[lo + a0[b]]
        f.parents[lo] = a0[b] + 1
    return mask, a0


class AncestorLoop(cs.ConditionalLoop):
    """pinned init -> (ancestor resample -> pinned update)*; `resample` takes the data and reference of the step being entered"""

    def resample(self, obs_rows, ref, ess_frac=None, density=True):
        res = [ancestor_resample(self.o, f, self.nb, obs_rows, ref, ess_frac, density) for f in self.f]
        self.mask = np.array([res[self.assign[b]][0][b] for b in range(self.B)])
        self.a0 = np.array([res[self.assign[b]][1][b] for b in range(self.B)])
        self.gen.resample("blocks", np.array(self.parents), self.mask.copy(), self.nb)
        self.gen.set_rows(self.rows[:, :self.d])
        return self.mask


# ----------------------------------------------------------------------------- the invariance experiment at T = 8
INV_T = 8


def invariance_setup(models):
    """(model, ys [T, 2], reference paths [B, T, 2] drawn from the exact smoother, mu, Sigma): block_conditional_spec's setup and seeds at T = 8"""
    m = models.lgssm2()
    ys = np.asarray(models.simulate(m, INV_T, seed=cs.INV_DATA_SEED))
    mu, Sigma = cs.smoother(m, ys)
    rng = np.random.default_rng(cs.INV_REF_SEED)
    ref = rng.multivariate_normal(mu.ravel(), Sigma, size=cs.INV_B).reshape(cs.INV_B, INV_T, 2)
    return m, ys, ref, mu, Sigma


def invariance_run(step, models):
    """step = (initialize(obs, ref), resample(obs, ref), update(obs, ref), sample()): pinned initialise, (ancestor resample, pinned update) x 7, one
    trajectory per block.  Returns (z of the means, z of the variances, share of blocks whose x_1 is no longer the reference's)"""
    m, ys, ref, mu, Sigma = invariance_setup(models)
    initialize, resample, update, sample = step
    obs = lambda t: np.tile(ys[t], (cs.INV_B, 1))
    initialize(obs(0), ref[:, 0])
    for t in range(1, INV_T):
        resample(obs(t), ref[:, t])
        update(obs(t), ref[:, t])
    traj = np.asarray(sample()).reshape(cs.INV_B, INV_T, 2)
    zm, zv = cs.invariance_bounds(traj, mu, Sigma, cs.INV_B)
    return zm, zv, float(np.mean(np.any(traj[:, 0] != ref[:, 0], axis=1)))
