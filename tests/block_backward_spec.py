"""Backward simulation per block (gpf.h gpf_block_backward_sample; FFBSi, Godsill, Doucet & West 2004), restated in NumPy from what a caller sees:

  Store       per step s (1-based): x[s] the latent columns and lw[s] the log-weights in the step's FINAL order -- read back after the step's last call
              (history_column(s, c) of the then current step, state.log_weights) --, obs[s] the per-block observation rows the step was entered with in
              the block order of that moment (a resample across blocks moves them with its block ancestors), and the resamples of the step as
              tests/block_history_spec.py records them (state.parents, block_resampled, block_ancestors).  Nothing is read from the device's store.
  backward    draw j of block b, slot = b n_samples + j, T steps, E the epoch of the call:
                step T   block_trajectories_spec.draw_indices: WeightSummary of the block's current weights, targets_multinomial at epoch E, upper_bound;
                step s   = T-1 .. lo: p the held particle of step s + 1, pm = g_{s+1}[p] its recorded parent (the step's composed resample maps), c = pm //
                         bs; lwa = lw[s][block c] + logtrans(P_b, x[s][block c], x[s+1][p], obs[s+1][p // bs]) (block_ancestor_spec.logtrans);
                         WeightSummary(lwa, particles of block c); target = targets_multinomial at epoch E + (T - s) of the same slot; a = upper_bound;
                         p = c bs + a -- or pm where the summary is bad or all -Inf.
              Returns traj [B, n_samples, hi - lo + 1, d] and the 1-based global indices [B, n_samples, hi - lo + 1]; a block with NaN / +Inf weights: 0, NaN.
  StoreLoop   the plain block-wise filter on the CPU oracle (block_conditional_spec.ConditionalLoop without a reference) feeding a Store: the host tests'
              filter.

The oracle's pieces are test infrastructure only.  Helper module, no tests."""
import numpy as np

import block_conditional_spec as cs
from block_ancestor_spec import logtrans
from block_history_spec import Genealogy, resample_map


class Store:
    def __init__(self, n, block_size, d):
        self.n, self.bs, self.d = int(n), min(int(block_size), int(n)), int(d)
        self.gen = Genealogy(self.n)
        self.lw, self.obs = [], []

    steps = property(lambda self: self.gen.steps)
    B = property(lambda self: (self.n + self.bs - 1) // self.bs)

    def begin_step(self, obs_rows):
        """pf_initialize_blocks / pf_update_blocks returned; obs_rows = None: a whole-filter call"""
        self.gen.begin_step(np.zeros((self.n, self.d)))
        self.lw.append(None)
        self.obs.append(None if obs_rows is None else np.array(obs_rows, np.float64).reshape(self.B, -1))

    def resample_blocks(self, parents, block_resampled):
        self.gen.resample("blocks", np.array(parents), np.array(block_resampled, bool), self.bs)

    def resample_across(self, parents, block_ancestors):
        """pf_resample_across_blocks fired: global parents; the step's observation rows move with the blocks"""
        self.gen.resample("global", np.array(parents))
        self.obs[-1] = self.obs[-1][np.asarray(block_ancestors, np.int64) - 1]

    def resample_global(self, parents):
        self.gen.resample("global", np.array(parents))

    def end_step(self, x, lw):
        """after the step's last call: its latent columns [n, d] and log-weights in their final order"""
        self.gen.set_rows(np.asarray(x, np.float64).reshape(self.n, self.d))
        self.lw[-1] = np.array(lw, np.float64)

    def x(self, s):
        return self.gen.rows[s - 1]

    def step_map(self, s):
        """g_s[p]: the particle of step s - 1's final order that particle p of step s's final order was copied from"""
        idx = np.arange(self.n, dtype=np.int64)
        for ev in reversed(self.gen.events[s - 1]):
            idx = resample_map(ev, self.n)[idx]
        return idx


def backward(o, name, P, store, seed, epoch, n_samples, lo=1, hi=None, trans=True):
    """trans=False: logtrans = 0 (independent categorical draws per step where every block resampled: the reduction the host test checks)"""
    T, bs, n, d, B = store.steps, store.bs, store.n, store.d, store.B
    hi = T if hi is None else hi
    assert 1 <= lo <= hi <= T
    P = np.asarray(P, np.float64)
    ns = int(n_samples)
    traj = np.full((B, ns, hi - lo + 1, d), np.nan)
    idx = np.zeros((B, ns, hi - lo + 1), np.int64)
    maps = {s: store.step_map(s) for s in range(lo + 1, T + 1)}
    lwT = np.ascontiguousarray(store.lw[T - 1])
    for b in range(B):
        b0, b1 = b * bs, min((b + 1) * bs, n)
        Pb = P[b] if P.ndim == 2 else P
        ws = o.WeightSummary(np.ascontiguousarray(lwT[b0:b1]), b1 - b0)
        if ws.bad:
            continue
        p = b0 + o.upper_bound(ws.cdf, o.targets_multinomial(int(seed), int(epoch), b * ns, ns, ws.S)).astype(np.int64)
        for s in range(T, lo - 1, -1):                                        # p: the held particles of step s, one per draw
            if s <= hi:
                traj[b, :, s - lo] = store.x(s)[p]
                idx[b, :, s - lo] = p + 1
            if s == lo:
                break
            pm = maps[s][p]
            new = pm.copy()
            for held in np.unique(p):                                         # (the draws that hold the same particle share their ancestor weights)
                sel = p == held
                par = int(pm[sel][0])
                c0 = par // bs * bs
                c1 = min(c0 + bs, n)
                lwa = store.lw[s - 2][c0:c1].copy()
                if trans:
                    with np.errstate(invalid="ignore"):
                        lwa = lwa + logtrans(name, Pb, store.x(s - 1)[c0:c1], store.x(s)[held], store.obs[s - 1][held // bs])
                wa = o.WeightSummary(np.ascontiguousarray(lwa), c1 - c0)
                if wa.bad or wa.uniform:
                    continue                                                  # the recorded parent
                t_all = o.targets_multinomial(int(seed), int(epoch) + (T - (s - 1)), b * ns, ns, wa.S)
                new[sel] = c0 + o.upper_bound(wa.cdf, np.ascontiguousarray(t_all[sel]))
            p = new
    return traj, idx


class StoreLoop:
    """initialise -> (resample blocks -> update)* of the plain block-wise filter on the CPU oracle, recorded into a Store"""

    def __init__(self, o, model, n, bs, seed, keep_prev=False, param_sets=None, assign=None):
        self.L = cs.ConditionalLoop(o, model, n, bs, seed, keep_prev, param_sets=param_sets, assign=assign)
        self.store = Store(n, bs, model.dim)
        self.d = model.dim

    def _end(self):
        self.store.end_step(self.L.rows[:, :self.d], self.L.lw)

    def initialize(self, obs_rows):
        self.L.initialize(obs_rows)
        self.store.begin_step(obs_rows)
        self._end()

    def resample(self, ess_frac=None):
        mask = self.L.resample(ess_frac, conditional=False)
        self.store.resample_blocks(self.L.parents, mask)
        self._end()
        return mask

    def update(self, obs_rows):
        self.L.update(obs_rows)
        self.store.begin_step(obs_rows)
        self._end()

    epoch = property(lambda self: self.L.epoch)
    seed = property(lambda self: self.L.f[0].seed)


# ----------------------------------------------------------------------------- the law experiment: lgssm2, T = 8, against the exact smoother
# Seeds: those of the sibling experiments (block_conditional_spec), not chosen here.  FFBSi is consistent, not unbiased: the first update leaves a block
# about 5 % of its particles' worth of effective sample size (s0 = 1 against sr = 0.5, sq = 0.1), and the smoothed variance of step 1 is inflated by a bias
# of order 1 / N.  The restatement's worst unit on the CPU oracle's filter (tests/test_block_backward_host.py) at 64 / 128 / 256 particles per block:
# 28.2 / 13.3 / 4.19 -- so 256, the smallest of the three inside the bound of 5.
LAW_T, LAW_B, LAW_SEED, LAW_DATA_SEED = 8, 1024, cs.INV_SEED, cs.INV_DATA_SEED
LAW_N = 256


def law_setup(models):
    m = models.lgssm2()
    ys = np.asarray(models.simulate(m, LAW_T, seed=LAW_DATA_SEED))
    mu, Sigma = cs.smoother(m, ys)
    return m, ys, mu, Sigma


def law_units(traj, mu, Sigma):
    """(|mean - mu| in standard errors, |var / Sigma_tt - 1| in units of sqrt(2 / B)) of one path per block, pooled over the blocks"""
    return cs.invariance_bounds(np.asarray(traj).reshape(LAW_B, LAW_T, 2), mu, Sigma, LAW_B)
