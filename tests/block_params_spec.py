"""Expected results of per-block model parameters (gpf.h gpf_set_block_params), built from the CPU oracle only: the reference's loop over
sub-states with per-view arguments, `for b in blocks; pf_update!(state[b], new_args_b, argdiffs, observations[b]); end` (src/update.jl:12-25
on a sub-state, src/view.jl:35-48).  Block b of the device state must equal block b of an oracle filter created with the parameters of
block b -- same seed, epochs and particle ids -- so K distinct parameter sets need K oracle filters; `assign[b]` names block b's set.

Imported by tests/test_gpu_block_params.py (device vs this) and tests/test_block_params_host.py (the known-answer rehearsal)."""
from __future__ import annotations

import numpy as np

# ---- the known answer: lgssm2 log-likelihood surface over a theta grid, several replicate blocks per theta, data from one grid point.
# Fixed from the oracle rehearsal (tests/test_block_params_host.py), never from a device run: the device equals the oracle bit for bit.
KA_GRID = [(rho, sr) for rho in (0.9, 0.95, 0.99) for sr in (0.3, 0.5, 0.8)]
KA_TRUE = (0.99, 0.5)                 # the data-generating point (a grid point)
KA_DATA_SEED = 1                      # models.simulate seed: Kalman ranks KA_TRUE first by ~16 nats
KA_T, KA_REPS, KA_NB, KA_SEED = 100, 4, 2048, 29
# per theta: log-mean-exp over its replicate blocks of log_ml_estimate(state[b]) (an unbiased likelihood estimate from KA_REPS x KA_NB particles)
# within [-KA_TOL_BELOW, +KA_TOL_ABOVE] of kalman_loglik(theta).  The log of an unbiased estimate is biased low, most for the theta far from the data
# (particle degeneracy): the rehearsal's worst is -3.9 nats (rho 0.9, sr 0.5), its largest excess +0.45.
KA_TOL_BELOW, KA_TOL_ABOVE = 6.0, 1.5


def ka_setup(models):
    """(models per grid point, data ys [T, 2], assign[b] = grid index of block b, N): blocks interleave the grid points"""
    ms = [models.lgssm2(rho=r, sr=s) for r, s in KA_GRID]
    ys = np.asarray(models.simulate(models.lgssm2(rho=KA_TRUE[0], sr=KA_TRUE[1]), KA_T, seed=KA_DATA_SEED))
    B = len(KA_GRID) * KA_REPS
    assign = np.arange(B) % len(KA_GRID)
    return ms, ys, assign, B * KA_NB


def ka_summary(lml_blocks, assign, ms, ys, models):
    """per grid point: (log-mean-exp of its blocks' estimates, Kalman log-likelihood)"""
    def lme(v):
        m = np.max(v)
        return m + np.log(np.mean(np.exp(v - m)))
    est = np.array([lme(np.asarray(lml_blocks)[assign == k]) for k in range(len(ms))])
    exact = np.array([models.kalman_loglik(m, ys) for m in ms])
    return est, exact


class ParamBlocksOracle:
    """K oracle filters, filter k created with param_sets[k]; block b of the composed state is block b of filter assign[b].

    own_only = False: every filter runs the repository's block helpers (oracle.initialize_blocks / update_blocks / resample_blocks /
    rejuvenate_blocks) over ALL its blocks.  own_only = True: each filter steps only the blocks assigned to it -- the same loops
    restricted to those blocks; blocks never interact, so the composed state is the same at 1/K of the work (checked by
    tests/test_block_params_host.py)."""

    def __init__(self, o, model_id, param_sets, assign, N, nb, seed, keep_prev=True, own_only=False):
        self.o, self.N, self.nb = o, int(N), int(nb)
        self.assign = np.asarray(assign)
        self.B = (self.N + self.nb - 1) // self.nb
        assert self.assign.shape == (self.B,)
        self.f = [o.OracleFilter(model_id, np.asarray(p, np.float64), N, seed, keep_prev=keep_prev) for p in param_sets]
        self.own_only = own_only

    def _range(self, b):
        return b * self.nb, min((b + 1) * self.nb, self.N)

    def _own(self, k):
        return np.flatnonzero(self.assign == k)

    def initialize(self, obs_rows, strata=None, layout="contiguous"):
        for k, f in enumerate(self.f):
            if not self.own_only:
                self.o.initialize_blocks(f, self.nb, obs_rows, strata=strata, layout=layout)
                continue
            lib = self.o.lib()
            for b in self._own(k):                                   # oracle.initialize_blocks restricted to the own blocks
                a, e = self._range(b)
                rows, lw = np.zeros((e - a, f.W)), np.zeros(e - a)
                ob = np.ascontiguousarray(obs_rows[b], np.float64)
                if strata is not None:
                    v = np.ascontiguousarray(strata, np.float64)
                    lib.o_init_strata(f.model, f.params, f.seed, f.epoch, a, e - a, f.W, ob, v, v.size, int(layout != "contiguous"),
                                      self.o.olog(float(v.size)), rows, lw)
                else:
                    lib.o_init(f.model, f.params, f.seed, f.epoch, a, e - a, f.W, ob, rows, lw)
                f.rows[a:e] = rows; f.lw[a:e] = lw
            f.lml_est = 0.0; f.parents = np.arange(1, f.n + 1, dtype=np.int64)
            f.epoch += 1; f.has_prev = False
        return self

    def update(self, obs_rows, proposals=None, strata=None, layout="interleaved"):
        for k, f in enumerate(self.f):
            if not self.own_only:
                self.o.update_blocks(f, self.nb, obs_rows, proposals=proposals, strata=strata, layout=layout)
                continue
            e0 = f.epoch
            for b in self._own(k):                                   # oracle.update_blocks restricted to the own blocks
                a, e = self._range(b)
                f.epoch = e0
                ob = np.asarray(obs_rows[b], np.float64)
                if strata is not None:
                    f[a:e].update(ob, strata=strata, layout=layout)
                else:
                    f[a:e].update(ob, proposal=bool(proposals[b]) if proposals is not None else False)
            f.epoch = e0 + 1
        return self

    def resample(self, method="residual", ess_frac=None):
        """the blocks that resampled (bool per block)"""
        mask = np.zeros(self.B, bool)
        for k, f in enumerate(self.f):
            own = self._own(k)
            if not self.own_only:
                mk = self.o.resample_blocks(f, self.nb, method, ess_frac=ess_frac)
                mask[own] = mk[own]
                continue
            e0 = f.epoch
            for b in own:                                            # oracle.resample_blocks restricted to the own blocks
                a, e = self._range(b)
                v = f[a:e]
                f.epoch = e0
                go = ess_frac is None or v.effective_sample_size() < ess_frac * v.n
                if go:
                    v.resample(method, check=False)
                mask[b] = go
            f.epoch = e0 + 1
        return mask

    def rejuvenate(self, obs_rows, method="move", mask=None, n_iters=1):
        """the accepted moves over the blocks that took part"""
        acc = 0
        for k, f in enumerate(self.f):
            mk = self.assign == k
            if mask is not None:
                mk = mk & np.asarray(mask, bool)
            acc += self.o.rejuvenate_blocks(f, self.nb, obs_rows, method, mask=mk, n_iters=n_iters)   # (a block outside mk is skipped)
        return acc

    def _compose(self, attr):
        parts = []
        for b in range(self.B):
            a, e = self._range(b)
            parts.append(getattr(self.f[self.assign[b]], attr)[a:e])
        return np.concatenate(parts)

    @property
    def rows(self):
        return self._compose("rows")

    @property
    def lw(self):
        return self._compose("lw")

    @property
    def parents(self):
        return self._compose("parents")

    def block_lml(self):
        return np.array([self.f[self.assign[b]][slice(*self._range(b))].log_ml_estimate() for b in range(self.B)])

    def block_ess(self):
        return np.array([self.f[self.assign[b]][slice(*self._range(b))].effective_sample_size() for b in range(self.B)])


def ka_oracle(o, models):
    """the known-answer run on the oracle: init, then T - 1 x (update with the locally optimal proposal in every block -- its constants are the
    block's own -- -> residual resample at ESS < N/2); per-block log-ML estimates"""
    ms, ys, assign, N = ka_setup(models)
    B = assign.size
    ref = ParamBlocksOracle(o, ms[0].model_id, [m.params for m in ms], assign, N, KA_NB, KA_SEED, keep_prev=False, own_only=True)
    ref.initialize(np.tile(ys[0], (B, 1)))
    for t in range(1, KA_T):
        ref.update(np.tile(ys[t], (B, 1)), proposals=np.ones(B, bool))
        ref.resample("residual", ess_frac=0.5)
    return ref.block_lml(), assign, ms, ys
