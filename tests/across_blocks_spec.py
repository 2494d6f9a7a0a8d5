"""Expected results of resampling ACROSS blocks (gpf.h gpf_resample_across_blocks), composed from the CPU oracle only: every block of an
OracleFilter is one super-particle with the log-weight log_ml_estimate(state[b]) (OracleSubState), a planner OracleFilter of B particles with
the filter's seed and epoch resamples them (src/resample.jl:19-175 one level up), whole blocks are copied in NumPy:

    rows'[b bs + i] = rows[a bs + i],  lw'[b bs + i] = lw[a bs + i] + (M - L[a]),  parents'[b bs + i] = a bs + i + 1,   a = A[b].

The device must equal this bit for bit (tests/test_gpu_across_blocks.py); the real-arithmetic properties -- mass conservation, every block's
estimate = M afterwards -- are checked against mpmath within the bound derived below (tests/test_across_blocks_host.py).  Helper module, no tests."""
from __future__ import annotations

import math

import numpy as np

import block_params_spec as bp

METHODS = ("multinomial", "residual", "stratified")


# ------------------------------------------------------------------------------------------- the plan and the copy
def block_logweights(f, bs: int) -> np.ndarray:
    """L[b] = log_ml_estimate(state[b]): log_ml_est + logsumexp(block b) - log(block_size), the double block_stats reports"""
    assert f.n % bs == 0
    return np.array([f[a:a + bs].log_ml_estimate() for a in range(0, f.n, bs)])


class Plan:
    """ess, M, A (0-based), invalid of the planner: an OracleFilter of B particles (its model and rows are unused) with log-weights L,
    log_ml_est = 0, gid0 = 0, the given seed and RNG epoch.  resample = False: ess and M only (the gate did not fire)."""

    def __init__(self, o, model_id, params, L, seed, epoch, method, sort_particles=True, check="warn", resample=True):
        L = np.ascontiguousarray(L, np.float64)
        self.L, self.B = L, L.size
        if np.isnan(L).any() or (L == np.inf).any():
            raise o.OracleError("Invalid weights (NaN).")              # a block with NaN / +Inf weights: refused whatever `check` says
        self.invalid = bool((L == -np.inf).all())
        if self.invalid and check is True:
            raise o.OracleError("Invalid weights.")
        p = o.OracleFilter(model_id, params, self.B, seed)
        p.lw = L.copy(); p.epoch = int(epoch)
        self.ess = p.effective_sample_size()
        self.M = p.log_ml_estimate()
        self.A = None
        if resample:
            p.resample(method, sort_particles=sort_particles, check=False)
            self.A = p.parents - 1
        with np.errstate(invalid="ignore"):
            self.delta = np.where(L == -np.inf, 0.0, self.M - L)     # once per source block, in double


def gate(ess: float, ess_frac, B: int) -> bool:
    """ess_frac None / NaN / < 0: always; else ess < ess_frac * B (a NaN ESS -- all -Inf -- does not fire, like the reference's `<`)"""
    if ess_frac is None or ess_frac != ess_frac or ess_frac < 0:
        return True
    return bool(ess < ess_frac * B)


def copy_blocks(rows, lw, A, delta, bs):
    """(rows', lw', parents') of the block copy"""
    src = (np.asarray(A, np.int64)[:, None] * bs + np.arange(bs)[None, :]).ravel()
    with np.errstate(invalid="ignore"):
        return rows[src].copy(), lw[src] + np.repeat(np.asarray(delta)[A], bs), src + 1


def resample_across_blocks(o, f, bs: int, method: str = "multinomial", ess_frac=None, sort_particles: bool = True, check="warn"):
    """the call on an OracleFilter, in place.  Returns the Plan (A = None when the gate did not fire; .resampled says which).  Refusals raise
    and change nothing; an accepted call advances the epoch once."""
    if method not in METHODS:
        raise o.OracleError(f"Resampling method {method} not recognized.")
    if bs < 1 or f.n % bs != 0:
        raise o.OracleError("blocks must be congruent")
    L = block_logweights(f, bs)
    plan = Plan(o, f.model, f.params, L, f.seed, f.epoch, method, sort_particles, check, resample=False)
    plan.resampled = gate(plan.ess, ess_frac, plan.B)
    if plan.resampled:
        plan = Plan(o, f.model, f.params, L, f.seed, f.epoch, method, sort_particles, check)
        plan.resampled = True
        f.rows, f.lw, f.parents = copy_blocks(f.rows, f.lw, plan.A, plan.delta, bs)
    f.epoch += 1
    return plan


def resample_across_param_blocks(ref: bp.ParamBlocksOracle, method: str = "multinomial", ess_frac=None, sort_particles: bool = True, check="warn"):
    """the same on the composed state of block_params_spec.ParamBlocksOracle: block b then carries the parameters of block A[b], so it moves
    into the oracle filter of that parameter set -- `assign` becomes `assign[A]`.  The per-block observations travel the same way: the caller
    passes obs_rows[A] to the next rejuvenate."""
    o, bs, f0 = ref.o, ref.nb, ref.f[0]
    assert ref.N % bs == 0 and all(f.epoch == f0.epoch and f.lml_est == f0.lml_est for f in ref.f)
    L = ref.block_lml()
    plan = Plan(o, f0.model, f0.params, L, f0.seed, f0.epoch, method, sort_particles, check, resample=False)
    plan.resampled = gate(plan.ess, ess_frac, plan.B)
    if plan.resampled:
        plan = Plan(o, f0.model, f0.params, L, f0.seed, f0.epoch, method, sort_particles, check)
        plan.resampled = True
        rows, lw, parents = copy_blocks(ref.rows, ref.lw, plan.A, plan.delta, bs)
        ref.assign = ref.assign[plan.A]
        for b in range(ref.B):
            fk, (a, e) = ref.f[ref.assign[b]], ref._range(b)
            fk.rows[a:e] = rows[a:e]; fk.lw[a:e] = lw[a:e]; fk.parents[a:e] = parents[a:e]
    for f in ref.f:
        f.epoch += 1
    return plan


# ------------------------------------------------------------------------------------------- test states with uneven block weights
def block_data(models, m, B, T, seed=7):
    """ys[b][t]: a perturbed copy of one simulated sequence per block"""
    base = np.asarray(models.simulate(m, T))
    return base[None, :, :] + 0.3 * np.random.default_rng(seed).standard_normal((B,) + base.shape)


def uneven_oracle(o, m, ys, N, bs, seed, keep_prev=True):
    """an OracleFilter after a block-wise initialisation and len(ys[0]) - 1 block-wise updates, every block on its own data"""
    f = o.OracleFilter(m.model_id, m.params, N, seed, keep_prev=keep_prev)
    o.initialize_blocks(f, bs, ys[:, 0])
    for t in range(1, ys.shape[1]):
        o.update_blocks(f, bs, ys[:, t])
    return f


# ------------------------------------------------------------------------------------------- the bound of the real-arithmetic properties
# In real arithmetic the copy conserves the whole filter's mass and gives every block the mass M + log bs - log_ml_est:
#     l_b = logsumexp(block b),  L_b = lml + l_b - log bs,  M = logsumexp(L) - log B,  new block b: l_a + (M - L_a) = M + log bs - lml,
#     logsumexp over the B new blocks = log B + M + log bs - lml = logsumexp(L) + log bs - lml = logsumexp(all lw).
# The spec computes L, M, delta and lw + delta in Float64 and fixed point.  With U = 2^-53 (one correctly rounded operation, relative):
#     lam_b: |L_b - (lml + l_b - log bs)| <= e_b + U (|lml + lse_b| + |L_b|) + 4 U log bs
#            e_b = the bound of hp_weights.Softmax(block b).lse(): the K-bit quantisation D / S of the block's weights (K = fix_K(bs)),
#            the conversion of S and log_'s 2 ulp; then the two Float64 operations of `(lml + lse) - log_(bs)` and log_(bs)'s own 2 ulp
#     mu:    |M - (logsumexp(L) - log B)| <= e_P + U (|lse_P| + |M|) + 4 U log B          the same for the planner's B weights (K = fix_K(B))
#     eta_a: |delta_a - (M - L_a)| <= U |delta_a|                                           the subtraction
#     eps_p: |lw'_p - (lw_p + delta_a)| <= U |lw'_p|                                        the addition
# A block's new mass is l_a + delta_a up to max eps; delta_a = M - L_a + eta_a; L_a = lml + l_a - log bs + lam_a; logsumexp(L) is within
# max lam of T + lml - log bs, T = logsumexp(all lw before).  So for every new block b
#     |mass'_b - (T - log B)| <= 2 max lam + mu + max eta + max eps,
# hence the same for |logsumexp(all lw after) - T|; and M itself is within max lam + mu of T - log B + lml - log bs, so the block estimate after
# the call, lml + mass'_b - log bs in real arithmetic, is within 3 max lam + 2 mu + max eta + max eps of M.  ONE bound serves both checks:
#     BOUND = 3 max lam + 2 mu + max eta + max eps.
# (The estimate the spec REPORTS afterwards adds the lam' of its own evaluation on the new weights.)  Nothing here is fitted to an output.
U = 2.0 ** -53


def lam_of(lw, L, bs, lml_est=0.0) -> float:
    """max_b lam_b for the blocks of `lw` whose reported estimates are L"""
    import hp_weights as hw
    lam = 0.0
    for b in range(len(L)):
        if not np.isfinite(L[b]):
            continue                                                  # an all -Inf block: L = -Inf exactly, mass 0
        lse = hw.Softmax(lw[b * bs:(b + 1) * bs]).lse()
        lam = max(lam, lse.e + U * (abs(lml_est + float(lse.v)) + abs(L[b])) + 4 * U * math.log(max(bs, 2)))
    return lam


def property_bound(L_before, M, delta, lw_before, lw_after, bs, lml_est=0.0) -> float:
    """BOUND of the derivation above, from mpmath enclosures of the spec's fixed-point logsumexp (hp_weights.Softmax.lse)"""
    import hp_weights as hw
    B = len(L_before)
    lam = lam_of(lw_before, L_before, bs, lml_est)
    lseP = hw.Softmax(L_before).lse()
    mu = lseP.e + U * (abs(float(lseP.v)) + abs(M)) + 4 * U * math.log(max(B, 2))
    delta, lw_after = np.asarray(delta), np.asarray(lw_after)
    eta = U * float(np.max(np.abs(delta[np.isfinite(delta)]), initial=0.0))
    eps = U * float(np.max(np.abs(lw_after[np.isfinite(lw_after)]), initial=0.0))
    return 3 * lam + 2 * mu + eta + eps


def mp_logsumexp(v):
    """logsumexp of a Float64 vector in mpmath (hp_reference precision)"""
    import hp_reference as hp
    v = [float(x) for x in v if x != -np.inf]
    if not v:
        return -hp.M.inf
    m = max(v)
    return hp.mpf(m) + hp.M.log(hp.M.fsum([hp.M.exp(hp.mpf(x) - hp.mpf(m)) for x in v]))


# ------------------------------------------------------------------------------------------- the known answer: an adaptive theta grid (SMC^2's outer level)
# block_params_spec's grid (9 theta x 4 replicate blocks of lgssm2, data from KA_TRUE), smaller blocks and fewer steps so that the oracle rehearsal
# takes seconds.  Loop: block-wise update with the locally optimal proposal -> residual resample inside the blocks at ESS < nb / 2 -> resample
# ACROSS the blocks at ESS < B / 2, theta following A.  The whole filter's log_ml_estimate then estimates the grid evidence
# log mean_k exp(kalman_loglik(theta_k)).  Fixed from the oracle rehearsal (tests/test_across_blocks_host.py), never from a device run: the
# device equals the oracle bit for bit.
XKA_T, XKA_NB, XKA_SEED = 30, 512, 29
XKA_METHOD = "stratified"
# whole-filter estimate - exact grid evidence, within [-XKA_TOL_BELOW, +XKA_TOL_ABOVE]: the log of an unbiased estimate is biased low (Jensen), so
# the band is asymmetric.  Rehearsal (oracle, seeds 29..36): -0.815 at the recorded seed 29; worst below -0.815, largest excess +0.462; the
# data-generating theta holds 23..36 of the 36 blocks at the end, 24 at seed 29; 2..4 of the 29 outer calls fire.  Margins as
# block_params_spec.KA_TOL_BELOW / KA_TOL_ABOVE: about 1.5 x the worst shortfall below, 2..3 x the largest excess above.
XKA_TOL_BELOW, XKA_TOL_ABOVE = 1.5, 1.0


def xka_setup(models):
    ms = [models.lgssm2(rho=r, sr=s) for r, s in bp.KA_GRID]
    ys = np.asarray(models.simulate(models.lgssm2(rho=bp.KA_TRUE[0], sr=bp.KA_TRUE[1]), XKA_T, seed=bp.KA_DATA_SEED))
    B = len(bp.KA_GRID) * bp.KA_REPS
    assign = np.arange(B) % len(bp.KA_GRID)
    return ms, ys, assign, B * XKA_NB


def xka_evidence(ms, ys, models) -> float:
    ll = np.array([models.kalman_loglik(m, ys) for m in ms])
    return float(ll.max() + np.log(np.mean(np.exp(ll - ll.max()))))


def xka_oracle(o, models, seed=XKA_SEED):
    """(whole-filter log_ml_estimate, final assign, the composed oracle, ms, ys, the plans) of the rehearsal"""
    ms, ys, assign, N = xka_setup(models)
    B = assign.size
    ref = bp.ParamBlocksOracle(o, ms[0].model_id, [m.params for m in ms], assign, N, XKA_NB, seed, keep_prev=False, own_only=True)
    ref.initialize(np.tile(ys[0], (B, 1)))
    plans = []
    for t in range(1, XKA_T):
        ref.update(np.tile(ys[t], (B, 1)), proposals=np.ones(B, bool))
        ref.resample("residual", ess_frac=0.5)
        plans.append(resample_across_param_blocks(ref, XKA_METHOD, ess_frac=0.5))
    whole = o.OracleFilter(ms[0].model_id, ms[0].params, N, seed)   # log_ml_estimate(state) of the composed state, in the library's fixed point
    whole.lw = ref.lw; whole.lml_est = ref.f[0].lml_est
    est = whole.log_ml_estimate()
    return est, ref.assign.copy(), ref, ms, ys, plans
