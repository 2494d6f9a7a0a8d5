"""Pairwise smoothing per block (gpf.h gpf_block_smooth_pairs), restated in NumPy from what a caller sees -- the Store of
tests/block_backward_spec.py, as tests/block_smooth_spec.py, whose walk this is (block_smooth_spec.walk with pair_sums=True):

  pairs       block b, T steps: c = b, W = q / S of the block's current WeightSummary; then for s = T .. lo + 1 the lineage check, and for every target j
              of block c in step s, one at a time in ASCENDING order:  W[j] == 0: the target is skipped entirely.  Otherwise lwa, (m, f), q, D and r as
              block_smooth_spec.smooth (r = the indicator of the recorded parent where f != 0), then
                  t = W[j] * r;    acc = acc + t;    A[:, c] = A[:, c] + t * x_s[j][c]   for every latent column c
              (one multiply, one add).  W = acc, c = cp.  Written for the steps in [lo, hi]:
                  mean_s[c]      = tree(W x[:, c])                                   (block_smooth_spec.moments' mean)
                  second_s[a][c] = tree((W x[:, a]) x[:, c])  for a <= c, mirrored
                  cross_s[a][c]  = tree(x_s[:, a] A[:, c])    for the pair (s, s + 1), s + 1 <= hi, with A of the walk from s + 1 to s
              with the tree of DESIGN.md 3.5 (block_smooth_spec.tree_sum).
  Returns mean [B, ns, d], second [B, ns, d, d], cross [B, ns - 1, d, d], the 1-based lineage blocks [B, ns]; with return_A=True also the dictionary
  (b, s) -> A [particles of block c_s, d] of every walked pair.  NaN / 0 where gpf.h says so.

The oracle's pieces (max_flags, fixq, fix_K, WeightSummary) are test infrastructure only.  Helper module, no tests."""
import numpy as np

import block_backward_spec as bsp
import block_conditional_spec as cs
from block_smooth_spec import tree_sum, walk


def second_of(w, x):
    d = x.shape[1]
    out = np.empty((d, d))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(d):
            for c in range(a, d):
                out[a, c] = out[c, a] = tree_sum((w * x[:, a]) * x[:, c])
    return out


def cross_of(x, A):
    d = x.shape[1]
    out = np.empty((d, d))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(d):
            for c in range(d):
                out[a, c] = tree_sum(x[:, a] * A[:, c])
    return out


def pairs(o, name, P, store, lo=1, hi=None, trans=True, fallback=False, return_A=False, skip=True):
    """trans, fallback, skip: as block_smooth_spec.walk"""
    hi = store.steps if hi is None else hi
    assert 1 <= lo <= hi <= store.steps
    B, d, ns = store.B, store.d, hi - lo + 1
    mean, second, cross = np.full((B, ns, d), np.nan), np.full((B, ns, d, d), np.nan), np.full((B, ns - 1, d, d), np.nan)
    blocks = np.zeros((B, ns), np.int64)
    As = {}
    for b, s, c, w, x, A in walk(o, name, P, store, lo, trans, fallback, pair_sums=True, skip=skip):
        if A is not None:
            As[(b, s)] = A                                                    # of the pair (s, s + 1)
            if s + 1 <= hi:
                cross[b, s - lo] = cross_of(x, A)
        if s <= hi:
            with np.errstate(invalid="ignore", over="ignore"):
                mean[b, s - lo] = [tree_sum(w * x[:, col]) for col in range(d)]
            second[b, s - lo] = second_of(w, x)
            blocks[b, s - lo] = c + 1
    return (mean, second, cross, blocks) + ((As,) if return_A else ())


# ----------------------------------------------------------------------------- the law experiment: lgssm2, T = 8, against the exact smoother
# Model, data and seeds: block_backward_spec's (the sibling experiments').  Statistic: the across-block average of every entry of cross_s and second_s
# against the exact Sigma[s, s+1] + mu_s mu_{s+1}' and Sigma[s, s] + mu_s mu_s' of block_conditional_spec.smoother, in across-block standard errors (std
# over blocks / sqrt(B)).  As the smoothed mean, these are consistent and not unbiased: the bias of a block's value is of order 1 / N, the standard
# error of the average falls as 1 / sqrt(B N).  LAW_B = 512 is fixed first, as in block_smooth_spec; the worst units of the restatement on the CPU
# oracle's filter at 64 / 128 / 256 particles per block are in LAW_REHEARSED (tests/test_block_pairs_host.py asserts the chosen one); LAW_N is the
# smallest of the three inside the bound of 5.
LAW_T, LAW_SEED = bsp.LAW_T, bsp.LAW_SEED
LAW_B = 512
LAW_SIGMAS = cs.INV_SIGMAS
LAW_REHEARSED = {64: 8.38, 128: 4.23, 256: 2.12}                              # (second alone: 8.14 / 4.15 / 1.92; cross alone: 8.38 / 4.23 / 2.12)
LAW_N = 128
# The three wrong answers of law_controls on the same runs, lgssm2's default rotation theta = 0.1, worst unit at 64 / 128 / 256: cross transposed
# 35.4 / 49.7 / 75.5, mean_s (x) mean_{s+1} 8.47 / 9.71 / 16.0, the pair (s - 1, s) stored at s 20.8 / 37.0 / 59.5 -- each outside the bound.


def law_exact(mu, Sigma):
    """the exact smoother's (second [T, 2, 2], cross [T - 1, 2, 2]); Sigma is the joint covariance of the path, [2 T, 2 T] in step-major order"""
    mu = np.asarray(mu).reshape(LAW_T, 2)
    S = np.asarray(Sigma).reshape(LAW_T, 2, LAW_T, 2)
    second = np.stack([S[s, :, s, :] + np.outer(mu[s], mu[s]) for s in range(LAW_T)])
    cross = np.stack([S[s, :, s + 1, :] + np.outer(mu[s], mu[s + 1]) for s in range(LAW_T - 1)])
    return second, cross


def law_units(values, exact):
    """values [B, ...] per block, exact [...] -> |average - exact| in across-block standard errors"""
    values = np.asarray(values)
    return np.abs(values.mean(axis=0) - exact) / (values.std(axis=0, ddof=1) / np.sqrt(values.shape[0]))


def law_controls(cross, mean, exact_cross):
    """the worst unit of three wrong cross moments: transposed; the independence mistake mean_s (x) mean_{s+1}; the pair (s - 1, s) stored at s"""
    cross, mean = np.asarray(cross), np.asarray(mean)
    transposed = law_units(cross.transpose(0, 1, 3, 2), exact_cross)
    independent = law_units(mean[:, :-1, :, None] * mean[:, 1:, None, :], exact_cross)
    shifted = law_units(cross[:, :-1], exact_cross[1:])
    return {"transposed": float(transposed.max()), "independent": float(independent.max()), "shifted": float(shifted.max())}
