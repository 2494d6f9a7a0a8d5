"""Marginal smoothing per block (gpf.h gpf_block_smooth; FFBSm, Hürzeler & Künsch 1998, Doucet, Godsill & Andrieu 2000), restated in NumPy from what a
caller sees -- the Store of tests/block_backward_spec.py (every step's latent columns, log-weights, observation rows and resamples, read back through
the public interface; nothing from the device's store):

  walk        block b, T steps: c = b, W = q / S of the block's current WeightSummary; then for s = T .. lo + 1: the targets are the particles of block c
              in step s, pm = g_s[targets] their recorded parents; all in one block cp (else the lineage is undefined: NaN and 0 from step s - 1 down);
              for every target j, one at a time in ascending order: lwa = lw[s-1][block cp] + logtrans(P_b, x[s-1][block cp], x[s][j], obs[s][c])
              (block_ancestor_spec.logtrans), (m, f) = max_flags(lwa), q = fixq(lwa, m, fix_K(particles of cp)), D = the exact integer sum of q,
              r = q / D in float64 -- or the indicator of pm[j] where f != 0 --, acc = acc + W[j] * r (one multiply, one add).  W = acc, c = cp.
              Written once, for smooth and for tests/block_pairs_spec.py (pair_sums=True: its statements per pair (i, j) beside acc's).
  smooth      at every step of the walk in [lo, hi]: mean = tree(W x), var = tree(W (x - mean)^2) with the tree of DESIGN.md 3.5, restated as in
              tests/test_block_estimates_host.py.
  Returns mean, var [B, hi - lo + 1, d], weights [B, hi - lo + 1, bs] (0 beyond a short block) and the 1-based lineage blocks [B, hi - lo + 1].  A block
  with NaN / +Inf current weights: NaN everywhere, blocks 0.

The oracle's pieces (max_flags, fixq, fix_K, WeightSummary) are test infrastructure only.  Helper module, no tests."""
import numpy as np

import block_backward_spec as bsp
import block_conditional_spec as cs
from block_ancestor_spec import logtrans

CHUNK = 2048


def tree_sum(t):
    """DESIGN.md 3.5 for one chunk: the perfect binary tree over the term index, neighbours first, missing terms +0.0"""
    assert 1 <= t.size <= CHUNK
    buf = np.zeros(CHUNK)
    buf[:t.size] = t
    w = 1
    while w < CHUNK:
        buf[0::2 * w] = buf[0::2 * w] + buf[w::2 * w]
        w *= 2
    return buf[0]


def moments(w, x):
    """(mean [d], var [d]) of the columns of x under the weights w"""
    d = x.shape[1]
    mu, s2 = np.empty(d), np.empty(d)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(d):
            mu[c] = tree_sum(w * x[:, c])
            dd = x[:, c] - mu[c]
            dd = dd * dd
            s2[c] = tree_sum(w * dd)
    return mu, s2


def walk(o, name, P, store, lo=1, trans=True, fallback=False, pair_sums=False, skip=True):
    """the walk of every block, written once for smooth and block_pairs_spec.pairs: yields (b, s, c, w, x, A) for s = T, T - 1, ... down to lo or to the
    step below which the lineage of final block b is undefined -- c the (0-based) block of the lineage at step s, w the smoothing weights and x the rows of
    its particles, A the pair sums of the walk from s + 1 to s (pair_sums=True, s < T; else None).  A block with NaN / +Inf current weights yields nothing.
    trans=False: logtrans = 0; fallback=True: every r_ij is the indicator of the recorded parent (the two reductions the host tests check); skip=False:
    the pairwise form WITHOUT its rule that a target of weight 0 is skipped -- a mistake, for the negative control of tests/test_hp_block_pairs.py"""
    T, bs, n, d, B = store.steps, store.bs, store.n, store.d, store.B
    P = np.asarray(P, np.float64)
    maps = {s: store.step_map(s) for s in range(lo + 1, T + 1)}
    lwT = np.ascontiguousarray(store.lw[T - 1])
    for b in range(B):
        Pb = P[b] if P.ndim == 2 else P
        c, c0, c1 = b, b * bs, min((b + 1) * bs, n)
        ws = o.WeightSummary(np.ascontiguousarray(lwT[c0:c1]), c1 - c0)
        if ws.bad:
            continue
        w, A = ws.q.astype(np.float64) / np.float64(ws.S), None
        for s in range(T, lo - 1, -1):                                        # w: the smoothing weights of block c's particles at step s
            x = store.x(s)[c0:c1]
            yield b, s, c, w, x, A
            if s == lo:
                break
            pm = maps[s][c0:c1]
            born = pm // bs
            if born.min() != born.max():
                break                                                         # the lineage is undefined from step s - 1 down
            cp = int(born[0])
            p0, p1 = cp * bs, min((cp + 1) * bs, n)
            lwc, xc = store.lw[s - 2][p0:p1], store.x(s - 1)[p0:p1]
            K = o.fix_K(p1 - p0)
            acc, A = np.zeros(p1 - p0), np.zeros((p1 - p0, d)) if pair_sums else None
            for j in range(c1 - c0):
                if pair_sums and skip and w[j] == 0:
                    continue                                                  # the pairwise form skips the target entirely: 0 * x is not +0.0 for every x
                lwa = lwc.copy()                                              # (for acc alone the skip would change no bit: acc >= +0.0, r finite and >= 0)
                if trans:
                    with np.errstate(invalid="ignore"):
                        lwa = lwc + logtrans(name, Pb, xc, x[j], store.obs[s - 1][c])
                m, f = o.max_flags(np.ascontiguousarray(lwa))
                if f != 0 or fallback:
                    r = np.zeros(p1 - p0)
                    r[pm[j] - p0] = 1.0
                else:
                    q = o.fixq(np.ascontiguousarray(lwa), m, K)
                    r = q.astype(np.float64) / np.float64(int(q.sum(dtype=np.uint64)))
                with np.errstate(invalid="ignore", over="ignore"):
                    t = w[j] * r
                    acc = acc + t
                    if pair_sums:
                        for col in range(d):
                            A[:, col] = A[:, col] + t * x[j, col]
            w, c, c0, c1 = acc, cp, p0, p1


def smooth(o, name, P, store, lo=1, hi=None, trans=True, fallback=False):
    """trans, fallback: as walk"""
    hi = store.steps if hi is None else hi
    assert 1 <= lo <= hi <= store.steps
    B, ns = store.B, hi - lo + 1
    mean, var = np.full((B, ns, store.d), np.nan), np.full((B, ns, store.d), np.nan)
    weights = np.full((B, ns, store.bs), np.nan)
    blocks = np.zeros((B, ns), np.int64)
    for b, s, c, w, x, _ in walk(o, name, P, store, lo, trans, fallback):
        if s <= hi:
            mean[b, s - lo], var[b, s - lo] = moments(w, x)
            weights[b, s - lo] = 0.0
            weights[b, s - lo, :w.size] = w
            blocks[b, s - lo] = c + 1
    return mean, var, weights, blocks


# ----------------------------------------------------------------------------- two kernels, one law: backward simulation's step-s indices against W_s
# 16 blocks of 16 lgssm2 particles, T = 6, k = 4096 backward draws per block: count / k of every (block, step, particle) cell against W_s, in units of
# sqrt(W (1 - W) / k), over the cells with k W >= 5.  The two restatements on the oracle's filter (tests/test_block_smooth_host.py), same seeds: the worst
# cell is PAIR_REHEARSED units.
PAIR_B, PAIR_N, PAIR_T, PAIR_K, PAIR_SEED = 16, 16, 6, 4096, 17
PAIR_SIGMAS = cs.INV_SIGMAS
PAIR_REHEARSED = 3.41


def pair_units(idx, weights, bs):
    """idx [B, k, T] 1-based global indices of backward simulation, weights [B, T, bs] -> (worst standardised deviation, cells compared)"""
    B, k, T = idx.shape
    worst, cells = 0.0, 0
    for b in range(B):
        for s in range(T):
            local = idx[b, :, s] - 1 - (idx[b, :, s] - 1) // bs * bs
            count = np.bincount(local, minlength=bs).astype(np.float64)
            W = weights[b, s]
            use = (k * W >= 5) & (W * (1 - W) > 0)                         # (a cell of weight 1 has no spread to measure against)
            z = np.abs(count[use] / k - W[use]) / np.sqrt(W[use] * (1 - W[use]) / k)
            cells += int(use.sum())
            worst = max(worst, float(z.max()) if z.size else 0.0)
    return worst, cells


# ----------------------------------------------------------------------------- the law experiment: lgssm2, T = 8, against the exact smoother
# Model, data and seeds: block_backward_spec's (the sibling experiments').  Statistic: the across-block average of the smoothed mean of every step and
# column against mu_s, in across-block standard errors (std over blocks / sqrt(B)).  FFBSm is consistent, not unbiased: the bias of a block's smoothed
# mean is of order 1 / N while the standard error of the average falls as 1 / sqrt(B N), so fewer blocks make the bound easier and more particles too.
# LAW_B = 512 is fixed first (the CPU rehearsal takes 9 / 18 / 37 s at 64 / 128 / 256 particles per block; at 64 and 256 blocks the worst units were
# 4.25 / 1.60 / 1.32 and 6.14 / 1.76 / 1.33).  The rehearsed worst units of the restatement on the oracle's filter at 512 blocks are in LAW_REHEARSED;
# LAW_N = 128 is the smallest of the three inside the bound of 5.
LAW_T, LAW_SEED = bsp.LAW_T, bsp.LAW_SEED
LAW_B = 512
LAW_SIGMAS = cs.INV_SIGMAS
LAW_REHEARSED = {64: 7.46, 128: 4.16, 256: 2.23}
LAW_N = 128


def law_units(mean, mu):
    """mean [B, T, 2] smoothed means per block, mu the exact smoother's means -> |average - mu| in across-block standard errors, [T, 2]"""
    mean = np.asarray(mean)
    B = mean.shape[0]
    return np.abs(mean.mean(axis=0) - np.asarray(mu).reshape(mean.shape[1:])) / (mean.std(axis=0, ddof=1) / np.sqrt(B))
