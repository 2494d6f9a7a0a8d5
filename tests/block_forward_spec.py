"""Forward-only smoothing per block (gpf.h gpf_forward_enable_blocks, gpf_block_forward_moments; Del Moral, Doucet & Singh 2010), restated
in NumPy from what a caller sees -- the Store of tests/block_backward_spec.py, read forwards, one step at a time:

  layout      T^j = [ sum (d) | second, upper triangle | cross (d x d, row = the earlier step) | first (d) | first2, upper triangle ], F(d) doubles
  first       closing step 1: sum = first = x, second = first2 = x[a] * x[c], cross = +0.0
  close       closing step s >= 2, block by block and ONE LOOP OVER THE TARGETS j of block c: pm = g_s[j] the recorded parents, all in one block c' (else
              every T of block c is NaN); lwa = lw_{s-1}[c'] + logtrans(P_c, x_{s-1}[c'], x_s[j], obs_s[c]); (m, f) = max_flags(lwa); q = fixq(lwa, m,
              fix_K(particles of c')), D = the exact integer sum of q -- or q = the indicator of pm[j], D = 1 where f != 0 --; the candidates with q == 0
              are dropped, the others taken in ascending order: h = cumulative sum from +0.0 of (double)q * T_{s-1}[i], xb the same of (double)q *
              x_{s-1}[i] (one multiply, one add); e = h / (double)D, xbar = xb / (double)D; sum = e + x, second = e + x[a] * x[c], cross = e + xbar[a] *
              x[c], first = e, first2 = e.
  query       out[b][f] = tree(W * T[:, f]) with W = q / S of the block's current WeightSummary and the tree of DESIGN.md 3.5 (block_smooth_spec.tree_sum);
              last2 = block_pairs_spec.second_of(W, x); a block with NaN / +Inf current weights: NaN.
  forward     the query after step t of a Store: first, then close for s = 2 .. t, then query.  P: the filter's parameters or [B, n_params] rows, the
              same at every close (the callers change no parameter on the way and resample across blocks with one parameter set only).

Switches, as block_pairs_spec.pairs: trans=False: logtrans = 0; fallback=True: every q is the indicator of the recorded parent.  Two mistakes, for the
negative controls of tests/test_block_forward_host.py: parent_x=True takes x_{s-1} of the recorded parent instead of xbar; divide=False leaves out the
division by D.

The oracle's pieces (max_flags, fixq, fix_K, WeightSummary) are test infrastructure only.  Helper module, no tests."""
from collections import namedtuple

import numpy as np

from block_ancestor_spec import logtrans
from block_pairs_spec import second_of
from block_smooth_spec import tree_sum

Moments = namedtuple("Moments", "sum second cross first first2 last2 n_steps")


def F_of(d):
    return d + d * (d + 1) // 2 + d * d + d + d * (d + 1) // 2


def offsets(d):
    """the first index of (sum, second, cross, first, first2) in T and F"""
    tri = d * (d + 1) // 2
    return 0, d, d + tri, d + tri + d * d, d + tri + d * d + d, F_of(d)


def triangle(x):
    """x [n, d] (or [d]) -> [n, d (d + 1) / 2] (or [d (d + 1) / 2]), the products x[a] * x[c] for a <= c, a outer"""
    ia, ic = np.triu_indices(x.shape[-1])
    return x[..., ia] * x[..., ic]


def first(x):
    x = np.asarray(x, np.float64)
    n, d = x.shape
    with np.errstate(invalid="ignore", over="ignore"):
        tri = triangle(x)
    return np.concatenate([x, tri, np.zeros((n, d * d)), x, tri], axis=1)


def ascending_sum(q, rows, buf):
    """sum_i (double)q_i * rows[i] over the candidates with q_i != 0 in ascending i, from +0.0, one multiply and one add per term (np.cumsum adds in
    order; buf [len(q) + 1, columns] is scratch whose row 0 is the +0.0 the sums start from)"""
    live = np.flatnonzero(q)
    k = live.size
    np.multiply(q[live].astype(np.float64)[:, None], rows[live], out=buf[1:k + 1])
    return np.cumsum(buf[:k + 1], axis=0)[-1]


def close(o, name, P, T_prev, x_prev, lw_prev, x, pm, obs, bs, trans=True, fallback=False, parent_x=False, divide=True):
    """the statistics of step s >= 2 in its final order x [n, d] from the record of step s - 1; pm [n] = g_s; obs [B, .] the rows step s was entered with,
    in the current block order; P: one parameter vector or [B, n_params] rows"""
    x, x_prev, lw_prev, T_prev = (np.asarray(a, np.float64) for a in (x, x_prev, lw_prev, T_prev))
    P = np.asarray(P, np.float64)
    n, d = x.shape
    o_sum, o_sec, o_cross, o_first, _, F = offsets(d)
    T = np.full((n, F), np.nan)
    for c, c0 in enumerate(range(0, n, bs)):
        c1 = min(c0 + bs, n)
        born = pm[c0:c1] // bs
        if born.min() != born.max():
            continue                                                          # the lineage of block c is undefined: NaN
        p0 = int(born[0]) * bs
        p1 = min(p0 + bs, n)
        K = o.fix_K(p1 - p0)
        Pc = P[c] if P.ndim == 2 else P
        lwc, xc = np.ascontiguousarray(lw_prev[p0:p1]), x_prev[p0:p1]
        Tx = np.hstack([T_prev[p0:p1], xc])                                   # (h and xb are sums of the same q over the same candidates)
        buf = np.zeros((p1 - p0 + 1, F + d))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for j in range(c0, c1):
                lwa = lwc + logtrans(name, Pc, xc, x[j], obs[c]) if trans else lwc.copy()
                m, f = o.max_flags(np.ascontiguousarray(lwa))
                if f != 0 or fallback:
                    q = np.zeros(p1 - p0, np.uint64)
                    q[pm[j] - p0] = 1
                else:
                    q = o.fixq(np.ascontiguousarray(lwa), m, K)
                D = np.float64(int(q.sum(dtype=np.uint64))) if divide else np.float64(1.0)
                t = ascending_sum(q, Tx, buf) / D                             # e, then xbar
                xbar = xc[pm[j] - p0] if parent_x else t[F:]
                t[o_sum:o_sec] = t[o_sum:o_sec] + x[j]
                t[o_sec:o_cross] = t[o_sec:o_cross] + triangle(x[j])
                t[o_cross:o_first] = t[o_cross:o_first] + np.outer(xbar, x[j]).ravel()
                T[j] = t[:F]
    return T


def statistics(o, name, P, store, t=None, **kw):
    """T [n, F] of step t (default: the store's last) in its final order"""
    t = store.steps if t is None else t
    assert 1 <= t <= store.steps
    T = first(store.x(1))
    for s in range(2, t + 1):
        T = close(o, name, P, T, store.x(s - 1), store.lw[s - 2], store.x(s), store.step_map(s), store.obs[s - 1], store.bs, **kw)
    return T


def mirrored(tri, d):
    out = np.empty(tri.shape[:-1] + (d, d))
    k = 0
    for a in range(d):
        for c in range(a, d):
            out[..., a, c] = out[..., c, a] = tri[..., k]
            k += 1
    return out


def query(o, T, x, lw, bs, n_steps):
    """the weighted trees of T under the blocks' current normalised weights"""
    T, x, lw = np.asarray(T, np.float64), np.asarray(x, np.float64), np.asarray(lw, np.float64)
    n, d = x.shape
    B = (n + bs - 1) // bs
    o_sum, o_sec, o_cross, o_first, o_first2, F = offsets(d)
    flat, last2 = np.full((B, F), np.nan), np.full((B, d, d), np.nan)
    for b in range(B):
        c0, c1 = b * bs, min((b + 1) * bs, n)
        ws = o.WeightSummary(np.ascontiguousarray(lw[c0:c1]), c1 - c0)
        if ws.bad:
            continue
        W = ws.q.astype(np.float64) / np.float64(ws.S)
        with np.errstate(invalid="ignore", over="ignore"):
            flat[b] = [tree_sum(W * T[c0:c1, f]) for f in range(F)]
        last2[b] = second_of(W, x[c0:c1])
    return Moments(flat[:, o_sum:o_sec], mirrored(flat[:, o_sec:o_cross], d), flat[:, o_cross:o_first].reshape(B, d, d), flat[:, o_first:o_first2],
                   mirrored(flat[:, o_first2:], d), last2, n_steps)


def forward(o, name, P, store, t=None, **kw):
    """what gpf_block_forward_moments returns after step t of the store (default: its last step), whose x and lw are in their current order"""
    t = store.steps if t is None else t
    return query(o, statistics(o, name, P, store, t, **kw), store.x(t), store.lw[t - 1], store.bs, t)
