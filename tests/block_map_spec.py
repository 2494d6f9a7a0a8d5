"""The most probable path per block (gpf.h gpf_block_map_path; particle Viterbi, Godsill, Doucet & West 2001), restated in NumPy from what a caller sees
-- the Store of tests/block_backward_spec.py (every step's latent columns, observation rows and resamples, read back through the public interface;
nothing from the device's store; no weight is read):

  logprior    the model member of gpf_models.hpp, the same statements: log mu(x_1) without the terms free of x
  transrest   likewise: the part of log f(x | xp) that is free of xp but not of x (line_model's outlier term); None for a model that has none
  grid        final block b: the lineage c_1 .. c_T (block_store_walk's check: all recorded parents of block c_{s+1} in one block; else None), the rows
              X_s of block c_s, the node scores N_s = loglik(P_b, X_s, obs_s[c_s]) [+ transrest for s >= 2, one add] by the oracle's o_loglik_rows, the
              prior LP = logprior(P_b, X_1, obs_1[c_1]) and LT_s[i, j] = logtrans(P_b, X_s[i], X_{s+1}[j], obs_{s+1}[c_{s+1}]) (block_ancestor_spec.logtrans)
  map_paths   DESIGN.md 5.9: v_T = N_T; s = T-1 .. 1: over j ASCENDING val = LT_s[:, j] + v[j], taken where val > best (from -Inf, ptr 0); v = N_s + best;
              step 1: tot = LP + v, the smallest i attaining the maximum of the non-NaN totals; the trace p_{s+1} = ptr_s[p_s].
              Returns path [B, hi - lo + 1, d], the 1-based global indices [B, hi - lo + 1] and logp [B]; NaN / 0 / NaN for an undefined lineage or all-NaN
              totals, NaN / 0 / -Inf where the maximum is -Inf.
  brute_force all bs^T sequences of a block with the right-nested total LP[i_1] + (N_1[i_1] + (LT_1[i_1, i_2] + (N_2[i_2] + ... + N_T[i_T]))) as one array
              of shape (cnt_1, .., cnt_T).  Rounded addition is monotone, so its maximum is map_paths' logp bit for bit.

The switches are the negative controls (mistakes a kernel could make), all off by default: node=False drops the node score; obs_next=False reads obs_s
where logtrans wants obs_{s+1}; rest=False omits transrest (these three change the totals, in map_paths and brute_force alike); first_tie=False lets the
LARGEST j win a tie; ptr_trace=False follows the recorded genealogy (the first target whose recorded parent is p_s) where the trace wants ptr (these two
change map_paths' path and leave every total alone).

The oracle's pieces are test infrastructure only.  Helper module, no tests."""
import numpy as np

from block_ancestor_spec import logtrans

MODEL_ID = {"lgssm2": 1, "bearings4": 2, "sv1": 3, "object_motion": 4, "line_model": 5}


def logprior(name, P, x, obs):
    """x: [n, d] step-1 latents, obs: the data vector of step 1 -> [n]"""
    P, obs = np.asarray(P, np.float64), np.asarray(obs, np.float64)
    x = np.atleast_2d(np.asarray(x, np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        if name == "lgssm2":
            a0 = x[:, 0] * P[18]
            a1 = x[:, 1] * P[18]
            return -0.5 * (a0 * a0 + a1 * a1)
        if name == "bearings4":
            z0 = (x[:, 0] - P[0]) / P[4]
            z1 = (x[:, 1] - P[1]) / P[5]
            z2 = (x[:, 2] - P[2]) / P[6]
            z3 = (x[:, 3] - P[3]) / P[7]
            return -0.5 * ((z0 * z0 + z1 * z1) + (z2 * z2 + z3 * z3))
        if name == "sv1":
            z = (x[:, 0] - P[0]) / P[3]
            return -0.5 * (z * z)
        if name == "object_motion":
            return np.array([logtrans(name, P, np.zeros((1, 2)), xi, obs)[0] for xi in x])
        if name == "line_model":
            return np.where(x[:, 1] != 0, P[5], P[6]) + P[7] if obs[1] != 0 else np.full(len(x), P[7])
    raise ValueError(name)


def transrest(name, P, x, obs):
    """x: [n, d], obs: the data vector of x's own step -> [n], or None for a model without the term"""
    if name != "line_model":
        if name not in MODEL_ID:
            raise ValueError(name)
        return None
    P, obs = np.asarray(P, np.float64), np.asarray(obs, np.float64)
    x = np.atleast_2d(np.asarray(x, np.float64))
    return np.where(x[:, 1] != 0, P[5], P[6]) if obs[1] != 0 else np.zeros(len(x))


def loglik(o, name, P, x, obs):
    x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, np.float64)))
    out = np.empty(len(x))
    o.lib().o_loglik_rows(MODEL_ID[name], np.ascontiguousarray(P, np.float64), x, x.shape[1], len(x), np.ascontiguousarray(obs, np.float64), out)
    return out


class Grid:
    """what the recursion of one final block reads; every list is indexed by s - 1"""

    def __init__(self, lin, X, LP, N, LT):
        self.lin, self.X, self.LP, self.N, self.LT = lin, X, LP, N, LT

    T = property(lambda self: len(self.X))


def lineage(store, maps, b):
    """[c_1 .. c_T] (0-based blocks), or None where some step's recorded parents sit in two blocks"""
    bs, n = store.bs, store.n
    lin = [b]
    for s in range(store.steps, 1, -1):
        c = lin[0]
        born = maps[s][c * bs:min((c + 1) * bs, n)] // bs
        if born.min() != born.max():
            return None
        lin.insert(0, int(born[0]))
    return lin


def grid(o, name, Pb, store, maps, b, node=True, obs_next=True, rest=True):
    lin = lineage(store, maps, b)
    if lin is None:
        return None
    T, bs, n = store.steps, store.bs, store.n
    X = [store.x(s)[lin[s - 1] * bs:min((lin[s - 1] + 1) * bs, n)] for s in range(1, T + 1)]
    ob = [store.obs[s - 1][lin[s - 1]] for s in range(1, T + 1)]
    N, LT = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(1, T + 1):
            ns = loglik(o, name, Pb, X[s - 1], ob[s - 1]) if node else np.zeros(len(X[s - 1]))
            tr = transrest(name, Pb, X[s - 1], ob[s - 1]) if rest and s >= 2 else None
            N.append(ns if tr is None else ns + tr)
        for s in range(1, T):
            obs_lt = ob[s] if obs_next else ob[s - 1]
            LT.append(np.stack([logtrans(name, Pb, X[s - 1], xj, obs_lt) for xj in X[s]], axis=1))
    return Grid(lin, X, logprior(name, Pb, X[0], ob[0]), N, LT)


def _maps(store):
    return {s: store.step_map(s) for s in range(2, store.steps + 1)}


def _params(P, b):
    P = np.asarray(P, np.float64)
    return P[b] if P.ndim == 2 else P


def recursion(G, first_tie=True):
    """(tot [cnt_1], [ptr_1 .. ptr_{T-1}])"""
    v, ptrs = G.N[-1], []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(G.T - 1, 0, -1):
            cnt = len(G.X[s - 1])
            best, ptr = np.full(cnt, -np.inf), np.zeros(cnt, np.int64)
            for j in range(len(G.X[s])):
                val = G.LT[s - 1][:, j] + v[j]
                take = val > best if first_tie else val >= best
                best, ptr = np.where(take, val, best), np.where(take, j, ptr)
            v = G.N[s - 1] + best
            ptrs.insert(0, ptr)
        return G.LP + v, ptrs


def map_paths(o, name, P, store, lo=1, hi=None, node=True, obs_next=True, rest=True, first_tie=True, ptr_trace=True):
    T, bs, n, d, B = store.steps, store.bs, store.n, store.d, store.B
    hi = T if hi is None else hi
    assert 1 <= lo <= hi <= T
    path, idx, logp = np.full((B, hi - lo + 1, d), np.nan), np.zeros((B, hi - lo + 1), np.int64), np.full(B, np.nan)
    maps = _maps(store)
    for b in range(B):
        G = grid(o, name, _params(P, b), store, maps, b, node, obs_next, rest)
        if G is None:
            continue
        tot, ptrs = recursion(G, first_tie)
        ok = ~np.isnan(tot)
        if not ok.any():
            continue
        logp[b] = m = tot[ok].max()
        if m == -np.inf:
            continue
        p = int(np.flatnonzero(ok & (tot == m))[0])
        for s in range(1, T + 1):
            gi = G.lin[s - 1] * bs + p
            if lo <= s <= hi:
                path[b, s - lo], idx[b, s - lo] = store.x(s)[gi], gi + 1
            if s < T:
                if ptr_trace:
                    p = int(ptrs[s - 1][p])
                else:
                    c0 = G.lin[s] * bs
                    kids = np.flatnonzero(maps[s + 1][c0:c0 + len(G.X[s])] == gi)
                    p = int(kids[0]) if kids.size else 0
    return path, idx, logp


def brute_force(o, name, P, store, b, node=True, obs_next=True, rest=True):
    """the right-nested totals of all sequences of final block b, shape (cnt_1, .., cnt_T); None for an undefined lineage"""
    G = grid(o, name, _params(P, b), store, _maps(store), b, node, obs_next, rest)
    if G is None:
        return None
    with np.errstate(invalid="ignore", over="ignore"):
        R = G.N[-1]
        for s in range(G.T - 1, 0, -1):
            lt = G.LT[s - 1].reshape(G.LT[s - 1].shape + (1,) * (R.ndim - 1))
            R = G.N[s - 1].reshape((-1,) + (1,) * R.ndim) + (lt + R[None])
        return G.LP.reshape((-1,) + (1,) * (R.ndim - 1)) + R


def local_path(store, idx_row):
    """the 1-based global indices of one block's full path -> the indices within their blocks, a tuple"""
    return tuple(int(i - 1) % store.bs for i in idx_row)


def maximum(tot):
    """(the maximum of the non-NaN totals or NaN, the index tuples that attain it)"""
    ok = ~np.isnan(tot)
    if not ok.any():
        return np.nan, []
    m = tot[ok].max()
    return m, [tuple(int(k) for k in w) for w in np.argwhere(ok & (tot == m))]
