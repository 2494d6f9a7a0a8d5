"""Test-side specification of pf_coalesce! / pf_introduce! (include/gpf.h gpf_coalesce, gpf_introduce), built from the oracle's
existing primitives only (o_init / o_step / o_init_proposal / o_step_proposal, o_fixq = exp_fix, o_lse_from, o_fix_K, olog)."""
import numpy as np

M64 = (1 << 64) - 1


def intro_seed(seed: int, epoch: int) -> int:
    """mix(s, e) of gpf.h gpf_introduce (64-bit wrap-around arithmetic)"""
    z = (seed ^ ((epoch * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _max_key(w):
    b = np.ascontiguousarray(w, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def _max_unkey(k):
    b = np.where(k >> np.uint64(63) != 0, k & np.uint64(M64 >> 1), ~k)
    out = b.view(np.float64).copy()
    out[k == 0] = -np.inf
    return out


def coalesce_expected(o, rows, lw, cols):
    """(rows, lw, parents 1-based) after gpf_coalesce with the key columns `cols`; groups in ascending order of first occurrence"""
    rows = np.ascontiguousarray(rows, np.float64)
    lw = np.ascontiguousarray(lw, np.float64)
    n_old = lw.size
    if np.any(np.isnan(lw)) or np.any(lw == np.inf):
        raise ValueError("Invalid weights.")
    keys = np.ascontiguousarray(rows[:, list(cols)]).view(np.uint64)
    kv = np.ascontiguousarray(keys).view(np.dtype((np.void, keys.shape[1] * 8))).ravel()
    _, first, inv = np.unique(kv, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # group ids by first occurrence
    rank = np.empty_like(order); rank[order] = np.arange(order.size)
    gid = rank[inv.ravel()]
    first = first[order]
    G = first.size
    gk = np.zeros(G, np.uint64)
    np.maximum.at(gk, gid, _max_key(lw))
    m = _max_unkey(gk)
    K = o.fix_K(n_old)
    with np.errstate(invalid="ignore"):
        d = lw - m[gid]                                      # (-Inf - -Inf = NaN: exp_fix gives 0)
    q = np.empty(n_old, np.uint64)
    o.lib().o_fixq(np.ascontiguousarray(d), n_old, 0.0, K, 0, q)   # exp_fix(d - 0.0) = exp_fix(d)
    S = np.zeros(G, np.uint64)
    np.add.at(S, gid, q)
    ratio = o.olog(float(G)) - o.olog(float(n_old))
    L = o.lib()
    lse = np.array([L.o_lse_from(float(m[g]), int(S[g]), K, 4 if m[g] == -np.inf else 0) for g in range(G)])
    return rows[first].copy(), lse + ratio, first.astype(np.int64) + 1


def introduce_rows(o, model_id, params, W, keep_prev, seed, epoch, n_old, n_add, obs_hist, proposal=False):
    """the n_add new particles of gpf_introduce: rows and log-weights"""
    L = o.lib()
    P = np.ascontiguousarray(params, np.float64)
    s2 = intro_seed(seed, epoch)
    obs_hist = np.atleast_2d(np.asarray(obs_hist, np.float64))
    T = obs_hist.shape[0]
    rows = np.zeros((n_add, W)); lw = np.zeros(n_add)
    f = L.o_init_proposal if (proposal and T == 1) else L.o_init
    f(model_id, P, s2, 0, n_old, n_add, W, np.ascontiguousarray(obs_hist[0]), rows, lw)
    for e in range(1, T):
        out = np.empty_like(rows)
        f = L.o_step_proposal if (proposal and e == T - 1) else L.o_step
        f(model_id, P, s2, e, n_old, n_add, W, int(keep_prev), np.ascontiguousarray(obs_hist[e]), rows, out, lw)
        rows = out
    return rows, lw


def introduce_expected(o, f, n_add, obs_hist, proposal=False):
    """(rows, lw, parents, lml_est) of OracleFilter `f`'s state after gpf_introduce (f itself untouched; epoch = f.epoch at the call)"""
    new_rows, new_lw = introduce_rows(o, f.model, f.params, f.W, f.keep_prev, f.seed, f.epoch, f.n, n_add, obs_hist, proposal)
    old_lw = f.lw + f.lml_est if f.lml_est != 0.0 else f.lw.copy()
    return (np.vstack([f.rows, new_rows]), np.concatenate([old_lw, new_lw]),
            np.concatenate([np.asarray(f.parents, np.int64), np.zeros(n_add, np.int64)]), 0.0)


def set_state(f, rows, lw, parents, lml_est, epoch_step=0):
    """put a state into an OracleFilter (its count follows the rows)"""
    f.rows, f.lw, f.parents, f.lml_est = np.ascontiguousarray(rows), np.ascontiguousarray(lw), np.asarray(parents, np.int64), float(lml_est)
    f.n = f.lw.size
    f.epoch += epoch_step
    return f


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
