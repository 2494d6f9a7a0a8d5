"""The most probable path per block (gpf.h gpf_block_map_path) against its DEFINITION: the same dynamic programme in mpmath, from the models of
tests/hp_reference.py (natural parameters only; `model.params` is never read).

  logprior    log mu(x_1) of the Gen program -- the full density (normal_logpdf, log_bernoulli, uniform_discrete) minus its x-free constants: the
              log sigma + log(2 pi) / 2 of every normal.  line_model keeps log(1 / n_slopes), which the member keeps too (it is free of x and changes no
              comparison).
  transrest   Ref.logtrans(full=True) minus Ref.logtrans minus the x-free constants of the transition's normals: what is left depends on x alone.  It is
              identically zero for four models (x_free_rest returns it for the pinning test) and the outlier's Bernoulli term for line_model.
  total       S(path) = logprior + (n_1 + (lt_12 + (n_2 + ... + n_T))) as an E: the value of the definition and, by E propagation through the statements of
              DESIGN.md 5.9 in their order (one rounded add per nesting level), a bound on how far a Float64 evaluation of the same total may land.
  best        the maximum of S.v over ALL bs^T sequences of the block, by the exact recursion on the mpmath values (max and + are exact there).

check_map asserts, per checked block, on the reference's own verdicts and derived bounds alone:
    S(returned).v >= max S.v - (S(returned).e + S(best).e)        the returned path is a maximiser as far as Float64 can tell
    |logp - S(returned).v| <= S(returned).e                       logp is the returned path's total
The first holds for a correct Float64 recursion because its logp is the Float64 total F of the returned path and F(returned) >= F(best) (the host
test: rounded addition is monotone), so S(returned) + e >= F(returned) >= F(best) >= S(best) - e.  Helper module, no tests."""
import numpy as np

import block_map_spec as msp
import hp_reference as hp
from hp_reference import E, M

NEG_INF = -M.inf


def _c(ref, key, sigma=None):
    return ref.sc(key, sigma)[1]                                             # log sigma + log(2 pi)/2 as an E


def trans_const(ref):
    """the x-free part of the full transition log-density"""
    n = ref.name
    if n == "lgssm2":
        return -_c(ref, "sq").scale2(1)
    if n == "sv1":
        return -_c(ref, "sigma")
    if n == "bearings4":
        return -_c(ref, "sp").scale2(1) - _c(ref, "sv").scale2(1)
    if n == "object_motion":
        return -_c(ref, "sy")
    return E(0.0)


def x_free_rest(ref, xp, x, obs):
    """full - reduced - constant of the transition density: zero for a model without transrest (the pinning test), -Inf transitions excluded"""
    return (ref.logtrans(xp, x, obs, full=True).v - ref.logtrans(xp, x, obs).v) - trans_const(ref).v


def transrest(ref, x, obs):
    """the part of log f(x | xp) free of xp but not of x, or None"""
    if ref.name != "line_model":
        return None
    return ref.logtrans(x, x, obs, full=True)                                # (xp = x: the slope persists; what is left is the outlier's term, or 0)


def logprior(ref, x, obs):
    I, n = ref.info, ref.name
    if n == "lgssm2":
        c = ref.sc("s0")
        return hp.normal2_logpdf(x[0], x[1], E(0.0), E(0.0), I["s0"], c) + c[1].scale2(1)
    if n == "bearings4":
        tot = None
        for k in range(4):
            c = ref.sc(("s", k), I["s"][k])
            t = hp.normal_logpdf(x[k], E(I["mu"][k]), I["s"][k], c) + c[1]
            tot = t if tot is None else tot + t
        return tot
    if n == "sv1":
        sd0 = E(I["sigma"]) / (1.0 - E(I["phi"]) * I["phi"]).sqrt()          # the stationary law N(mu, sigma^2 / (1 - phi^2))
        c = hp._sigma_consts(sd0)
        return hp.normal_logpdf(x[0], E(I["mu"]), None, c) + c[1]
    if n == "object_motion":                                                 # the first step is a transition from (still, 0)
        return ref.logtrans([0.0, 0.0], x, obs, full=True) + _c(ref, "sy")
    if n == "line_model":
        lp = -E(float(len(I["slopes"]))).log(1.0)
        return lp + hp.log_bernoulli(I["p_out"], x[1] != 0.0) if obs[1] != 0.0 else lp
    raise ValueError(n)


class Block:
    """the grid of one final block in the reference: rows, observation rows, and the scores as E, formed on demand and kept"""

    def __init__(self, ref, store, lin):
        self.ref, self.T = ref, store.steps
        bs, n = store.bs, store.n
        self.X = [store.x(s)[lin[s - 1] * bs:min((lin[s - 1] + 1) * bs, n)] for s in range(1, self.T + 1)]
        self.ob = [store.obs[s - 1][lin[s - 1]] for s in range(1, self.T + 1)]
        self._n, self._lt, self._lp = {}, {}, {}

    def node(self, s, i):
        if (s, i) not in self._n:
            x, ob = [float(v) for v in self.X[s - 1][i]], [float(v) for v in self.ob[s - 1]]
            v = self.ref.loglik(x, ob)
            tr = transrest(self.ref, x, ob) if s >= 2 else None
            self._n[s, i] = v if tr is None else v + tr
        return self._n[s, i]

    def lt(self, s, i, j):
        """log f(x_{s+1}^j | x_s^i) without its x_s-free terms, obs of step s + 1"""
        if (s, i, j) not in self._lt:
            self._lt[s, i, j] = self.ref.logtrans([float(v) for v in self.X[s - 1][i]], [float(v) for v in self.X[s][j]], [float(v) for v in self.ob[s]])
        return self._lt[s, i, j]

    def prior(self, i):
        if i not in self._lp:
            self._lp[i] = logprior(self.ref, [float(v) for v in self.X[0][i]], [float(v) for v in self.ob[0]])
        return self._lp[i]

    def total(self, p):
        """S(p) as an E, right-nested; E(-Inf) where a transition has no density"""
        R = self.node(self.T, p[-1])
        for s in range(self.T - 1, 0, -1):
            lt = self.lt(s, p[s - 1], p[s])
            if lt.v == NEG_INF:
                return E(NEG_INF)
            R = self.node(s, p[s - 1]) + (lt + R)
        return self.prior(p[0]) + R

    def best(self):
        """(max S.v over all sequences, a maximiser) by the exact recursion on the values"""
        v = [self.node(self.T, j).v for j in range(len(self.X[-1]))]
        ptrs = []
        for s in range(self.T - 1, 0, -1):
            nv, pt = [], []
            for i in range(len(self.X[s - 1])):
                vals = [self.lt(s, i, j).v + v[j] for j in range(len(v))]
                j = max(range(len(vals)), key=lambda k: vals[k])
                nv.append(self.node(s, i).v + vals[j]); pt.append(j)
            v = nv
            ptrs.insert(0, pt)
        tot = [self.prior(i).v + v[i] for i in range(len(v))]
        i = max(range(len(tot)), key=lambda k: tot[k])
        p = [i]
        for pt in ptrs:
            p.append(pt[p[-1]])
        return tot[i], tuple(p)


def check_map(refs, store, blocks, path, idx, logp, label):
    """the two assertions for every block of `blocks` (all with a defined lineage and a finite maximum); returns the worst |logp - S| / bound"""
    maps = {s: store.step_map(s) for s in range(2, store.steps + 1)}
    worst = 0.0
    for b in blocks:
        lin = msp.lineage(store, maps, b)
        assert lin is not None, (label, b)
        G = Block(refs[b], store, lin)
        assert np.all(idx[b] >= 1) and np.isfinite(logp[b]), (label, b, "no path returned")
        assert [(int(i) - 1) // store.bs for i in idx[b]] == lin, (label, b, "the indices leave the lineage")
        p = msp.local_path(store, idx[b])
        for s in range(1, store.steps + 1):
            assert np.array_equal(path[b, s - 1], store.x(s)[idx[b, s - 1] - 1]), (label, b, s, "the path is not the rows of its indices")
        S = G.total(p)
        top, arg = G.best()
        Sb = G.total(arg)
        assert np.isfinite(S.e) and np.isfinite(Sb.e) and S.e < 1e-9 * max(1.0, abs(float(S.v))), (label, b, "vacuous bound", S, Sb)
        assert S.v >= top - (S.e + Sb.e), (label, b, "not a maximiser", p, arg, float(top - S.v), S.e + Sb.e)
        d = float(abs(hp.mpf(float(logp[b])) - S.v))
        assert d <= S.e, (label, b, "logp is not the returned path's total", float(logp[b]), S, d)
        worst = max(worst, d / S.e if S.e > 0 else 0.0)
    return worst
