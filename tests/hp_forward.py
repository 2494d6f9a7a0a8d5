"""Forward-only smoothing per block (gpf.h gpf_block_forward_moments) against its DEFINITION: check_forward, driven with plain arrays --
the Store of tests/block_backward_spec.py filled from what a caller sees and the seven outputs of the implementation under test (the NumPy restatement
in tests/test_hp_block_forward.py, the device in tests/test_gpu_hp_block_forward.py).  Who produced the outputs is unknown here.

  values   In the reals the definition is the sum over steps of the pairwise smoother's: sum = sum_s mean_s, second = sum_s second_s, cross = sum_s cross_s,
           first = mean_1, first2 = second_1, last2 = second_T -- so the mpmath values are those of hp_checks.reference_walk (the walk BACKWARDS from T
           over the whole store, hw.smooth_step's pair sums, hw.mean / hw.second / hw.cross), which shares no statement with the forward recursion.
  bounds   The Float64 bound of every output entry is derived by running the statements of DESIGN.md 5.8 FORWARDS in E arithmetic (hp_reference.E: the
           real value and a bound on the Float64 evaluation, one half ulp per correctly rounded operation): T_1 = [x | x x' | 0 | x | x x'] (one product),
           then for every target the candidates in ascending order,  h = h + r_ij * T_{s-1}^i[f]  (a product and an addition each), with r_ij = E(p_ij,
           w_err): hw.Softmax's real probability and its bound for the counts, their sum, the conversions and one division (ancestor_softmax: exactly what
           the reference walk uses); one more rounding for the division by D, which the statements take after the sum (the division inside w_err is then
           counted twice: a bound, not an estimate); the increments x, x[a] * x[c] and xbar[a] * x[c] with their own roundings; the query's W * T with W's
           bound, the product's rounding and the tree's level count over sum |terms| (hw.mean's form, with T's bound beside W's).  A dead or certainly
           flushed candidate (Softmax.dead) has q = 0 and is skipped, a target on its fallback gives r = 1 to its recorded parent.  Nothing is fitted.
  identity The forward recursion's own real value is compared with the backward walk's: they must agree to IDENTITY_REL of the entry's scale, far below
           any Float64 bound -- the algebraic identity the feature rests on, in 160-bit arithmetic, on every checked case.
  guard    the family's: every entry's bound relative to max(1, |value|) goes into Violations' pool, whose median must stay below 1e-12.
No value is skipped: there is no draw and no decision in this feature.  Helper module, no tests."""
import numpy as np

import hp_checks as hc
import hp_reference as hp
import hp_weights as hw
from hp_reference import E, M, mpf

IDENTITY_REL = 1e-40                                                          # (PREC = 160 bits: 2^-160 = 7e-49 per operation)
NAMES = ("sum", "second", "cross", "first", "first2", "last2")


def _zero(shape):
    out = np.empty(shape, object)
    out.fill(None)
    return out


def weighted_tree(W, vals, n):
    """sum_j W_j * v_j as an E for the statement tree_j(W^j * v^j): W's bound times |v|, v's bound times |W|, the product's rounding, the tree one rounding
    per level over sum |terms| (hw.mean's form with a bound on the values too)"""
    v = M.fsum([w.v * t.v for w, t in zip(W, vals)])
    at = float(sum(abs(float(w.v)) * abs(float(t.v)) for w, t in zip(W, vals)))
    part = float(sum(abs(float(t.v)) * w.e + abs(float(w.v)) * t.e + w.e * t.e for w, t in zip(W, vals)))
    term_err = part + hw.U * (at + part)
    return E(v, term_err + hw._tree_err(n, at + term_err))


def lineage_blocks(store, blocks):
    """{step: the blocks whose statistics the checked blocks' lineages read at that step}, or None where a lineage is undefined"""
    T, bs = store.steps, store.bs
    need = {T: sorted(set(blocks))}
    for s in range(T, 1, -1):
        pm, prev = store.step_map(s), set()
        for c in need[s]:
            c0, c1 = hc._span(store.n, bs, c)
            born = pm[c0:c1] // bs
            if born.min() != born.max():
                return None
            prev.add(int(born[0]))
        need[s - 1] = sorted(prev)
    return need


def forward_E(refs, store, blocks):
    """{block: {name: array of E}} -- the statements of DESIGN.md 5.8 in E arithmetic for the checked blocks (refs[c]: the Ref of block c's parameters,
    constant over the run); a block with NaN / +Inf current weights: None"""
    T, bs, n, d = store.steps, store.bs, store.n, store.d
    need = lineage_blocks(store, blocks)
    assert need is not None, "an undefined lineage: not a case of this check"
    tri = [(a, c) for a in range(d) for c in range(a, d)]
    stat = {}                                                                 # block -> [particle][entry] of the step closed last
    for c in need[1]:
        c0, c1 = hc._span(n, bs, c)
        rows = []
        for x in np.asarray(store.x(1)[c0:c1], np.float64):
            xe = [E(float(t)) for t in x]
            sq = [xe[a] * xe[cc] for a, cc in tri]
            rows.append(xe + sq + [E(0.0)] * (d * d) + xe + sq)
        stat[c] = rows
    for s in range(2, T + 1):
        pm, new = store.step_map(s), {}
        for c in need[s]:
            c0, c1 = hc._span(n, bs, c)
            cp = int(pm[c0] // bs)
            p0, p1 = hc._span(n, bs, cp)
            lwc, xc, prev = store.lw[s - 2][p0:p1], np.asarray(store.x(s - 1)[p0:p1], np.float64), stat[cp]
            xce = [[E(float(t)) for t in row] for row in xc]
            rows = []
            for j in range(c0, c1):
                xj = np.asarray(store.x(s)[j], np.float64)
                sm = hw.ancestor_softmax(refs[c], lwc, xc, xj, store.obs[s - 1][c])
                if sm is hw.FALLBACK:
                    r = {int(pm[j] - p0): E(1.0)}
                else:
                    we = sm.w_err()
                    r = {i: E(sm.p[i], we[i]) for i in range(p1 - p0) if not sm.dead[i]}
                F = len(prev[0])
                h, xb = [E(0.0)] * F, [E(0.0)] * d
                for i in sorted(r):                                           # ascending, one product and one addition per term
                    h = [acc + r[i] * t for acc, t in zip(h, prev[i])]
                    xb = [acc + r[i] * t for acc, t in zip(xb, xce[i])]
                one = E(1.0)
                e, xbar = [t * one for t in h], [t * one for t in xb]         # the division by D: one rounding
                xe = [E(float(t)) for t in xj]
                k, row = 0, []
                for a in range(d):
                    row.append(e[k] + xe[a]); k += 1
                for a, cc in tri:
                    row.append(e[k] + xe[a] * xe[cc]); k += 1
                for a in range(d):
                    for cc in range(d):
                        row.append(e[k] + xbar[a] * xe[cc]); k += 1
                row += e[k:]
                rows.append(row)
            new[c] = rows
        stat = new
    lwT, out = np.asarray(store.lw[T - 1], np.float64), {}
    for b in blocks:
        c0, c1 = hc._span(n, bs, b)
        if np.isnan(lwT[c0:c1]).any() or (lwT[c0:c1] == np.inf).any():
            out[b] = None
            continue
        W = hw.norm_weights(hw.Softmax(lwT[c0:c1]))
        flat = [weighted_tree(W, [row[f] for row in stat[b]], c1 - c0) for f in range(len(stat[b][0]))]
        x, ws = np.asarray(store.x(T)[c0:c1], np.float64), hw.Weighted(W)

        def full(off):
            m = _zero((d, d))
            for k, (a, cc) in enumerate(tri):
                m[a, cc] = m[cc, a] = flat[off + k]
            return m
        o_sec, o_cross, o_first, o_first2 = d, d + len(tri), d + len(tri) + d * d, d + len(tri) + d * d + d
        last2 = _zero((d, d))
        for a in range(d):
            for cc in range(d):
                last2[a, cc] = hw.second(ws, x, min(a, cc), max(a, cc))
        out[b] = {"sum": np.array(flat[:d], object), "second": full(o_sec), "cross": np.array(flat[o_cross:o_first], object).reshape(d, d),
                  "first": np.array(flat[o_first:o_first2], object), "first2": full(o_first2), "last2": last2}
    return out


def backward_values(refs, store, blocks, walk=None):
    """{block: {name: array of mpf}} -- the sums over steps of the reference walk's moments (hp_checks.reference_walk, pairs=True); None: a NaN block"""
    T, d = store.steps, store.d
    out = {}
    for ev in hc.reference_walk(refs, store, blocks, pairs=True) if walk is None else walk:
        if ev[0] == "nan":
            out[ev[1]] = None
        elif ev[0] == "step":
            b, s, c, c0, c1, W, e_max, A = ev[1:]
            acc = out.setdefault(b, {"sum": np.array([mpf(0)] * d, object), "second": np.array([mpf(0)] * (d * d), object).reshape(d, d),
                                     "cross": np.array([mpf(0)] * (d * d), object).reshape(d, d)})
            ws, x = hw.Weighted(W), np.asarray(store.x(s)[c0:c1], np.float64)
            mean = np.array([hw.mean(ws, x[:, a]).v for a in range(d)], object)
            second = np.array([[hw.second(ws, x, min(a, cc), max(a, cc)).v for cc in range(d)] for a in range(d)], object)
            acc["sum"], acc["second"] = acc["sum"] + mean, acc["second"] + second
            if A is not None:                                                  # the pair (s, s + 1)
                acc["cross"] = acc["cross"] + np.array([[hw.cross(x, A, a, cc).v for cc in range(d)] for a in range(d)], object)
            if s == 1:
                acc["first"], acc["first2"] = mean, second
            if s == T:
                acc["last2"] = second
        else:
            assert ev[0] == "fallbacks", ev[0]                                # (an undefined lineage is not a case of this check)
    return out


def check_forward(v, refs, store, blocks, out, label, walk=None):
    """out: the seven outputs (sum, second, cross, first, first2, last2, n_steps) of the implementation under test for all blocks of `store`.  Every
    entry of the checked blocks against E(value of the backward walk, bound of the forward statements); the forward statements' own real value against
    the backward walk's (the identity); NaN for a NaN block; second, first2 and last2 exactly symmetric.  Returns the worst err / bound per output."""
    assert out[6] == store.steps, (label, "n_steps", out[6], store.steps)
    fwd, back = forward_E(refs, store, blocks), backward_values(refs, store, blocks, walk)
    worst = hc._Worst()
    for b in blocks:
        if fwd[b] is None or back[b] is None:
            assert fwd[b] is None and back[b] is None
            assert all(np.isnan(np.asarray(out[k])[b]).all() for k in range(6)), (label, b, "a NaN block")
            continue
        for k, name in enumerate(NAMES):
            got, bound, value = np.asarray(out[k])[b], fwd[b][name], back[b][name]
            if got.ndim == 2 and name != "cross":
                assert hc.bits_equal_nan(got, got.T).all(), (label, b, name, "not symmetric")
            for at in np.ndindex(got.shape):
                scale = max(1.0, abs(float(value[at])))
                assert abs(bound[at].v - value[at]) <= IDENTITY_REL * scale, (label, b, name, at, "the forward and the backward form differ in the reals")
                want = E(value[at], bound[at].e)
                v.value(f"{label}: {name}", (b,) + at, got[at], want)
                worst.add(name, got[at], want)
    worst.show(label)
    return worst.by
