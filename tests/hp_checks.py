"""The checks of tests/test_hp_models.py (CPU oracle under test) and tests/test_gpu_hp.py (device filter under test): drive a filter through
an adapter, and after every operation compare every particle's row and log-weight with tests/hp_reference.py's prediction from
(seed, particle id, epoch, previous row), within the reference's own derived bound.  Helper module, no tests."""
import numpy as np

import hp_reference as hp
from hp_reference import E

MEDIAN_REL_TOL = 1e-12        # the bound may not go vacuous: median over a case's particles, relative to max(1, |value|)
MAX_UNDECIDABLE = 2           # MH: particles whose |log u - alpha| is below alpha's bound


# ------------------------------------------------------------------------------------------- adapters
class OracleAdapter:
    def __init__(self, g, o, model, n, seed):
        self.g, self.o, self.model, self.n, self.seed, self.f = g, o, model, n, seed, None

    rows = property(lambda s: s.f.rows.copy())
    lw = property(lambda s: s.f.lw.copy())

    def initialize(self, obs, proposal=False, strata=None, layout="contiguous"):
        self.f = self.o.OracleFilter(self.model.model_id, self.model.params, self.n, self.seed, keep_prev=True)      # a new filter: epoch 0
        self.f.initialize(obs, proposal=proposal, strata=strata, layout=layout)

    def update(self, obs, proposal=False, strata=None, layout="interleaved"):
        self.f.update(obs, proposal=proposal, strata=strata, layout=layout)

    def resample(self, method):
        self.f.resample(method, check=False)

    def rejuvenate(self, method, n_iters, q=None):
        self.f.rejuvenate(method, n_iters, proposal=q)
        return self.f.n_accepted

    def rejuvenate_uncounted(self, method, n_iters):
        self.f.rejuvenate(method, n_iters)

    def step_ess(self, obs, ess_threshold):
        go = self.f.effective_sample_size() < ess_threshold * self.f.n
        if go:
            self.f.resample("multinomial", check=False)
        self.f.update(obs)
        return bool(go)


class DeviceAdapter:
    def __init__(self, g, o, model, n, seed):
        self.g, self.model, self.n, self.seed, self.st = g, model, n, seed, None

    rows = property(lambda s: s.st.traces)
    lw = property(lambda s: s.st.log_weights)

    def _prop(self):
        return self.g.locally_optimal if self.model.name == "lgssm2" else self.g.line_fixed

    def initialize(self, obs, proposal=False, strata=None, layout="contiguous"):
        g, rest = self.g, []
        if strata is not None:
            rest.append(list(strata))
        if proposal:
            rest += [self._prop(), ()]
        self.st = g.pf_initialize(self.model, (), obs, *rest, self.n, seed=self.seed, keep_prev=True, layout=layout)

    def update(self, obs, proposal=False, strata=None, layout="interleaved"):
        if strata is not None:
            self.g.pf_update(self.st, (), (), obs, list(strata), layout=layout)
        elif proposal:
            self.g.pf_update(self.st, (), (), obs, self._prop(), ())
        else:
            self.g.pf_update(self.st, (), (), obs)

    def resample(self, method):
        self.g.pf_resample(self.st, method, check=False)

    def _move_proposal(self, q):
        return self.g.locally_optimal_move if self.model.name == "lgssm2" else self.g.outlier_propose(q[0])

    def rejuvenate(self, method, n_iters, q=None):
        args = () if q is None else (self._move_proposal(q),)
        self.g.pf_rejuvenate(self.st, None, args, n_iters, method=method, count=True)
        return self.st.n_accepted

    def rejuvenate_uncounted(self, method, n_iters):
        """without `count` the move is left to the pf_update that follows: it runs inside the update kernel"""
        self.g.pf_rejuvenate(self.st, None, (), n_iters, method=method)

    def step_ess(self, obs, ess_threshold):
        return bool(self.g.pf_step_ess(self.st, (), (), obs, ess_threshold=ess_threshold, method="multinomial", check=False))


# ------------------------------------------------------------------------------------------- the checked run
class Violations:
    def __init__(self):
        self.bad, self.tols = [], []

    def value(self, what, i, got, want: E):
        d, t = hp.differs(got, want)
        self.tols.append(hp.rel_tol(want))
        if not d <= t:
            self.bad.append((what, i, float(got), hp.M.nstr(want.v, 20), d, t))

    def exact(self, what, i, got, want):
        if not (np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64) or got == want):
            self.bad.append((what, i, float(got), float(want), None, 0.0))

    def finish(self, label):
        assert not self.bad, f"{label}: {len(self.bad)} values off the reference, first {self.bad[:3]}"
        if self.tols:
            med = float(np.median(self.tols))
            assert med < MEDIAN_REL_TOL, f"{label}: median derived tolerance {med:.3g} is not below {MEDIAN_REL_TOL}"
        return max(self.tols) if self.tols else 0.0


class Run:
    """one filter of `model` under test through adapter `a`; mirrors the epoch count of DESIGN.md 3.1 (every randomness-consuming
    pf_* call advances it by one)"""

    def __init__(self, a, model, n, seed, ref=None, gid0=0):
        self.a, self.model, self.n, self.seed = a, model, n, seed
        self.ref = ref or hp.Ref(model)
        self.d, self.epoch, self.has_prev, self.obs = model.dim, 0, False, None
        self.disc = hp.DISCRETE[model.name]

    def _row(self, v, what, i, got, want, prev=None):
        for k in range(self.d):
            if k in self.disc:
                v.exact(f"{what} x[{k}]", i, got[k], float(want[k].v))
            elif want[k].e == 0.0:
                v.exact(f"{what} x[{k}]", i, got[k], float(want[k].v))
            else:
                v.value(f"{what} x[{k}]", i, got[k], want[k])
        if prev is not None:
            for k in range(self.d):
                v.exact(f"{what} x_prev[{k}]", i, got[self.d + k], prev[k])

    def initialize(self, obs, proposal=False, strata=None, layout="contiguous"):
        obs = np.ascontiguousarray(obs, np.float64)
        self.epoch = 0
        self.a.initialize(obs, proposal=proposal, strata=strata, layout=layout)
        rows, lw, v = self.a.rows, self.a.lw, Violations()
        for i in range(self.n):
            if strata is not None:
                x, wf = hp.initialize_stratified(self.ref, self.seed, self.epoch, i, i, self.n, obs, list(strata), layout != "contiguous", proposal)
            elif proposal:
                x, wf = hp.update_proposal(self.ref, self.seed, self.epoch, i, None, obs, first=True)
            else:
                x, wf = hp.initialize(self.ref, self.seed, self.epoch, i, obs)
            self._row(v, "initialize", i, rows[i], x)
            v.value("initialize lw", i, lw[i], wf(list(rows[i, :self.d])))
        self.epoch, self.has_prev, self.obs = 1, False, obs
        return v.finish(f"{self.model.name} initialize")

    def update(self, obs, proposal=False, strata=None, layout="interleaved"):
        obs = np.ascontiguousarray(obs, np.float64)
        rows0, lw0 = self.a.rows, self.a.lw
        self.a.update(obs, proposal=proposal, strata=strata, layout=layout)
        rows, lw, v = self.a.rows, self.a.lw, Violations()
        for i in range(self.n):
            xp = list(rows0[i, :self.d])
            if strata is not None:
                x, wf = hp.update_stratified(self.ref, self.seed, self.epoch, i, i, self.n, xp, obs, list(strata), layout != "contiguous")
            elif proposal:
                x, wf = hp.update_proposal(self.ref, self.seed, self.epoch, i, xp, obs)
            else:
                x, wf = hp.update(self.ref, self.seed, self.epoch, i, xp, obs)
            self._row(v, "update", i, rows[i], x, prev=xp)
            v.value("update lw", i, lw[i], E(lw0[i]) + wf(list(rows[i, :self.d])))
        self.epoch += 1
        self.has_prev, self.obs = True, obs
        return v.finish(f"{self.model.name} update")

    def resample(self, method="multinomial"):
        self.a.resample(method)
        self.epoch += 1

    def check_conjugacy(self, rows0, lw0, first):
        """lgssm2 with the locally optimal proposal: the increment is log N(y; A x', (sq^2 + sr^2) I) whatever x was drawn"""
        rows, lw, v = self.a.rows, self.a.lw, Violations()
        for i in range(self.n):
            xp = None if first else list(rows0[i, :self.d])
            w = self.ref.proposal_weight(first, xp, self.obs, list(rows[i, :self.d]))          # for its derived bound
            want = E(self.ref.marginal_loglik(first, xp, self.obs), w.e)
            v.value("conjugacy lw", i, lw[i], want if first else E(lw0[i]) + want)
        return v.finish("lgssm2 conjugacy identity")

    def reweight(self, n_iters=1, q=None):
        rows0, lw0 = self.a.rows, self.a.lw
        self.a.rejuvenate("reweight", n_iters, q)
        rows, lw, v = self.a.rows, self.a.lw, Violations()
        first = not self.has_prev
        for i in range(self.n):
            x, xp, ws = list(rows0[i, :self.d]), list(rows0[i, self.d:2 * self.d]), E(0.0)
            for it in range(n_iters):
                xn, wf = hp.move_reweight_iter(self.ref, self.seed, self.epoch, i, it, first, xp, x, self.obs, q[0] if q else None, q is not None)
                ws, x = ws + wf(xn), xn
            self._row(v, "reweight", i, rows[i], x, prev=xp)
            v.value("reweight lw", i, lw[i], E(lw0[i]) + ws)
        self.epoch += 1
        return v.finish(f"{self.model.name} move_reweight")

    def _mh_expect(self, i, rows0, n_iters, q):
        """(expected latent after the moves, accepted count) of particle i, or None when an accept decision is within the bound"""
        first, acc = not self.has_prev, 0
        x, xp = [E(t) for t in rows0[i, :self.d]], list(rows0[i, self.d:2 * self.d])
        for it in range(n_iters):
            xn, af, logu = hp.mh_move(self.ref, self.seed, self.epoch, i, it, first, xp, x, self.obs, q[0] if q else None, q is not None)
            alpha = af(xn)
            if abs(float(logu.v - alpha.v)) <= alpha.e + logu.e:
                return None
            if logu.v < alpha.v:
                x, acc = xn, acc + 1
        return x, acc

    def mh(self, n_iters=1, q=None):
        rows0, lw0 = self.a.rows, self.a.lw
        n_acc = self.a.rejuvenate("move", n_iters, q)
        rows, lw, v = self.a.rows, self.a.lw, Violations()
        undecidable, want_acc = [], 0
        for i in range(self.n):
            exp = self._mh_expect(i, rows0, n_iters, q)
            if exp is None:
                undecidable.append(i)
                continue
            want_acc += exp[1]
            self._row(v, "mh", i, rows[i], exp[0], prev=list(rows0[i, self.d:2 * self.d]))
            v.exact("mh lw", i, lw[i], lw0[i])
        self.epoch += 1
        assert len(undecidable) <= MAX_UNDECIDABLE, undecidable
        assert want_acc <= n_acc <= want_acc + n_iters * len(undecidable), (n_acc, want_acc, undecidable)
        v.finish(f"{self.model.name} mh")
        return len(undecidable)

    def mh_then_update(self, obs, n_iters=1):
        """pf_rejuvenate without a count, then pf_update: on the device the move runs inside the update kernel.  The moved latent is what the
        updated row keeps as x_{t-1}: checked there, then the update is predicted from it."""
        obs = np.ascontiguousarray(obs, np.float64)
        rows0, lw0 = self.a.rows, self.a.lw
        self.a.rejuvenate_uncounted("move", n_iters)
        self.a.update(obs)
        rows, lw, v, d = self.a.rows, self.a.lw, Violations(), self.d
        undecidable = []
        for i in range(self.n):
            exp = self._mh_expect(i, rows0, n_iters, None)
            if exp is None:
                undecidable.append(i)
                continue
            self._row(v, "fused move", i, rows[i, d:2 * d], exp[0])
            xp = list(rows[i, d:2 * d])
            x, wf = hp.update(self.ref, self.seed, self.epoch + 1, i, xp, obs)
            self._row(v, "fused update", i, rows[i], x)
            v.value("fused update lw", i, lw[i], E(lw0[i]) + wf(list(rows[i, :d])))
        self.epoch += 2
        self.has_prev, self.obs = True, obs
        assert len(undecidable) <= MAX_UNDECIDABLE, undecidable
        v.finish(f"{self.model.name} move fused into update")
        return len(undecidable)

    def step_ess(self, obs, ess_threshold=0.5):
        """pf_step_ess: (resample if ESS < threshold N), update, in one call.  The resampled x_{t-1} is what the new row keeps in its second
        half: an old row, from which the update is predicted; the weights restart from 0 after a multinomial resample."""
        obs = np.ascontiguousarray(obs, np.float64)
        rows0, lw0 = self.a.rows, self.a.lw
        resampled = self.a.step_ess(obs, ess_threshold)
        rows, lw, v, d = self.a.rows, self.a.lw, Violations(), self.d
        if resampled:
            self.epoch += 1
            old = {tuple(r[:d].view(np.uint64)) for r in np.ascontiguousarray(rows0)}
        for i in range(self.n):
            xp = list(rows[i, d:2 * d])
            if resampled:
                assert tuple(np.ascontiguousarray(rows[i, d:2 * d]).view(np.uint64)) in old, i
            else:
                for k in range(d):
                    v.exact("step_ess x_prev", i, xp[k], rows0[i, k])
            x, wf = hp.update(self.ref, self.seed, self.epoch, i, xp, obs)
            self._row(v, "step_ess", i, rows[i], x)
            v.value("step_ess lw", i, lw[i], E(0.0 if resampled else lw0[i]) + wf(list(rows[i, :d])))
        self.epoch += 1
        self.has_prev, self.obs = True, obs
        v.finish(f"{self.model.name} step_ess")
        return resampled


# ------------------------------------------------------------------------------------------- fixtures of the cases
def case_data(g, model, T):
    """the project's own synthetic data for `model` (models.simulate); line_model's fixture is the reference's: y_t = t * slope"""
    if model.name == "line_model":
        return np.array([g.models.line_obs(t + 1, 1.0) + [0.3 * (t + 1), 0.0] for t in range(T)])
    return np.asarray(g.models.simulate(model, T))


# ------------------------------------------------------------------------------------------- per-block model parameters
class OracleBlocks:
    """block b is block b of an oracle filter created with block b's parameters (tests/block_params_spec.py)"""

    def __init__(self, g, o, models, n, nb, seed):
        from block_params_spec import ParamBlocksOracle
        self.p = ParamBlocksOracle(o, models[0].model_id, [m.params for m in models], np.arange(len(models)), n, nb, seed, keep_prev=True, own_only=True)

    rows = property(lambda s: s.p.rows.copy())
    lw = property(lambda s: s.p.lw.copy())

    def initialize(self, obs_rows):
        self.p.initialize(obs_rows)

    def update(self, obs_rows, proposals=None):
        self.p.update(obs_rows, proposals=proposals)


class DeviceBlocks:
    def __init__(self, g, o, models, n, nb, seed):
        self.g, self.models, self.n, self.nb, self.seed, self.st = g, models, n, nb, seed, None

    rows = property(lambda s: s.st.traces)
    lw = property(lambda s: s.st.log_weights)

    def initialize(self, obs_rows):
        self.st = self.g.pf_initialize_blocks(self.models[0], (), obs_rows, self.n, self.nb, seed=self.seed, keep_prev=True, params=list(self.models))

    def update(self, obs_rows, proposals=None):
        props = None if proposals is None else [self.g.locally_optimal if p else None for p in proposals]
        self.g.pf_update_blocks(self.st, (), (), obs_rows, self.nb, props)


class BlockRun:
    """many small filters in one state, block b under the natural parameters of models[b]; every block runs under the call's one epoch,
    particles keep their global ids"""

    def __init__(self, a, models, n, nb, seed):
        self.a, self.models, self.n, self.nb, self.seed, self.epoch = a, models, n, nb, seed, 0
        self.refs = [hp.Ref(m) for m in models]
        self.rowcheck = Run(None, models[0], n, seed, ref=self.refs[0])

    def initialize(self, obs_rows):
        self.a.initialize(obs_rows)
        rows, lw, v, d = self.a.rows, self.a.lw, Violations(), self.models[0].dim
        for i in range(self.n):
            b = i // self.nb
            x, wf = hp.initialize(self.refs[b], self.seed, 0, i, obs_rows[b])
            self.rowcheck._row(v, f"block {b} initialize", i, rows[i], x)
            v.value(f"block {b} initialize lw", i, lw[i], wf(list(rows[i, :d])))
        self.epoch = 1
        return v.finish("block-params initialize")

    def update(self, obs_rows, proposals=None):
        rows0, lw0 = self.a.rows, self.a.lw
        self.a.update(obs_rows, proposals)
        rows, lw, v, d = self.a.rows, self.a.lw, Violations(), self.models[0].dim
        for i in range(self.n):
            b = i // self.nb
            xp = list(rows0[i, :d])
            if proposals is not None and proposals[b]:
                x, wf = hp.update_proposal(self.refs[b], self.seed, self.epoch, i, xp, obs_rows[b])
            else:
                x, wf = hp.update(self.refs[b], self.seed, self.epoch, i, xp, obs_rows[b])
            self.rowcheck._row(v, f"block {b} update", i, rows[i], x, prev=xp)
            v.value(f"block {b} update lw", i, lw[i], E(lw0[i]) + wf(list(rows[i, :d])))
        self.epoch += 1
        return v.finish("block-params update")


# ------------------------------------------------------------------------------------------- the math spec: edge vectors and the domain table
import math                                                                                    # noqa: E402

NAN, INF = math.nan, math.inf
DBL_MIN, DBL_MAX, TINY = 2.2250738585072014e-308, 1.7976931348623157e308, 5e-324
LN2 = hp.M.log(2)
T8 = 0.41421356237309503            # atan2_'s switch between the two argument ranges (tan(pi / 8) rounded)
SQRT2_MANTISSA = 0x6A09E667F3BCD    # log_'s switch of the mantissa range


def _nbr(xs):
    """every x with its two Float64 neighbours"""
    xs = np.asarray(xs, np.float64)
    return np.concatenate([xs, np.nextafter(xs, -np.inf), np.nextafter(xs, np.inf)])


def exp_points(rng):
    switches = np.array([float((hp.mpf(k) + 0.5) * LN2) for k in range(-1021, 1024)])          # range reduction k -> k + 1
    x = np.concatenate([rng.uniform(-708.0, 709.0, 20000), _nbr(switches), rng.uniform(-1e-3, 1e-3, 2000), 10.0 ** rng.uniform(-300, -3, 500),
                        -10.0 ** rng.uniform(-300, -3, 500), [0.0, -0.0, 1e-300, -1e-300, -708.0, 709.0, 1.0, -1.0]])
    return x[(x >= -708.0) & (x <= 709.0)]


def u52_extremes():
    return np.array([(k + 0.5) * 2.0 ** -52 for k in (0, 1, 2, 2 ** 52 - 2, 2 ** 52 - 1)])


def log_points(rng):
    k = np.arange(1, 54)
    pow2 = 2.0 ** np.arange(-1022, 1024)
    sqrt2 = (np.arange(1, 2047, dtype=np.uint64) << np.uint64(52) | np.uint64(SQRT2_MANTISSA)).view(np.float64)      # sqrt(2) 2^j, every normal exponent
    return np.concatenate([np.exp(rng.uniform(-708.0, 709.0, 20000)), 1.0 + 2.0 ** -k[:52], 1.0 - 2.0 ** -k, pow2, _nbr(sqrt2), [DBL_MAX, DBL_MIN],
                           u52_extremes(), np.arange(1.0, 70.0), 2.0 ** -np.arange(0.0, 53.0)])


def sincos_points(rng):
    e = _nbr(np.arange(0, 9) / 8.0)
    return np.concatenate([e[(e > 0.0) & (e < 1.0)], u52_extremes(), rng.uniform(0.0, 1.0, 20000), 2.0 ** -rng.uniform(1, 60, 2000)])


def atan2_points(rng):
    t = _nbr([T8])
    ys, xs = [], []
    for sy in (1.0, -1.0):
        for sx in (1.0, -1.0):
            for a, b in [(1.0, 1.0), (3.7, 3.7), (TINY, TINY), (DBL_MAX, DBL_MAX), (1e-300, 1e300), (1e300, 1e-300), (1e-300, 1.0), (1.0, 1e-300),
                         (1e-310, 1.0), (1.0, 1e-310), (1e300, 1.0), (1.0, 1e300)] + [(v, 1.0) for v in t] + [(1.0, v) for v in t] + [(3.0 * v, 3.0) for v in t]:
                ys.append(sy * a); xs.append(sx * b)
    for a, b in [(0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 2.5e-300), (-3e300, 0.0)]:            # the four axes
        ys.append(a); xs.append(b)
    mag = 10.0 ** rng.uniform(-150, 150, 4000)
    return (np.concatenate([ys, rng.uniform(-4, 4, 20000), mag * rng.uniform(-1, 1, 4000)]),
            np.concatenate([xs, rng.uniform(-4, 4, 20000), mag[::-1] * rng.uniform(-1, 1, 4000)]))


def neglog_points(rng):
    """the 64-bit uniforms U whose k = U >> 12 sits at a switch of the 64-entry table (the top 6 mantissa bits of 2k + 1), its neighbours,
    the extremes, and a random sample"""
    ks = [0, 1, 2, 3, 2 ** 52 - 1, 2 ** 52 - 2]
    for e in range(7, 53):                                  # 2k + 1 in [2^e, 2^(e+1))
        for i in range(64):
            k0 = ((1 << e) + (i << (e - 6))) >> 1           # first k of table entry i
            ks += [k for k in (k0 - 1, k0, k0 + 1) if 0 <= k < 2 ** 52]
    ks = np.array(ks, dtype=np.uint64)
    U = np.concatenate([ks << np.uint64(12), (ks << np.uint64(12)) | np.uint64(0xFFF), rng.integers(0, 2 ** 64, 20000, dtype=np.uint64, endpoint=False)])
    return U


# The domain table of DESIGN.md 3.2, one tuple per row: (function, inputs, result).  A result is a Float64 compared by bit pattern, "nan" for
# any NaN (the sign and payload of a NaN an operation produces are not IEEE-specified and differ between x86 and gfx950).
PI_D, PIO2_D, PIO4_D = 3.141592653589793, 1.5707963267948966, 0.7853981633974483
EXP_709 = 8.218407461554972e+307
EXP_M708 = 3.307553003638408e-308
DOMAIN_TABLE = [
    # exp_: NaN -> NaN; x > 709 -> +Inf (saturates: e^x is finite up to 709.78); x < -708 -> 0 (flushes: e^x is a normal number down to -708.396)
    ("exp", (NAN,), "nan"), ("exp", (INF,), INF), ("exp", (-INF,), 0.0), ("exp", (0.0,), 1.0), ("exp", (-0.0,), 1.0),
    ("exp", (TINY,), 1.0), ("exp", (-TINY,), 1.0), ("exp", (1e-300,), 1.0), ("exp", (-1e-300,), 1.0),
    ("exp", (709.0,), EXP_709), ("exp", (math.nextafter(709.0, INF),), INF), ("exp", (709.78,), INF), ("exp", (DBL_MAX,), INF),
    ("exp", (-708.0,), EXP_M708), ("exp", (math.nextafter(-708.0, -INF),), 0.0), ("exp", (-708.39,), 0.0), ("exp", (-745.0,), 0.0), ("exp", (-DBL_MAX,), 0.0),
    # log_: positive normal arguments only.  Everything else is read as sign-less bits with an implicit leading 1: FINITE GARBAGE, never NaN / Inf
    ("log", (1.0,), 0.0), ("log", (DBL_MAX,), 709.782712893384), ("log", (DBL_MIN,), -708.3964185322641),
    ("log", (0.0,), -709.0895657128241), ("log", (TINY,), -709.0895657128241), ("log", (math.nextafter(DBL_MIN, 0.0),), -708.3964185322641),
    ("log", (-0.0,), 710.475860073944), ("log", (-1.0,), 1419.565425786768), ("log", (-2.5,), 1420.481716518642),
    ("log", (INF,), 709.782712893384), ("log", (-INF,), 2129.348138680152), ("log", (NAN,), 710.1881780014921),
    # sincos2pi: u in [0, 2^28) by periodicity (exact at the multiples of 1/8 apart from the sign of a zero); NaN -> NaN; negative u: only the
    # multiples of 1/4 are pinned (the octant fold leaves the polynomials' range in between); |u| >= 2^28 and +-Inf: unspecified (int overflow)
    ("sincos", (0.0,), (0.0, 1.0)), ("sincos", (-0.0,), (0.0, 1.0)), ("sincos", (0.25,), (1.0, -0.0)), ("sincos", (0.5,), (-0.0, -1.0)),
    ("sincos", (0.75,), (-1.0, 0.0)), ("sincos", (1.0,), (0.0, 1.0)), ("sincos", (1.5,), (-0.0, -1.0)), ("sincos", (2.0,), (0.0, 1.0)),
    ("sincos", (-0.25,), (-1.0, 0.0)), ("sincos", (TINY,), (3e-323, 1.0)), ("sincos", (1e-300,), (6.283185307179586e-300, 1.0)),
    ("sincos", (NAN,), ("nan", "nan")),
    # atan2_: the sign of a zero y is dropped (the result for y = -0 is that for y = +0: +0 or +pi, where IEEE gives -0 / -pi); the sign of a
    # zero x is irrelevant; (0, 0) -> 0; Inf / Inf -> NaN (IEEE: +-pi/4, +-3pi/4); one infinite argument: as IEEE; any NaN -> NaN
    ("atan2", (0.0, 1.0), 0.0), ("atan2", (-0.0, 1.0), 0.0), ("atan2", (0.0, -1.0), PI_D), ("atan2", (-0.0, -1.0), PI_D),
    ("atan2", (0.0, 0.0), 0.0), ("atan2", (-0.0, 0.0), 0.0), ("atan2", (0.0, -0.0), 0.0), ("atan2", (-0.0, -0.0), 0.0),
    ("atan2", (1.0, 0.0), PIO2_D), ("atan2", (1.0, -0.0), PIO2_D), ("atan2", (-1.0, 0.0), -PIO2_D), ("atan2", (-1.0, -0.0), -PIO2_D),
    ("atan2", (TINY, TINY), PIO4_D), ("atan2", (TINY, -TINY), 2.356194490192345), ("atan2", (-TINY, -1.0), -PI_D), ("atan2", (TINY, -1.0), PI_D),
    ("atan2", (INF, INF), "nan"), ("atan2", (INF, -INF), "nan"), ("atan2", (-INF, -INF), "nan"), ("atan2", (-INF, INF), "nan"),
    ("atan2", (INF, 1.0), PIO2_D), ("atan2", (-INF, -0.0), -PIO2_D), ("atan2", (1.0, INF), 0.0), ("atan2", (1.0, -INF), PI_D),
    ("atan2", (-1.0, -INF), -PI_D), ("atan2", (0.0, INF), 0.0), ("atan2", (-0.0, -INF), PI_D),
    ("atan2", (NAN, 1.0), "nan"), ("atan2", (1.0, NAN), "nan"), ("atan2", (NAN, NAN), "nan"),
    ("atan2", (1e-300, 1e300), 0.0), ("atan2", (1e300, 1e-300), PIO2_D),
]
WHICH = {"exp": 0, "log": 1, "sincos": 2, "atan2": 3, "neglog": 7}


def same_bits(got, want):
    """`want`: a Float64 (compared by bit pattern) or "nan" (any NaN)"""
    if isinstance(want, str):
        return math.isnan(got)
    return np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)


def bits_equal_nan(a, b):
    """uint64 views equal, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------------------------------- log_ behind the resize family
GARBAGE = [-709.0895657128241, 1419.565425786768, 710.1881780014921, 710.475860073944, 709.782712893384, 2129.348138680152]


def check_no_log_garbage(lw, lw_before):
    """after an optimal resize every weight is finite and inside what the algorithm can produce: a kept particle carries lw + ratio, a
    resampled one logsumexp(B) - log(a) + ratio with min q <= B <= S and 1 <= a <= n', ratio = log n' - log n (resize.jl:189-195).  A log_ fed a
    zero count (-709.09) or a non-number (1419.57, 710.19) would show as an offset of hundreds of nats."""
    lw, lw_before = np.asarray(lw), np.asarray(lw_before)
    assert np.isfinite(lw).all(), lw
    for gv in GARBAGE:
        assert (np.abs(np.abs(lw) - abs(gv)) > 1.0).all(), (gv, lw)
    ratio = math.log(lw.size) - math.log(lw_before.size)
    assert (lw <= lse(lw_before) + ratio + 1e-9).all() and (lw >= lw_before.min() - math.log(lw.size) + ratio - 1e-9).all(), (lw, lw_before)


def optimal_resize_cases():
    for n_old in (2, 3, 8, 100):
        for n_new in (1, 2):
            if n_new > n_old:
                continue
            dominant = np.full(n_old, -30.0); dominant[n_old // 2] = 0.0
            yield n_old, n_new, "dominant", dominant
            yield n_old, n_new, "equal", np.full(n_old, -1.25)
            yield n_old, n_new, "two heavy", np.concatenate([[0.0, -0.1], np.full(n_old - 2, -5.0)])


def lse(lw):
    m = np.max(lw)
    return m + math.log(np.exp(lw - m).sum())
