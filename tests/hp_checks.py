"""The checks of tests/test_hp_models.py (CPU oracle under test) and tests/test_gpu_hp.py (device filter under test): drive a filter through
an adapter, and after every operation compare every particle's row and log-weight with tests/hp_reference.py's prediction from
(seed, particle id, epoch, previous row), within the reference's own derived bound.  tests/test_hp_weights.py and
tests/test_gpu_hp_weights.py drive the weight side and the resize family (tests/hp_weights.py) through the same Run.  Helper module, no tests."""
import numpy as np

import hp_reference as hp
import hp_weights as hw
from hp_reference import E

MEDIAN_REL_TOL = 1e-12        # the bound may not go vacuous: median over a case's particles, relative to max(1, |value|)
MAX_TOL = {}                  # largest derived bound per weight-side quantity over the cases run so far: the table of DESIGN.md 3.3,
                              # printed by `python tests/test_hp_weights.py`


def sum_guard(sm):
    """What the bound of a sum over a weight vector (ESS, log-ML, mean, var, a proportion) may not exceed, relative to max(1, |value|).
    Every particle is off by up to half a count and the largest weight alone is 2^K counts, so S and a weighted numerator are each off by up
    to N / 2^(K+1) relative: N 2^-K for the two.  A second moment amplifies a weight's error by (x - mu)^2 / var, taken as at most 64 (8
    standard deviations).  Never below the guard of the per-particle values."""
    return max(MEDIAN_REL_TOL, 64.0 * sm.n * 2.0 ** -sm.K)
MAX_UNDECIDABLE = 2           # MH: particles whose |log u - alpha| is below alpha's bound; resampling: slots whose target is within the
                              # quantisation bound of a CDF boundary (multinomial, stratified; the residual resampler: none at all)


# ------------------------------------------------------------------------------------------- adapters
class OracleAdapter:
    def __init__(self, g, o, model, n, seed):
        self.g, self.o, self.model, self.n, self.seed, self.f = g, o, model, n, seed, None

    rows = property(lambda s: s.f.rows.copy())
    lw = property(lambda s: s.f.lw.copy())
    parents = property(lambda s: s.f.parents.copy())
    history = False
    keep_prev = True

    def initialize(self, obs, proposal=False, strata=None, layout="contiguous"):
        self.f = self.o.OracleFilter(self.model.model_id, self.model.params, self.n, self.seed, keep_prev=self.keep_prev, history=self.history)      # a new filter: epoch 0
        self.f.initialize(obs, proposal=proposal, strata=strata, layout=layout)

    def update(self, obs, proposal=False, strata=None, layout="interleaved"):
        self.f.update(obs, proposal=proposal, strata=strata, layout=layout)

    def resample(self, method, alpha=None, sort_particles=True):
        return bool(self.f.resample(method, priority_alpha=alpha, sort_particles=sort_particles, check=False))

    def resample_view(self, sl, method, alpha=None):
        """pf_resample!(state[sl], method): (the verdict, the view's own 1-based parents)"""
        v = self.f[sl]
        invalid = bool(v.resample(method, priority_alpha=alpha, check=False))
        return invalid, np.array(v.parents)

    def resize(self, n_new, method, alpha=None):
        return bool(self.f.resize(n_new, method, priority_alpha=alpha, check=False))

    def resize_refused(self, n_new, method):
        """check=True on invalid weights: the call raises"""
        try:
            self.f.resize(n_new, method, check=True)
        except self.o.OracleError:
            return True
        return False

    def replicate(self, k, layout):
        self.f.replicate(k, layout=layout)

    def dereplicate(self, k, layout, method):
        self.f.dereplicate(k, layout=layout, method=method)

    def coalesce(self, cols):
        """pf_coalesce has no function of its own in oracle.py: what is under test here is the test-side specification the GPU parity
        tests hold the device to (tests/coalesce_spec.py), applied to the oracle filter's state"""
        import coalesce_spec as cs
        f = self.f
        rows, lw, par = cs.coalesce_expected(self.o, f.rows, f.lw, cols if cols is not None else range(2 * f.d if f.keep_prev else f.d))
        cs.set_state(f, rows, lw, par, f.lml_est)

    def introduce(self, hist, n_add, proposal=False):
        """pf_introduce has no function of its own in oracle.py either: the test-side specification of tests/coalesce_spec.py"""
        import coalesce_spec as cs
        rows, lw, par, lml = cs.introduce_expected(self.o, self.f, n_add, hist, proposal=proposal)
        cs.set_state(self.f, rows, lw, par, lml, epoch_step=1)

    def sample_unweighted(self, k):
        return self.f.sample_unweighted(k)[1] - 1

    def set_lw(self, lw):
        self.f.lw = np.array(lw, np.float64)

    def set_rows(self, rows):
        self.f.rows = np.array(rows, np.float64)

    # the getters and statistics (utils.jl:148-178, statistics.jl:13-14, 48-50, 91-101); addr: a column, or (step, column) for a past choice
    def ess(self):
        return self.f.effective_sample_size()

    def lml_estimate(self):
        return self.f.log_ml_estimate()

    def log_norm_weights(self):
        return self.f.log_norm_weights()

    def norm_weights(self):
        return self.f.norm_weights()

    def column(self, addr):
        return self.f.history_column(*addr) if isinstance(addr, tuple) else self.f.column(addr)

    # proportionmap and the block-wise estimates have no function of their own in oracle.py: what is under test here is the composition the
    # GPU parity tests use as the oracle (tests/test_gpu_block_estimates.py): WeightSummary of the (block's) weights + o_wsum over its rows
    def _wsum(self, lw, x, pw, c=0.0):
        s = self.o.WeightSummary(np.ascontiguousarray(lw), len(lw))
        return self.o.lib().o_wsum(s.q, s.S, np.ascontiguousarray(x, np.float64).reshape(-1, 1), 1, 0, len(lw), pw, float(c))

    def mean(self, addr):
        return self.f.history_mean(*addr) if isinstance(addr, tuple) else self.f.mean(addr)

    def var(self, addr):
        return self.f.history_var(*addr) if isinstance(addr, tuple) else self.f.var(addr)

    def proportionmap(self, addr):
        x = self.column(addr)
        return {float(v): self._wsum(self.f.lw, x, 3, v) for v in np.unique(x)}

    def block_stats(self, nb):
        vs = [self.f[a:b] for a, b in self.o.blocks_of(self.f, nb)]
        return np.array([v.effective_sample_size() for v in vs]), np.array([v.log_ml_estimate() for v in vs])

    def block_moments(self, nb, col):
        mu, s2 = [], []
        for a, b in self.o.blocks_of(self.f, nb):
            lw, x = self.f.lw[a:b], self.f.rows[a:b, col]
            mu.append(self._wsum(lw, x, 1))
            s2.append(self._wsum(lw, x, 2, mu[-1]))
        return np.array(mu), np.array(s2)

    def block_proportionmap(self, nb, col):
        vals = np.unique(self.f.rows[:, col])
        return vals, np.array([[self._wsum(self.f.lw[a:b], self.f.rows[a:b, col], 3, v) for v in vals] for a, b in self.o.blocks_of(self.f, nb)])

    def rejuvenate(self, method, n_iters, q=None):
        self.f.rejuvenate(method, n_iters, proposal=q)
        return self.f.n_accepted

    def rejuvenate_uncounted(self, method, n_iters):
        self.f.rejuvenate(method, n_iters)

    def step_ess(self, obs, ess_threshold, method="multinomial"):
        go = self.f.effective_sample_size() < ess_threshold * self.f.n
        if go:
            self.f.resample(method, check=False)
        self.f.update(obs)
        return bool(go)


class DeviceAdapter:
    def __init__(self, g, o, model, n, seed):
        self.g, self.model, self.n, self.seed, self.st = g, model, n, seed, None

    rows = property(lambda s: s.st.traces)
    lw = property(lambda s: s.st.log_weights)
    parents = property(lambda s: s.st.parents)
    history = False
    keep_prev = True

    def _prop(self):
        return self.g.locally_optimal if self.model.name == "lgssm2" else self.g.line_fixed

    def initialize(self, obs, proposal=False, strata=None, layout="contiguous"):
        g, rest = self.g, []
        if strata is not None:
            rest.append(list(strata))
        if proposal:
            rest += [self._prop(), ()]
        kw = {"history": 8} if self.history else {}
        self.st = g.pf_initialize(self.model, (), obs, *rest, self.n, seed=self.seed, keep_prev=self.keep_prev, layout=layout, **kw)

    def update(self, obs, proposal=False, strata=None, layout="interleaved"):
        if strata is not None:
            self.g.pf_update(self.st, (), (), obs, list(strata), layout=layout)
        elif proposal:
            self.g.pf_update(self.st, (), (), obs, self._prop(), ())
        else:
            self.g.pf_update(self.st, (), (), obs)

    def _prio(self, alpha):
        return None if alpha is None else self.g.Tempering(alpha)

    def resample(self, method, alpha=None, sort_particles=True):
        kw = {"sort_particles": sort_particles} if method == "stratified" else {}
        return self._invalid(lambda check: self.g.pf_resample(self.st, method, priority_fn=self._prio(alpha), check=check, **kw))

    def resample_view(self, sl, method, alpha=None):
        """the whole filter as a view is the library's local resample: its parents are the source's (tests/test_sorted_multinomial.py)"""
        v = self.st[sl]
        try:
            invalid = self._invalid(lambda check: self.g.pf_resample(v, method, priority_fn=self._prio(alpha), check=check))
            whole = v.start == 0 and v.step == 1 and v.n_particles == self.st.n_particles
            return invalid, (self.st.parents if whole else v.parents)
        finally:
            v.close()

    check = False

    def _invalid(self, call):
        """check=False is the fully asynchronous path and reports nothing: the verdict is None (unknown).  With `self.check = "warn"` (the
        synchronising path) the library's own verdict comes back"""
        import warnings
        if self.check is False:
            call(False)
            return None
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            call(self.check)
        return any("Invalid weights" in str(x.message) for x in w)

    def resize(self, n_new, method, alpha=None):
        if method == "optimal":                                                      # takes no priority (resize.jl:149)
            return self._invalid(lambda check: self.g.pf_resize(self.st, n_new, method, check=check))
        return self._invalid(lambda check: self.g.pf_resize(self.st, n_new, method, priority_fn=self._prio(alpha), check=check))

    def resize_refused(self, n_new, method):
        try:
            self.g.pf_resize(self.st, n_new, method, check=True)
        except self.g.ErrorException:
            return True
        return False

    def replicate(self, k, layout):
        self.g.pf_replicate(self.st, k, layout=layout)

    def dereplicate(self, k, layout, method):
        self.g.pf_dereplicate(self.st, k, layout=layout, method=method)

    def coalesce(self, cols):
        self.g.pf_coalesce(self.st, by=None if cols is None else tuple(cols))

    def introduce(self, hist, n_add, proposal=False):
        if proposal:
            self.g.pf_introduce(self.st, hist, self._prop(), (), n_add)
        else:
            self.g.pf_introduce(self.st, hist, n_add)

    def sample_unweighted(self, k):
        return self.g.sample_unweighted_traces(self.st, k, return_indices=True)[1] - 1

    def set_lw(self, lw):
        self.st.log_weights = np.array(lw, np.float64)

    def set_rows(self, rows):
        self.st.traces = np.array(rows, np.float64)

    def ess(self):
        return self.g.effective_sample_size(self.st)

    def lml_estimate(self):
        return self.g.log_ml_estimate(self.st)

    def log_norm_weights(self):
        return self.g.get_log_norm_weights(self.st)

    def norm_weights(self):
        return self.g.get_norm_weights(self.st)

    def column(self, addr):
        return self.st.history_column(*addr) if isinstance(addr, tuple) else self.st.column(addr)

    def mean(self, addr):
        return self.g.mean(self.st, addr)

    def var(self, addr):
        return self.g.var(self.st, addr)

    def proportionmap(self, addr):
        return self.g.proportionmap(self.st, addr)

    def block_stats(self, nb):
        return self.g.block_stats(self.st, nb)

    def block_moments(self, nb, col):
        return self.g.block_mean(self.st, nb, col), self.g.block_var(self.st, nb, col)

    def block_proportionmap(self, nb, col):
        return self.g.block_proportionmap(self.st, nb, col)

    def _move_proposal(self, q):
        return self.g.locally_optimal_move if self.model.name == "lgssm2" else self.g.outlier_propose(q[0])

    def rejuvenate(self, method, n_iters, q=None):
        args = () if q is None else (self._move_proposal(q),)
        self.g.pf_rejuvenate(self.st, None, args, n_iters, method=method, count=True)
        return self.st.n_accepted

    def rejuvenate_uncounted(self, method, n_iters):
        """without `count` the move is left to the pf_update that follows: it runs inside the update kernel"""
        self.g.pf_rejuvenate(self.st, None, (), n_iters, method=method)

    def step_ess(self, obs, ess_threshold, method="multinomial"):
        return bool(self.g.pf_step_ess(self.st, (), (), obs, ess_threshold=ess_threshold, method=method, check=False))


# ------------------------------------------------------------------------------------------- the checked run
class Violations:
    def __init__(self):
        self.bad, self.tols, self.by, self.vacuous = [], [], {}, []

    def value(self, what, i, got, want: E, guard=None):
        """`guard`: a sum over many particles is not pooled into the median of the per-particle bounds (thousands of them would hide it): its
        own bound must stay below `guard` (sum_guard)"""
        d, t = hp.differs(got, want)
        r = hp.rel_tol(want)
        if guard is None:
            self.tols.append(r)
        elif not r < guard:
            self.vacuous.append((what, i, r, guard))
        self.by[what] = max(self.by.get(what, 0.0), r)
        if not d <= t:
            self.bad.append((what, i, float(got), hp.M.nstr(want.v, 20), d, t))

    def exact(self, what, i, got, want):
        if not (np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64) or got == want):
            self.bad.append((what, i, float(got), float(want), None, 0.0))

    def finish(self, label):
        assert not self.bad, f"{label}: {len(self.bad)} values off the reference, first {self.bad[:3]}"
        assert not self.vacuous, f"{label}: derived bounds of sums above their guard, (what, index, bound, guard) {self.vacuous[:3]}"
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
        self.lml = E(0.0)                  # the running log-ML estimate (resample.jl:178-182), carried with its bound

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

    def initialize(self, obs, proposal=False, strata=None, layout="contiguous", check=True):
        """check=False: the rows and weights are some filter's state for the weight-side checks; what they are is the other tests' business"""
        obs = np.ascontiguousarray(obs, np.float64)
        self.epoch = 0
        self.a.initialize(obs, proposal=proposal, strata=strata, layout=layout)
        if not check:
            self.epoch, self.has_prev, self.obs, self.lml = 1, False, obs, E(0.0)
            return 0.0
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
        self.epoch, self.has_prev, self.obs, self.lml = 1, False, obs, E(0.0)
        return v.finish(f"{self.model.name} initialize")

    def update(self, obs, proposal=False, strata=None, layout="interleaved", check=True):
        obs = np.ascontiguousarray(obs, np.float64)
        rows0, lw0 = self.a.rows, self.a.lw
        self.a.update(obs, proposal=proposal, strata=strata, layout=layout)
        if not check:
            self.epoch, self.has_prev, self.obs = self.epoch + 1, True, obs
            return 0.0
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

    def _note(self, what, v):
        v.finish(f"{self.model.name} {what}")
        for k, t in v.by.items():
            k = k.split(" (")[0]
            MAX_TOL[k] = max(MAX_TOL.get(k, 0.0), t)

    def _lml_estimate(self, v, what, sm):
        if self.lml.v == -hp.M.inf:                       # a resample of all -Inf weights: logsumexp = -Inf, for good
            assert self.a.lml_estimate() == -np.inf, what
        else:
            v.value(what, 0, self.a.lml_estimate(), hw.lml_estimate_from(self.lml, sm), guard=sum_guard(sm))

    def _check_resampled(self, label, method, alpha, sort_particles, rows0, lw0, n_new, invalid, K=None):
        """after a resample / resize under epoch self.epoch: ancestors against the reference's (tests/hp_weights.py), the gathered rows bit for
        bit, the new log-weights and the log-ML estimate.  Returns the number of undecidable slots (residual: asserted 0)."""
        a, n_old = self.a, len(lw0)
        parents0 = np.asarray(a.parents) - 1
        lp = lw0 if alpha is None else np.float64(alpha) * lw0                   # priority_fn.(log_weights), Float64 like the reference
        sm, ref, bad = hw.reference_ancestors(lp, method, self.seed, self.epoch, n_new, sort_particles, K)
        assert invalid is None or invalid == sm.invalid, (label, invalid)      # None: a check=False call on the device reports no verdict
        left_out = hw.check_ancestors(ref, parents0, sm, label)
        if method == "residual":
            assert not bad and left_out == 0, f"{label}: residual resampling with undecidable copy counts {bad[:4]} / tail slots {ref.undecidable[:4]}"
        else:
            assert left_out <= MAX_UNDECIDABLE, (label, ref.undecidable)
        if method == "multinomial_sorted":
            assert (np.diff(parents0) >= 0).all(), f"{label}: the ancestors of the sorted multinomial are not non-decreasing"
        rows, lw = a.rows, a.lw
        assert rows.shape[0] == n_new and np.array_equal(np.ascontiguousarray(rows).view(np.uint64), np.ascontiguousarray(rows0[parents0]).view(np.uint64)), f"{label}: gathered rows"
        v = Violations()
        if alpha is None:
            assert (lw == 0.0).all(), f"{label}: weights after the resample are not 0"
        else:
            want = hw.weights_after(lw0, lp, parents0, n_new)
            for j in range(n_new):
                v.value("lw after a resample under a priority", j, lw[j], want[j])
        # the log-ML estimate: the running sum grows by logsumexp(RAW lw) - log N_old; the getter adds logsumexp(new lw) - log N_new
        if np.all(lw0 == -np.inf):
            self.lml = E(-hp.M.inf)
        else:
            self.lml = self.lml + (hw.Softmax(lw0, K).lse() - hw.log_n(n_old))
        self._lml_estimate(v, "log_ml_estimate", hw.Softmax(lw))
        self._note(label, v)
        return left_out

    def resample(self, method="multinomial", alpha=None, sort_particles=True):
        rows0, lw0 = self.a.rows, self.a.lw
        invalid = self.a.resample(method, alpha, sort_particles)
        left_out = self._check_resampled(f"resample {method}", method, alpha, sort_particles, rows0, lw0, self.n, invalid)
        self.epoch += 1
        return left_out

    def resample_view(self, sl, method="multinomial", alpha=None):
        """pf_resample!(state[sl], method) for a contiguous or strided slice (view.jl:35-48, resample.jl:185-187, :205-218): the view's
        weights alone, K from ITS particle count; slot j of the view reads the resample id start + j -- the strata of a stratified
        resample are local to the view (j of n), their uniforms those of the ids start + j, and a tile total of the sorted multinomial
        reads id start + first; ancestors local to the view; no log-ML update: the new weights keep the view's total,
        logsumexp(lw) - log n each, or lw[a] - lp[a] + logsumexp(lw) - logsumexp(lw[a] - lp[a]) under a priority.  Rows and weights
        outside the view: bit-unchanged.  Returns the number of undecidable slots."""
        rows0, lw0 = self.a.rows, self.a.lw
        invalid, parents = self.a.resample_view(sl, method, alpha)
        idx = np.arange(self.n)[sl]
        n, label = len(idx), f"resample {method} of the view {sl.start}:{sl.stop}:{sl.step}"
        lwv = lw0[idx]
        lp = lwv if alpha is None else np.float64(alpha) * lwv
        K = hw.fix_K(n)
        sm, ref, _ = hw.reference_ancestors(lp, method, self.seed, self.epoch, None, True, K, slot0=int(idx[0]))
        assert invalid is None or invalid == sm.invalid, (label, invalid)
        parents0 = np.asarray(parents)[:n] - 1
        left_out = hw.check_ancestors(ref, parents0, sm, label)
        assert left_out <= MAX_UNDECIDABLE, (label, ref.undecidable)
        if method == "multinomial_sorted":
            assert (np.diff(parents0) >= 0).all(), f"{label}: the ancestors of the sorted multinomial are not non-decreasing"
        rows, lw = self.a.rows, self.a.lw
        bits = lambda x: np.ascontiguousarray(x).view(np.uint64)
        assert rows.shape == rows0.shape and np.array_equal(bits(rows[idx]), bits(rows0[idx][parents0])), f"{label}: gathered rows"
        out = np.ones(self.n, bool)
        out[idx] = False
        assert np.array_equal(bits(rows[out]), bits(rows0[out])), f"{label}: rows outside the view changed"
        assert np.array_equal(bits(lw[out]), bits(lw0[out])), f"{label}: weights outside the view changed"
        v = Violations()
        total = hw.Softmax(lwv, K).lse()
        if alpha is None:
            want = [total - hw.log_n(n)] * n
        else:
            want = hw.weights_after(lwv, lp, parents0, total=total)
        for j in range(n):
            v.value("lw of a view after its resample", j, lw[idx[j]], want[j])
        self._lml_estimate(v, "log_ml_estimate", hw.Softmax(lw))                 # the running estimate is the parent's, untouched
        self._note(label, v)
        self.epoch += 1
        return left_out

    def resize(self, n_new, method="multinomial", alpha=None):
        """pf_resize (resize.jl:46-124): n_new slots over the old weights; K is sized for the larger of the two counts"""
        rows0, lw0 = self.a.rows, self.a.lw
        invalid = self.a.resize(n_new, method, alpha)
        left_out = self._check_resampled(f"resize {method}", method, alpha, True, rows0, lw0, n_new, invalid, K=hw.fix_K(max(self.n, n_new)))
        self.n = self.a.n = n_new
        self.epoch += 1
        return left_out

    def sample_unweighted(self, k):
        """Gen.sample_unweighted_traces: k categorical draws, slot j of an epoch of its own; the filter is left as it was"""
        rows0, lw0 = self.a.rows, self.a.lw
        idx = self.a.sample_unweighted(k)
        sm = hw.Softmax(lw0)
        left_out = hw.check_ancestors(hw.multinomial(sm, self.seed, self.epoch, k), idx, sm, "sample_unweighted")
        assert np.array_equal(self.a.rows, rows0) and np.array_equal(self.a.lw, lw0)
        assert left_out <= MAX_UNDECIDABLE
        self.epoch += 1
        return left_out

    # ---- the rest of the resize family (resize.jl:149-334) against tests/hp_weights.py
    def _same_rows(self, label, rows, rows0, parents0):
        assert rows.shape[0] == len(parents0) and np.array_equal(np.ascontiguousarray(rows).view(np.uint64), np.ascontiguousarray(rows0[parents0]).view(np.uint64)), f"{label}: gathered rows"

    def _weights(self, v, what, lw, want):
        """one expected weight per slot; None: -Inf exactly"""
        assert len(lw) == len(want), (what, len(lw), len(want))
        for j, w in enumerate(want):
            if w is None:
                assert lw[j] == -np.inf, (what, j, lw[j])
            else:
                v.value(what[j] if isinstance(what, list) else what, j, lw[j], w)

    def _getter_after(self, v, lw):
        """the getter over new weights, the running estimate untouched"""
        sm = hw.Softmax(lw)
        if sm.invalid:
            assert self.a.lml_estimate() == -np.inf
        else:
            self._lml_estimate(v, "log_ml_estimate", sm)

    def resize_optimal(self, n_new):
        """pf_resize(..., "optimal") (resize.jl:149-219).  The threshold and every keep decision must be decidable by the reference: a wrong
        keep set changes every slot after it.  Returns the number of undecidable picks."""
        a, rows0, lw0 = self.a, self.a.rows, self.a.lw
        label = f"optimal resize {len(lw0)} -> {n_new}"
        ref = hw.optimal_resize(lw0, n_new, self.seed, self.epoch)
        assert not ref.und_threshold and not ref.und_keep, f"{label}: threshold {ref.und_threshold[:4]} / keep tests {ref.und_keep[:4]} within the bound: not a case"
        invalid = a.resize(n_new, "optimal")
        assert invalid is None or invalid == ref.invalid, (label, invalid, ref.invalid)
        parents0 = np.asarray(a.parents) - 1
        assert parents0.shape == (n_new,) and ((parents0 >= 0) & (parents0 < len(lw0))).all(), label
        assert np.array_equal(parents0[:ref.n_keep], ref.keep), f"{label}: the kept particles, ascending"
        skip = set(ref.picks.undecidable)
        wrong = [(j, int(g_), w) for j, (g_, w) in enumerate(zip(parents0[ref.n_keep:], ref.picks.anc)) if j not in skip and g_ != w]
        assert not wrong, f"{label}: {len(wrong)} picks off the reference (eps {ref.picks.eps:.3g}), first (slot, got, want) {wrong[:4]}"
        assert len(skip) <= MAX_UNDECIDABLE, (label, ref.picks.undecidable)
        assert not np.isin(parents0[ref.n_keep:], ref.keep).any(), f"{label}: a kept particle was picked again"
        if not ref.invalid:
            assert not ref.sm.dead[parents0].any(), f"{label}: a particle more than 708 below the maximum was chosen"
        rows, lw, v = a.rows, a.lw, Violations()
        self._same_rows(label, rows, rows0, parents0)
        self._weights(v, ["optimal resize: lw of a kept particle"] * ref.n_keep + ["optimal resize: lw of a resampled particle"] * (n_new - ref.n_keep), lw, ref.weights)
        self._getter_after(v, lw)
        self._note(label, v)
        self.n = a.n = n_new
        self.n_keep = ref.n_keep
        self.epoch += 1
        return len(skip)

    def resize_refused(self, n_new, method="optimal"):
        """check=True on invalid weights raises and leaves the filter as it was"""
        rows0, lw0, par0 = self.a.rows, self.a.lw, np.asarray(self.a.parents).copy()
        assert self.a.resize_refused(n_new, method)
        assert np.array_equal(self.a.rows, rows0, equal_nan=True) and np.array_equal(self.a.lw, lw0) and np.array_equal(self.a.parents, par0)

    def dereplicate_sample(self, k, layout="contiguous"):
        """pf_dereplicate(..., method="sample") (resize.jl:281-293).  Returns the number of undecidable draws."""
        a, rows0, lw0 = self.a, self.a.rows, self.a.lw
        label = f"dereplicate {len(lw0)} / {k} {layout}"
        ref, want, sms = hw.dereplicate_sample(lw0, k, layout, self.seed, self.epoch)
        a.dereplicate(k, layout, "sample")
        n_new = len(lw0) // k
        parents0 = np.asarray(a.parents) - 1
        assert parents0.shape == (n_new,), label
        groups, skip, wrong = hw.replicate_groups(len(lw0), k, layout), set(ref.undecidable), []
        for j, (got, wnt) in enumerate(zip(parents0, ref.anc)):
            assert got in groups[j], f"{label}: output {j} holds {got}, no member of its group"
            assert sms[j].invalid or not sms[j].dead[groups[j].index(got)], f"{label}: output {j} drew a flushed particle"
            if j not in skip and got != wnt:
                wrong.append((j, int(got), wnt))
        assert not wrong, f"{label}: {len(wrong)} draws off the reference (eps {ref.eps:.3g}), first (output, got, want) {wrong[:4]}"
        assert len(skip) <= MAX_UNDECIDABLE, (label, ref.undecidable)
        rows, lw, v = a.rows, a.lw, Violations()
        self._same_rows(label, rows, rows0, parents0)
        self._weights(v, "dereplicate sample: lw", lw, want)
        self.n = a.n = n_new
        self._getter_after(v, lw)
        self._note(label, v)
        self.epoch += 1
        return len(skip)

    def replicate_round_trip(self, k, layout="contiguous"):
        """pf_replicate then pf_dereplicate(method="keepfirst"): both exact, no randomness, the log-ML getter unchanged in real arithmetic"""
        a, rows0, lw0, n = self.a, self.a.rows, self.a.lw, len(self.a.lw)
        idx = np.repeat(np.arange(n), k) if layout == "contiguous" else np.tile(np.arange(n), k)      # repeat(x; inner=k) / repeat(x, k), :238
        a.replicate(k, layout)
        v = Violations()
        assert np.array_equal(np.asarray(a.parents) - 1, idx), layout
        self._same_rows(f"replicate {layout}", a.rows, rows0, idx)
        assert np.array_equal(a.lw.view(np.uint64), lw0[idx].view(np.uint64))
        self.n = a.n = n * k
        self._getter_after(v, a.lw)
        a.dereplicate(k, layout, "keepfirst")
        first = np.arange(0, n * k, k) if layout == "contiguous" else np.arange(n)                  # :274
        assert np.array_equal(np.asarray(a.parents) - 1, first), layout
        assert np.array_equal(np.ascontiguousarray(a.rows).view(np.uint64), np.ascontiguousarray(rows0).view(np.uint64))
        assert np.array_equal(a.lw.view(np.uint64), lw0.view(np.uint64))
        self.n = a.n = n
        self._getter_after(v, a.lw)
        self._note(f"replicate / dereplicate {layout}", v)

    def coalesce(self, cols=None):
        """pf_coalesce (resize.jl:309-334); cols: the key columns, None = every state column.  Returns the number of groups."""
        a, rows0, lw0 = self.a, self.a.rows, self.a.lw
        n_old = len(lw0)
        label = f"coalesce {n_old} by {cols}"
        key = list(cols) if cols is not None else list(range(2 * self.d if a.keep_prev else self.d))
        first, want, groups = hw.coalesce(rows0, lw0, key)
        sm0, before = hw.Softmax(lw0), a.lml_estimate()
        a.coalesce(cols)
        parents0 = np.asarray(a.parents) - 1
        assert len(a.lw) == len(groups), f"{label}: {len(a.lw)} groups, the definition has {len(groups)}"
        assert np.array_equal(parents0, first), f"{label}: parents are the groups' first members in order of first occurrence"
        assert np.all(np.diff(parents0) > 0)
        rows, lw, v = a.rows, a.lw, Violations()
        self._same_rows(label, rows, rows0, parents0)
        self._weights(v, "coalesce: lw", lw, want)
        self.n = a.n = len(groups)
        # log_ml_estimate is unchanged in real arithmetic: the two getters agree within the sum of their bounds, each derived
        sm1 = hw.Softmax(lw)
        if sm0.invalid:
            assert before == -np.inf and a.lml_estimate() == -np.inf
        elif self.lml.v != -hp.M.inf:
            e0, e1 = hw.lml_estimate_from(self.lml, sm0), hw.lml_estimate_from(self.lml, sm1)
            assert e0.e < sum_guard(sm0) * max(1.0, abs(float(e0.v))) and abs(a.lml_estimate() - before) <= e0.e + e1.e, (label, before, a.lml_estimate(), e0, e1)
            self._lml_estimate(v, "log_ml_estimate", sm1)
        self._note(label, v)
        return len(groups)

    def introduce(self, hist, n_add, proposal=False):
        """pf_introduce (resize.jl:351-421, include/gpf.h gpf_introduce).  New particle j: particle id n_old + j, the streams of the seed
        mix(seed, epoch at the call), epochs 0 .. T-1: initialize, then T - 1 updates from the prior (the proposal at the last step when one is
        given); its weight the sum of the step log-likelihoods in step order.  A keep_prev row stores x_T and x_{T-1}: both are checked against
        the chain, which then goes on from the STORED values (and scores them), so only x_1 .. x_{T-2} are carried with their bounds."""
        a, d = self.a, self.d
        hist = np.ascontiguousarray(np.atleast_2d(np.asarray(hist, np.float64)))
        T, n_old = hist.shape[0], self.n
        rows0, lw0, par0 = a.rows, a.lw, np.asarray(a.parents).copy()
        a.introduce(hist, n_add, proposal)
        rows, lw, par, v = a.rows, a.lw, np.asarray(a.parents), Violations()
        assert rows.shape[0] == lw.shape[0] == par.shape[0] == n_old + n_add
        # ---- the old particles: lw += log_ml_est where it is not 0, ONE Float64 addition of one running estimate c inside the bound carried
        assert np.array_equal(np.ascontiguousarray(rows[:n_old]).view(np.uint64), np.ascontiguousarray(rows0).view(np.uint64))
        assert np.array_equal(par[:n_old], par0) and (par[n_old:] == 0).all()
        if self.lml.v == 0 and self.lml.e == 0.0:
            assert np.array_equal(lw[:n_old].view(np.uint64), lw0.view(np.uint64)), "introduce with log_ml_est = 0 touched the old weights"
        else:
            c, cands = float(self.lml.v), []
            lo, hi = float(self.lml.v) - self.lml.e, float(self.lml.v) + self.lml.e
            assert self.lml.e < MEDIAN_REL_TOL * max(1.0, abs(c))
            for step in (-np.inf, np.inf):
                x = c if step < 0 else np.nextafter(c, np.inf)
                while lo <= x <= hi:
                    if np.array_equal((lw0 + x).view(np.uint64), lw[:n_old].view(np.uint64)):
                        cands.append(x)
                    x = np.nextafter(x, step)
            assert cands, "introduce: the old weights are not lw + c for any Float64 c within the bound of the running log-ML estimate"
        self.lml = E(0.0)
        # ---- the new particles
        s2 = hp.mix(self.seed, self.epoch)
        for j in range(n_add):
            i, gid = n_old + j, n_old + j
            got_x, got_p = rows[i, :d], rows[i, d:2 * d]
            x, ws = None, []
            for e in range(T):
                last, first = e == T - 1, e == 0
                if e == T - 1 and T >= 2:                    # x_{T-1} is stored: checked against the chain, which goes on from the stored value
                    self._row(v, "introduce x_prev", i, got_p, x)
                    x = [float(t) for t in got_p]
                if e >= 1:
                    ws.append(self.ref.loglik(x, hist[e - 1]))
                if last and proposal:
                    xn, wf = hp.update_proposal(self.ref, s2, e, gid, x, hist[e], first=first)
                elif first:
                    xn, wf = hp.initialize(self.ref, s2, e, gid, hist[e])
                else:
                    xn, wf = hp.update(self.ref, s2, e, gid, x, hist[e])
                xprev, x = x, xn
            self._row(v, "introduce", i, got_x, x)
            if T == 1:
                for k in range(d):
                    v.exact("introduce x_prev (T = 1)", i, got_p[k], 0.0)
            ws.append(wf(list(got_x)))
            tot = ws[0]
            for w in ws[1:]:
                tot = tot + w
            v.value("introduce lw", i, lw[i], tot)
            if proposal and self.model.name == "lgssm2":   # conjugacy: the last increment is log N(y; A x', (sq^2 + sr^2) I) whatever x was drawn
                tot = None
                for w in ws[:-1] + [E(self.ref.marginal_loglik(T == 1, None if T == 1 else xprev, hist[T - 1]), ws[-1].e)]:
                    tot = w if tot is None else tot + w
                v.value("introduce conjugacy lw", i, lw[i], tot)
        self.n = a.n = n_old + n_add
        self._lml_estimate(v, "log_ml_estimate", hw.Softmax(lw))
        self._note("introduce", v)
        self.epoch += 1
        self.obs = hist[-1]

    # ---- getters and statistics against the definitions
    def check_summaries(self, addrs=(), discrete=()):
        """effective_sample_size, log_ml_estimate, get_log_norm_weights, get_norm_weights, and mean / var (addrs) / proportionmap (discrete)
        of columns of the current step or (step, column) addresses of a past one"""
        a, lw, v = self.a, self.a.lw, Violations()
        sm = hw.Softmax(lw)
        if sm.invalid:                                                       # utils.jl:100-107: lognorm / softmax of all -Inf are NaN
            assert np.isnan(a.ess()) and np.isnan(a.norm_weights()).all() and np.isnan(a.log_norm_weights()).all()
        else:
            v.value("ess", 0, a.ess(), sm.ess(), guard=sum_guard(sm))
            self._lml_estimate(v, "log_ml_estimate", sm)
            got_l, got_w = a.log_norm_weights(), a.norm_weights()
            for i, (wl, ww) in enumerate(zip(hw.log_norm_weights(sm), hw.norm_weights(sm))):
                if lw[i] == -np.inf:
                    assert got_l[i] == -np.inf and got_w[i] == 0.0, i
                    continue
                v.value("log_norm_weights", i, got_l[i], wl)
                v.value("norm_weights", i, got_w[i], ww)
        for addr in addrs:
            x = a.column(addr)
            v.value(f"mean ({addr})", 0, a.mean(addr), hw.mean(sm, x), guard=sum_guard(sm))
            v.value(f"var ({addr})", 0, a.var(addr), hw.var(sm, x), guard=sum_guard(sm))
        for addr in discrete:
            x, pm = a.column(addr), a.proportionmap(addr)
            assert sorted(pm) == sorted(float(t) for t in np.unique(x)), addr
            for val, got in pm.items():
                v.value(f"proportion ({addr} = {val})", 0, got, hw.proportion(sm, x, val), guard=sum_guard(sm))
        self._note("getters and statistics", v)               # one case: the median bound is over all its values

    def check_blocks(self, nb, col, discrete_col=None):
        """block_stats, block_mean / block_var and block_proportionmap: block b is the sub-state of its particles (view.jl:16-48)"""
        a, lw, rows, v = self.a, self.a.lw, self.a.rows, Violations()
        ess, lml = a.block_stats(nb)
        mu, s2 = a.block_moments(nb, col)
        if discrete_col is not None:
            vals, pr = a.block_proportionmap(nb, discrete_col)
            assert np.array_equal(vals, np.unique(rows[:, discrete_col]))
        for b, i0 in enumerate(range(0, self.n, nb)):
            sm = hw.Softmax(lw[i0:i0 + nb])
            x = rows[i0:i0 + nb, col]
            if sm.invalid:                                                   # the uniform fallback answers mean / var / proportions
                assert np.isnan(ess[b]) and lml[b] == -np.inf, b
            else:
                v.value("block ess", b, ess[b], sm.ess(), guard=sum_guard(sm))
                v.value("block log_ml_estimate", b, lml[b], hw.lml_estimate_from(self.lml, sm), guard=sum_guard(sm))
            v.value("block mean", b, mu[b], hw.mean(sm, x), guard=sum_guard(sm))
            v.value("block var", b, s2[b], hw.var(sm, x), guard=sum_guard(sm))
            if discrete_col is not None:
                xd = rows[i0:i0 + nb, discrete_col]
                for k, val in enumerate(vals):
                    v.value(f"block proportion ({val})", b, pr[b, k], hw.proportion(sm, xd, val), guard=sum_guard(sm))
        self._note(f"blocks of {nb}", v)

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

    def step_ess(self, obs, ess_threshold=0.5, must_decide=False, method="multinomial"):
        """pf_step_ess: (resample if ESS < threshold N), update, in one call.  The resampled x_{t-1} is what the new row keeps in its second
        half: an old row, from which the update is predicted; the weights restart from 0 after a multinomial resample."""
        obs = np.ascontiguousarray(obs, np.float64)
        rows0, lw0 = self.a.rows, self.a.lw
        resampled = self.a.step_ess(obs, ess_threshold) if method == "multinomial" else self.a.step_ess(obs, ess_threshold, method)
        rows, lw, v, d = self.a.rows, self.a.lw, Violations(), self.d
        # the verdict ESS < threshold N is the reference's wherever the reference can tell
        sm0 = hw.Softmax(lw0)
        ess, cut = sm0.ess(), E(ess_threshold) * float(self.n)
        decidable = abs(float(ess.v - cut.v)) > ess.e + cut.e
        assert decidable or not must_decide, f"step_ess: ESS {ess} against {cut} is not decidable: choose another threshold"
        if decidable:
            assert resampled == bool(ess.v < cut.v), (resampled, ess, cut)
        if resampled:
            # the resample of the call, seen through the update that followed it: ancestors, the gathered x_{t-1}, the log-ML estimate
            parents0 = np.asarray(self.a.parents) - 1
            assert method in ("multinomial", "multinomial_sorted"), method       # the forms whose weights restart from 0 with every slot drawn
            ref = (hw.multinomial if method == "multinomial" else hw.sorted_multinomial)(sm0, self.seed, self.epoch)
            assert hw.check_ancestors(ref, parents0, sm0, "step_ess resample") <= MAX_UNDECIDABLE
            if method == "multinomial_sorted":
                assert (np.diff(parents0) >= 0).all(), "step_ess: the ancestors of the sorted multinomial are not non-decreasing"
            assert np.array_equal(np.ascontiguousarray(rows[:, d:2 * d]).view(np.uint64), np.ascontiguousarray(rows0[parents0][:, :d]).view(np.uint64))
            self.lml = self.lml + (sm0.lse() - hw.log_n(self.n))
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
        self._lml_estimate(v, "log_ml_estimate", hw.Softmax(lw))
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


# ------------------------------------------------------------------------------------------- ancestor sampling, backward simulation, smoothing
# tests/test_hp_block_smoothing.py (the NumPy restatements on the CPU oracle's filter) and tests/test_gpu_hp_block_smoothing.py (the device) drive
# these three with plain arrays: the Store of tests/block_backward_spec.py filled from what a caller sees, the seed, the epoch and the outputs
# of the implementation under test.  Who produced the outputs is unknown here.  Every tolerance is an E bound of tests/hp_weights.py.
class _Worst:
    """the worst err / bound per quantity of ONE call of a check, printed when the call ends (profiles/hp_block_smoothing.md)"""

    def __init__(self):
        self.by = {}

    def add(self, what, got, want: E):
        if want.e > 0.0 and np.isfinite(got):
            d, t = hp.differs(got, want)
            self.by[what] = max(self.by.get(what, 0.0), d / t)

    def show(self, label, left=None):
        und = "" if left is None else f", undecidable draws {sum(left.values())} (most per block and step {max(left.values(), default=0)})"
        print(f"{label}: worst err / bound {({k: round(r, 3) for k, r in self.by.items()})}{und}")


def _span(n, bs, b):
    return b * bs, min((b + 1) * bs, n)


def smoothing_guard(n, K, e_max):
    """sum_guard for weights formed from inexact exponents: the counts' N 2^-K as there, plus the relative error expm1(2 e_max) that an absolute
    error e_max of the exponents (and of their maximum) is of every weight, the same factor 64 for a second moment"""
    return max(MEDIAN_REL_TOL, 64.0 * (n * 2.0 ** -K + np.expm1(2.0 * e_max)))


def check_logtrans(v, refs, bs, blocks, rows, x_ref, obs, got, label):
    """block_ancestor_log_weights with log_weights = 0 is logtrans itself, up to the terms free of xp that an implementation may drop: over a
    block's particles the intervals [full_i - got_i +- e_i] must share a point (full: the complete Gen log-density, e_i: the derived bound of
    Ref.logtrans).  -Inf (line_model: another slope) is exact.  Returns the worst (max lower end - min upper end) / (sum of the two bounds)."""
    rows, got = np.asarray(rows, np.float64), np.asarray(got, np.float64)
    worst = 0.0
    for b in blocks:
        i0, i1 = _span(len(got), bs, b)
        lo_i = hi_i = None
        for i in range(i0, i1):
            d = len(x_ref[b])
            full, part = refs[b].logtrans(list(rows[i, :d]), list(x_ref[b]), obs[b], full=True), refs[b].logtrans(list(rows[i, :d]), list(x_ref[b]), obs[b])
            if full.v == -hp.M.inf:
                v.exact(f"{label}: logtrans of an impossible transition", i, got[i], -np.inf)
                continue
            if not np.isfinite(got[i]):
                v.bad.append((f"{label}: logtrans", i, float(got[i]), hp.M.nstr(part.v, 20), None, part.e))
                continue
            v.tols.append(hp.rel_tol(part))
            c = full.v - hp.mpf(float(got[i]))
            if lo_i is None or c - part.e > lo_i[0]:
                lo_i = (c - part.e, i, part.e)
            if hi_i is None or c + part.e < hi_i[0]:
                hi_i = (c + part.e, i, part.e)
        if lo_i is not None:
            gap, room = float(lo_i[0] - hi_i[0]), lo_i[2] + hi_i[2]
            worst = max(worst, gap / room + 1.0 if room > 0.0 else 0.0)     # 0: the two extreme centres coincide, 1: the intervals just touch
            if gap > 0:
                v.bad.append((f"{label}: block {b}: no common constant", (lo_i[1], hi_i[1]), float(got[lo_i[1]]), float(got[hi_i[1]]), gap, room))
    print(f"{label}: worst err / bound {round(worst, 3)}")
    return worst


def check_ancestor(v, refs, bs, blocks, rows, lw, x_ref, obs, seed, epoch, resampled, parents, label):
    """a_0 of pf_resample_blocks(..., conditional=True, reference=, observations=): rows / lw the state BEFORE the call, parents / resampled after
    it.  Slot 0 of a block that resampled holds parent a_0 + 1; the decidable draws equal hw.ancestor_draw, a -Inf or flushed candidate is never
    drawn, invalid ancestor weights give a_0 = 0.  A block that did not resample drew nothing and is left out of the result: the caller asserts
    which blocks it expects.  Returns {block: undecidable draws}."""
    rows, lw, left = np.asarray(rows, np.float64), np.asarray(lw, np.float64), {}
    for b in blocks:
        if not resampled[b]:
            continue
        i0, i1 = _span(len(lw), bs, b)
        d = len(x_ref[b])
        got = int(parents[i0]) - 1
        a, und, sm = hw.ancestor_draw(refs[b], lw[i0:i1], rows[i0:i1, :d], x_ref[b], obs[b], seed, epoch, i0)
        left[b] = int(und)
        if sm is hw.FALLBACK:
            v.exact(f"{label}: a_0 under invalid ancestor weights", b, got, 0)
            continue
        if not 0 <= got < i1 - i0 or sm.dead[got]:
            v.bad.append((f"{label}: a_0 is no candidate of weight", b, got, a, None, 0.0))
        elif not und:
            v.exact(f"{label}: a_0", b, got, a)
    _Worst().show(label, left)
    assert all(k <= MAX_UNDECIDABLE for k in left.values()), (label, left)
    return left


def check_backward(v, refs, store, blocks, seed, epoch, idx, label):
    """indices [B, n_samples, T] (1-based, global) of block_backward_trajectories(..., return_indices=True) over all T steps of `store`, the call
    made under `epoch`: step T against the categorical draw hw.multinomial, every transition against hw.backward_step GIVEN the particle the
    implementation holds at the step above.  Returns {(block, step): undecidable draws}."""
    T, bs, n = store.steps, store.bs, store.n
    idx, left = np.asarray(idx), {}
    ns = idx.shape[1]
    lwT = np.asarray(store.lw[T - 1], np.float64)
    maps = {s: store.step_map(s) for s in range(2, T + 1)}
    for b in blocks:
        b0, b1 = _span(n, bs, b)
        if np.isnan(lwT[b0:b1]).any() or (lwT[b0:b1] == np.inf).any():
            for j in range(ns):
                for s in range(T):
                    v.exact(f"{label}: index of a NaN block", (b, j, s), idx[b, j, s], 0)
            continue
        sm = hw.Softmax(lwT[b0:b1])
        left[(b, T)] = hw.check_ancestors(hw.multinomial(sm, seed, epoch, ns, slot0=b * ns), idx[b, :, T - 1] - 1 - b0, sm, f"{label}: block {b} step T")
        for s in range(T - 1, 0, -1):                                           # the step being drawn; the held particle is of step s + 1
            cache, und_s = {}, 0
            for j in range(ns):
                p, got = int(idx[b, j, s]) - 1, int(idx[b, j, s - 1]) - 1
                pm = int(maps[s + 1][p])
                c0, c1 = _span(n, bs, pm // bs)
                a, und, sm = hw.backward_step(refs[b], store.lw[s - 1][c0:c1], store.x(s)[c0:c1], store.x(s + 1)[p], store.obs[s][p // bs], seed, epoch + (T - s),
                                              b * ns + j, sm=cache.get(p))
                cache[p] = sm
                if sm is hw.FALLBACK:
                    v.exact(f"{label}: a held particle no candidate leads to takes its recorded parent", (b, j, s), got, pm)
                    continue
                if not c0 <= got < c1 or sm.dead[got - c0]:
                    v.bad.append((f"{label}: the drawn index is no candidate of weight", (b, j, s), got, c0 + a, None, 0.0))
                elif und:
                    und_s += 1
                else:
                    v.exact(f"{label}: backward index", (b, j, s), got, c0 + a)
            left[(b, s)] = und_s
    _Worst().show(label, left)
    assert all(k <= MAX_UNDECIDABLE for k in left.values()), (label, left)
    return left


def pairs_guard(n, K, e_max, scale, value):
    """What the bound of a RAW second or lag-one cross moment sum_i W_i g_i, g = x[a] x[c] (or sum_ij t_ij x_s^i[a] x_{s+1}^j[c]), may not exceed,
    relative to max(1, |value|) as Violations.value measures it: smoothing_guard's form with the amplification 128 in place of 64, on the entry's
    own scale m = sqrt(m_aa m_cc), m_aa = sum W x[a]^2 and m_cc = sum W x[c]^2 the raw second moments of the two columns (of steps s and s + 1
    for a cross moment):

        max(MEDIAN_REL_TOL, 128 (N 2^-K + expm1(2 e_max))) max(1, m) / max(1, |value|).

    Where the 128 comes from.  As in sum_guard every weight is off by up to half a count whatever its size, N 2^-K relative for the numerator
    and S together, and by expm1(2 e_max) of itself; a weight's error enters the sum times |g_i|.  Under sum_guard's own condition -- no particle
    further than 8 standard deviations from the weighted mean -- x[a]^2 <= (|mu_a| + 8 sigma_a)^2 <= 2 mu_a^2 + 128 sigma_a^2 <= 128 (mu_a^2 +
    sigma_a^2) = 128 m_aa, so |g_i| <= sqrt(128 m_aa 128 m_cc) = 128 m: twice sum_guard's 64, because an uncentred moment also carries the mean.
    The part proportional to the weights needs less: sum W |g| <= m by Cauchy-Schwarz, amplification 1.  On the diagonal m = value and the guard
    is the plain constant; an off-diagonal or cross entry can be near 0 while its terms are not (a correlation near 0), and a rounding is
    proportional to the terms, so there the bound is held against m: a mistake of meaning (a transposed, shifted, centred or independent entry)
    moves an entry by a fraction of m, twelve orders of magnitude above this.  The roundings of the accumulation into A and of the tree, (targets
    + levels + 4) 2^-53 of sum |terms| <= m, are below N 2^-K for K <= 52 and sit inside the same constant.  Derived, not fitted to any output:
    a condition on the case, which changes its inputs if its own bounds do not stay below it."""
    return max(MEDIAN_REL_TOL, 128.0 * (n * 2.0 ** -K + np.expm1(2.0 * e_max))) * max(1.0, scale) / max(1.0, abs(value))


def reference_walk(refs, store, blocks, lo=None, stop=1, pairs=False):
    """The walk of the reference, written once for check_smooth and check_pairs as the kernels share block_store_walk: the list of what the
    definition says of every checked block b, from step T down to max(stop, lo[b]) --
        ("nan", b)                                   current weights with NaN / +Inf: everything of the block is NaN, its lineage 0;
        ("step", b, s, c, c0, c1, W, e_max, A)       step s: the lineage is in block c = particles [c0, c1), W one E per particle (hw.norm_weights
                                                     at T, hw.smooth_step below), e_max the largest bound of an ancestor weight met so far, A the pair
                                                     sums of the walk from s + 1 to s (pairs=True and s < T, else None);
        ("undefined", b, s)                          the particles of step s have their recorded parents in several blocks: no lineage below s;
        ("fallbacks", k)                             last: the (target, step) pairs that took the fallback.
    The targets' observation row is that of THEIR block c at step s + 1, the candidates are the block cp of their recorded parents, the parameters
    the final block b's.  A list, so that two checks of one case share one walk (pairs=True serves both)."""
    T, bs, n = store.steps, store.bs, store.n
    lwT, fallbacks, out = np.asarray(store.lw[T - 1], np.float64), 0, []
    for b in blocks:
        c, (c0, c1) = b, _span(n, bs, b)
        if np.isnan(lwT[c0:c1]).any() or (lwT[c0:c1] == np.inf).any():
            out.append(("nan", b))
            continue
        W, e_max, A = hw.norm_weights(hw.Softmax(lwT[c0:c1])), 0.0, None
        for s in range(T, 0, -1):
            out.append(("step", b, s, c, c0, c1, W, e_max, A))
            if s == max(1, stop, (lo or {}).get(b, 1)):
                break
            pm = store.step_map(s)[c0:c1]
            born = pm // bs
            if born.min() != born.max():
                out.append(("undefined", b, s))
                break
            cp = int(born[0])
            p0, p1 = _span(n, bs, cp)
            lwc, xc, xt = store.lw[s - 2][p0:p1], store.x(s - 1)[p0:p1], store.x(s)[c0:c1]
            W, fell, em, *A = hw.smooth_step(refs[b], W, xt, lwc, xc, store.obs[s - 1][c], pm - p0, pairs=pairs)
            A = A[0] if pairs else None
            fallbacks, e_max = fallbacks + len(fell), max(e_max, em)
            c, c0, c1 = cp, p0, p1
    return out + [("fallbacks", fallbacks)]


def check_smooth(v, refs, store, blocks, mean, var, weights, lineage, label, lo=None, walk=None):
    """mean, var [B, T, d], weights [B, T, bs], lineage [B, T] of block_smoothed_moments(..., return_weights=True, return_blocks=True) over all T
    steps of `store`: W_T against the block's normalised weights, every step below against hw.smooth_step applied from T downward, mean and variance
    against hw.mean / hw.var under the reference's W.  `lo`: {block: the lowest step checked} (default 1: all).  `walk`: reference_walk(refs, store,
    blocks, lo) where the caller has it already.  Returns the number of (target, step) pairs that took the fallback."""
    d, worst = store.d, _Worst()
    for ev in reference_walk(refs, store, blocks, lo) if walk is None else walk:
        if ev[0] == "nan":
            b = ev[1]
            assert np.isnan(mean[b]).all() and np.isnan(var[b]).all() and np.isnan(weights[b]).all() and (lineage[b] == 0).all(), (label, b, "a NaN block")
        elif ev[0] == "undefined":                                              # the lineage is undefined from step s - 1 down
            b, s = ev[1:]
            assert np.isnan(mean[b, :s - 1]).all() and np.isnan(var[b, :s - 1]).all() and np.isnan(weights[b, :s - 1]).all() and (lineage[b, :s - 1] == 0).all()
        elif ev[0] == "step":
            b, s, c, c0, c1, W, e_max, _ = ev[1:]
            what = f"{label}: W (block {b}, step {s})"
            assert lineage[b, s - 1] == c + 1, (label, b, s, lineage[b], c + 1)
            lws = np.asarray(store.lw[s - 1], np.float64)[c0:c1]
            for i, w in enumerate(W):
                if lws[i] == -np.inf or (w.v == 0 and w.e == 0.0):
                    v.exact(what + ", a particle of weight 0", i, weights[b, s - 1, i], 0.0)
                else:
                    v.value(what, i, weights[b, s - 1, i], w)
                    worst.add("W", weights[b, s - 1, i], w)
            assert np.all(weights[b, s - 1, c1 - c0:] == 0.0), (label, b, s, "beyond a short block")
            ws, guard = hw.Weighted(W), smoothing_guard(c1 - c0, hw.fix_K(c1 - c0), e_max)
            for col in range(d):
                x = store.x(s)[c0:c1, col]
                for name, got, want in (("mean", mean[b, s - 1, col], hw.mean(ws, x)), ("var", var[b, s - 1, col], hw.var(ws, x))):
                    v.value(f"{label}: smoothed {name}", (b, s, col), got, want, guard=guard)
                    worst.add(name, got, want)
        else:
            fallbacks = ev[1]
    worst.show(label)
    return fallbacks


def check_pairs(v, refs, store, blocks, mean, second, cross, lineage, label, lo=None, steps=None, walk=None):
    """mean [B, ns, d], second [B, ns, d, d], cross [B, ns - 1, d, d], lineage [B, ns] of block_smoothed_pair_moments(..., steps=, return_blocks=True)
    against the definition: the walk of check_smooth (reference_walk, pairs=True) from step T of `store`; at every step of the window
    the lineage, mean against hw.mean, every entry of second against hw.second and second exactly symmetric; for every pair (s, s + 1) of the window
    every entry of cross against hw.cross over hw.smooth_step's pair sums.  `steps` = (lo, hi): a windowed call -- walked from T, written for [lo, hi]
    only, ns = hi - lo + 1 steps and hi - lo pairs (default: all T).  `lo`: {block: the lowest step checked}.  NaN and lineage 0 for a NaN block and
    below the step where the lineage is undefined, the pair whose lower step is undefined included.  The sums' own bounds must stay below
    smoothing_guard (mean) and pairs_guard (second, cross).

    A particle of smoothing weight exactly 0 may hold a non-finite latent (it is a target the walk skips entirely).  By the statements of 5.7 the
    entries of ITS step that multiply that column are NaN -- mean[col], second[col][.] and second[.][col] (0 * Inf), cross_s[col][.] of the pair
    above it (Inf * A with A = +0.0) -- and are asserted to be; everything else, the pair below it and all lower steps, is finite and compared
    with the reference, in which the particle contributes nothing.  Returns the fallbacks of the walk."""
    T, d = store.steps, store.d
    wlo, whi = (1, T) if steps is None else steps
    ns = whi - wlo + 1
    assert mean.shape[1:] == (ns, d) and second.shape[1:] == (ns, d, d) and cross.shape[1:] == (ns - 1, d, d) and lineage.shape[1:] == (ns,), (label, "shapes")
    worst, diag_above, room = _Worst(), None, {}

    def value(name, at, got, want, guard):
        """one compared sum: the violation, the worst err / bound, and how much of its guard the reference's own bound takes"""
        v.value(f"{label}: {name}", at, got, want, guard=guard)
        key = name.split()[-1]
        worst.add(key, got, want)
        room[key] = max(room.get(key, 0.0), hp.rel_tol(want) / guard)

    for ev in reference_walk(refs, store, blocks, lo, stop=wlo, pairs=True) if walk is None else walk:
        if ev[0] == "nan":
            b = ev[1]
            assert np.isnan(mean[b]).all() and np.isnan(second[b]).all() and np.isnan(cross[b]).all() and (lineage[b] == 0).all(), (label, b, "a NaN block")
        elif ev[0] == "undefined":                                              # steps below s and every pair whose lower step is below s
            b, k = ev[1], ev[2] - wlo
            assert np.isnan(mean[b, :k]).all() and np.isnan(second[b, :k]).all() and np.isnan(cross[b, :k]).all() and (lineage[b, :k] == 0).all(), (label, b, ev[2])
        elif ev[0] == "step":
            b, s, c, c0, c1, W, e_max, A = ev[1:]
            ws, x, k = hw.Weighted(W), np.array(store.x(s)[c0:c1], np.float64), s - wlo
            odd = ~np.isfinite(x)
            assert all(W[i].v == 0 and W[i].e == 0.0 for i in np.nonzero(odd.any(axis=1))[0]), (label, b, s, "a non-finite row of a particle of weight: not a case")
            nan_col = odd.any(axis=0)
            x[odd] = 0.0                                                        # in the definition a particle of weight 0 contributes nothing
            diag = [float(hw.second(ws, x, a, a).v) for a in range(d)]
            n_c, K = c1 - c0, hw.fix_K(c1 - c0)
            if s <= whi:
                assert lineage[b, k] == c + 1, (label, b, s, lineage[b], c + 1)
                assert bits_equal_nan(second[b, k], second[b, k].T).all(), (label, b, s, "second is not symmetric")
                for a in range(d):
                    if nan_col[a]:
                        assert np.isnan(mean[b, k, a]) and np.isnan(second[b, k, a]).all(), (label, b, s, a, "0 * Inf")
                        continue
                    value("smoothed mean", (b, s, a), mean[b, k, a], hw.mean(ws, x[:, a]), smoothing_guard(n_c, K, e_max))
                    for col in range(a, d):
                        if nan_col[col]:
                            continue
                        want = hw.second(ws, x, a, col)
                        guard = pairs_guard(n_c, K, e_max, math.sqrt(diag[a] * diag[col]), float(want.v))
                        value("second", (b, s, a, col), second[b, k, a, col], want, guard)
                        value("second", (b, s, col, a), second[b, k, col, a], want, guard)
            if A is not None and s + 1 <= whi and s >= wlo:                     # the pair (s, s + 1)
                for a in range(d):
                    if nan_col[a]:
                        assert np.isnan(cross[b, k, a]).all(), (label, b, s, a, "Inf * +0.0")
                        continue
                    for col in range(d):
                        want = hw.cross(x, A, a, col)
                        guard = pairs_guard(n_c, K, e_max, math.sqrt(diag[a] * diag_above[col]), float(want.v))
                        value("cross", (b, s, a, col), cross[b, k, a, col], want, guard)
            diag_above = diag
        else:
            fallbacks = ev[1]
    worst.show(label)
    print(f"{label}: worst bound / guard {({k: float(f'{r:.2g}') for k, r in room.items()})}")
    return fallbacks


def _both(x):
    return set(np.unique(x)) == {0.0, 1.0}


def moving_inputs(store, blocks, held=None, travelling=False, label="object_motion"):
    """object_motion: what a case must hold before anything is compared -- every checked block has both `moving` states among its candidates at
    some step below T, both appear among the targets / held particles, the covariate obs[1] differs between consecutive steps and between the
    checked blocks, and the blocks' observation rows differ.  Blocks of five and seven particles rarely keep both states through every resample, so
    the (block, step) pairs whose candidates hold both are returned and printed: those are where the Bernoulli rows are chosen between.
    `travelling`: the nested filter, whose rows move between blocks -- two blocks may then hold copies of one row, and more than one checked block,
    not every one, must hold both states."""
    T, bs, n = store.steps, store.bs, store.n
    seen, both = set(), []
    for b in blocks:
        b0, b1 = _span(n, bs, b)
        both += [(b, s) for s in range(1, T) if _both(store.x(s)[b0:b1, 0])]
        for s in range(1, T):
            assert store.obs[s - 1][b][1] != store.obs[s][b][1], ("the covariate does not change between steps", b, s)
        seen |= set(np.unique(store.x(T)[b0:b1, 0] if held is None else held[b]))
    with_both = {b for b, _ in both}
    print(f"{label}: candidates of both `moving` states at (block, step) {both}")
    assert len(with_both) > 1 if travelling else with_both == set(blocks), ("candidates of one `moving` state only", sorted(set(blocks) - with_both))
    assert seen == {0.0, 1.0}, ("targets of one `moving` state only", seen)
    if not travelling:
        for s in range(T):
            rows = [tuple(store.obs[s][b]) for b in blocks]
            assert len(set(rows)) == len(rows) and len({r[1] for r in rows}) == len(rows), ("blocks share an observation row or a covariate", s)
    return both


def moving_ancestor_inputs(bs, blocks, calls, label="object_motion"):
    """the same for ancestor sampling; calls: one (rows before the call, reference [B, d], observations [B, n_obs]) per ancestor resample.  Every
    checked block has both `moving` states among its candidates in some call (returned and printed: which) and enters with a moving and with a
    still reference over the calls; the covariates differ between the calls and between the checked blocks, and so do the observation rows."""
    both = []
    for b in blocks:
        for t, (rows, ref, obs) in enumerate(calls):
            i0, i1 = _span(len(rows), bs, b)
            if _both(np.asarray(rows)[i0:i1, 0]):
                both.append((b, t + 1))
        assert _both([ref[b][0] for _, ref, _ in calls]), ("a block whose reference has one `moving` state only", b)
        cov = [obs[b][1] for _, _, obs in calls]
        assert len(set(cov)) == len(cov), ("the covariate does not change between steps", b)
    print(f"{label}: candidates of both `moving` states at (block, call) {both}")
    assert {b for b, _ in both} == set(blocks), ("candidates of one `moving` state only", sorted(set(blocks) - {b for b, _ in both}))
    for _, _, obs in calls:
        r = [tuple(obs[b]) for b in blocks]
        assert len(set(r)) == len(r) and len({x[1] for x in r}) == len(r), "blocks share an observation row or a covariate"
    return both


def moving_references(ref):
    """[B, T, d] reference values of object_motion whose `moving` flag alternates over blocks and steps: every block enters with a moving and with a
    still reference"""
    ref = np.array(ref, np.float64)
    B, T = ref.shape[:2]
    ref[..., 0] = (np.arange(B)[:, None] + np.arange(T)[None, :]) % 2
    return ref


def case_model(g, name):
    """the models of these cases: where the defaults make two parameters equal -- bearings4's sp = sv, object_motion's p(moving|still) =
    1 - p(moving|moving) -- exchanging them would change nothing, so they are set apart; sb as in the block-wise device tests"""
    if name == "bearings4":
        return g.models.bearings4(sb=0.5, sp=0.002, sv=0.0005)
    if name == "object_motion":
        return g.models.object_motion(p_stay=0.9, p_start=0.3)
    return g.models.line_model() if name == "line_model" else g.models.by_name(name)


def moving_obs(base, seed=8, lo=0.02, hi=0.15):
    """[B, T, 2] observation rows for object_motion from `base` (any per-block data): the covariate obs[1] -- the velocity a moving object adds --
    becomes a small value of its own per block and step, so that the measured position does not tell the two `moving` states apart and blocks of
    seven particles keep both; against sy = 0.01 a covariate of another block or step is still many standard deviations off.  The seed is the
    first at which moving_inputs holds at every shape of the tests (block sizes 7, 129, 513; 3 and 4 steps), found on the CPU oracle's filter"""
    ys = np.array(base, np.float64)
    ys[..., 1] = np.random.default_rng(seed).uniform(lo, hi, ys.shape[:2])
    return ys
