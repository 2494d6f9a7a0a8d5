"""Host-side mirror of the reference's operator interface for the hot path.

Same names, argument meaning and error behaviour as GenParticleFilters.jl v0.2.3 (Julia's `f!`
is spelled `f` here; the Julia glue in julia/GenParticleFiltersAMD.jl keeps the bang):

    pf_initialize(model, model_args, observations, n_particles)        src/initialize.jl:31-44
    pf_update(state, new_args, argdiffs, observations)                 src/update.jl:12-25
    pf_resample(state, method; priority_fn, check[, sort_particles])   src/resample.jl:19-175
    pf_rejuvenate(state, kern, kern_args, n_iters; method)             src/rejuvenate.jl:18-90
    pf_coalesce(state; by) / pf_introduce(state, ..., n)               src/resize.jl:309-421
    effective_sample_size / get_ess / log_ml_estimate / get_lml_est /
    get_log_weights / get_log_norm_weights / get_norm_weights          src/utils.jl:148-186
    mean / var                                                         src/statistics.jl:13-14,48-50

Every call goes through the C ABI of libgpf_hip.so (include/gpf.h); nothing is computed on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import warnings
from collections import namedtuple

import numpy as np

from . import _lib
from .models import NativeModel

RESAMPLE_METHODS = {"multinomial": 0, "residual": 1, "stratified": 2,
                    "multinomial_sorted": 4}   # opt-in extension (gpf.h GPF_RESAMPLE_MULTINOMIAL_SORTED): ancestors come out non-decreasing
REJUVENATE_METHODS = {"move": 0, "reweight": 1}


class ErrorException(RuntimeError):
    """Julia's ErrorException, raised where the reference calls error(...)."""


class Tempering:
    """priority_fn = w -> alpha * w (reference test/resample.jl:15 uses alpha = 1/2); evaluated on the GPU."""

    def __init__(self, alpha: float):
        self.alpha = float(alpha)

    def __call__(self, w):
        return self.alpha * w


# native rejuvenation kernels (the `kern` argument of pf_rejuvenate)
class _NativeKernel:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return f"<native kernel {self.name}>"


# native proposal for the custom-proposal forms of pf_initialize / pf_update (src/initialize.jl:46-62, src/update.jl:79-96)
locally_optimal = _NativeKernel("locally_optimal")     # exact conditional q(x_t | x_{t-1}, y_t); lgssm2 only
# the proposals of the reference's own tests for line_model as one native proposal: slope ~ uniform_discrete(0, 0) at the
# first step (test/initialize.jl:16-17), outlier ~ bernoulli(0.0) at every step (test/initialize.jl:18-19, test/update.jl:42-43)
line_fixed = _NativeKernel("line_fixed")
_PROPOSAL_IDS = {"locally_optimal": 1, "line_fixed": 2}


def _proposal_id(proposal) -> int:
    if not isinstance(proposal, _NativeKernel) or proposal.name not in _PROPOSAL_IDS:
        raise ErrorException("device filters support native proposals only (`locally_optimal`, `line_fixed`)")
    return _PROPOSAL_IDS[proposal.name]

mh = _NativeKernel("mh")                        # Gen.mh(trace, select(current step latent))
move_reweight = _NativeKernel("move_reweight")  # move_reweight(trace, selection), src/rejuvenate.jl:125-132


def _pd(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class DeviceParticleFilterState:
    """Device-resident counterpart of Gen.ParticleFilterState{U} (fields traces / new_traces /
    log_weights / log_ml_est / parents).  Owns an opaque libgpf handle."""

    def __init__(self, model: NativeModel, n_particles: int, seed: int = 1, keep_prev: bool = False,
                 device: int = 0, n_global: int | None = None, gid0: int = 0, stream: int | None = None,
                 history: int = 0, history_blocks: bool = False, history_weights: bool = False):
        self._L = _lib.load()
        self.model, self.n_particles, self.seed = model, int(n_particles), int(seed)
        self.keep_prev = bool(keep_prev)
        self._params = np.ascontiguousarray(model.params, np.float64)
        cfg = _lib.GpfConfig()
        cfg.abi_version, cfg.model, cfg.n_params = _lib.ABI_VERSION, model.model_id, self._params.size
        cfg.keep_prev, cfg.params = int(self.keep_prev), _pd(self._params)
        cfg.n_particles = self.n_particles
        cfg.n_global = self.n_particles if n_global is None else int(n_global)
        cfg.gid0, cfg.seed, cfg.device, cfg.stream = int(gid0), self.seed, int(device), stream
        self._h = C.c_void_p()
        st = self._L.gpf_create(C.byref(cfg), C.byref(self._h))
        if st != _lib.OK:
            msg = self._L.gpf_last_error(None).decode()
            self._h = None
            raise ErrorException(f"gpf_create failed ({st}): {msg}")
        d, w = C.c_int32(), C.c_int32()
        self._L.gpf_state_dim(self._h, C.byref(d), C.byref(w))
        self.dim, self.row_width = d.value, w.value
        self.history_blocks = bool(history and history_blocks)
        self.history_weights = bool(self.history_blocks and history_weights)   # ... with the records of a backward pass (gpf_history_enable_blocks_weights)
        if history:                      # trajectory store for `history` time steps (persistent-trace queries); history_blocks: the block-wise
            enable = self._L.gpf_history_enable_blocks if history_blocks else self._L.gpf_history_enable   # calls feed it too (gpf.h)
            if self.history_weights:
                enable = self._L.gpf_history_enable_blocks_weights
            self._check(enable(self._h, int(history)))

    # -- state[idxs] / view(state, idxs): a sub-state over a range start:step:stop or over ANY vector of distinct indices
    #    (src/view.jl:35-48 takes `idxs::AbstractVector`; the reference's tests use contiguous and strided ranges, state[1:50],
    #    state[k:5:100]).  0-based half-open Python slices / ranges, or a list / NumPy array of 0-based indices.
    def __getitem__(self, idx):
        if isinstance(idx, slice):
            start, stop, step = idx.indices(self.n_particles)
        elif isinstance(idx, range):
            start, stop, step = idx.start, idx.stop, idx.step
        elif isinstance(idx, (list, tuple, np.ndarray)):
            ix = np.asarray(idx)
            if ix.dtype == bool:                                    # state[mask], like Julia's logical indexing
                if ix.shape != (self.n_particles,):
                    raise ErrorException("a boolean index must have one entry per particle")
                ix = np.flatnonzero(ix)
            if ix.ndim != 1 or ix.size == 0 or not np.issubdtype(ix.dtype, np.integer):
                raise ErrorException("device sub-states over an index vector need a non-empty 1-D integer array")
            return DeviceParticleFilterSubState(self, int(ix[0]), ix.size, 0, index=np.ascontiguousarray(ix, np.int64))
        else:
            raise TypeError("device sub-states: use state[a:b], state[a:b:step] or state[index_vector]")
        if step < 1 or stop <= start:
            raise ErrorException("device sub-states cover non-empty ranges with a positive step")
        return DeviceParticleFilterSubState(self, start, (stop - start + step - 1) // step, step)

    def view(self, idx):
        return self[idx]

    # -- plumbing
    def _check(self, st: int):
        if st != _lib.OK:
            raise ErrorException(self._L.gpf_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.gpf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self._L.gpf_synchronize(self._h))

    def checkpoint(self) -> np.ndarray:
        """gpf.h gpf_checkpoint_save: the whole state (population, log-weights, parents, log-ML estimate, RNG epoch, latest observation) as one uint8 array;
        `restore` on a state created with the same arguments continues bit for bit"""
        nb = C.c_int64(0)
        self._check(self._L.gpf_checkpoint_size(self._h, C.byref(nb)))
        out = np.empty(nb.value, np.uint8)
        self._check(self._L.gpf_checkpoint_save(self._h, out.ctypes.data, nb.value))
        return out

    def restore(self, blob):
        """gpf.h gpf_checkpoint_load"""
        blob = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, np.uint8)
        self._check(self._L.gpf_checkpoint_load(self._h, blob.ctypes.data, blob.size))
        return self

    def set_lazy_search(self, enable: bool = True):
        """gpf.h gpf_set_lazy_search: pf_resample(state, "multinomial") leaves its ancestor search to the pf_update that follows (one fused
        kernel); same results, off by default"""
        self._check(self._L.gpf_set_lazy_search(self._h, int(bool(enable))))
        return self

    # -- fields of ParticleFilterState
    @property
    def log_weights(self) -> np.ndarray:
        out = np.empty(self.n_particles)
        self._check(self._L.gpf_get_log_weights(self._h, _pd(out), out.size))
        return out

    @log_weights.setter
    def log_weights(self, lw):
        lw = np.ascontiguousarray(lw, np.float64)
        self._check(self._L.gpf_set_log_weights(self._h, _pd(lw), lw.size))

    @property
    def parents(self) -> np.ndarray:
        out = np.empty(self.n_particles, np.int64)
        self._check(self._L.gpf_get_parents(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), out.size))
        return out

    @property
    def log_ml_est(self) -> float:
        # the running estimate alone = log_ml_estimate - (logsumexp(lw) - log N); exposed via get_lml_est
        raise AttributeError("use get_lml_est(state); the running log_ml_est lives on the device")

    @property
    def traces(self) -> np.ndarray:
        """(n_particles, row_width) Float64 rows: columns 0..dim-1 = x_t, dim..2dim-1 = x_{t-1} if keep_prev."""
        out = np.empty((self.n_particles, self.row_width))
        self._check(self._L.gpf_get_rows(self._h, _pd(out), out.size))
        return out

    @traces.setter
    def traces(self, rows):
        rows = np.ascontiguousarray(rows, np.float64)
        self._check(self._L.gpf_set_rows(self._h, _pd(rows), rows.size))

    def column(self, col: int) -> np.ndarray:
        out = np.empty(self.n_particles)
        self._check(self._L.gpf_get_column(self._h, int(col), _pd(out), out.size))
        return out

    def history_column(self, step: int, col: int) -> np.ndarray:
        """trace[step => col] of every current particle (step is 1-based like the Julia address t => :name)"""
        out = np.empty(self.n_particles)
        self._check(self._L.gpf_history_column(self._h, int(step), int(col), _pd(out), out.size))
        return out

    # -- measurement hooks
    def kernel_timing(self, kernel_id: int, enable: bool = True):
        self._check(self._L.gpf_kernel_timing(self._h, kernel_id, int(enable)))

    def kernel_time(self, kernel_id: int):
        ms, cnt = C.c_double(), C.c_int64()
        self._check(self._L.gpf_kernel_time(self._h, kernel_id, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def debug_math(self, which: int, a, b=None):
        a = np.ascontiguousarray(a, np.float64)
        b = a if b is None else np.ascontiguousarray(b, np.float64)
        o1, o2 = np.empty_like(a), np.empty_like(a)
        self._check(self._L.gpf_debug_math(self._h, which, _pd(a), _pd(b), a.size, _pd(o1), _pd(o2)))
        return o1, o2


class DeviceParticleFilterSubState(DeviceParticleFilterState):
    """ParticleFilterSubState (src/view.jl:16-22): aliases particles start, start+step, ... (count of them) of `source`; every pf_* function
    accepts it, with the reference's sub-state semantics (local parents, no log-ML update on resampling, weights reset to
    the block average, log_ml_estimate relative to the source's running estimate)."""

    def __init__(self, source: DeviceParticleFilterState, start: int, count: int, step: int = 1, index=None):
        self.source = source                     # keeps the parent alive
        self.start, self.step = int(start), int(step)
        self.index = index                       # state[idxs] over an arbitrary index vector (step == 0)
        self._L = source._L
        self.model, self.seed, self.keep_prev = source.model, source.seed, source.keep_prev
        self.n_particles, self.dim, self.row_width = int(count), source.dim, source.row_width
        self._h = C.c_void_p()
        if index is not None:
            st = self._L.gpf_view_create_indexed(source._h, index.ctypes.data_as(C.POINTER(C.c_int64)), int(count), C.byref(self._h))
        else:
            st = self._L.gpf_view_create_strided(source._h, int(start), int(step), int(count), C.byref(self._h))
        if st != _lib.OK:
            self._h = None
            raise ErrorException(self._L.gpf_last_error(source._h).decode())


ParticleFilterState = DeviceParticleFilterState
ParticleFilterSubState = DeviceParticleFilterSubState
ParticleFilterView = (DeviceParticleFilterState, DeviceParticleFilterSubState)      # src/view.jl:32-33 (Union; use with isinstance)


def _obs_vector(observations) -> np.ndarray:
    o = observations
    if type(o) is np.ndarray and o.dtype == np.float64 and o.ndim == 1 and o.flags.c_contiguous:
        return o                                   # (the usual call: a row of the observation matrix -- nothing to convert)
    return np.ascontiguousarray(np.atleast_1d(np.asarray(o, np.float64)))


# ----------------------------------------------------------------------------- the four operations
def pf_initialize(model: NativeModel, model_args: tuple, observations, *rest, seed: int = 1,
                  keep_prev: bool = False, device: int = 0, dynamic: bool = False, **kw) -> DeviceParticleFilterState:
    """src/initialize.jl:31-44.  `model_args` is accepted for signature parity; native models take their
    time-varying inputs through the per-step data vector `observations`. `dynamic` has no meaning for
    fixed-shape device rows and is ignored."""
    # pf_initialize(model, args, obs, n_particles) | (model, args, obs, strata, n_particles; layout) |
    # (model, args, obs, proposal, proposal_args, n_particles)
    layout = kw.pop("layout", "contiguous")                        # initialize.jl:66
    strata = None
    if len(rest) == 1:
        proposal, n_particles = None, rest[0]
    elif len(rest) == 2:
        proposal, strata, n_particles = None, _strata_values(model, rest[0], "initialize"), rest[1]
    elif len(rest) == 3:
        proposal, n_particles = rest[0], rest[2]
        _proposal_id(proposal)
    elif len(rest) == 4:                                            # (strata, proposal, proposal_args, n): initialize.jl:111-129
        strata, proposal, n_particles = _strata_values(model, rest[0], "initialize"), rest[1], rest[3]
        _proposal_id(proposal)
    else:
        raise TypeError("pf_initialize(model, model_args, observations, [strata,] [proposal, proposal_args,] n_particles)")
    state = DeviceParticleFilterState(model, n_particles, seed=seed, keep_prev=keep_prev, device=device, **kw)
    obs = _obs_vector(observations)
    if strata is not None and proposal is not None:
        state._check(state._L.gpf_initialize_strata_proposal(state._h, _pd(obs), obs.size, _pd(strata), strata.size, int(_layout_id(layout)),
                                                             _proposal_id(proposal)))
    elif strata is not None:
        state._check(state._L.gpf_initialize_strata(state._h, _pd(obs), obs.size, _pd(strata), strata.size, int(_layout_id(layout))))
    elif proposal is None:
        state._check(state._L.gpf_initialize(state._h, _pd(obs), obs.size))
    else:
        state._check(state._L.gpf_initialize_proposal(state._h, _pd(obs), obs.size, _proposal_id(proposal)))
    return state


def choiceproduct(*choices):
    """src/utils.jl:57-98: the strata as a list of choice maps {address: value}: `choiceproduct(("moving", [False, True]))`.
    A dict {address: values} or several (address, values) tuples give the Cartesian product."""
    import itertools
    if len(choices) == 1 and isinstance(choices[0], dict):
        choices = tuple(choices[0].items())
    return [dict(c) for c in itertools.product(*[[(addr, v) for v in vals] for addr, vals in choices])]


def _layout_id(layout) -> bool:
    if layout not in ("contiguous", "interleaved"):
        raise ValueError("layout must be 'contiguous' or 'interleaved'")
    return layout == "interleaved"


def _strata_values(model, strata, phase: str = "update") -> np.ndarray:
    """strata: an iterable of choice maps over the model's ONE discrete latent address (or of plain values); a model may
    stratify a different address at its first step (`phase` = "initialize") than later ("update")"""
    addr = model.info.get("strata_address")
    if isinstance(addr, dict):
        addr = addr[phase]
    if addr is None:
        raise ErrorException(f"model {model.name} has no discrete latent to stratify over")
    vals = []
    for st in strata:
        if isinstance(st, dict):
            if set(st.keys()) != {addr}:
                raise ErrorException(f"device strata constrain the address {addr!r} only, got {sorted(st.keys())}")
            st = st[addr]
        vals.append(float(st))
    if not 1 <= len(vals) <= 8:
        raise ErrorException("1..8 strata supported")
    return np.ascontiguousarray(vals, np.float64)


def pf_update(state: DeviceParticleFilterState, new_args: tuple, argdiffs: tuple, observations,
              proposal=None, proposal_args: tuple = (), *, layout: str = "interleaved"):
    """src/update.jl:12-25 (default proposal), :79-96 (custom proposal: log weight = model_score_diff -
    fwd_proposal_score, src/translate.jl:86-105) and :193-210 (stratified: the 5th argument is the strata).
    Returns `state`, like the reference (update.jl:24)."""
    obs = _obs_vector(observations)
    if proposal is None:
        # (an ESS-triggered loop has this call on its critical path -- the GPU idles between the ESS read and this launch: the address
        #  as an integer instead of a ctypes pointer object, 0.8 us instead of 2.3)
        st = state._L.gpf_update(state._h, obs.ctypes.data, obs.size)
        if st != _lib.OK:
            state._check(st)
    elif isinstance(proposal, _NativeKernel):
        state._check(state._L.gpf_update_proposal(state._h, _pd(obs), obs.size, _proposal_id(proposal)))
    elif isinstance(proposal, (list, tuple)) or hasattr(proposal, "__iter__"):
        strata = _strata_values(state.model, proposal)
        state._check(state._L.gpf_update_strata(state._h, _pd(obs), obs.size, _pd(strata), strata.size, int(_layout_id(layout))))
    else:
        _proposal_id(proposal)
    return state


def pf_step_ess(state: DeviceParticleFilterState, new_args: tuple, argdiffs: tuple, observations, *, ess_threshold: float = 0.5,
                method: str = "multinomial", rejuvenate=None, n_iters: int = 1, check="warn", sort_particles: bool = True) -> bool:
    """One iteration of the reference's README loop (README.md:66-77) in ONE call (gpf.h gpf_step_ess):

        if effective_sample_size(state) < ess_threshold * n_particles
            pf_resample!(state, method; check, sort_particles)
            pf_rejuvenate!(state, kern, (), n_iters; method = rejuvenate)      # rejuvenate: None | "move" | "reweight"
        end
        pf_update!(state, new_args, argdiffs, observations)

    The results are those of the separate calls, bit for bit; the steps that do not resample do not wait for the host's ESS decision
    (the propagate is enqueued speculatively behind the reduction, which leaves its verdict on the device).  Returns whether it resampled."""
    if method not in RESAMPLE_METHODS:
        raise ErrorException(f"Resampling method {method} not recognized.")
    if rejuvenate is not None and rejuvenate not in REJUVENATE_METHODS:
        raise ErrorException(f"Method {rejuvenate} not recognized.")
    if check not in (True, False, "warn"):
        raise ValueError("check must be True, 'warn' or False")
    check_id = 2 if check is True else (1 if check == "warn" else 0)
    obs = _obs_vector(observations)
    res, inv = C.c_int32(0), C.c_int32(0)
    st = state._L.gpf_step_ess(state._h, obs.ctypes.data, obs.size, float(ess_threshold), RESAMPLE_METHODS[method], int(sort_particles), check_id,
                               -1 if rejuvenate is None else REJUVENATE_METHODS[rejuvenate], int(n_iters), C.byref(res),
                               C.byref(inv) if check_id != 0 else None, None)
    if st != _lib.OK:
        raise ErrorException(state._L.gpf_last_error(state._h).decode())
    if check == "warn" and inv.value:
        warnings.warn("Invalid weights (all -Inf or zero): resampled with uniform weights.")   # utils.jl:120-135
    return bool(res.value)


def _resample(state, method_id: int, priority_fn, check, sort_particles: bool):
    if check not in (True, False, "warn"):
        raise ValueError("check must be True, 'warn' or False")
    check_id = 2 if check is True else (1 if check == "warn" else 0)
    inv = C.c_int32(0)
    inv_ptr = C.byref(inv) if check_id != 0 else None          # check=false: fully asynchronous
    err_handle = state._h
    if (priority_fn is None and isinstance(state, DeviceParticleFilterSubState) and state.start == 0 and state.index is None
            and state.n_particles == state.source.n_particles and os.environ.get("GPF_VIEW_RESAMPLE") != "eager"):
        # pf_resample!(state[1:end], ...): the library resamples the whole filter with the sub-state semantics itself
        # (gpf_resample_local: same result, no eager gather, no copies through the view handle)
        err_handle = state.source._h
        st = state._L.gpf_resample_local(err_handle, method_id, int(sort_particles), check_id, inv_ptr)
    elif priority_fn is None or isinstance(priority_fn, Tempering):
        alpha = float("nan") if priority_fn is None else priority_fn.alpha
        st = state._L.gpf_resample(state._h, method_id, alpha, int(sort_particles), check_id, inv_ptr)
    else:
        lw = state.log_weights
        try:
            lp = np.ascontiguousarray(priority_fn(lw), np.float64)
            if lp.shape != lw.shape:
                raise TypeError
        except TypeError:
            lp = np.array([priority_fn(float(w)) for w in lw], np.float64)
        st = state._L.gpf_resample_with_priorities(state._h, method_id, _pd(lp), int(sort_particles), check_id, inv_ptr)
    if st != _lib.OK:
        raise ErrorException(state._L.gpf_last_error(err_handle).decode())     # error("Invalid weights."), ...
    if check == "warn" and inv.value:
        warnings.warn("Invalid weights (all -Inf or zero): resampled with uniform weights.")   # utils.jl:120-135
    return state


def pf_multinomial_resample(state, *, priority_fn=None, check="warn"):
    """src/resample.jl:48-65"""
    return _resample(state, 0, priority_fn, check, True)


def pf_residual_resample(state, *, priority_fn=None, check="warn"):
    """src/resample.jl:85-120"""
    return _resample(state, 1, priority_fn, check, True)


def pf_stratified_resample(state, *, priority_fn=None, check="warn", sort_particles: bool = True):
    """src/resample.jl:143-175"""
    return _resample(state, 2, priority_fn, check, sort_particles)


def pf_multinomial_sorted_resample(state, *, priority_fn=None, check="warn"):
    """OPT-IN extension, not a reference method: pf_multinomial_resample! (src/resample.jl:48-65) with the N uniforms drawn already sorted
    (uniform spacings in exact integers): offspring counts ~ Multinomial(N, w) as for "multinomial", `state.parents`
    non-decreasing instead of an i.i.d. sequence (src/resample.jl:59) -- the ancestor search is a streaming merge, the row gather reads
    ascending rows."""
    return _resample(state, RESAMPLE_METHODS["multinomial_sorted"], priority_fn, check, True)


def pf_resample(state, method: str = "multinomial", **kwargs):
    """src/resample.jl:19-30 (+ the opt-in "multinomial_sorted")"""
    if method == "multinomial_sorted":
        return pf_multinomial_sorted_resample(state, **kwargs)
    if method == "multinomial":
        return pf_multinomial_resample(state, **kwargs)
    if method == "residual":
        return pf_residual_resample(state, **kwargs)
    if method == "stratified":
        return pf_stratified_resample(state, **kwargs)
    raise ErrorException(f"Resampling method {method} not recognized.")


def pf_resample_blocks(state, block_size: int, method: str = "multinomial", *, priority_fn=None, ess_frac=None, sort_particles: bool = True, check="warn",
                       conditional: bool = False, reference=None, observations=None):
    """Many small filters in one state: the batched form of

        for b in blocks:                                   # consecutive blocks of block_size particles
            if ess_frac is None or get_ess(state[b]) < ess_frac * len(b):
                pf_resample(state[b], method, sort_particles=..., check=...)

    (sub-states: src/view.jl:16-48, src/resample.jl:185-187,205-218; the README loop README.md:60-79 per block) in ONE kernel
    launch (gpf.h gpf_resample_blocks): one workgroup per block, everything out of LDS, the ESS test on the device.  Every block's
    result is bit-identical to the loop above run through views.  Returns the number of blocks that resampled.

    conditional=True: the conditional multinomial step of conditional SMC (Andrieu, Doucet & Holenstein 2010; gpf.h
    gpf_resample_blocks_conditional): in every block that resamples, slot 0 -- the retained particle -- keeps itself (parent 0), the other slots
    draw exactly as in the plain call.  Multinomial only, no priority_fn, blocks of at most 2048 particles.

    conditional=True, reference=ref_t, observations=obs_t: particle Gibbs with ancestor sampling (Lindsten, Jordan & Schoen 2014; gpf.h
    gpf_resample_blocks_ancestor): slot 0 draws its ancestor with probability proportional to w_i f(ref_t | x_i) instead of keeping itself.
    ref_t (n_blocks, dim) and obs_t (n_blocks, n_obs) are the arguments of the pf_update_blocks(..., reference=ref_t) that follows: the step
    being entered.  Everything else is the conditional call."""
    if reference is not None and not conditional:
        raise ValueError("reference= selects ancestor sampling, a form of the conditional step: pass conditional=True")
    if reference is not None and observations is None:
        raise ValueError("reference= needs observations=: the data vector of the step being entered, as the update that follows takes it")
    if observations is not None and reference is None:
        raise ValueError("observations= is read by ancestor sampling only: pass reference= as well")
    if method not in RESAMPLE_METHODS:
        raise ErrorException(f"Resampling method {method} not recognized.")
    if conditional and method != "multinomial":
        raise ValueError(f"conditional=True is multinomial only: forcing one slot is not a valid conditional scheme for {method} resampling")
    if conditional and priority_fn is not None:
        raise ValueError("conditional=True takes no priority_fn")
    if check not in (True, False, "warn"):
        raise ValueError("check must be True, 'warn' or False")
    if isinstance(state, DeviceParticleFilterSubState):
        raise ErrorException("pf_resample_blocks works on the whole filter")
    if priority_fn is not None and not isinstance(priority_fn, Tempering):
        raise ErrorException("block-wise resampling takes priority_fn = None or Tempering(alpha) (w -> alpha w)")
    check_id = 2 if check is True else (1 if check == "warn" else 0)
    inv, cnt = C.c_int32(0), C.c_int64(0)
    if reference is not None:
        obs = _block_obs(state, observations, block_size)
        ref = _block_reference(state, reference, obs.shape[0])
        st = state._L.gpf_resample_blocks_ancestor(state._h, RESAMPLE_METHODS[method], int(block_size), float("nan") if ess_frac is None else float(ess_frac),
                                                   check_id, _pd(obs), obs.shape[1], _pd(ref), ref.shape[1], C.byref(inv), C.byref(cnt))
        if st not in (_lib.OK, _lib.ERR_INVALID_WEIGHTS):        # (a refused call: the state, its epoch and the mask of the last call are untouched)
            raise ErrorException(state._L.gpf_last_error(state._h).decode())
    elif conditional:
        st = state._L.gpf_resample_blocks_conditional(state._h, RESAMPLE_METHODS[method], int(block_size),
                                                      float("nan") if ess_frac is None else float(ess_frac), check_id, C.byref(inv), C.byref(cnt))
        if st != _lib.OK:                                        # (a refused call: the state, its epoch and the mask of the last call are untouched)
            raise ErrorException(state._L.gpf_last_error(state._h).decode())
    else:
        st = state._L.gpf_resample_blocks(state._h, RESAMPLE_METHODS[method], int(block_size),
                                          float("nan") if priority_fn is None else float(priority_fn.alpha), int(sort_particles),
                                          float("nan") if ess_frac is None else float(ess_frac), check_id, C.byref(inv), C.byref(cnt))
    state._n_blocks_last = (state.n_particles + int(block_size) - 1) // int(block_size) if int(block_size) > 0 else 0
    if st != _lib.OK:
        raise ErrorException(state._L.gpf_last_error(state._h).decode())
    if check == "warn" and inv.value:
        warnings.warn("Invalid weights (all -Inf or zero) in some block: resampled with uniform weights.")
    return int(cnt.value)


def _block_obs(state, observations, block_size: int) -> np.ndarray:
    nb = (state.n_particles + int(block_size) - 1) // int(block_size)
    obs = np.ascontiguousarray(observations, np.float64)
    if obs.ndim == 1:
        obs = obs.reshape(nb, -1)
    if obs.ndim != 2 or obs.shape[0] != nb:
        raise ErrorException(f"one observation vector per block expected: {nb} rows, got an array of shape {obs.shape}")
    return obs


def _block_reference(state, reference, n_blocks: int) -> np.ndarray:
    """the reference rows of a pinned step as a contiguous (n_blocks, k) array; k is checked against the model by the library"""
    ref = np.ascontiguousarray(reference, np.float64)
    if ref.ndim != 2 or ref.shape[0] != n_blocks:
        raise ErrorException(f"one reference row per block expected: shape ({n_blocks}, {state.model.dim}), got an array of shape {ref.shape}")
    return ref


def block_params_rows(model: NativeModel, params, n_particles: int, block_size: int) -> np.ndarray:
    """the [n_blocks][n_params] rows gpf_set_block_params takes, checked on the host: `params` is an array with one parameter vector per block
    (the layout of csrc/gpf_models.hpp, derived constants included) or a list of NativeModel descriptors of `model`'s kind, whose `params` --
    built by the model constructors, derived constants and all -- become the rows"""
    if int(block_size) < 1:
        raise ErrorException("block_size < 1")
    bs = min(int(block_size), max(int(n_particles), 1))                 # (clamped to the particle count, as in the C ABI)
    nb = (int(n_particles) + bs - 1) // bs
    if isinstance(params, (list, tuple)) and any(isinstance(m, NativeModel) for m in params):
        if not all(isinstance(m, NativeModel) for m in params):
            raise ErrorException("per-block parameters: a list of NativeModel descriptors or an array, not a mixture")
        bad = [m.name for m in params if m.model_id != model.model_id]
        if bad:
            raise ErrorException(f"per-block parameters: the state's model is {model.name}, got descriptors of {sorted(set(bad))}")
        vecs = [np.asarray(m.params, np.float64).ravel() for m in params]
        if any(v.size != vecs[0].size for v in vecs):
            raise ErrorException("per-block parameters: the descriptors' parameter vectors differ in length")
        rows = np.stack(vecs) if vecs else np.zeros((0, 0))
    else:
        rows = np.asarray(params, np.float64)
    if rows.ndim != 2 or rows.shape[0] != nb:
        raise ErrorException(f"one parameter vector per block expected: {nb} rows, got an array of shape {rows.shape}")
    if rows.shape[1] != np.asarray(model.params).size:
        raise ErrorException(f"{model.name} takes {np.asarray(model.params).size} parameters per block, got {rows.shape[1]}")
    return np.ascontiguousarray(rows, np.float64)


def set_block_params(state, params, block_size: int | None = None):
    """for b in blocks: the model arguments of state[b] -- pf_update!(state[b], new_args_b, argdiffs, observations[b]) with a parameter vector PER
    BLOCK (gpf.h gpf_set_block_params).  params: (n_blocks, n_params) array or a list of NativeModel descriptors of the state's model (see
    block_params_rows); None clears them.  While they are set, the block-wise calls use row b for block b, with this block_size only, and every
    call that would use the state's one parameter vector (pf_update, pf_initialize, the resize family, ...) raises.  Uploaded once."""
    if params is None:
        state._check(state._L.gpf_set_block_params(state._h, None, 0, 0))
        state._n_param_blocks = 0
        return state
    if block_size is None:
        raise ErrorException("set_block_params needs the block_size of the block-wise calls")
    rows = block_params_rows(state.model, params, state.n_particles, block_size)
    state._check(state._L.gpf_set_block_params(state._h, _pd(rows), rows.shape[1], int(block_size)))
    state._n_param_blocks = rows.shape[0]
    return state


def get_block_params(state) -> np.ndarray:
    """the per-block parameter rows as they stand, (n_blocks, n_params) (gpf.h gpf_get_block_params): after pf_resample_across_blocks the rows
    set_block_params uploaded, permuted by its block ancestors.  A checkpoint does not hold them: `set_block_params(state, get_block_params(state),
    block_size)` after `restore` continues bit for bit.  Raises when none are set."""
    nb = getattr(state, "_n_param_blocks", 0)
    if nb < 1:
        raise ErrorException("get_block_params: no per-block parameters are set (set_block_params)")
    out = np.empty((nb, int(np.asarray(state.model.params).size)))
    state._check(state._L.gpf_get_block_params(state._h, _pd(out), out.shape[1], nb))
    return out


def pf_resample_across_blocks(state, block_size: int, method: str = "multinomial", *, ess_frac=None, sort_particles: bool = True, check="warn"):
    """Resampling ACROSS blocks -- the outer level of SMC^2 / a nested or island filter (gpf.h gpf_resample_across_blocks): every block of
    block_size particles is one super-particle with the log-weight log_ml_estimate(state[b]) (`block_stats`); the blocks are resampled by the
    reference's resampler (src/resample.jl:19-175) on those B = n / block_size weights -- the ancestors of a filter of B particles with this state's
    seed at this state's RNG epoch -- and whole filters are copied: rows, parents, per-block parameters and observations, and the log-weights plus
    M - L[a], so that every block then carries the average mass M and the weights inside a block are kept.  ess_frac: resample only if the ESS of
    the block weights is below ess_frac * B.  Returns the 1-based block ancestors (int64, theta = theta[A - 1]), or None when the gate did not fire."""
    if method not in ("multinomial", "residual", "stratified"):
        raise ErrorException(f"Resampling method {method} not recognized.")
    if check not in (True, False, "warn"):
        raise ValueError("check must be True, 'warn' or False")
    if isinstance(state, DeviceParticleFilterSubState):
        raise ErrorException("pf_resample_across_blocks works on the whole filter")
    check_id = 2 if check is True else (1 if check == "warn" else 0)
    inv, res, ess = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    st = state._L.gpf_resample_across_blocks(state._h, RESAMPLE_METHODS[method], int(block_size), int(sort_particles),
                                             float("nan") if ess_frac is None else float(ess_frac), check_id, C.byref(inv), C.byref(res), C.byref(ess))
    if st != _lib.OK:
        raise ErrorException(state._L.gpf_last_error(state._h).decode())
    state._across_ess = ess.value
    if check == "warn" and inv.value:
        warnings.warn("Invalid block weights (all -Inf): blocks resampled with uniform weights.")
    if not res.value:
        return None
    state._n_blocks_last = 0                                     # (the mask of pf_resample_blocks no longer describes the blocks)
    state._n_across_blocks = state.n_particles // int(block_size)
    return block_ancestors(state)


def block_ancestors(state) -> np.ndarray:
    """the 1-based block ancestors of the last pf_resample_across_blocks that fired (gpf.h gpf_block_ancestors)"""
    out = np.zeros(max(getattr(state, "_n_across_blocks", 0), 1), np.int64)
    state._check(state._L.gpf_block_ancestors(state._h, out.ctypes.data_as(C.POINTER(C.c_int64))))
    return out[:getattr(state, "_n_across_blocks", 0)]


def pf_initialize_blocks(model: NativeModel, model_args: tuple, observations, n_particles: int, block_size: int, *, seed: int = 1,
                         keep_prev: bool = False, device: int = 0, strata=None, layout: str = "contiguous", params=None, history: int = 0,
                         reference=None, history_weights: bool = False, forward: bool = False):
    """many small filters in one state, each with its own data: block b (block_size consecutive particles) is initialised with
    observations[b] -- the batched form of per-view initialisation (gpf.h gpf_initialize_blocks).  strata: every block is initialised
    stratified by itself (src/initialize.jl:92-109 per sub-state, gpf.h gpf_initialize_blocks_strata), the same strata for all blocks.
    params: per-block model parameters (set_block_params) in force from this call on; `model` gives the model kind and the rows' length.
    history = T: the block-wise trajectory store for T time steps (gpf.h gpf_history_enable_blocks) -- past-step addresses (t, column) in
    block_mean / block_var / block_proportionmap, block_moments(..., step=t), and everything the whole-filter store answers.
    reference: conditional SMC (gpf.h gpf_initialize_blocks_ref) -- an (n_blocks, dim) array; slot 0 of block b (particle b * block_size) is
    pinned to reference[b] and weighted by log p(y_b | reference[b]); every other particle is what the call without a reference gives.  A
    per-call input (nothing is kept), default proposal only, all values finite; the values of discrete latents are the caller's business.
    history_weights: the store also records every step's log-weights and per-block observations (gpf.h gpf_history_enable_blocks_weights: 8 bytes more
    per particle and step), which block_backward_trajectories needs; raises without history=T.
    forward: forward-only smoothing per block (gpf.h gpf_forward_enable_blocks) -- every later block-wise step keeps the additive smoothing statistics
    that block_forward_moments returns, with a store or without one."""
    if reference is not None and strata is not None:
        raise ValueError("a reference is offered with the default proposal only, not with strata")
    if history_weights and not history:
        raise ValueError("history_weights=True needs the block-wise trajectory store: pass history=T as well")
    state = DeviceParticleFilterState(model, n_particles, seed=seed, keep_prev=keep_prev, device=device, history=history, history_blocks=bool(history),
                                      history_weights=bool(history_weights))
    if forward:
        state._check(state._L.gpf_forward_enable_blocks(state._h))
    obs = _block_obs(state, observations, block_size)
    if params is not None:
        set_block_params(state, params, block_size)
    if strata is not None:
        v = _strata_values(model, strata, "initialize")
        state._check(state._L.gpf_initialize_blocks_strata(state._h, _pd(obs), obs.shape[1], int(block_size), _pd(v), v.size, int(_layout_id(layout))))
        return state
    if reference is not None:
        ref = _block_reference(state, reference, obs.shape[0])
        state._check(state._L.gpf_initialize_blocks_ref(state._h, _pd(obs), obs.shape[1], int(block_size), _pd(ref), ref.shape[1]))
        return state
    state._check(state._L.gpf_initialize_blocks(state._h, _pd(obs), obs.shape[1], int(block_size)))
    return state


def pf_update_blocks(state, new_args: tuple, argdiffs: tuple, observations, block_size: int, proposals=None, *, strata=None, layout: str = "interleaved",
                     reference=None):
    """for b in blocks: pf_update!(state[b], new_args, argdiffs, observations[b]) (per-view updates, test/update.jl:179-189) in one launch.
    proposals: one entry per block, None (default proposal, update.jl:12-25) or the model's native proposal (update.jl:79-96) -- "Update with
    different proposals per view" in one launch (gpf.h gpf_update_blocks_proposal).
    reference: conditional SMC (gpf.h gpf_update_blocks_ref) -- an (n_blocks, dim) array; slot 0 of block b is pinned to reference[b], its
    log-weight becomes lw + log p(y_b | reference[b]), its x_{t-1} columns (keep_prev) are its incoming latent; every other particle is what the
    call without a reference gives.  A per-call input, default proposal only (ValueError with proposals= or strata=), all values finite.  A
    rejuvenation move on slot 0 changes the retained value at the current step."""
    if reference is not None and (proposals is not None or strata is not None):
        raise ValueError("a reference is offered with the default proposal only, not with proposals= or strata=")
    obs = _block_obs(state, observations, block_size)
    if reference is not None:
        ref = _block_reference(state, reference, obs.shape[0])
        state._check(state._L.gpf_update_blocks_ref(state._h, _pd(obs), obs.shape[1], int(block_size), _pd(ref), ref.shape[1]))
        return state
    if strata is not None:                                       # every block stratified by itself (src/update.jl:193-210 per sub-state)
        if proposals is not None:
            raise ErrorException("block-wise updates take strata or per-block proposals, not both")
        v = _strata_values(state.model, strata)
        state._check(state._L.gpf_update_blocks_strata(state._h, _pd(obs), obs.shape[1], int(block_size), _pd(v), v.size, int(_layout_id(layout))))
        return state
    if proposals is None:
        state._check(state._L.gpf_update_blocks(state._h, _pd(obs), obs.shape[1], int(block_size)))
        return state
    if len(proposals) != obs.shape[0]:
        raise ErrorException(f"one proposal (or None) per block expected: {obs.shape[0]}, got {len(proposals)}")
    native = [q for q in proposals if q is not None]
    pid = _proposal_id(native[0]) if native else 1
    if any(_proposal_id(q) != pid for q in native):
        raise ErrorException("the blocks' native proposals must be the same one")
    flags = np.ascontiguousarray([0 if q is None else 1 for q in proposals], np.int32)
    state._check(state._L.gpf_update_blocks_proposal(state._h, _pd(obs), obs.shape[1], int(block_size), flags.ctypes.data_as(C.POINTER(C.c_int32)), pid))
    return state


BlockRun = namedtuple("BlockRun", ["lml", "ess", "resampled"])


def pf_run_blocks(state, observations, block_size: int, method: str = "multinomial", *, ess_frac=0.5, sort_particles: bool = True) -> BlockRun:
    """A whole series per block in ONE launch (gpf.h gpf_run_blocks) -- bit for bit the loop

        for t in range(T):
            pf_resample_blocks(state, block_size, method, ess_frac=ess_frac, sort_particles=sort_particles, check=False)
            pf_update_blocks(state, (t,), (None,), observations[:, t], block_size)

    on an initialised state: rows, log-weights, parents, the RNG epoch (+ 2 T) and the per-block observations are what the loop leaves, so
    every later call continues identically and runs of T1 and T2 steps compose to one of T1 + T2.  observations: (n_blocks, T, n_obs), or
    (T, n_obs) -- one series shared by all blocks, the SMC^2 / particle-marginal MH case (the blocks differ by set_block_params).
    ess_frac=None: every block resamples at every step.  Default proposals only; no rejuvenation, store or reference path inside the run.
    Returns BlockRun(lml, ess, resampled), each (n_blocks, T): log_ml_estimate(state[b]) and effective_sample_size(state[b]) after step t's
    update (block_stats) and whether block b resampled at step t (block_resampled).  Blocks with NaN / +Inf weights are left alone by the
    resample and propagated anyway; the call then raises "Invalid weights (NaN)." after the whole run."""
    if method not in ("multinomial", "residual", "stratified"):
        raise ErrorException(f"Resampling method {method} not recognized.")
    if isinstance(state, DeviceParticleFilterSubState):
        raise ErrorException("pf_run_blocks works on the whole filter")
    if int(block_size) < 1:
        raise ErrorException("block_size < 1")
    nb = (state.n_particles + min(int(block_size), max(state.n_particles, 1)) - 1) // min(int(block_size), max(state.n_particles, 1))
    obs = np.ascontiguousarray(observations, np.float64)
    if obs.ndim == 3 and obs.shape[0] == nb and obs.shape[1] >= 1:
        shared = False
    elif obs.ndim == 2 and obs.shape[0] >= 1:
        shared = True
    else:
        raise ErrorException(f"observations of shape ({nb}, T, n_obs), or (T, n_obs) for one series shared by all blocks, expected: got {obs.shape}")
    T = obs.shape[0] if shared else obs.shape[1]
    ess, lml, res = np.empty((T, nb)), np.empty((T, nb)), np.zeros((T, nb), np.int32)
    inv = C.c_int32(0)
    st = state._L.gpf_run_blocks(state._h, _pd(obs), obs.shape[-1], T, int(shared), int(block_size), RESAMPLE_METHODS[method], int(sort_particles),
                                 float("nan") if ess_frac is None else float(ess_frac), _pd(ess), _pd(lml),
                                 res.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(inv))
    if st != _lib.OK:
        raise ErrorException(state._L.gpf_last_error(state._h).decode())
    state._n_blocks_last = 0                                     # (no pf_resample_blocks for block_resampled to refer to, as after the loop's last update)
    return BlockRun(lml.T, ess.T, (res & 1).astype(bool).T)      # (views of the library's [T][n_blocks] arrays: no transposed copies)


def pf_rejuvenate_blocks(state, kern=None, kern_args: tuple = (), n_iters: int = 1, *, method: str = "move", only_resampled: bool = False,
                         count: bool = False):
    """for b in blocks: pf_rejuvenate!(state[b], ...) with the block's own latest observation; only_resampled: only the blocks the last
    pf_resample_blocks resampled (the README loop rejuvenates inside its `if`)"""
    if method not in REJUVENATE_METHODS:
        raise ErrorException(f"Method {method} not recognized.")
    acc = C.c_uint64(0)
    state._check(state._L.gpf_rejuvenate_blocks(state._h, REJUVENATE_METHODS[method], int(n_iters), int(only_resampled), C.byref(acc) if count else None))
    return int(acc.value) if count else state


def block_resampled(state) -> np.ndarray:
    """which blocks the last pf_resample_blocks resampled (bool per block)"""
    out = np.zeros(getattr(state, "_n_blocks_last", 0), np.int32)
    state._check(state._L.gpf_block_resampled(state._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out.astype(bool)


def block_stats(state, block_size: int):
    """(effective_sample_size(state[b]), log_ml_estimate(state[b])) of every block, src/utils.jl:163-178, in one launch"""
    nb = (state.n_particles + int(block_size) - 1) // int(block_size)
    ess, lml = np.empty(nb), np.empty(nb)
    state._check(state._L.gpf_block_stats(state._h, int(block_size), _pd(ess), _pd(lml)))
    return ess, lml


def block_ancestor_log_weights(state, block_size: int, observations, reference):
    """lwa_i = lw_i + log f(reference[b] | x_i) up to terms that do not depend on x_i, b = i // block_size: the weights the ancestor of slot 0 is
    drawn from in pf_resample_blocks(..., conditional=True, reference=...), and what a backward simulation needs (gpf.h
    gpf_block_ancestor_log_weights).  One launch, any block size; the state is not changed."""
    if isinstance(state, DeviceParticleFilterSubState):
        raise ErrorException("block_ancestor_log_weights works on the whole filter")
    obs = _block_obs(state, observations, block_size)
    ref = _block_reference(state, reference, obs.shape[0])
    out = np.empty(state.n_particles)
    state._check(state._L.gpf_block_ancestor_log_weights(state._h, int(block_size), _pd(obs), obs.shape[1], _pd(ref), ref.shape[1], _pd(out)))
    return out


def _block_column(state, addr, who: str):
    """addr -> (step, column): step 0 = the current step; (t, column) = the past choice t => column, which needs the block-wise trajectory store"""
    if isinstance(addr, tuple):
        if not getattr(state, "history_blocks", False):
            raise ErrorException(f"{who}: a past-step address (t, column) needs a block-wise trajectory store (pf_initialize_blocks(..., history=T)), "
                                 "which this state does not have")
        if int(addr[0]) < 1:
            raise ErrorException(f"{who}: the step of a past-step address is 1-based (step 1 = the initialisation); use a plain column for the current step")
        return int(addr[0]), int(addr[1])
    return 0, (None if addr is None else int(addr))


def _block_moments(state, block_size: int, want_mean: bool, want_var: bool, step: int = 0):
    nb = (state.n_particles + int(block_size) - 1) // int(block_size)
    width = state.dim if step else state.row_width                 # (the store keeps the latent columns, not the row width)
    mu = np.empty((nb, width)) if want_mean else None
    s2 = np.empty((nb, width)) if want_var else None
    if step:
        state._check(state._L.gpf_block_history_moments(state._h, int(step), int(block_size), _pd(mu) if want_mean else None, _pd(s2) if want_var else None))
    else:
        state._check(state._L.gpf_block_moments(state._h, int(block_size), _pd(mu) if want_mean else None, _pd(s2) if want_var else None))
    return mu, s2


def _block_pick(state, a: np.ndarray, col):
    if col is None:
        return a
    if not 0 <= col < a.shape[1]:
        raise ErrorException("bad column")
    return np.ascontiguousarray(a[:, col])


def block_moments(state, block_size: int, step: int | None = None):
    """([mean(state[b], c) for c in columns], [var(state[b], c) ...]) of every block, src/statistics.jl:13-14,48-50 on sub-states:
    two [n_blocks, row_width] arrays from one launch, bit-identical to the loop over views.  A block with NaN / +Inf weights is NaN.
    step=t (1-based, step 1 = the initialisation): the past choices t => c of the block-wise trajectory store instead (gpf.h
    gpf_block_history_moments): two [n_blocks, dim] arrays.  step=None is the current step; step < 1 raises."""
    if step is not None:
        _block_column(state, (step, 0), "block_moments")
        return _block_moments(state, block_size, True, True, int(step))
    return _block_moments(state, block_size, True, True)


def block_mean(state, block_size: int, addr=None) -> np.ndarray:
    """mean(state[b], addr) of every block in one launch: [n_blocks] for a column or a past-step address (t, column), [n_blocks, row_width]
    for addr=None"""
    step, col = _block_column(state, addr, "block_mean")
    return _block_pick(state, _block_moments(state, block_size, True, False, step)[0], col)


def block_var(state, block_size: int, addr=None) -> np.ndarray:
    """var(state[b], addr) (population form) of every block in one launch: [n_blocks] for a column or a past-step address (t, column),
    [n_blocks, row_width] for addr=None"""
    step, col = _block_column(state, addr, "block_var")
    return _block_pick(state, _block_moments(state, block_size, False, True, step)[1], col)


def block_proportionmap(state, block_size: int, addr, max_values: int = 256):
    """proportionmap(state[b], addr) of every block, src/statistics.jl:91-101 on sub-states: (values, proportions[n_blocks, n_values]).
    The distinct values are read from the column over all blocks (a value a block does not hold has proportion 0.0 there); each
    launch answers 16 values for all blocks.  addr = (t, column): the past choice t => column (block-wise trajectory store)."""
    step, col = _block_column(state, addr, "block_proportionmap")
    if col is None:
        raise ErrorException("block_proportionmap: give a column")
    nb = (state.n_particles + int(block_size) - 1) // int(block_size)
    if not 0 <= col < (state.dim if step else state.row_width):
        raise ErrorException("bad column")
    vals = np.unique(state.history_column(step, col) if step else state.column(col))
    if vals.size > max_values:
        raise ErrorException(f"proportionmap: {vals.size} distinct values; the column does not look discrete")
    out = np.empty((nb, vals.size))
    for k0 in range(0, vals.size, 16):
        chunk = np.ascontiguousarray(vals[k0:k0 + 16], np.float64)
        part = np.empty((nb, chunk.size))
        if step:
            state._check(state._L.gpf_block_history_proportion(state._h, step, int(block_size), col, _pd(chunk), int(chunk.size), _pd(part)))
        else:
            state._check(state._L.gpf_block_proportion(state._h, int(block_size), col, _pd(chunk), int(chunk.size), _pd(part)))
        out[:, k0:k0 + chunk.size] = part
    return vals, out


def _rejuvenate(state, method_id: int, n_iters: int, want_count: bool):
    acc = C.c_uint64(0)
    st = state._L.gpf_rejuvenate(state._h, method_id, int(n_iters), C.byref(acc) if want_count else None)
    state._check(st)
    state.n_accepted = acc.value if want_count else None
    return state


def pf_move_accept(state, kern=mh, kern_args: tuple = (), n_iters: int = 1, *, count: bool = False):
    """src/rejuvenate.jl:40-53 with the native mh kernel; kern_args = () -> Gen.mh(trace, selection) on the current step's latent,
    kern_args = (proposal[, proposal_args]) with a MoveProposal -> Gen.mh(trace, proposal, proposal_args): accept iff
    log(rand()) < weight - fwd_score + bwd_score"""
    if kern is not mh:
        raise ErrorException("device states support the native `mh` kernel only (arbitrary Julia/Python callables are out of scope)")
    if kern_args and isinstance(kern_args[0], MoveProposal):
        mp = kern_args[0]
        q = np.asarray(mp.params, np.float64)
        acc = C.c_uint64(0)
        st = state._L.gpf_rejuvenate_with_proposal(state._h, 0, mp.proposal_id, _pd(q) if q.size else None, int(q.size), int(n_iters),
                                                   C.byref(acc) if count else None)
        state._check(st)
        state.n_accepted = acc.value if count else None
        return state
    return _rejuvenate(state, 0, n_iters, count)


class MoveProposal:
    """a native proposal for move_reweight(trace, proposal, proposal_args) (src/rejuvenate.jl:134-148):
    `locally_optimal_move` (lgssm2: q = p(x_t | x_{t-1}, y_t)), `outlier_propose(q)` (line_model: the current step's outlier ~ bernoulli(q),
    the proposal of test/rejuvenate.jl:19-27)"""

    def __init__(self, name, proposal_id, params=()):
        self.name, self.proposal_id, self.params = name, proposal_id, tuple(float(p) for p in params)

    def __repr__(self):
        return f"<native move proposal {self.name}{self.params}>"


locally_optimal_move = MoveProposal("locally_optimal", 1)


def outlier_propose(q: float) -> MoveProposal:
    import math
    return MoveProposal("outlier_propose", 2, (q, math.log(q) if q > 0 else -math.inf, math.log1p(-q) if q < 1 else -math.inf))


def pf_move_reweight(state, kern=move_reweight, kern_args: tuple = (), n_iters: int = 1, *, count: bool = False):
    """src/rejuvenate.jl:74-90 with the native move_reweight kernel; kern_args = () -> the selection variant (rejuvenate.jl:125-132),
    kern_args = (proposal[, proposal_args]) with a MoveProposal -> the proposal variant (rejuvenate.jl:134-148)"""
    if kern is not move_reweight:
        raise ErrorException("device states support the native `move_reweight` kernel only")
    if kern_args and isinstance(kern_args[0], MoveProposal):
        mp = kern_args[0]
        q = np.asarray(mp.params, np.float64)
        st = state._L.gpf_rejuvenate_proposal(state._h, mp.proposal_id, _pd(q) if q.size else None, int(q.size), int(n_iters))
        state._check(st)
        state.n_accepted = state.n_particles * int(n_iters)
        return (state, state.n_accepted) if count else state
    return _rejuvenate(state, 1, n_iters, count)


def pf_rejuvenate(state, kern=None, kern_args: tuple = (), n_iters: int = 1, *, method: str = "move", **kwargs):
    """src/rejuvenate.jl:18-27"""
    if method == "move":
        return pf_move_accept(state, mh if kern is None else kern, kern_args, n_iters, **kwargs)
    if method == "reweight":
        return pf_move_reweight(state, move_reweight if kern is None else kern, kern_args, n_iters, **kwargs)
    raise ErrorException(f"Method {method} not recognized.")


# ----------------------------------------------------------------------------- resize family (src/resize.jl)
def _refresh_count(state):
    n = C.c_int64()
    state._check(state._L.gpf_n_particles(state._h, C.byref(n)))
    state.n_particles = n.value


def _resize(state, n_particles: int, method_id: int, priority_fn, check):
    if check not in (True, False, "warn"):
        raise ValueError("check must be True, 'warn' or False")
    if priority_fn is not None and not isinstance(priority_fn, Tempering):
        raise ErrorException("device resize supports priority_fn = nothing or Tempering(alpha)")
    check_id = 2 if check is True else (1 if check == "warn" else 0)
    inv = C.c_int32(0)
    alpha = float("nan") if priority_fn is None else priority_fn.alpha
    st = state._L.gpf_resize(state._h, int(n_particles), method_id, alpha, check_id, C.byref(inv) if check_id else None)
    if st == _lib.ERR_INVALID_WEIGHTS:
        raise ErrorException(state._L.gpf_last_error(state._h).decode())
    state._check(st)
    _refresh_count(state)
    if check == "warn" and inv.value:
        warnings.warn("Invalid weights (all -Inf or zero): resampled with uniform weights.")
    return state


def pf_multinomial_resize(state, n_particles: int, *, priority_fn=None, check="warn"):
    """src/resize.jl:46-68"""
    return _resize(state, n_particles, 0, priority_fn, check)


def pf_residual_resize(state, n_particles: int, *, priority_fn=None, check="warn"):
    """src/resize.jl:87-124"""
    return _resize(state, n_particles, 1, priority_fn, check)


def pf_optimal_resize(state, n_particles: int, *, check="warn"):
    """src/resize.jl:149-200 (Fearnhead & Clifford): n_particles must not exceed the current count"""
    return _resize(state, n_particles, 3, None, check)


def pf_resize(state, n_particles: int, method: str = "multinomial", **kwargs):
    """src/resize.jl:16-28"""
    if method == "multinomial":
        return pf_multinomial_resize(state, n_particles, **kwargs)
    if method == "residual":
        return pf_residual_resize(state, n_particles, **kwargs)
    if method == "optimal":
        return pf_optimal_resize(state, n_particles, **kwargs)
    raise ErrorException(f"Resampling method {method} not recognized.")


def pf_replicate(state, n_replicates: int, *, layout: str = "contiguous"):
    """src/resize.jl:236-244"""
    state._check(state._L.gpf_replicate(state._h, int(n_replicates), int(layout != "contiguous")))
    _refresh_count(state)
    return state


def pf_dereplicate(state, n_replicates: int, *, layout: str = "contiguous", method: str = "keepfirst"):
    """src/resize.jl:267-297"""
    if method not in ("keepfirst", "sample"):
        raise ErrorException(f"Method {method} not recognized.")
    state._check(state._L.gpf_dereplicate(state._h, int(n_replicates), int(layout != "contiguous"), int(method == "sample")))
    _refresh_count(state)
    return state


_COALESCE_ALL = (None, "get_choices", "identity")


def _coalesce_mask(state, by) -> int:
    """the key columns of pf_coalesce as gpf_coalesce's bit mask (0 = every state column)"""
    msg = ("native coalescing accepts by = None / 'get_choices' / 'identity' (every state column), a current-step column "
           "or a tuple of current-step columns")
    if isinstance(by, str) or by is None:
        if by not in _COALESCE_ALL:
            raise ErrorException(f"{msg}; got {by!r}")
        return 0
    if callable(by):
        raise ErrorException(f"{msg}; a Python callable has no native form")
    cols = by if isinstance(by, (tuple, list)) else (by,)
    mask = 0
    for c in cols:
        if isinstance(c, tuple):
            raise ErrorException(f"{msg}; the past-step address {c!r} is not")
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < state.dim:
            raise ErrorException(f"{msg}; got {c!r}")
        mask |= 1 << int(c)
    if mask == 0:
        raise ErrorException(f"{msg}; got an empty key")
    return mask


def pf_coalesce(state, by=None):
    """src/resize.jl:309-334 (gpf.h gpf_coalesce): particles whose key columns are bitwise equal become one particle -- the group's first
    member, weight logsumexp(group) + log(n_new / n_old).  Groups come out in ascending order of first occurrence (the reference: Dict
    order), so `state.parents` is strictly increasing.  by: None / 'get_choices' / 'identity' = every state column (with keep_prev the
    previous state too), a column, or a tuple of columns of the current step."""
    mask = _coalesce_mask(state, by)
    n = C.c_int64(0)
    st = state._L.gpf_coalesce(state._h, mask, C.byref(n))
    state._check(st)
    _refresh_count(state)
    return state


def pf_introduce(state, *args):
    """src/resize.jl:351-421 (gpf.h gpf_introduce): append n_particles trajectories generated over the whole observation history.
        pf_introduce(state, observations, n_particles)
        pf_introduce(state, model, model_args, observations, n_particles)
        pf_introduce(state, observations, proposal, proposal_args, n_particles)
        pf_introduce(state, model, model_args, observations, proposal, proposal_args, n_particles)
    observations: the per-step data vectors of steps 1..t (a (t, obs_dim) array; one vector = t = 1).  proposal: a native proposal
    (`locally_optimal`, `line_fixed`), applied at the last step.  model / model_args are accepted for signature parity; the model must
    be the state's own."""
    model = None
    if len(args) == 2:
        obs, proposal, n = args[0], None, args[1]
    elif len(args) == 4 and isinstance(args[0], NativeModel):
        model, obs, proposal, n = args[0], args[2], None, args[3]
    elif len(args) == 4:
        obs, proposal, n = args[0], args[1], args[3]
    elif len(args) == 6:
        model, obs, proposal, n = args[0], args[2], args[3], args[5]
    else:
        raise TypeError("pf_introduce(state, [model, model_args,] observations, [proposal, proposal_args,] n_particles)")
    if model is not None:
        mp = np.ascontiguousarray(model.params, np.float64)
        if model.model_id != state.model.model_id or mp.shape != state._params.shape or mp.tobytes() != state._params.tobytes():
            raise ErrorException("pf_introduce: a device filter introduces particles of its own model (same model id and parameters)")
    pid = 0 if proposal is None else _proposal_id(proposal)
    ob = np.asarray(obs, np.float64)
    if ob.ndim == 1:
        ob = ob[None, :]
    if ob.ndim != 2 or ob.shape[0] < 1:
        raise ErrorException("pf_introduce: observations must be the data vectors of steps 1..t, t >= 1")
    ob = np.ascontiguousarray(ob)
    state._check(state._L.gpf_introduce(state._h, _pd(ob), ob.shape[1], ob.shape[0], int(n), pid))
    _refresh_count(state)
    return state


# ----------------------------------------------------------------------------- summaries (src/utils.jl)
def effective_sample_size(state) -> float:
    out = C.c_double()
    state._check(state._L.gpf_effective_sample_size(state._h, C.byref(out)))
    return out.value


get_ess = effective_sample_size


def log_ml_estimate(state) -> float:
    out = C.c_double()
    state._check(state._L.gpf_log_ml_estimate(state._h, C.byref(out)))
    return out.value


get_lml_est = log_ml_estimate


def get_log_weights(state) -> np.ndarray:
    return state.log_weights


def get_log_norm_weights(state) -> np.ndarray:
    out = np.empty(state.n_particles)
    state._check(state._L.gpf_get_log_norm_weights(state._h, _pd(out), out.size))
    return out


def get_norm_weights(state) -> np.ndarray:
    out = np.empty(state.n_particles)
    state._check(state._L.gpf_get_norm_weights(state._h, _pd(out), out.size))
    return out


def get_traces(state) -> np.ndarray:
    return state.traces


def sample_unweighted_traces(state, n_samples: int, return_indices: bool = False):
    """Gen.sample_unweighted_traces(state, n_samples) (src/utils.jl:189-194 extends it to sub-states): n i.i.d. particles drawn
    with probability proportional to their weights; the filter itself is left untouched."""
    rows = np.empty((int(n_samples), state.row_width))
    idx = np.empty(int(n_samples), np.int64)
    state._check(state._L.gpf_sample_unweighted(state._h, int(n_samples), _pd(rows), idx.ctypes.data_as(C.POINTER(C.c_int64))))
    return (rows, idx) if return_indices else rows


def _store_steps(state, steps, who):
    """the steps a query of the block-wise store walks -> (lo, hi).  steps=None: all recorded steps; steps=t: that step; steps=(lo, hi): a range"""
    if steps is None:
        k = C.c_int32(0)
        state._check(state._L.gpf_history_steps(state._h, C.byref(k)))
        lo, hi = 1, int(k.value)
    elif isinstance(steps, (tuple, list)):
        lo, hi = int(steps[0]), int(steps[1])
    else:
        lo = hi = int(steps)
    if lo < 1 or hi < 1:
        raise ErrorException(who + ": steps are 1-based (step 1 = the initialisation)")
    return lo, hi


def _store_blocks(state, block_size, lo, hi, who, n_samples=None):
    """... -> (block size clamped to the particle count, number of blocks); n_samples: of a query that draws"""
    if n_samples is None:
        if hi < lo or int(block_size) < 1:
            raise ErrorException(who + ": need lo <= hi and block_size >= 1")
    elif hi < lo or int(n_samples) < 1 or int(block_size) < 1:
        raise ErrorException(who + ": need lo <= hi, n_samples >= 1 and block_size >= 1")
    bs = min(int(block_size), max(state.n_particles, 1))
    return bs, (state.n_particles + bs - 1) // bs


def _store_weights(state, who):
    """the queries that walk the store's weight records (a backward pass): refuse a state without them"""
    if not getattr(state, "history_weights", False):
        raise ErrorException(who + " needs the block-wise trajectory store with its weight records "
                             "(pf_initialize_blocks(..., history=T, history_weights=True)), which this state does not have")


def _pi64(a):
    """an optional int64 output: None (not asked for) stays None"""
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def block_sample_trajectories(state, block_size: int, n_samples: int = 1, steps=None, return_indices: bool = False):
    """for b in blocks; sample_unweighted_traces(state[b], n_samples); end (src/utils.jl:7,189-194 on sub-states, src/view.jl:35-48): the reference's
    traces are persistent, so every draw is a whole path of block b.  One launch for all blocks (gpf.h gpf_block_sample_trajectories); needs the
    block-wise trajectory store (pf_initialize_blocks(..., history=T)).  Returns [n_blocks, n_samples, n_steps, dim]: the latent columns of the drawn
    particle's ancestors, and with return_indices=True also the [n_blocks, n_samples] int64 indices (1-based, inside the block) of the drawn
    current particles.  steps=None: all recorded steps; steps=t: that step; steps=(lo, hi): a range, 1-based and inclusive (step 1 = the
    initialisation).  A block with NaN / +Inf weights gets index 0 and NaN paths.  Advances the RNG epoch once; the filter is left untouched."""
    if not getattr(state, "history_blocks", False):
        raise ErrorException("block_sample_trajectories needs a block-wise trajectory store (pf_initialize_blocks(..., history=T)), which this state does not have")
    lo, hi = _store_steps(state, steps, "block_sample_trajectories")
    _, nb = _store_blocks(state, block_size, lo, hi, "block_sample_trajectories", n_samples)
    traj = np.empty((nb, int(n_samples), hi - lo + 1, state.dim))
    idx = np.empty((nb, int(n_samples)), np.int64) if return_indices else None
    state._check(state._L.gpf_block_sample_trajectories(state._h, int(block_size), int(n_samples), lo, hi, _pd(traj), _pi64(idx)))
    return (traj, idx) if return_indices else traj


def block_backward_trajectories(state, block_size: int, n_samples: int = 1, steps=None, return_indices: bool = False):
    """backward simulation per block (FFBSi; gpf.h gpf_block_backward_sample): draw j of block b takes its step-T particle exactly as
    block_sample_trajectories does, then re-draws the particle of every earlier step s among the particles of the block its lineage occupied, from
    the step's recorded weights times the transition density towards the particle held at s + 1 -- smoothed paths that do not share the coalesced
    genealogy.  One launch for all blocks, draws and steps; needs pf_initialize_blocks(..., history=T, history_weights=True).  Returns
    [n_blocks, n_samples, n_steps, dim], and with return_indices=True also the [n_blocks, n_samples, n_steps] int64 indices (1-based, GLOBAL, in the
    final order of their step) of the held particles.  steps as in block_sample_trajectories; the walk always starts at the last step.  A block with
    NaN / +Inf weights gets indices 0 and NaN paths.  Under set_block_params every step uses the drawing block's CURRENT parameter row.  Advances the
    RNG epoch by T - lo + 1; the filter is left untouched."""
    _store_weights(state, "block_backward_trajectories")
    lo, hi = _store_steps(state, steps, "block_backward_trajectories")
    _, nb = _store_blocks(state, block_size, lo, hi, "block_backward_trajectories", n_samples)
    traj = np.empty((nb, int(n_samples), hi - lo + 1, state.dim))
    idx = np.empty((nb, int(n_samples), hi - lo + 1), np.int64) if return_indices else None
    state._check(state._L.gpf_block_backward_sample(state._h, int(block_size), int(n_samples), lo, hi, _pd(traj), _pi64(idx)))
    return (traj, idx) if return_indices else traj


def _block_smooth(state, block_size, steps, who, want_mean, want_var, want_weights, want_blocks):
    _store_weights(state, who)
    lo, hi = _store_steps(state, steps, who)
    bs, nb = _store_blocks(state, block_size, lo, hi, who)
    mu = np.empty((nb, hi - lo + 1, state.dim)) if want_mean else None
    s2 = np.empty((nb, hi - lo + 1, state.dim)) if want_var else None
    w = np.empty((nb, hi - lo + 1, bs)) if want_weights else None
    blocks = np.empty((nb, hi - lo + 1), np.int64) if want_blocks else None
    state._check(state._L.gpf_block_smooth(state._h, int(block_size), lo, hi, _pd(mu) if want_mean else None, _pd(s2) if want_var else None,
                                           _pd(w) if want_weights else None, _pi64(blocks)))
    return mu, s2, w, blocks


def block_smoothed_moments(state, block_size: int, steps=None, return_weights: bool = False, return_blocks: bool = False):
    """marginal smoothing per block (FFBSm; gpf.h gpf_block_smooth): the smoothed mean and variance of every latent column at every step of every block,
    under the deterministic smoothing weights W_s^i = sum_j W_{s+1}^j w_s^i f(x_{s+1}^j | x_s^i) / sum_l w_s^l f(x_{s+1}^j | x_s^l) -- what
    block_backward_trajectories estimates with draws, without their Monte-Carlo noise.  One launch for all blocks and steps, O(block_size^2) per block
    and step; needs pf_initialize_blocks(..., history=T, history_weights=True).  Returns (mean, var), each [n_blocks, n_steps, dim]; with
    return_weights=True also the weights [n_blocks, n_steps, block_size] (by position inside the lineage's block, 0 beyond a short block); with
    return_blocks=True also the [n_blocks, n_steps] int64 1-based block the lineage occupied at each step.  steps as in block_backward_trajectories; the
    walk always starts at the last step.  A block with NaN / +Inf weights, and the steps below a whole-filter resample, read NaN (blocks 0).  Under
    set_block_params every step uses the final block's CURRENT parameter row.  Nothing is drawn: the RNG epoch and the filter are left untouched."""
    mu, s2, w, blocks = _block_smooth(state, block_size, steps, "block_smoothed_moments", True, True, bool(return_weights), bool(return_blocks))
    return (mu, s2) + ((w,) if return_weights else ()) + ((blocks,) if return_blocks else ())


def block_smoothed_weights(state, block_size: int, steps=None):
    """the smoothing weights of block_smoothed_moments alone: [n_blocks, n_steps, block_size]"""
    return _block_smooth(state, block_size, steps, "block_smoothed_weights", False, False, True, False)[2]


BlockForwardMoments = namedtuple("BlockForwardMoments", "sum second cross first first2 last2 n_steps")


def block_forward_moments(state, block_size: int) -> BlockForwardMoments:
    """forward-only smoothing per block (gpf.h gpf_block_forward_moments; needs pf_initialize_blocks(..., forward=True)): after the current step t, per
    block, sum = sum_s E[x_s | y_1:t] (n_blocks, dim), second = sum_s E[x_s x_s' | y_1:t], cross = sum_s E[x_s x_{s+1}' | y_1:t] (row = the earlier
    step), first = E[x_1 | y_1:t], first2 = E[x_1 x_1' | y_1:t], last2 = E[x_t x_t' | y_1:t] (n_blocks, dim, dim each) and n_steps = t -- the sums over
    steps of block_smoothed_pair_moments without a store.  The M-step of a linear model reads second - last2 (steps < t), second - first2 (steps > 1)
    and cross.  Nothing is drawn and nothing changes; a block with NaN / +Inf weights reads NaN."""
    bs = max(min(int(block_size), state.n_particles), 1)                     # (the library clamps the size and refuses one below 1)
    nb = (state.n_particles + bs - 1) // bs
    d = state.dim
    vec = lambda: np.empty((nb, d))
    mat = lambda: np.empty((nb, d, d))
    out = (vec(), mat(), mat(), vec(), mat(), mat())
    t = C.c_int32()
    state._check(state._L.gpf_block_forward_moments(state._h, int(block_size), *[_pd(a) for a in out], C.byref(t)))
    return BlockForwardMoments(*out, int(t.value))


def block_smoothed_pair_moments(state, block_size: int, steps=None, return_blocks: bool = False):
    """pairwise smoothing per block (gpf.h gpf_block_smooth_pairs): the E-step of particle EM.  Beside block_smoothed_moments' mean, the second moments
    second[b, s] = sum_i W_s^i x_s^i x_s^i' and the lag-one cross moments cross[b, s][a, c] = sum_ij t_ij x_s^i[a] x_{s+1}^j[c] under the pairwise smoothing
    weights t_ij = W_{s+1}^j w_s^i f(x_{s+1}^j | x_s^i) / sum_l w_s^l f(x_{s+1}^j | x_s^l) -- the particle estimates of E[x_s x_s' | y_1:T] and
    E[x_s x_{s+1}' | y_1:T].  One launch for all blocks and steps, no block_size x block_size array anywhere; needs pf_initialize_blocks(..., history=T,
    history_weights=True).  Returns (mean [n_blocks, n_steps, dim], second [n_blocks, n_steps, dim, dim], cross [n_blocks, n_steps - 1, dim, dim]);
    entry o of cross is the pair of the steps lo + o and lo + o + 1, and a single step has an empty cross.  With return_blocks=True also
    block_smoothed_moments' blocks.  steps, NaN blocks, undefined lineages (NaN for every pair that touches an undefined step), per-block parameters and
    effects (none) as in block_smoothed_moments; mean is that call's, bit for bit."""
    who = "block_smoothed_pair_moments"
    _store_weights(state, who)
    lo, hi = _store_steps(state, steps, who)
    _, nb = _store_blocks(state, block_size, lo, hi, who)
    d = state.dim
    mu, second, cross = np.empty((nb, hi - lo + 1, d)), np.empty((nb, hi - lo + 1, d, d)), np.empty((nb, hi - lo, d, d))
    blocks = np.empty((nb, hi - lo + 1), np.int64) if return_blocks else None
    state._check(state._L.gpf_block_smooth_pairs(state._h, int(block_size), lo, hi, _pd(mu), _pd(second), _pd(cross) if hi > lo else None, _pi64(blocks)))
    return (mu, second, cross) + ((blocks,) if return_blocks else ())


def block_map_trajectories(state, block_size: int, steps=None, return_indices: bool = False, return_log_density: bool = False):
    """the most probable path per block (particle Viterbi; gpf.h gpf_block_map_path, Godsill, Doucet & West 2001): over the sequences that take one
    particle of the block's lineage at every recorded step, the maximiser of log mu(x_1) + sum_s log f(x_s | x_{s-1}) + sum_s log g(y_s | x_s), by
    max-plus dynamic programming -- what block_proportionmap's per-step modes do not give, because marginal modes need not form a likely path.  One launch
    for all blocks and steps, O(block_size^2) per block and step; needs pf_initialize_blocks(..., history=T, history_weights=True).  Returns the paths
    [n_blocks, n_steps, dim]; with return_indices=True also the [n_blocks, n_steps] int64 indices (1-based, GLOBAL, in the final order of their step) of
    the path's particles; with return_log_density=True also [n_blocks], the maximum -- comparable between paths of one block, not a normalised density
    (the constants of the transition and the initial law are omitted).  steps as in block_backward_trajectories; the recursion always runs over all
    steps.  A block whose lineage is undefined at any step (a whole-filter resample) or that has no path of positive density reads NaN paths and
    indices 0.  Under set_block_params every step uses the final block's CURRENT parameter row.  Nothing is drawn: the RNG epoch and the filter are
    left untouched."""
    who = "block_map_trajectories"
    _store_weights(state, who)
    lo, hi = _store_steps(state, steps, who)
    _, nb = _store_blocks(state, block_size, lo, hi, who)
    path = np.empty((nb, hi - lo + 1, state.dim))
    idx = np.empty((nb, hi - lo + 1), np.int64) if return_indices else None
    logp = np.empty(nb) if return_log_density else None
    state._check(state._L.gpf_block_map_path(state._h, int(block_size), lo, hi, _pd(path), _pi64(idx),
                                             _pd(logp) if return_log_density else None))
    out = (path,) + ((idx,) if return_indices else ()) + ((logp,) if return_log_density else ())
    return out if len(out) > 1 else path


# ----------------------------------------------------------------------------- statistics (src/statistics.jl)
def _addr_values(state, addr) -> np.ndarray:
    """the values at one address over all particles: a column of the current step, or (t, column) for a past choice"""
    return state.history_column(int(addr[0]), int(addr[1])) if isinstance(addr, tuple) else state.column(int(addr))


def _functional(f, state, addrs):
    if not addrs:
        raise ErrorException("native models have no return value: give at least one address")
    vals = [_addr_values(state, a) for a in addrs]
    try:
        fv = np.asarray(f(*vals), np.float64)
        if fv.shape != vals[0].shape:
            raise TypeError
    except (TypeError, ValueError):
        fv = np.array([f(*xs) for xs in zip(*vals)], np.float64)              # scalar closure: broadcast(f, ...)
    return fv


def mean(*args) -> float:
    """mean(state, addr), src/statistics.jl:13-14.  addr = column of the current-step latent, or a pair
    (t, column) for a PAST choice `t => column` (reference README.md:97; needs pf_initialize(..., history=T)).
    mean(f, state, addrs...), src/statistics.jl:28-35: weighted mean of a host closure of the values at the addresses
    (the values and the normalised weights are read back; f may be vectorised over NumPy arrays or scalar)."""
    if callable(args[0]):
        f, state, addrs = args[0], args[1], args[2:]
        return float(np.sum(get_norm_weights(state) * _functional(f, state, addrs)))
    state, addr = args
    out = C.c_double()
    if isinstance(addr, tuple):
        state._check(state._L.gpf_history_mean(state._h, int(addr[0]), int(addr[1]), C.byref(out)))
    else:
        state._check(state._L.gpf_mean(state._h, int(addr), C.byref(out)))
    return out.value


def var(*args) -> float:
    """var(state, addr), population form (src/statistics.jl:48-50); addr as in mean().
    var(f, state, addrs...), src/statistics.jl:65-76: var(fvals, Weights(w), corrected=false)."""
    if callable(args[0]):
        f, state, addrs = args[0], args[1], args[2:]
        w, fv = get_norm_weights(state), _functional(f, state, addrs)
        mu = np.sum(w * fv) / np.sum(w)
        return float(np.sum(w * (fv - mu) ** 2) / np.sum(w))
    state, addr = args
    out = C.c_double()
    if isinstance(addr, tuple):
        state._check(state._L.gpf_history_var(state._h, int(addr[0]), int(addr[1]), C.byref(out)))
    else:
        state._check(state._L.gpf_var(state._h, int(addr), C.byref(out)))
    return out.value


def proportionmap(state, addr, max_values: int = 256) -> dict:
    """proportionmap(state, addr), src/statistics.jl:91-101: {value: sum of normalised weights of the particles holding it}
    for a discrete-valued column (addr = column, or (t, column) for a past choice).  The distinct values are read from
    the column; each proportion is a weighted reduction on the device."""
    step, col = (int(addr[0]), int(addr[1])) if isinstance(addr, tuple) else (0, int(addr))
    vals = np.unique(state.history_column(step, col) if step else state.column(col))
    if vals.size > max_values:
        raise ErrorException(f"proportionmap: {vals.size} distinct values; the column does not look discrete")
    out = {}
    for v in vals:
        p = C.c_double()
        state._check(state._L.gpf_proportion(state._h, step, col, float(v), C.byref(p)))
        out[float(v)] = p.value
    return out
