"""The whole series per block in one launch on a filter with the block-wise trajectory store (gpf.h gpf_run_blocks_history) next to the loop of calls it
stands for and next to gpf_run_blocks on a filter without a store.  Per case three states from the same observations and seed -- a store without and with
the weight records, and no store -- and on them, alternating:
    loop       (store states) for t: pf_resample_blocks(st, bs, method, ess_frac=0.5, check=False); pf_update_blocks(st, ..., ys[:, t], bs)
    loop_c     (store states) the same 2 T calls through the C ABI with invalid = n_resampled = NULL; one synchronisation at the end
    run_hist   (store states) pf_run_blocks_history(st, ys, bs, method, ess_frac=0.5)
    run        (no store)     pf_run_blocks(st, ys, bs, method, ess_frac=0.5): the yardstick
Before every timed call the state is initialised again (not timed; that also frees the store's steps), so every call of a case does the same work.  Wall
time around each call, ending in a synchronisation; median, minimum, maximum over --reps after --warmup.  Kernel time (gpf_kernel_timing) from --kreps
further calls: GPF_K_SEARCH + GPF_K_STEP, which hold k_block_resample + k_step of the loop and the one kernel of the runs; the loop's snapshot, compose and
staging kernels are not in it.  alloc_ms: the call's 2 T device allocations (T slabs, T maps of the call's sizes) made and freed through the HIP runtime
directly, the median of --reps.  After the timing two fresh states run the loop and the one call and the state and one query of the store are compared.

    python tools/block_run_history_bench.py [--reps 5] [--warmup 1] [--kreps 2] [--cases 0,1] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from block_run_bench import K_SEARCH, K_STEP, NAN, pd
from block_smooth_bench import data, model_of, stats

# (model, n_blocks, block_size, T, method)
CASES = [("lgssm2", 10_000, 100, 100, "residual"), ("lgssm2", 64, 2048, 32, "residual")]
MAX_OBS = 4


def alloc_ms(n, d, n_blocks, T, weights, reps):
    hip = C.CDLL("libamdhip64.so")
    slab = 8 * (n * d + (n + n_blocks * MAX_OBS if weights else 0))
    ts = []
    for _ in range(reps):
        ptrs = [C.c_void_p() for _ in range(2 * T)]
        t0 = time.perf_counter()
        for k, p in enumerate(ptrs):
            assert hip.hipMalloc(C.byref(p), C.c_size_t(slab if k < T else 4 * n)) == 0
        ts.append(time.perf_counter() - t0)
        for p in ptrs:
            hip.hipFree(p)
    return 1e3 * float(np.median(ts))


def case(g, name, n_blocks, nb, T, method, reps, warmup, kreps, out):
    m = model_of(g, name)
    ys = np.ascontiguousarray(data(g, m, n_blocks, T + 1))
    y0, yrun = np.ascontiguousarray(ys[:, 0]), np.ascontiguousarray(ys[:, 1:])
    ysteps = [np.ascontiguousarray(yrun[:, t]) for t in range(T)]
    n, n_obs, mid = n_blocks * nb, y0.shape[1], g.api.RESAMPLE_METHODS[method]
    make = lambda **kw: g.pf_initialize_blocks(m, (1,), y0, n, nb, seed=3, **kw)
    states = {"store": make(history=T + 1), "store_weights": make(history=T + 1, history_weights=True), "plain": make()}

    def reset(st):
        st._check(st._L.gpf_initialize_blocks(st._h, pd(y0), n_obs, nb))
        st.synchronize()

    def loop(st):
        for t in range(T):
            g.pf_resample_blocks(st, nb, method, ess_frac=0.5, check=False)
            g.pf_update_blocks(st, (t + 2,), (None,), ysteps[t], nb)
        st.synchronize()

    def loop_c(st):
        for t in range(T):
            st._check(st._L.gpf_resample_blocks(st._h, mid, nb, NAN, 1, 0.5, 0, None, None))
            st._check(st._L.gpf_update_blocks(st._h, pd(ysteps[t]), n_obs, nb))
        st.synchronize()

    calls = {}
    for k in ("store", "store_weights"):
        calls[k + ".loop"] = (states[k], loop)
        calls[k + ".loop_c"] = (states[k], loop_c)
        calls[k + ".run_hist"] = (states[k], lambda st: g.pf_run_blocks_history(st, yrun, nb, method, ess_frac=0.5))
    calls["plain.run"] = (states["plain"], lambda st: g.pf_run_blocks(st, yrun, nb, method, ess_frac=0.5))
    times = {c: [] for c in calls}
    for r in range(warmup + reps):
        for c, (st, f) in calls.items():
            reset(st)
            t0 = time.perf_counter()
            f(st)
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[c].append(dt)
    row = dict(model=name, n_blocks=n_blocks, block_size=nb, T=T, method=method, ess_frac=0.5, dim=m.dim)
    for c, (st, f) in calls.items():
        ks = []
        for _ in range(kreps):
            reset(st)                                                          # (before the timers go on: the initialising kernel is booked under GPF_K_STEP too)
            st.kernel_timing(K_STEP, True); st.kernel_timing(K_SEARCH, True)
            f(st)
            (ms_a, n_a), (ms_b, n_b) = st.kernel_time(K_STEP), st.kernel_time(K_SEARCH)
            st.kernel_timing(K_STEP, False); st.kernel_timing(K_SEARCH, False)
            ks.append((ms_a + ms_b, n_a + n_b))
        row[c] = dict(stats(times[c]), kernel_ms_per_call=float(np.median([k[0] for k in ks])), launches_per_call=int(ks[0][1]))
    for st in states.values():
        st.close()
    for k, w in (("store", False), ("store_weights", True)):
        row[k + ".alloc_ms"] = alloc_ms(n, m.dim, n_blocks, T, w, reps)
        row[k + ".added_bytes_per_call"] = (8 * (m.dim + (1 if w else 0)) + 4) * n * T
    # the same results: two fresh states, the loop on one, the call on the other
    p, q = (make(history=T + 1, history_weights=True) for _ in range(2))
    loop(p)
    g.pf_run_blocks_history(q, yrun, nb, method, ess_frac=0.5)
    row["same_results"] = bool(np.array_equal(p.log_weights, q.log_weights) and np.array_equal(p.traces, q.traces) and np.array_equal(p.parents, q.parents)
                               and np.array_equal(p.history_column(1, 0), q.history_column(1, 0))
                               and all(np.array_equal(x, y) for x, y in zip(g.block_smoothed_moments(p, nb, steps=(T - 1, T + 1)), g.block_smoothed_moments(q, nb, steps=(T - 1, T + 1)))))
    p.close(); q.close()
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kreps", type=int, default=2)
    ap.add_argument("--cases", default=None)
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "a") as out:
        for k in (int(c) for c in a.cases.split(",")) if a.cases else range(len(CASES)):
            case(g, *CASES[k], a.reps, a.warmup, a.kreps, out)


if __name__ == "__main__":
    main()
