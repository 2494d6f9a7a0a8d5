"""A whole series per block in one launch (gpf.h gpf_run_blocks) next to the loop of calls it stands for, on ONE state, alternating:
    loop       for t: pf_resample_blocks(st, bs, method, ess_frac=0.5, check=False); pf_update_blocks(st, ..., ys[:, t], bs)     the package's calls: the
               resample reads its count back, so every iteration synchronises once
    loop_c     the same 2 T calls through the C ABI with invalid = n_resampled = NULL: nothing is read back, the host runs ahead of the device; one
               synchronisation at the end.  The stricter yardstick
    run        pf_run_blocks(st, ys, bs, method, ess_frac=0.5)                                        one call, outputs read back
    run_shared (--shared cases) the same with ONE series for all blocks, (T, n_obs)
Before every timed call the state is initialised again from the same observations and seed (not timed), so every call of a case does the same work and the
calls are comparable (the epoch goes on, so the draws differ from call to call); after the timing two fresh states run the loop and the one call
and their rows, log-weights, parents and log-ML estimates are compared bit for bit (same_results).  Wall time around each call, ending in a
synchronisation; median, minimum, maximum over --reps after --warmup.  Kernel time (gpf_kernel_timing, the dispatches' own durations) from --kreps
further calls with the timers on: the loop's is k_block_resample (GPF_K_SEARCH) + k_step (GPF_K_STEP), the run's k_block_run (booked under GPF_K_STEP);
the loop's staging kernels are not in it.

    python tools/block_run_bench.py [--reps 7] [--warmup 2] [--kreps 2] [--cases 0,1,2] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from block_smooth_bench import data, model_of, stats

# (model, n_blocks, block_size, T, method, also the shared-series form)
CASES = [("lgssm2", 10_000, 100, 100, "residual", True), ("bearings4", 10_000, 100, 100, "residual", False), ("lgssm2", 64, 2048, 32, "residual", False)]
K_STEP, K_SEARCH = 0, 3
NAN = float("nan")


def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def case(g, name, n_blocks, nb, T, method, with_shared, reps, warmup, kreps, out):
    m = model_of(g, name)
    ys = np.ascontiguousarray(data(g, m, n_blocks, T + 1))
    y0, yrun = np.ascontiguousarray(ys[:, 0]), np.ascontiguousarray(ys[:, 1:])
    ysteps = [np.ascontiguousarray(yrun[:, t]) for t in range(T)]
    yshared = np.ascontiguousarray(yrun[0])
    st = g.pf_initialize_blocks(m, (1,), y0, n_blocks * nb, nb, seed=3)
    L, h, mid, n_obs = st._L, st._h, g.api.RESAMPLE_METHODS[method], y0.shape[1]

    def reset():
        st._check(L.gpf_initialize_blocks(h, pd(y0), n_obs, nb))
        st.synchronize()

    def loop():
        for t in range(T):
            g.pf_resample_blocks(st, nb, method, ess_frac=0.5, check=False)
            g.pf_update_blocks(st, (t + 2,), (None,), ysteps[t], nb)
        st.synchronize()

    def loop_c():
        for t in range(T):
            st._check(L.gpf_resample_blocks(h, mid, nb, NAN, 1, 0.5, 0, None, None))
            st._check(L.gpf_update_blocks(h, pd(ysteps[t]), n_obs, nb))
        st.synchronize()

    calls = {"loop": loop, "loop_c": loop_c, "run": lambda: g.pf_run_blocks(st, yrun, nb, method, ess_frac=0.5)}
    if with_shared:
        calls["run_shared"] = lambda: g.pf_run_blocks(st, yshared, nb, method, ess_frac=0.5)
    times = {c: [] for c in calls}
    for r in range(warmup + reps):
        for c, f in calls.items():
            reset()
            t0 = time.perf_counter()
            f()
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[c].append(dt)
    kernel = {}
    for c, f in calls.items():
        for _ in range(kreps):
            reset()                                                            # (before the timers go on: the initialising kernel is booked under GPF_K_STEP too)
            st.kernel_timing(K_STEP, True); st.kernel_timing(K_SEARCH, True)
            f()
            (ms_a, n_a), (ms_b, n_b) = st.kernel_time(K_STEP), st.kernel_time(K_SEARCH)
            st.kernel_timing(K_STEP, False); st.kernel_timing(K_SEARCH, False)
            kernel.setdefault(c, []).append((ms_a + ms_b, n_a + n_b))
        kernel[c] = dict(kernel_ms_per_call=float(np.median([k[0] for k in kernel[c]])), launches_per_call=int(kernel[c][0][1]))
    # the same results: two fresh states at the same epoch, the loop on one, the call on the other
    p, q = (g.pf_initialize_blocks(m, (1,), y0, n_blocks * nb, nb, seed=3) for _ in range(2))
    for t in range(T):
        g.pf_resample_blocks(p, nb, method, ess_frac=0.5, check=False)
        g.pf_update_blocks(p, (t + 2,), (None,), ysteps[t], nb)
    r = g.pf_run_blocks(q, yrun, nb, method, ess_frac=0.5)
    same = bool(np.array_equal(p.log_weights, q.log_weights) and np.array_equal(p.traces, q.traces) and np.array_equal(p.parents, q.parents)
                and np.array_equal(g.block_stats(p, nb)[1], r.lml[:, -1]))
    p.close(); q.close()
    row = dict(model=name, n_blocks=n_blocks, block_size=nb, T=T, method=method, ess_frac=0.5)
    for c in calls:
        row[c] = dict(stats(times[c]), **kernel[c])
    row["same_results"] = same
    row["resampled_share"] = float(r.resampled.mean())
    row["run_over_loop"] = row["run"]["median_ms"] / row["loop"]["median_ms"]
    row["run_over_loop_c"] = row["run"]["median_ms"] / row["loop_c"]["median_ms"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()
    st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kreps", type=int, default=2)
    ap.add_argument("--cases", default="0,1,2")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "a") as out:
        for k in (int(c) for c in a.cases.split(",")):
            case(g, *CASES[k], a.reps, a.warmup, a.kreps, out)


if __name__ == "__main__":
    main()
