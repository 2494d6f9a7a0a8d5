"""Resampling across blocks (gpf.h gpf_resample_across_blocks) on the device: what one fired call costs next to what it replaces.

Many small filters (10^4 x 100 and 10^3 x 1024 particles) of lgssm2 (W = 2) and bearings4 with keep_prev (W = 8), after a few block-wise steps:
  - wall time of ONE fired pf_resample_across_blocks call, the read-back of the block ancestors included (median over --reps calls after
    --warmup; the weights are put back between calls, outside the timed region, so that every call resamples the same uneven blocks);
  - the baseline a user of the library without the call has for the same effect: block_stats, the block ancestors on the host (NumPy), the
    rows and log-weights read back (get_traces / get_log_weights), permuted block-wise on the host, and written back (traces / log_weights
    setters).  It leaves the parents and the per-block observations behind, which the host cannot set at all;
  - the gather kernel's own time from the library's kernel timing (gpf_kernel_timing, GPF_K_GATHER: the one k_block_gather launch of the call) next
    to its algorithmic bytes 2 (8 W + 16) n and the rate that makes.
The kernels of a call and their count come from a profiler run of `--trace N` (N fired calls per case and nothing else after set-up:
    rocprofv3 --kernel-trace --stats -- python tools/across_blocks_bench.py --trace 20).

    python tools/across_blocks_bench.py [--reps 30] [--warmup 5] [--method multinomial] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpf_amd as g                                   # noqa: E402

CASES = [("lgssm2", False, 10_000, 100), ("lgssm2", False, 1_000, 1024), ("bearings4", True, 10_000, 100), ("bearings4", True, 1_000, 1024)]


def prepare(model_name, keep_prev, n_blocks, nb, steps=3):
    m = g.models.by_name(model_name)
    N = n_blocks * nb
    base = np.asarray(g.models.simulate(m, steps + 1))
    ys = base[None, :, :] + 0.2 * np.random.default_rng(1).standard_normal((n_blocks,) + base.shape)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, nb, seed=3, keep_prev=keep_prev)
    for t in range(1, steps + 1):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
    st.synchronize()
    return st


def timed_us(f, reset, reps, warmup):
    ts = []
    for k in range(warmup + reps):
        reset()
        t0 = time.perf_counter(); f(); dt = (time.perf_counter() - t0) * 1e6
        if k >= warmup:
            ts.append(dt)
    return float(np.median(ts)), float(np.min(ts))


def host_baseline(st, nb, rng):
    """the same effect with the calls the library had before: everything through the host"""
    ess, L = g.block_stats(st, nb)
    B = L.size
    w = np.exp(L - L.max()); w /= w.sum()
    A = rng.choice(B, size=B, p=w)                                   # (multinomial ancestors; any host resampler costs about the same)
    M = L.max() + np.log(np.mean(np.exp(L - L.max())))
    rows, lw = st.traces, st.log_weights
    W = rows.shape[1]
    st.traces = rows.reshape(B, nb, W)[A].reshape(-1, W)
    st.log_weights = (lw.reshape(B, nb)[A] + (M - L[A])[:, None]).ravel()
    return A


def run_case(model_name, keep_prev, n_blocks, nb, reps, warmup, method, out):
    st = prepare(model_name, keep_prev, n_blocks, nb)
    W, N = st.row_width, n_blocks * nb
    lw0 = st.log_weights

    def reset():
        st.log_weights = lw0                                        # the same uneven block weights for every call (rows may be any)
        st.synchronize()

    row = dict(case="resample_across_blocks", model=model_name, keep_prev=keep_prev, W=W, n_blocks=n_blocks, block_size=nb, reps=reps, method=method,
               algorithmic_bytes=2 * (8 * W + 16) * N)
    fired = []
    row["call_wall_us"], row["call_wall_min_us"] = timed_us(lambda: fired.append(g.pf_resample_across_blocks(st, nb, method, check=False) is not None),
                                                            reset, reps, warmup)
    assert all(fired)
    # the gather kernel's own duration (dispatch begin to end, as a kernel trace reports it)
    st.kernel_timing(g._lib.K_GATHER, True)
    for _ in range(reps):
        reset(); g.pf_resample_across_blocks(st, nb, method, check=False)
    st.synchronize()
    ms, cnt = st.kernel_time(g._lib.K_GATHER)
    st.kernel_timing(g._lib.K_GATHER, False)
    row["gather_launches_per_call"] = cnt / reps
    row["gather_kernel_us"] = ms * 1e3 / max(cnt, 1)
    row["gather_TB_per_s"] = row["algorithmic_bytes"] / (row["gather_kernel_us"] * 1e-6) / 1e12
    rng = np.random.default_rng(5)
    nrep = max(3, reps // 5)
    row["host_baseline_wall_us"], row["host_baseline_wall_min_us"] = timed_us(lambda: host_baseline(st, nb, rng), reset, nrep, 1)
    row["ratio_host_baseline_to_call"] = row["host_baseline_wall_us"] / row["call_wall_us"]
    # the call must do what it says: every block's estimate is the average mass afterwards
    reset()
    L = g.block_stats(st, nb)[1]
    A = g.pf_resample_across_blocks(st, nb, method, check=False)
    M = L.max() + np.log(np.mean(np.exp(L - L.max())))
    assert A is not None and np.max(np.abs(g.block_stats(st, nb)[1] - M)) < 1e-9
    print(json.dumps(row), flush=True)
    out.write(json.dumps(row) + "\n")
    st.close()


def trace(n_calls, method):
    """nothing but n_calls fired calls per case after set-up: for a profiler's kernel trace"""
    for model_name, keep_prev, n_blocks, nb in CASES:
        st = prepare(model_name, keep_prev, n_blocks, nb)
        lw0 = st.log_weights
        for _ in range(n_calls):
            st.log_weights = lw0
            g.pf_resample_across_blocks(st, nb, method, check=False)
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--method", default="multinomial")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    if a.trace:
        return trace(a.trace, a.method)
    with open(a.out, "w") as out:
        for case in CASES:
            run_case(*case, a.reps, a.warmup, a.method, out)


if __name__ == "__main__":
    main()
