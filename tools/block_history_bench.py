"""The block-wise trajectory store (gpf.h gpf_history_enable_blocks, gpf_block_history_moments): what a query and the recording cost.

Many small filters (10^4 x 100 and 10^3 x 1024 particles) of lgssm2 (d = 2) and bearings4 (d = 4), keep_prev, T = 20 steps of the README loop per
block (residual pf_resample_blocks at ESS < N / 2, mh rejuvenation of the resampled blocks, pf_update_blocks with per-block data):
  - wall time of ONE block_moments(state, bs, step=t) call, read-back included (median over --reps calls after --warmup), for t = T, T / 2 and 1:
    the further back, the more ancestor maps a lane follows;
  - the baseline, what the numbers cost without the per-block query: a filter of the same size with the whole-filter store answers history_column
    per latent column plus log_weights, and NumPy forms the per-block weighted means on the host;
  - the recording cost: microseconds per pf_update_blocks (synchronised) with and without the store, same seed and data.
The kernels' own times come from a profiler run of `--trace N` (N query calls per case and step, nothing else after set-up:
    rocprofv3 --kernel-trace --stats -- python tools/block_history_bench.py --trace 20), which also shows one launch per call.

    python tools/block_history_bench.py [--reps 30] [--warmup 5] [--out FILE.jsonl]
    python tools/block_history_bench.py --no-store TAG [--out FILE.jsonl]                 the store-less update timings alone (appends): runs on the parent's build too
    python tools/block_history_bench.py --kernel-times TRACE.csv --trace 20 [--out FILE]  per case and step the kernel's median time from that trace (appends)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpf_amd as g                                   # noqa: E402

T = 20
STEPS = (20, 10, 1)
CASES = [("lgssm2", 10_000, 100), ("lgssm2", 1_000, 1024), ("bearings4", 10_000, 100), ("bearings4", 1_000, 1024)]


def data(m, n_blocks):
    base = np.asarray(g.models.simulate(m, T))
    return base[None, :, :] + 0.2 * np.random.default_rng(1).standard_normal((n_blocks,) + base.shape)


def prepare(model_name, n_blocks, nb, history):
    """the README loop per block; returns the state and the synchronised wall time of every pf_update_blocks in microseconds"""
    m = g.models.by_name(model_name)
    ys = data(m, n_blocks)
    kw = dict(history=history) if history else {}                 # (--no-store also runs on a build from before the store)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, keep_prev=True, **kw)
    st.synchronize()
    upd = []
    for t in range(1, T):
        g.pf_resample_blocks(st, nb, "residual", ess_frac=0.5, check=False)
        g.pf_rejuvenate_blocks(st, None, (), 1, method="move", only_resampled=True)
        st.synchronize()
        t0 = time.perf_counter()
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
        st.synchronize()
        upd.append((time.perf_counter() - t0) * 1e6)
    return st, upd


def prepare_plain(model_name, n_blocks, nb):
    """a filter of the same size with the whole-filter store: what answered past-step questions before the block-wise store"""
    m = g.models.by_name(model_name)
    ys = np.asarray(g.models.simulate(m, T))
    N = n_blocks * nb
    st = g.pf_initialize(m, (1,), ys[0], N, seed=3, keep_prev=True, history=T)
    for t in range(1, T):
        if g.effective_sample_size(st) < 0.5 * N:
            g.pf_resample(st, "residual", check=False)
            g.pf_rejuvenate(st, g.mh, (), 1)
        g.pf_update(st, (t + 1,), (None,), ys[t])
    st.synchronize()
    return st


def host_block_means(st, nb, step):
    """history_column per column + log_weights, the per-block weighted mean in NumPy"""
    lw = st.log_weights.reshape(-1, nb)
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    return np.stack([(w * st.history_column(step, c).reshape(-1, nb)).sum(axis=1) for c in range(st.dim)], axis=1)


def median_us(f, reps, warmup):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts)), float(np.min(ts))


def run_case(model_name, n_blocks, nb, reps, warmup, out):
    st, upd_store = prepare(model_name, n_blocks, nb, T)
    bare, upd_bare = prepare(model_name, n_blocks, nb, 0)
    plain = prepare_plain(model_name, n_blocks, nb)
    d, N = st.dim, n_blocks * nb
    for step in STEPS:
        row = dict(case="block_history_moments", model=model_name, d=d, n_blocks=n_blocks, block_size=nb, T=T, step=step, maps_followed=T - step, reps=reps,
                   algorithmic_bytes=(8 * d + 8 + 4 * (T - step)) * N)
        row["query_wall_us"], row["query_wall_min_us"] = median_us(lambda: g.block_moments(st, nb, step=step), reps, warmup)
        row["mean_only_wall_us"], _ = median_us(lambda: g.block_mean(st, nb, (step, 0)), reps, warmup)
        row["baseline_host_wall_us"], row["baseline_host_wall_min_us"] = median_us(lambda: host_block_means(plain, nb, step), max(3, reps // 3), 2)
        row["ratio_baseline_to_query"] = row["baseline_host_wall_us"] / row["query_wall_us"]
        # the query must say what the host computation says about the SAME state (to rounding: the host sums in another order)
        mu = g.block_moments(st, nb, step=step)[0]
        ref = host_block_means(st, nb, step)
        row["max_abs_diff_to_host"] = float(np.abs(mu - ref).max())
        assert row["max_abs_diff_to_host"] < 1e-9 * max(1.0, float(np.abs(ref).max())), row
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
    row = dict(case="recording", model=model_name, d=d, n_blocks=n_blocks, block_size=nb, T=T,
               update_blocks_with_store_us=float(np.median(upd_store[2:])), update_blocks_without_store_us=float(np.median(upd_bare[2:])),
               snapshot_bytes_per_step=8 * d * N)
    row["recording_cost_us"] = row["update_blocks_with_store_us"] - row["update_blocks_without_store_us"]
    assert np.array_equal(st.traces, bare.traces) and np.array_equal(st.log_weights, bare.log_weights)      # the store changes no result
    print(json.dumps(row), flush=True)
    out.write(json.dumps(row) + "\n")
    for x in (st, bare, plain):
        x.close()


def no_store(out, tag):
    """the store-less recording leg alone: the same steps on any build (the parent commit's: the baseline of the recording cost)"""
    for model_name, n_blocks, nb in CASES:
        st, upd = prepare(model_name, n_blocks, nb, 0)
        row = dict(case="update_blocks_no_store", build=tag, model=model_name, n_blocks=n_blocks, block_size=nb, T=T,
                   update_blocks_without_store_us=float(np.median(upd[2:])), update_blocks_min_us=float(np.min(upd[2:])))
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        st.close()


def kernel_times(trace_csv, n_calls, out):
    """per case and step the median duration of the query kernel's dispatches in a rocprofv3 kernel trace of `--trace n_calls` (dispatch order =
    CASES x STEPS x n_calls)"""
    import csv
    rows = [r for r in csv.DictReader(open(trace_csv)) if "k_block_hist_moments" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(CASES) * len(STEPS) * n_calls, len(rows)
    k = 0
    for model_name, n_blocks, nb in CASES:
        for step in STEPS:
            grp = rows[k:k + n_calls]; k += n_calls
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in grp]
            names = {r["Kernel_Name"].split("(")[0].replace("void gpf::", "") for r in grp}
            assert len(names) == 1, names
            row = dict(case="kernel_time", model=model_name, n_blocks=n_blocks, block_size=nb, T=T, step=step, kernel=names.pop(), dispatches=n_calls,
                       kernel_median_us=float(np.median(ns)) / 1e3, kernel_min_us=min(ns) / 1e3, kernel_max_us=max(ns) / 1e3)
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")


def trace(n_calls):
    """nothing but n_calls queries per case and step after set-up: for a profiler's kernel trace"""
    for model_name, n_blocks, nb in CASES:
        st, _ = prepare(model_name, n_blocks, nb, T)
        for step in STEPS:
            for _ in range(n_calls):
                g.block_moments(st, nb, step=step)
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--no-store", metavar="TAG", default="", help="only the store-less update_blocks timings, labelled TAG")
    ap.add_argument("--kernel-times", metavar="TRACE.csv", default="", help="summarise the kernel trace of a `--trace N` run (give the same --trace N)")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    if a.kernel_times:
        with open(a.out, "a") as out:
            return kernel_times(a.kernel_times, a.trace, out)
    if a.no_store:
        with open(a.out, "a") as out:
            return no_store(out, a.no_store)
    if a.trace:
        return trace(a.trace)
    with open(a.out, "w") as out:
        for case in CASES:
            run_case(*case, a.reps, a.warmup, out)


if __name__ == "__main__":
    main()
