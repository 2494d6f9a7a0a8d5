"""Whole trajectories per block (gpf.h gpf_block_sample_trajectories): what ONE call costs, next to the same arrays assembled the only way
there was before it.

object_motion (d = 2), keep_prev, T = 50 steps of the README loop per block (residual pf_resample_blocks at ESS < N / 2, mh rejuvenation of the
resampled blocks, pf_update_blocks with per-block data), then per case
  - one_launch: wall time of block_sample_trajectories(state, bs, k, return_indices=True), both read-backs included (median / min over --reps calls
    after --warmup);
  - assembled: history_column for every (t, c) -- T d launches and T d synchronising copies of n doubles -- plus NumPy indexing with the SAME
    indices (the draws themselves are not timed: they are taken from the one-launch call), on the same state, the two forms alternating;
and the two results are compared bit for bit.
The kernel's own time comes from a profiler run of `--trace N` (N calls per case, nothing else after set-up:
    rocprofv3 --kernel-trace --stats -- python tools/block_trajectories_bench.py --trace 10), summarised by --kernel-times TRACE.csv --trace 10.

    python tools/block_trajectories_bench.py [--reps 20] [--warmup 3] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpf_amd as g                                   # noqa: E402

T = 50
# (n_blocks, block_size, [n_samples])
CASES = [(10_000, 100, [1, 16]), (8, 2048, [256])]


def prepare(n_blocks, nb):
    m = g.models.object_motion()
    base = np.asarray(g.models.simulate(m, T))
    ys = base[None, :, :] + 0.2 * np.random.default_rng(1).standard_normal((n_blocks,) + base.shape)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, keep_prev=True, history=T)
    resampled = 0
    for t in range(1, T):
        resampled += g.pf_resample_blocks(st, nb, "residual", ess_frac=0.5, check=False)
        g.pf_rejuvenate_blocks(st, None, (), 1, method="move", only_resampled=True)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
    st.synchronize()
    return st, resampled


def assembled(st, nb, idx):
    """[n_blocks, k, T, d] from T d history_column calls and host-side indexing"""
    part = (np.arange(idx.shape[0]) * nb)[:, None] + idx - 1
    out = np.empty(idx.shape + (T, st.dim))
    for t in range(1, T + 1):
        for c in range(st.dim):
            out[:, :, t - 1, c] = st.history_column(t, c)[part]
    return out


def run_case(n_blocks, nb, ks, reps, warmup, out):
    st, resampled = prepare(n_blocks, nb)
    for k in ks:
        for _ in range(warmup):
            traj, idx = g.block_sample_trajectories(st, nb, k, return_indices=True)
            ref = assembled(st, nb, idx)
            assert np.array_equal(traj, ref)                                   # the same arrays, bit for bit
        one, asm = [], []
        for r in range(reps):
            t0 = time.perf_counter()
            traj, idx = g.block_sample_trajectories(st, nb, k, return_indices=True)
            one.append((time.perf_counter() - t0) * 1e6)
            if r < max(3, reps // 4):                                          # (the assembled form takes a large multiple: fewer repeats)
                t0 = time.perf_counter()
                ref = assembled(st, nb, idx)
                asm.append((time.perf_counter() - t0) * 1e6)
                assert np.array_equal(traj, ref)
        row = dict(case="block_sample_trajectories", model="object_motion", d=st.dim, n_blocks=n_blocks, block_size=nb, T=T, n_samples=k, reps=reps,
                   block_resamples_during_set_up=int(resampled), output_bytes=int(traj.nbytes + idx.nbytes),
                   one_launch_wall_us=float(np.median(one)), one_launch_wall_min_us=float(np.min(one)),
                   assembled_wall_us=float(np.median(asm)), assembled_wall_min_us=float(np.min(asm)), assembled_reps=len(asm),
                   assembled_launches=T * st.dim, assembled_copy_bytes=int(8 * T * st.dim * n_blocks * nb))
        row["ratio_assembled_to_one_launch"] = row["assembled_wall_us"] / row["one_launch_wall_us"]
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
    st.close()


def trace(n_calls):
    """nothing but n_calls calls per case after set-up: for a profiler's kernel trace"""
    for n_blocks, nb, ks in CASES:
        st, _ = prepare(n_blocks, nb)
        for k in ks:
            for _ in range(n_calls):
                g.block_sample_trajectories(st, nb, k, return_indices=True)
        st.close()


def kernel_times(trace_csv, n_calls, out):
    """per case the median duration of the kernel's dispatches in a rocprofv3 kernel trace of `--trace n_calls` (dispatch order = CASES x n_calls)"""
    import csv
    rows = [r for r in csv.DictReader(open(trace_csv)) if "k_block_sample_traj" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == sum(len(ks) for _, _, ks in CASES) * n_calls, len(rows)
    i = 0
    for n_blocks, nb, ks in CASES:
        for k in ks:
            grp = rows[i:i + n_calls]; i += n_calls
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in grp]
            names = {r["Kernel_Name"].split("(")[0].replace("void gpf::", "") for r in grp}
            assert len(names) == 1, names
            row = dict(case="kernel_time", n_blocks=n_blocks, block_size=nb, T=T, n_samples=k, kernel=names.pop(), dispatches=n_calls,
                       kernel_median_us=float(np.median(ns)) / 1e3, kernel_min_us=min(ns) / 1e3, kernel_max_us=max(ns) / 1e3)
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--kernel-times", metavar="TRACE.csv", default="", help="summarise the kernel trace of a `--trace N` run (give the same --trace N)")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    if a.kernel_times:
        with open(a.out, "a") as out:
            return kernel_times(a.kernel_times, a.trace, out)
    if a.trace:
        return trace(a.trace)
    with open(a.out, "w") as out:
        for case in CASES:
            run_case(*case, a.reps, a.warmup, out)


if __name__ == "__main__":
    main()
