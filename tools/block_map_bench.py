"""The most probable path per block (gpf.h gpf_block_map_path): what one call costs next to the marginal smoother's moments on the same state -- the two
walk the same store and evaluate the same number of (target, candidate) pairs; the smoother normalises per target (two team reductions and an exp_fix per
pair), the max-plus recursion does not.

For every (model, n_blocks, block_size, T) of CASES: T steps of the block-wise filter with the weights mode of the store (multinomial
pf_resample_blocks at ESS < N / 2, pf_update_blocks with per-block data), then alternately on that one state the wall time of
    map        block_map_trajectories(state, bs, return_indices=True, return_log_density=True)   paths, indices and logp of all steps
    logp       the entry point with logp_out alone: the recursion without the trace and without the paths' read-back
    map_T      block_map_trajectories(state, bs, steps=T)     one step written, the LAST: the trace follows all T - 1 pointers
    map_1      block_map_trajectories(state, bs, steps=1)     one step written, the FIRST: the trace follows none
    moments    block_smoothed_moments(state, bs)              the yardstick: mean and var of all steps
read-back included (every call synchronises); median, minimum and maximum over --reps calls after --warmup.  trace_ms = map_T - map_1 (medians): the
T - 1 dependent loads of one lane per block, the same outputs on both sides.

    python tools/block_map_bench.py [--reps 10] [--warmup 2] [--cases 0,1,2] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from block_smooth_bench import data, model_of, stats

CASES = [("lgssm2", 10_000, 100, 100), ("bearings4", 10_000, 100, 100), ("lgssm2", 64, 2048, 32)]


def case(g, name, n_blocks, nb, T, reps, warmup, out):
    m = model_of(g, name)
    ys = data(g, m, n_blocks, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, history=T, history_weights=True)
    for t in range(1, T):
        g.pf_resample_blocks(st, nb, "multinomial", ess_frac=0.5, check=False)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
    st.synchronize()
    lp = np.empty(n_blocks)

    def logp_only():
        st._check(st._L.gpf_block_map_path(st._h, nb, 1, T, None, None, lp.ctypes.data_as(C.POINTER(C.c_double))))

    calls = {"map": lambda: g.block_map_trajectories(st, nb, return_indices=True, return_log_density=True), "logp": logp_only,
             "map_T": lambda: g.block_map_trajectories(st, nb, steps=T), "map_1": lambda: g.block_map_trajectories(st, nb, steps=1),
             "moments": lambda: g.block_smoothed_moments(st, nb)}
    times = {c: [] for c in calls}
    for r in range(warmup + reps):
        for c, f in calls.items():
            t0 = time.perf_counter()
            f()
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[c].append(dt)
    row = dict(model=name, n_blocks=n_blocks, block_size=nb, T=T, pairs=n_blocks * nb * nb * (T - 1))
    for c in calls:
        row[c] = stats(times[c])
    row["map_over_moments"] = row["map"]["median_ms"] / row["moments"]["median_ms"]
    row["trace_ms"] = row["map_T"]["median_ms"] - row["map_1"]["median_ms"]
    row["trace_share"] = row["trace_ms"] / row["map_T"]["median_ms"]
    row["ns_per_pair"] = row["logp"]["median_ms"] * 1e6 / row["pairs"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()
    st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="0,1,2")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "a") as out:
        for k in (int(c) for c in a.cases.split(",")):
            case(g, *CASES[k], a.reps, a.warmup, out)


if __name__ == "__main__":
    main()
