"""Marginal smoothing per block (gpf.h gpf_block_smooth): what one call costs, with and without the weights output, next to backward simulation with
n_samples = block_size on the same state -- the existing call that evaluates the same number of (target, candidate) pairs.

For every (model, n_blocks, block_size, T) of CASES: T steps of the block-wise filter with the weights mode of the store (multinomial
pf_resample_blocks at ESS < N / 2, pf_update_blocks with per-block data), then alternately on that one state the wall time of
    moments    block_smoothed_moments(state, bs)                        mean and var of all steps
    weights    block_smoothed_moments(state, bs, return_weights=True)   ... and the [n_blocks, T, bs] weights
    backward   block_backward_trajectories(state, bs, bs, steps=1)      the yardstick: bs draws per block, walked from T, step 1 returned
read-back included (every call synchronises); median, minimum and maximum over --reps calls after --warmup.  --yardstick-reps bounds the yardstick's
calls.

    python tools/block_smooth_bench.py [--reps 10] [--warmup 2] [--yardstick-reps 3] [--cases 0,1,2,3] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

CASES = [("lgssm2", 10_000, 100, 100), ("bearings4", 10_000, 100, 100), ("lgssm2", 64, 2048, 32), ("bearings4", 64, 2048, 32)]


def model_of(g, name):
    return g.models.bearings4(sb=0.5) if name == "bearings4" else g.models.by_name(name)


def data(g, m, n_blocks, T, seed=1):
    base = np.asarray(g.models.simulate(m, T))
    return base[None, :, :] + 0.2 * np.random.default_rng(seed).standard_normal((n_blocks,) + base.shape)


def stats(v):
    v = np.asarray(v) * 1e3
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), calls=int(v.size))


def case(g, name, n_blocks, nb, T, reps, warmup, yreps, out):
    m = model_of(g, name)
    ys = data(g, m, n_blocks, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, history=T, history_weights=True)
    for t in range(1, T):
        g.pf_resample_blocks(st, nb, "multinomial", ess_frac=0.5, check=False)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
    st.synchronize()
    calls = {"moments": lambda: g.block_smoothed_moments(st, nb), "weights": lambda: g.block_smoothed_moments(st, nb, return_weights=True),
             "backward": lambda: g.block_backward_trajectories(st, nb, nb, steps=1)}
    times = {c: [] for c in calls}
    for r in range(warmup + reps):
        for c, f in calls.items():
            if c == "backward" and r >= min(warmup, 1) + yreps:
                continue
            t0 = time.perf_counter()
            f()
            dt = time.perf_counter() - t0
            if r >= (min(warmup, 1) if c == "backward" else warmup):
                times[c].append(dt)
    row = dict(model=name, n_blocks=n_blocks, block_size=nb, T=T, pairs=n_blocks * nb * nb * (T - 1))
    for c in calls:
        row[c] = stats(times[c])
    row["moments_over_backward"] = row["moments"]["median_ms"] / row["backward"]["median_ms"]
    row["ns_per_pair"] = row["moments"]["median_ms"] * 1e6 / row["pairs"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()
    st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-reps", type=int, default=3)
    ap.add_argument("--cases", default="0,1,2,3")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "w") as out:
        for k in (int(c) for c in a.cases.split(",")):
            case(g, *CASES[k], a.reps, a.warmup, a.yardstick_reps, out)


if __name__ == "__main__":
    main()
