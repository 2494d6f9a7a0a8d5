"""Per-block posterior estimates (gpf.h gpf_block_moments) on the device: what one call costs next to what it replaces.

Many small filters (10^4 x 100 and 10^3 x 1024 particles) of lgssm2 (W = 2) and bearings4 with keep_prev (W = 8), after a few block-wise steps:
  - wall time of ONE block_moments call, read-back included (median over --reps calls after --warmup), next to one block_stats call on the same
    state -- the sibling with the same launch-plus-synchronise shape, which reads only the weights -- and one block_mean call (no variance pass);
  - the baseline the call replaces: the Python loop over views, mean(state[b], c) and var(state[b], c) per block and column, timed on --loop-blocks
    blocks (views created beforehand, and once more with their creation inside the loop), reported per block and scaled to all blocks.
The kernels' own times come from a profiler run of `--trace N` (N block_moments and N block_stats calls per case and nothing else after set-up:
    rocprofv3 --kernel-trace --stats -- python tools/block_estimates_bench.py --trace 20), which also shows one launch per call.

    python tools/block_estimates_bench.py [--reps 30] [--warmup 5] [--loop-blocks 200] [--out FILE.jsonl]
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
    base = np.asarray(g.models.simulate(m, steps + 2))
    ys = base[None, :, :] + 0.2 * np.random.default_rng(1).standard_normal((n_blocks,) + base.shape)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, nb, seed=3, keep_prev=keep_prev)
    for t in range(1, steps + 1):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
        g.pf_resample_blocks(st, nb, "residual", ess_frac=0.5, check=False)
    g.pf_update_blocks(st, (steps + 2,), (None,), ys[:, steps + 1], nb)
    st.synchronize()
    return st


def median_us(f, reps, warmup):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts)), float(np.min(ts))


def run_case(model_name, keep_prev, n_blocks, nb, reps, warmup, loop_blocks, out):
    st = prepare(model_name, keep_prev, n_blocks, nb)
    W, N = st.row_width, n_blocks * nb
    row = dict(case="block_moments", model=model_name, keep_prev=keep_prev, W=W, n_blocks=n_blocks, block_size=nb, reps=reps,
               algorithmic_bytes=(8 * W + 8) * N)
    row["moments_wall_us"], row["moments_wall_min_us"] = median_us(lambda: g.block_moments(st, nb), reps, warmup)
    row["mean_only_wall_us"], _ = median_us(lambda: g.block_mean(st, nb), reps, warmup)
    row["block_stats_wall_us"], row["block_stats_wall_min_us"] = median_us(lambda: g.block_stats(st, nb), reps, warmup)
    # the loop over views: mean and var of every column of a block, one call each
    nl = min(loop_blocks, n_blocks)
    views = [st[b * nb:(b + 1) * nb] for b in range(nl)]

    def loop(vs):
        for v in vs:
            for c in range(W):
                g.mean(v, c); g.var(v, c)

    loop(views[:10])                                                # warm-up
    t0 = time.perf_counter(); loop(views); t_loop = time.perf_counter() - t0
    for v in views:
        v.close()
    t0 = time.perf_counter()
    for b in range(nl):
        v = st[b * nb:(b + 1) * nb]; loop([v]); v.close()
    t_create = time.perf_counter() - t0
    row.update(loop_blocks=nl, loop_us_per_block=t_loop / nl * 1e6, loop_all_blocks_us=t_loop / nl * 1e6 * n_blocks,
               loop_with_view_creation_us_per_block=t_create / nl * 1e6)
    row["ratio_loop_to_one_call"] = row["loop_all_blocks_us"] / row["moments_wall_us"]
    row["ratio_moments_to_block_stats"] = row["moments_wall_us"] / row["block_stats_wall_us"]
    # the one call must say what the loop says
    mu, s2 = g.block_moments(st, nb)
    v = st[0:nb]
    assert all(mu[0, c] == g.mean(v, c) and s2[0, c] == g.var(v, c) for c in range(W))
    v.close()
    print(json.dumps(row), flush=True)
    out.write(json.dumps(row) + "\n")
    st.close()


def trace(n_calls):
    """nothing but n_calls block_moments and n_calls block_stats per case after set-up: for a profiler's kernel trace"""
    for model_name, keep_prev, n_blocks, nb in CASES:
        st = prepare(model_name, keep_prev, n_blocks, nb)
        for _ in range(n_calls):
            g.block_moments(st, nb)
        for _ in range(n_calls):
            g.block_stats(st, nb)
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-blocks", type=int, default=200)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    if a.trace:
        return trace(a.trace)
    with open(a.out, "w") as out:
        for case in CASES:
            run_case(*case, a.reps, a.warmup, a.loop_blocks, out)


if __name__ == "__main__":
    main()
