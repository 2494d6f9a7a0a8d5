"""Pairwise smoothing per block (gpf.h gpf_block_smooth_pairs): what one call costs next to the marginal smoother's moments on the same state -- the
sibling call that walks the same (target, candidate) pairs without the d multiply-adds per pair of the pair sums.

For every (model, n_blocks, block_size, T) of CASES (those of tools/block_smooth_bench.py): T steps of the block-wise filter with the weights mode of the
store (multinomial pf_resample_blocks at ESS < N / 2, pf_update_blocks with per-block data), then alternately on that one state the wall time of
    pairs      block_smoothed_pair_moments(state, bs)    mean, second and cross of all steps
    moments    block_smoothed_moments(state, bs)         the yardstick: mean and var of all steps
read-back included (every call synchronises); median, minimum and maximum over --reps calls after --warmup.

    python tools/block_pairs_bench.py [--reps 10] [--warmup 2] [--cases 0,1,2,3] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

from block_smooth_bench import CASES, data, model_of, stats


def case(g, name, n_blocks, nb, T, reps, warmup, out):
    m = model_of(g, name)
    ys = data(g, m, n_blocks, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, history=T, history_weights=True)
    for t in range(1, T):
        g.pf_resample_blocks(st, nb, "multinomial", ess_frac=0.5, check=False)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
    st.synchronize()
    calls = {"pairs": lambda: g.block_smoothed_pair_moments(st, nb), "moments": lambda: g.block_smoothed_moments(st, nb)}
    times = {c: [] for c in calls}
    for r in range(warmup + reps):
        for c, f in calls.items():
            t0 = time.perf_counter()
            f()
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[c].append(dt)
    row = dict(model=name, n_blocks=n_blocks, block_size=nb, T=T, n_pairs=n_blocks * nb * nb * (T - 1))
    for c in calls:
        row[c] = stats(times[c])
    row["pairs_over_moments"] = row["pairs"]["median_ms"] / row["moments"]["median_ms"]
    row["ns_per_pair"] = row["pairs"]["median_ms"] * 1e6 / row["n_pairs"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()
    st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="0,1,2,3")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "w") as out:
        for k in (int(c) for c in a.cases.split(",")):
            case(g, *CASES[k], a.reps, a.warmup, out)


if __name__ == "__main__":
    main()
