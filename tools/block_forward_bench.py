"""Forward-only smoothing per block (gpf.h gpf_forward_enable_blocks / gpf_block_forward_moments): what a close costs -- the pass inside every
pf_update_blocks of a state with the mode on -- next to the same step of a state without it, and next to the per-step share of the backward yardstick,
block_smoothed_pair_moments over a store of T steps divided by T.

For every (model, n_blocks, block_size, T) of CASES (those of tools/block_smooth_bench.py), on two states with the same seed and data, no store:
    step_plain          pf_update_blocks + synchronize, mode off
    step_forward        the same with forward=True: the close of the step that ends rides in front of the update
once with a multinomial pf_resample_blocks (ESS < N / 2) before every update -- the close composes and follows the step's ancestor map -- and once
without any resample (the map is the identity), the two states stepped alternately; then on the forward state
    query               block_forward_moments(state, bs): the current step's statistics into scratch, the weighted trees, the read-back
and, unless --no-yardstick, on a third state with history=T, history_weights=True after T steps
    pairs_per_step      block_smoothed_pair_moments(state, bs) / T
Wall times, median / minimum / maximum over --reps steps after --warmup.  close_ms = step_forward - step_plain (medians).
--plain-only: only step_plain (a tree without the mode measures the block-wise step it has).

    python tools/block_forward_bench.py [--reps 20] [--warmup 3] [--cases 0,1,2,3] [--no-yardstick] [--plain-only] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

from block_smooth_bench import CASES, data, model_of, stats


def steps_of(g, states, ys, nb, resample, reps, warmup, t0):
    """alternately one step of every state; returns {label: [seconds per pf_update_blocks]} and the next step index"""
    times = {k: [] for k in states}
    for r in range(warmup + reps):
        t = t0 + r
        for k, st in states.items():
            if resample:
                g.pf_resample_blocks(st, nb, "multinomial", ess_frac=0.5, check=False)
            st.synchronize()
            a = time.perf_counter()
            g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t % ys.shape[1]], nb)
            st.synchronize()
            if r >= warmup:
                times[k].append(time.perf_counter() - a)
    return times, t0 + warmup + reps


def case(g, name, n_blocks, nb, T, a, out):
    m = model_of(g, name)
    ys = data(g, m, n_blocks, max(T, 8))
    states = {"step_plain": g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3)}
    if not a.plain_only:
        states["step_forward"] = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, forward=True)
    d = m.dim
    row = dict(model=name, n_blocks=n_blocks, block_size=nb, n_pairs_per_step=n_blocks * nb * nb, F=d + d * (d + 1) // 2 + d * d + d + d * (d + 1) // 2)
    t = 1
    for label, resample in (("resample", True), ("no_resample", False)):
        times, t = steps_of(g, states, ys, nb, resample, a.reps, a.warmup, t)
        row[label] = {k: stats(v) for k, v in times.items()}
        if not a.plain_only:
            row[label]["close_ms"] = row[label]["step_forward"]["median_ms"] - row[label]["step_plain"]["median_ms"]
            row[label]["ns_per_pair"] = row[label]["close_ms"] * 1e6 / row["n_pairs_per_step"]
    if not a.plain_only:
        st, q = states["step_forward"], []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            g.block_forward_moments(st, nb)
            if r >= a.warmup:
                q.append(time.perf_counter() - t0)
        row["query"] = stats(q)
    for st in states.values():
        st.close()
    if not a.plain_only and not a.no_yardstick:
        ys = data(g, m, n_blocks, T)
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, history=T, history_weights=True)
        for s in range(1, T):
            g.pf_resample_blocks(st, nb, "multinomial", ess_frac=0.5, check=False)
            g.pf_update_blocks(st, (s + 1,), (None,), ys[:, s], nb)
        st.synchronize()
        p = []
        for r in range(1 + a.yreps):
            t0 = time.perf_counter()
            g.block_smoothed_pair_moments(st, nb)
            if r >= 1:
                p.append(time.perf_counter() - t0)
        st.close()
        row["pairs"] = stats(p)
        row["pairs_per_step_ms"] = row["pairs"]["median_ms"] / T
        row["close_over_yardstick"] = row["resample"]["close_ms"] / row["pairs_per_step_ms"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yreps", type=int, default=3)
    ap.add_argument("--cases", default="0,1,2,3")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "w") as out:
        for k in (int(c) for c in a.cases.split(",")):
            case(g, *CASES[k], a, out)


if __name__ == "__main__":
    main()
