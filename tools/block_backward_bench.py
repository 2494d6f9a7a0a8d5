"""Backward simulation per block (gpf.h gpf_block_backward_sample): what one call costs next to block_sample_trajectories on the same state, and what
recording the weights costs per step.

call   for every (model, n_blocks, block_size, T, n_samples) of CASES: T steps of the block-wise filter with the weights mode of the store (multinomial
       pf_resample_blocks at ESS < N / 2, pf_update_blocks with per-block data), then the two calls alternately on that one state: wall time of
       block_backward_trajectories(state, bs, k) and of block_sample_trajectories(state, bs, k), read-back of the paths included (both synchronise);
       median, minimum and maximum over --reps calls after --warmup.
step   us per step of pf_update_blocks + pf_resample_blocks (10^4 blocks of 100 particles, lgssm2, one synchronisation at the end of --steps steps)
       without a store, with the block-wise store, and with its weights mode; each mode a fresh state per round, the modes alternating, --reps rounds.
       --root DIR imports the package from another checkout (the parent commit's: the modes it knows), so that the same loop times both trees.

    python tools/block_backward_bench.py [--cases call,step] [--reps 20] [--warmup 3] [--steps 100] [--root DIR] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

CASES = [("lgssm2", 10_000, 100, 100, 1), ("bearings4", 10_000, 100, 100, 1), ("lgssm2", 64, 2048, 32, 16), ("bearings4", 64, 2048, 32, 16)]


def model_of(g, name):
    return g.models.bearings4(sb=0.5) if name == "bearings4" else g.models.by_name(name)


def data(g, m, n_blocks, T, seed=1):
    base = np.asarray(g.models.simulate(m, T))
    return base[None, :, :] + 0.2 * np.random.default_rng(seed).standard_normal((n_blocks,) + base.shape)


def stats(v):
    v = np.asarray(v) * 1e3
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))


def call_case(g, name, n_blocks, nb, T, k, reps, warmup, out):
    m = model_of(g, name)
    ys = data(g, m, n_blocks, T)
    st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, history=T, history_weights=True)
    for t in range(1, T):
        g.pf_resample_blocks(st, nb, "multinomial", ess_frac=0.5, check=False)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
    st.synchronize()
    calls = {"backward": lambda: g.block_backward_trajectories(st, nb, k), "ancestral": lambda: g.block_sample_trajectories(st, nb, k)}
    times = {c: [] for c in calls}
    distinct = {}
    for r in range(warmup + reps):
        for c, f in calls.items():
            t0 = time.perf_counter()
            traj = f()
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[c].append(dt)
            if k > 1:                                              # mean number of distinct x_1 among a block's draws
                distinct[c] = float(np.mean([len(np.unique(traj[b, :, 0], axis=0)) for b in range(min(n_blocks, 64))]))
    row = dict(case="call", model=name, n_blocks=n_blocks, block_size=nb, T=T, n_samples=k, reps=reps)
    for c in calls:
        row[c] = stats(times[c])
        if c in distinct:
            row[c]["distinct_x1_per_block"] = distinct[c]
    row["ratio_median"] = row["backward"]["median_ms"] / row["ancestral"]["median_ms"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n")
    st.close()


def step_case(g, steps, warmup, reps, out, with_weights):
    name, n_blocks, nb = "lgssm2", 10_000, 100
    m = model_of(g, name)
    Tn = steps + warmup + 1
    ys = data(g, m, n_blocks, 16)
    modes = {"no_store": {}, "store": dict(history=Tn)}
    if with_weights:
        modes["store_weights"] = dict(history=Tn, history_weights=True)
    res = {k: [] for k in modes}
    for _ in range(reps):
        for mode, kw in modes.items():
            st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, **kw)

            def loop(t0, cnt):
                for t in range(t0, t0 + cnt):
                    g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t % 16], nb)
                    g.pf_resample_blocks(st, nb, "multinomial", ess_frac=0.5, check=False)

            loop(1, warmup)
            st.synchronize()
            t0 = time.perf_counter()
            loop(1 + warmup, steps)
            st.synchronize()
            res[mode].append((time.perf_counter() - t0) / steps * 1e6)
            st.close()
    row = dict(case="step", model=name, n_blocks=n_blocks, block_size=nb, steps=steps, reps=reps, root=os.path.dirname(os.path.abspath(g.__file__)))
    for mode, v in res.items():
        row[mode] = dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)))
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="call,step")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import gpf_amd as g
    with_weights = hasattr(g, "block_backward_trajectories")
    with open(a.out, "w") as out:
        if "call" in a.cases and with_weights:
            for case in CASES:
                call_case(g, *case, a.reps, a.warmup, out)
        if "step" in a.cases:
            step_case(g, a.steps, max(a.warmup, 10), min(a.reps, 7), out, with_weights)


if __name__ == "__main__":
    main()
