"""Per-block model parameters (gpf.h gpf_set_block_params) on the device: what they cost, and a known answer.

(a) Cost.  Many small filters (10^4 x 100 and 10^3 x 1024 particles) of object_motion and lgssm2 with keep_prev run the step
    pf_update_blocks -> pf_resample_blocks(residual, ess_frac 0.5) -> pf_rejuvenate_blocks(move), once with the shared parameters and once with
    per-block parameters, alternating in the same process.  Reports us per step (wall clock over the timed steps, one synchronisation at the end)
    and the k_step / k_move dispatch times (gpf_kernel_timing: the kernels' own begin / end stamps).
(b) Known answer.  lgssm2 over a theta grid (rho x sigma_r), replicate blocks per theta, T steps of data simulated at one grid point, the locally
    optimal proposal in every block: each block's log_ml_estimate next to models.kalman_loglik for its theta.

    python tools/block_params_bench.py [--steps 50] [--warmup 5] [--reps 3] [--out FILE.jsonl]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpf_amd as g                                   # noqa: E402

K_STEP, K_MOVE = g._lib.K_STEP, g._lib.K_MOVE


def variants(model_name, n_sets=7):
    m = g.models
    if model_name == "lgssm2":
        return [m.lgssm2(rho=0.9 + 0.015 * k, sr=0.3 + 0.1 * k) for k in range(n_sets)]
    return [m.object_motion(p_stay=0.6 + 0.05 * k, sobs=0.2 + 0.05 * k) for k in range(n_sets)]


def run_case(model_name, n_blocks, nb, steps, warmup, reps, out):
    m = g.models.by_name(model_name)
    N = n_blocks * nb
    T = steps + warmup + 1
    base = np.asarray(g.models.simulate(m, T))
    ys = base[None, :, :] + 0.2 * np.random.default_rng(1).standard_normal((n_blocks,) + base.shape)
    sets = variants(model_name)
    rows = [sets[b % len(sets)] for b in range(n_blocks)]
    states = {}
    for mode in ("shared", "per_block"):
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], N, nb, seed=3, keep_prev=True, params=rows if mode == "per_block" else None)
        st.kernel_timing(K_STEP, True); st.kernel_timing(K_MOVE, True)
        states[mode] = st
    res = {k: [] for k in states}
    t_next = {k: 1 for k in states}
    for rep in range(reps):                                         # alternate: shared, per-block, shared, ...
        for mode, st in states.items():
            def step(t):
                g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
                g.pf_resample_blocks(st, nb, "residual", ess_frac=0.5, check=False)
                g.pf_rejuvenate_blocks(st, None, (), 1, method="move")
            t = t_next[mode]
            for _ in range(warmup if rep == 0 else 0):
                step(t % (T - 1) + 1); t += 1
            st.synchronize()
            k0 = {k: st.kernel_time(k) for k in (K_STEP, K_MOVE)}
            t0 = time.perf_counter()
            for _ in range(steps):
                step(t % (T - 1) + 1); t += 1
            st.synchronize()
            wall = (time.perf_counter() - t0) / steps * 1e6
            k1 = {k: st.kernel_time(k) for k in (K_STEP, K_MOVE)}
            kern = {g._lib.KERNEL_NAMES[k]: (k1[k][0] - k0[k][0]) * 1e3 / max(1, k1[k][1] - k0[k][1]) for k in (K_STEP, K_MOVE)}
            res[mode].append(dict(wall_us=wall, **{f"{n}_us": v for n, v in kern.items()}))
            t_next[mode] = t
    summary = dict(case="cost", model=model_name, n_blocks=n_blocks, block_size=nb, steps=steps, reps=reps)
    for mode in res:
        for key in res[mode][0]:
            summary[f"{mode}_{key}"] = float(np.median([r[key] for r in res[mode]]))
    for key in ("wall_us", "k_step_us", "k_move_us"):
        summary[f"ratio_{key}"] = summary[f"per_block_{key}"] / summary[f"shared_{key}"]
    print(json.dumps(summary), flush=True)
    out.write(json.dumps(summary) + "\n")
    for st in states.values():
        st.close()


def known_answer(out, T=100, reps=4, nb=2048, seed=29, data_seed=1, true=(0.99, 0.5)):
    grid = [(r, s) for r in (0.9, 0.95, 0.99) for s in (0.3, 0.5, 0.8)]
    ms = [g.models.lgssm2(rho=r, sr=s) for r, s in grid]
    ys = np.asarray(g.models.simulate(g.models.lgssm2(rho=true[0], sr=true[1]), T, seed=data_seed))
    B = len(grid) * reps
    assign = np.arange(B) % len(grid)
    st = g.pf_initialize_blocks(ms[0], (1,), np.tile(ys[0], (B, 1)), B * nb, nb, seed=seed, params=[ms[k] for k in assign])
    t0 = time.perf_counter()
    for t in range(1, T):
        g.pf_update_blocks(st, (t + 1,), (None,), np.tile(ys[t], (B, 1)), nb, proposals=[g.locally_optimal] * B)
        g.pf_resample_blocks(st, nb, "residual", ess_frac=0.5, check=False)
    lml = g.block_stats(st, nb)[1]
    wall = time.perf_counter() - t0
    st.close()
    for k, (r, s) in enumerate(grid):
        v = lml[assign == k]
        mx = float(np.max(v))
        row = dict(case="known_answer", rho=r, sigma_r=s, data_generating=(r, s) == true, blocks=[int(b) for b in np.flatnonzero(assign == k)],
                   block_log_ml=[float(x) for x in v], log_mean_exp=mx + math.log(float(np.mean(np.exp(v - mx)))),
                   kalman=g.models.kalman_loglik(ms[k], ys), T=T, block_size=nb, wall_s=wall)
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.devnull)
    ap.add_argument("--cases", default="cost,known")
    a = ap.parse_args()
    with open(a.out, "w") as out:
        if "cost" in a.cases:
            for model_name in ("object_motion", "lgssm2"):
                for n_blocks, nb in ((10_000, 100), (1_000, 1024)):
                    run_case(model_name, n_blocks, nb, a.steps, a.warmup, a.reps, out)
        if "known" in a.cases:
            known_answer(out)


if __name__ == "__main__":
    main()
