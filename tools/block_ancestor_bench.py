"""Ancestor sampling for conditional SMC per block on the device: what pf_resample_blocks(conditional=True, reference=...) costs next to
pf_resample_blocks(conditional=True), and what it buys.

(a) Two states of one seed side by side, timed alternately (conditional, ancestor, conditional, ...) in one process: the block-resample dispatch
    time from gpf_kernel_timing (the kernel's own begin / end stamps; the copy of the staged inputs is a launch of its own and not in it) and us per
    call on the host clock with one synchronisation at the end (wall = pinned update + resample, the staging included).  The conditional kernels are
    instruction for instruction those of the commit before this feature (tools/isa_diff.py), so "conditional" is the parent's kernel.  The run-to-run
    spread of each is the range of its per-round means.
(b) The share of blocks whose drawn path no longer starts at the reference's x_1 after a sweep of T = 8 steps -- lgssm2 defaults, 4096 blocks of 8
    particles, references from the exact smoother (the experiment of tests/block_ancestor_spec.py) -- with the plain conditional step and with
    ancestor sampling.

    python tools/block_ancestor_bench.py [--steps 100] [--warmup 10] [--reps 5] [--out FILE.jsonl] [--cases resample,renewal]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpf_amd as g                                   # noqa: E402

K_SEARCH = g._lib.K_SEARCH                            # (the block resample is timed under the search slot)
SHAPES = ((10_000, 100), (1_000, 2048))
MODELS = ("lgssm2", "bearings4")


def data(m, n_blocks, T, seed=1):
    base = np.asarray(g.models.simulate(m, T))
    rng = np.random.default_rng(seed)
    ys = base[None, :, :] + 0.2 * rng.standard_normal((n_blocks,) + base.shape)
    ref = rng.standard_normal((n_blocks, T, m.dim))
    if m.name == "bearings4":
        ref += np.array([1.0, 1.0, 0.0, 0.0])
    return ys, ref


def resample_case(model_name, n_blocks, nb, steps, warmup, reps, out):
    m = g.models.bearings4(sb=0.5) if model_name == "bearings4" else g.models.by_name(model_name)
    T = 32
    ys, ref = data(m, n_blocks, T)
    states = {}
    for mode in ("conditional", "ancestor"):
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, keep_prev=True, reference=ref[:, 0])
        st.kernel_timing(K_SEARCH, True)
        states[mode] = st

    def call(mode, st, t):                                 # (a pinned update in between, so that every resample meets fresh weights)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb, reference=ref[:, t])
        t1 = t % (T - 1) + 1
        kw = dict(reference=ref[:, t1], observations=ys[:, t1]) if mode == "ancestor" else {}
        g.pf_resample_blocks(st, nb, "multinomial", check=False, conditional=True, **kw)

    res = {k: [] for k in states}
    t = 1
    for rep in range(reps):
        for mode, st in states.items():
            for _ in range(warmup if rep == 0 else 2):
                call(mode, st, t % (T - 1) + 1); t += 1
            st.synchronize()
            k0 = st.kernel_time(K_SEARCH)
            t0 = time.perf_counter()
            for _ in range(steps):
                call(mode, st, t % (T - 1) + 1); t += 1
            st.synchronize()
            wall = (time.perf_counter() - t0) / steps * 1e6
            k1 = st.kernel_time(K_SEARCH)
            res[mode].append(((k1[0] - k0[0]) * 1e3 / max(1, k1[1] - k0[1]), wall))
    row = dict(case="resample", model=model_name, n_blocks=n_blocks, block_size=nb, steps=steps, reps=reps, note="wall = pinned update + resample")
    for mode, v in res.items():
        kern, wall = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        row[f"{mode}_kernel_us"] = float(np.median(kern)); row[f"{mode}_kernel_us_min"] = float(kern.min()); row[f"{mode}_kernel_us_max"] = float(kern.max())
        row[f"{mode}_wall_us"] = float(np.median(wall)); row[f"{mode}_wall_us_min"] = float(wall.min()); row[f"{mode}_wall_us_max"] = float(wall.max())
    row["ratio_kernel"] = row["ancestor_kernel_us"] / row["conditional_kernel_us"]
    row["ratio_wall"] = row["ancestor_wall_us"] / row["conditional_wall_us"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n")
    for st in states.values():
        st.close()


def renewal_case(out):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import block_ancestor_spec as asp                 # noqa: E402
    import block_conditional_spec as cs               # noqa: E402
    m, ys, ref, mu, Sigma = asp.invariance_setup(g.models)
    n, bs = cs.INV_B * cs.INV_N, cs.INV_N
    row = dict(case="renewal", model="lgssm2", n_blocks=cs.INV_B, block_size=bs, T=asp.INV_T)
    for mode in ("conditional", "ancestor"):
        obs = lambda t: np.tile(ys[t], (cs.INV_B, 1))
        st = g.pf_initialize_blocks(m, (1,), obs(0), n, bs, seed=cs.INV_SEED, history=asp.INV_T, reference=ref[:, 0])
        for t in range(1, asp.INV_T):
            kw = dict(reference=ref[:, t], observations=obs(t)) if mode == "ancestor" else {}
            g.pf_resample_blocks(st, bs, "multinomial", check=False, conditional=True, **kw)
            g.pf_update_blocks(st, (), (), obs(t), bs, reference=ref[:, t])
        traj = np.asarray(g.block_sample_trajectories(st, bs, 1)).reshape(cs.INV_B, asp.INV_T, 2)
        st.close()
        zm, zv = cs.invariance_bounds(traj, mu, Sigma, cs.INV_B)
        row[f"{mode}_x1_renewed"] = float(np.mean(np.any(traj[:, 0] != ref[:, 0], axis=1)))
        row[f"{mode}_max_z_mean"] = float(zm.max()); row[f"{mode}_max_z_var"] = float(zv.max())
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.devnull)
    ap.add_argument("--cases", default="resample,renewal")
    a = ap.parse_args()
    with open(a.out, "w") as out:
        if "resample" in a.cases:
            for name in MODELS:
                for n_blocks, nb in SHAPES:
                    resample_case(name, n_blocks, nb, a.steps, a.warmup, a.reps, out)
        if "renewal" in a.cases:
            renewal_case(out)


if __name__ == "__main__":
    main()
