"""Conditional SMC for block-wise filters on the device: what the pinned step and the conditional resample cost next to their plain twins, and
what the feature saves against the sequence a caller had to assemble before it.

(a) Pinned step against plain step, conditional resample against plain multinomial resample: two states of one seed side by side, timed
    alternately (plain, pinned, plain, ...) in one process; k_step / block-resample dispatch times from gpf_kernel_timing (the kernels' own begin /
    end stamps) and us per call on the host clock with one synchronisation at the end.  The plain kernels are instruction for instruction those of
    the commit before this feature (tools/isa_diff.py), so "plain" is the parent's kernel.  The run-to-run spread of the plain kernel -- the
    yardstick for the pinned one -- is the range of its per-round means.
(b) The loop: conditional resample + pinned update in two calls, against the hand-assembled form: plain resample, plain update, then slot 0 of every
    block patched through the host (traces / log_weights read back, rows and weights written) -- which cannot even restore slot 0's incoming
    weight without one more read before the update.

    python tools/block_conditional_bench.py [--steps 100] [--warmup 10] [--reps 5] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpf_amd as g                                   # noqa: E402

K_STEP, K_SEARCH = g._lib.K_STEP, g._lib.K_SEARCH     # (the block resample is timed under the search slot)
SHAPES = ((10_000, 100), (8, 100_000))
RES_SHAPES = ((10_000, 100), (1_000, 1024))           # (the conditional resample stops at 2048 particles per block: 8 x 10^5 is refused by design)


def data(m, n_blocks, T, seed=1):
    base = np.asarray(g.models.simulate(m, T))
    rng = np.random.default_rng(seed)
    ys = base[None, :, :] + 0.2 * rng.standard_normal((n_blocks,) + base.shape)
    ref = rng.standard_normal((n_blocks, T, m.dim))
    if m.name == "object_motion":
        ref[..., 0] = rng.integers(0, 2, (n_blocks, T))
    return ys, ref


def timed_rounds(states, call, kernel, steps, warmup, reps, T):
    """alternate the states; per state the per-round (kernel us per launch, wall us per call)"""
    res = {k: [] for k in states}
    t = 1
    for rep in range(reps):
        for mode, st in states.items():
            for _ in range(warmup if rep == 0 else 2):
                call(mode, st, t % (T - 1) + 1); t += 1
            st.synchronize()
            k0 = st.kernel_time(kernel)
            t0 = time.perf_counter()
            for _ in range(steps):
                call(mode, st, t % (T - 1) + 1); t += 1
            st.synchronize()
            wall = (time.perf_counter() - t0) / steps * 1e6
            k1 = st.kernel_time(kernel)
            res[mode].append(((k1[0] - k0[0]) * 1e3 / max(1, k1[1] - k0[1]), wall))
    return res


def summarise(case, res, extra):
    row = dict(case=case, **extra)
    for mode, v in res.items():
        kern, wall = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        row[f"{mode}_kernel_us"] = float(np.median(kern)); row[f"{mode}_kernel_us_min"] = float(kern.min()); row[f"{mode}_kernel_us_max"] = float(kern.max())
        row[f"{mode}_wall_us"] = float(np.median(wall)); row[f"{mode}_wall_us_min"] = float(wall.min()); row[f"{mode}_wall_us_max"] = float(wall.max())
    return row


def step_case(n_blocks, nb, steps, warmup, reps, out, model_name="object_motion"):
    m = g.models.by_name(model_name)
    T = 32
    ys, ref = data(m, n_blocks, T)
    states = {}
    for mode in ("plain", "pinned"):
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, keep_prev=True)
        st.kernel_timing(K_STEP, True)
        states[mode] = st

    def call(mode, st, t):
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb, reference=ref[:, t] if mode == "pinned" else None)

    row = summarise("step", timed_rounds(states, call, K_STEP, steps, warmup, reps, T), dict(model=model_name, n_blocks=n_blocks, block_size=nb, steps=steps, reps=reps))
    row["ratio_kernel"] = row["pinned_kernel_us"] / row["plain_kernel_us"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n")
    for st in states.values():
        st.close()


def resample_case(n_blocks, nb, steps, warmup, reps, out, model_name="object_motion"):
    m = g.models.by_name(model_name)
    T = 32
    ys, _ = data(m, n_blocks, T)
    states = {}
    for mode in ("plain", "conditional"):
        st = g.pf_initialize_blocks(m, (1,), ys[:, 0], n_blocks * nb, nb, seed=3, keep_prev=True)
        st.kernel_timing(K_SEARCH, True)
        states[mode] = st

    def call(mode, st, t):                                 # (an update in between, so that every resample meets fresh weights)
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
        g.pf_resample_blocks(st, nb, "multinomial", check=False, conditional=mode == "conditional")

    row = summarise("resample", timed_rounds(states, call, K_SEARCH, steps, warmup, reps, T), dict(model=model_name, n_blocks=n_blocks, block_size=nb, steps=steps, reps=reps,
                                                                                                    note="wall = update + resample"))
    row["ratio_kernel"] = row["conditional_kernel_us"] / row["plain_kernel_us"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n")
    for st in states.values():
        st.close()


def loop_case(n_blocks, nb, steps, warmup, reps, out, model_name="object_motion"):
    m = g.models.by_name(model_name)
    T = 32
    ys, ref = data(m, n_blocks, T)
    n = n_blocks * nb
    b0 = np.arange(0, n, nb)
    states = {mode: g.pf_initialize_blocks(m, (1,), ys[:, 0], n, nb, seed=3, keep_prev=True, reference=ref[:, 0]) for mode in ("library", "by_hand")}
    for st in states.values():
        st.kernel_timing(K_STEP, True)
    P = np.ascontiguousarray(m.params, np.float64)

    def loglik(x, ob):                                     # object_motion's observation density on the host (the hand-assembled form needs the model twice)
        z = (ob[:, 0] - x[:, 1]) * P[3]
        return -0.5 * z * z - P[4]

    def call(mode, st, t):
        if mode == "library":
            g.pf_resample_blocks(st, nb, "multinomial", check=False, conditional=True)
            g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb, reference=ref[:, t])
            return
        kept = st.traces[b0]                               # slot 0 before the resample moves it
        g.pf_resample_blocks(st, nb, "multinomial", check=False)
        rows = st.traces; rows[b0] = kept; st.traces = rows
        lw_in = st.log_weights[b0]                         # slot 0's incoming weight: gone after the update
        g.pf_update_blocks(st, (t + 1,), (None,), ys[:, t], nb)
        rows, lw = st.traces, st.log_weights
        new = np.zeros((b0.size, rows.shape[1])); new[:, :m.dim] = ref[:, t]; new[:, m.dim:2 * m.dim] = kept[:, :m.dim]
        rows[b0] = new; lw[b0] = lw_in + loglik(new, ys[:, t])
        st.traces = rows; st.log_weights = lw

    row = summarise("loop", timed_rounds(states, call, K_STEP, steps, warmup, reps, T), dict(model=model_name, n_blocks=n_blocks, block_size=nb, steps=steps, reps=reps))
    row["speedup_wall"] = row["by_hand_wall_us"] / row["library_wall_us"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n")
    for st in states.values():
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.devnull)
    ap.add_argument("--cases", default="step,resample,loop")
    a = ap.parse_args()
    with open(a.out, "w") as out:
        for n_blocks, nb in SHAPES if "step" in a.cases else ():
            step_case(n_blocks, nb, a.steps, a.warmup, a.reps, out)
        for n_blocks, nb in RES_SHAPES if "resample" in a.cases else ():
            resample_case(n_blocks, nb, a.steps, a.warmup, a.reps, out)
        if "loop" in a.cases:
            loop_case(SHAPES[0][0], SHAPES[0][1], max(10, a.steps // 5), a.warmup, a.reps, out)


if __name__ == "__main__":
    main()
