"""One conditional SMC sweep per block in one launch (gpf.h gpf_sweep_blocks) next to the loop of calls it stands for, alternating:
    loop       for t: pf_resample_blocks(tw, bs, "multinomial", conditional=True, ess_frac=0.5, check=False[, reference=ref[:, t], observations=ys[:, t]]);
               pf_update_blocks(tw, (), (), ys[:, t], bs, reference=ref[:, t]);  then block_sample_trajectories(tw, bs, 1)        the package's calls
    loop_c     the same 2 T + 1 calls through the C ABI with invalid = n_resampled = NULL and the path left on the device side of the call's copy (the
               trajectory call copies its one output, as it must): nothing else is read back, the host runs ahead of the device.  The stricter yardstick
    sweep      pf_sweep_blocks(st, ys, ref, bs, ancestor_sampling=..., ess_frac=0.5)                 one call, all five outputs read back
The loop needs the block-wise trajectory store and the sweep refuses one, so the two forms run on twins: `tw` with history = T + 1, `st` without.  Before
every timed call the state is initialised again from the same observations, reference and seed (not timed).  After the timing two fresh twins run
the loop and the one call and their paths, indices, rows, log-weights and parents are compared bit for bit (same_results).  Wall time around each
call, ending in a synchronisation; median, minimum, maximum over --reps after --warmup.  Kernel time (gpf_kernel_timing) from --kreps further calls with
the timers on: the loop's is the block resample (GPF_K_SEARCH) + k_step (GPF_K_STEP), the sweep's k_block_sweep (booked under GPF_K_STEP); the loop's
staging, snapshot and trajectory kernels are not in it.

    python tools/block_sweep_bench.py [--reps 7] [--warmup 2] [--kreps 2] [--cases 0,1,2,3] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from block_smooth_bench import data, model_of, stats

# (model, n_blocks, block_size, T, ancestor sampling)
CASES = [("lgssm2", 10_000, 100, 100, True), ("lgssm2", 10_000, 100, 100, False), ("lgssm2", 64, 2048, 32, True), ("lgssm2", 64, 2048, 32, False)]
K_STEP, K_SEARCH = 0, 3
MULTINOMIAL = 0


def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def case(g, name, n_blocks, nb, T, anc, reps, warmup, kreps, out):
    m = model_of(g, name)
    ys = np.ascontiguousarray(data(g, m, n_blocks, T + 1))
    ref = np.ascontiguousarray(np.random.default_rng(5).standard_normal((n_blocks, T + 1, m.dim)))
    y0, r0, yrun, rrun = (np.ascontiguousarray(x) for x in (ys[:, 0], ref[:, 0], ys[:, 1:], ref[:, 1:]))
    ysteps, rsteps = [np.ascontiguousarray(yrun[:, t]) for t in range(T)], [np.ascontiguousarray(rrun[:, t]) for t in range(T)]
    n, n_obs, d = n_blocks * nb, y0.shape[1], m.dim
    make = lambda **kw: g.pf_initialize_blocks(m, (1,), y0, n, nb, seed=3, reference=r0, **kw)
    st, tw = make(), make(history=T + 1)
    L = st._L
    path = np.empty((n_blocks, 1, T + 1, d))

    def reset(s):
        s._check(L.gpf_initialize_blocks_ref(s._h, pd(y0), n_obs, nb, pd(r0), d))
        s.synchronize()

    def loop(s=tw):
        for t in range(T):
            kw = dict(reference=rsteps[t], observations=ysteps[t]) if anc else {}
            g.pf_resample_blocks(s, nb, "multinomial", conditional=True, ess_frac=0.5, check=False, **kw)
            g.pf_update_blocks(s, (), (), ysteps[t], nb, reference=rsteps[t])
        r = g.block_sample_trajectories(s, nb, 1, return_indices=True)
        s.synchronize()
        return r

    def loop_c():
        h = tw._h
        for t in range(T):
            if anc:
                tw._check(L.gpf_resample_blocks_ancestor(h, MULTINOMIAL, nb, 0.5, 0, pd(ysteps[t]), n_obs, pd(rsteps[t]), d, None, None))
            else:
                tw._check(L.gpf_resample_blocks_conditional(h, MULTINOMIAL, nb, 0.5, 0, None, None))
            tw._check(L.gpf_update_blocks_ref(h, pd(ysteps[t]), n_obs, nb, pd(rsteps[t]), d))
        tw._check(L.gpf_block_sample_trajectories(h, nb, 1, 1, T + 1, pd(path), None))
        tw.synchronize()

    sweep = lambda s=st: g.pf_sweep_blocks(s, yrun, rrun, nb, ancestor_sampling=anc, ess_frac=0.5)
    calls = {"loop": (loop, tw), "loop_c": (loop_c, tw), "sweep": (sweep, st)}
    times = {c: [] for c in calls}
    for r in range(warmup + reps):
        for c, (f, s) in calls.items():
            reset(s)
            t0 = time.perf_counter()
            f()
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[c].append(dt)
    kernel = {}
    for c, (f, s) in calls.items():
        for _ in range(kreps):
            reset(s)                                                           # (before the timers go on: the initialising kernel is booked under GPF_K_STEP too)
            s.kernel_timing(K_STEP, True); s.kernel_timing(K_SEARCH, True)
            f()
            (ms_a, n_a), (ms_b, n_b) = s.kernel_time(K_STEP), s.kernel_time(K_SEARCH)
            s.kernel_timing(K_STEP, False); s.kernel_timing(K_SEARCH, False)
            kernel.setdefault(c, []).append((ms_a + ms_b, n_a + n_b))
        kernel[c] = dict(kernel_ms_per_call=float(np.median([k[0] for k in kernel[c]])), launches_per_call=int(kernel[c][0][1]))
    # the same results: two fresh twins at the same epoch, the loop on one, the call on the other
    p, q = make(history=T + 1), make()
    (tp, ti), r = loop(p), sweep(q)
    same = bool(np.array_equal(tp[:, 0], r.path) and np.array_equal(ti[:, 0], r.index) and np.array_equal(p.log_weights, q.log_weights)
                and np.array_equal(p.traces, q.traces) and np.array_equal(p.parents, q.parents) and np.array_equal(g.block_stats(p, nb)[1], r.lml[:, -1]))
    p.close(); q.close()
    row = dict(model=name, n_blocks=n_blocks, block_size=nb, T=T, ancestor_sampling=anc, ess_frac=0.5)
    for c in calls:
        row[c] = dict(stats(times[c]), **kernel[c])
    row["same_results"] = same
    row["resampled_share"] = float(r.resampled.mean())
    row["sweep_over_loop"] = row["sweep"]["median_ms"] / row["loop"]["median_ms"]
    row["sweep_median_below_loop_c_min"] = bool(row["sweep"]["median_ms"] < row["loop_c"]["min_ms"])
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()
    st.close(); tw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kreps", type=int, default=2)
    ap.add_argument("--cases", default="0,1,2,3")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "a") as out:
        for k in (int(c) for c in a.cases.split(",")):
            case(g, *CASES[k], a.reps, a.warmup, a.kreps, out)


if __name__ == "__main__":
    main()
