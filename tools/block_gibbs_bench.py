"""The particle Gibbs chain per block in one launch (gpf.h gpf_gibbs_blocks) next to the loops it stands for, alternating, K sweeps each:
    loop       the package's calls, a new handle per sweep: pf_initialize_blocks(..., seed=seeds[k], reference=path[:, 0]), pf_sweep_blocks[_backward],
               the path to the host and back as the next reference
    loop_c     the same device calls through the C ABI on ONE twin handle that is kept: gpf_initialize_blocks_ref, gpf_sweep_blocks[_backward] with only
               the path (backward: and its indices, which that call needs) read back and given to the next sweep.  The twin keeps the seed it was made
               with -- the C ABI has no call that changes it, so the sweeps repeat their noise: the same work, not the same numbers.  The stricter yardstick
    call       pf_gibbs_blocks(state, ys, ref, bs, seeds, backward=...)      one call; K paths and K x n_blocks estimates read back
The loop's kernels are the parent commit's, instruction for instruction (tools/isa_diff.py).  Wall time around each form, ending in a synchronisation;
median, minimum, maximum over --reps after --warmup.  Kernel time (gpf_kernel_timing, GPF_K_STEP) from --kreps further runs, each
reported: the call's one launch; of loop_c K x (k_init + k_block_sweep) -- the spread of the loop's sum is max - min over its --kreps values.
same_results: the call and the package loop agree bit for bit on paths and estimates.

    python tools/block_gibbs_bench.py [--reps 5] [--warmup 1] [--kreps 5] [--cases 0,1,2,3] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from block_smooth_bench import data, model_of, stats

CASES = [("lgssm2", 10_000, 100, 100, False), ("lgssm2", 10_000, 100, 100, True),      # (model, n_blocks, block_size, T, backward)
         ("lgssm2", 64, 2048, 32, False), ("lgssm2", 64, 2048, 32, True)]
K_STEP, SWEEPS = 0, 10


def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def case(g, name, B, bs, T, backward, reps, warmup, kreps, out):
    m = model_of(g, name)
    n, d = B * bs, m.dim
    ys = np.ascontiguousarray(data(g, m, B, T))
    ref0 = np.ascontiguousarray(np.random.default_rng(5).standard_normal((B, T, d)))
    y0, yrun, n_obs = np.ascontiguousarray(ys[:, 0]), np.ascontiguousarray(ys[:, 1:]), ys.shape[2]
    seeds = [1009 + 7 * k for k in range(SWEEPS)]
    st = g.pf_initialize_blocks(m, (1,), y0, n, bs, seed=3)
    tw = g.pf_initialize_blocks(m, (1,), y0, n, bs, seed=seeds[0], reference=ref0[:, 0])
    L = st._L
    sweep = g.pf_sweep_blocks_backward if backward else g.pf_sweep_blocks
    sweep_c = L.gpf_sweep_blocks_backward if backward else L.gpf_sweep_blocks
    path, idx = np.empty((B, T, d)), np.zeros((B, T) if backward else B, np.int64)

    def loop():
        ref, kept, lml = ref0, [], []
        for s in seeds:
            t = g.pf_initialize_blocks(m, (), y0, n, bs, seed=s, reference=ref[:, 0])
            sw = sweep(t, yrun, ref[:, 1:], bs, ancestor_sampling=True, ess_frac=0.5)
            ref = sw.path; kept.append(sw.path); lml.append(sw.lml[:, -1])
            t.close()
        return np.stack(kept, axis=1), np.stack(lml, axis=1)

    def loop_c():
        ref = ref0
        for _ in seeds:
            r0, rrun = np.ascontiguousarray(ref[:, 0]), np.ascontiguousarray(ref[:, 1:])
            tw._check(L.gpf_initialize_blocks_ref(tw._h, pd(y0), n_obs, bs, pd(r0), d))
            tw._check(sweep_c(tw._h, pd(yrun), n_obs, T - 1, 0, pd(rrun), d, bs, 1, 0.5, pd(path), idx.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, None))
            ref = path
        tw.synchronize()

    call = lambda: g.pf_gibbs_blocks(st, ys, ref0, bs, seeds, ancestor_sampling=True, backward=backward, ess_frac=0.5)
    calls = {"loop": (loop, None), "loop_c": (loop_c, tw), "call": (call, st)}
    times = {c: [] for c in calls}
    for r in range(warmup + reps):                                            # (alternating: the three see the same machine)
        for c, (f, _) in calls.items():
            t0 = time.perf_counter()
            f()
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[c].append(dt)
    row = dict(model=name, n_blocks=B, block_size=bs, T=T, sweeps=SWEEPS, backward=backward, ancestor_sampling=True, ess_frac=0.5)
    for c, (f, hk) in calls.items():
        row[c] = stats(times[c])
        if hk is not None:
            ks = []
            for _ in range(kreps):
                hk.kernel_timing(K_STEP, True)
                f()
                ms, launches = hk.kernel_time(K_STEP)
                hk.kernel_timing(K_STEP, False)
                ks.append(ms)
            row[c].update(kernel_ms=[float(k) for k in ks], kernel_median_ms=float(np.median(ks)), kernel_spread_ms=float(max(ks) - min(ks)),
                          launches=int(launches))
    (lp, ll), r = loop(), call()
    row["same_results"] = bool(np.array_equal(lp, r.paths) and np.array_equal(ll, r.lml))
    row["call_over_loop"] = row["call"]["median_ms"] / row["loop"]["median_ms"]
    row["call_over_loop_c"] = row["call"]["median_ms"] / row["loop_c"]["median_ms"]
    row["kernel_excess_ms"] = row["call"]["kernel_median_ms"] - row["loop_c"]["kernel_median_ms"]
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()
    st.close(); tw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kreps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(str(k) for k in range(len(CASES))))
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "a") as out:
        for k in (int(c) for c in a.cases.split(",")):
            case(g, *CASES[k], a.reps, a.warmup, a.kreps, out)


if __name__ == "__main__":
    main()
