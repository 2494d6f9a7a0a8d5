"""The particle-marginal MH move per block in one launch (gpf.h gpf_pmmh_blocks) next to the loop of calls it stands for, at acceptance shares 0, 1/4 and 1:
    loop       the package's calls: twin = pf_initialize_blocks(..., seed=s, params=proposed) (a second handle), pf_run_blocks(twin, ys[:, 1:]),
               block_stats of both, the accept test on the host, then get_traces / state.traces = / state.log_weights = / set_block_params with the
               accepted blocks merged in -- every row of every block crosses the bus twice
    loop_c     that loop's device calls alone, through the C ABI on a twin handle that is kept, with nothing read back: gpf_set_block_params,
               gpf_initialize_blocks, gpf_run_blocks with NULL outputs, one synchronisation.  No accept test and no replacement: the stricter yardstick
    call       pf_pmmh_blocks(state, ys, proposed, thr, bs, method, seed=s)        one call, two outputs of n_blocks words read back
The loop's kernels are the parent commit's, instruction for instruction (tools/isa_diff.py).  The thresholds come from a pilot call's estimates (-inf,
their upper quartile, +inf); the seed is fixed, so the share is exact.  Wall time around each call, ending in a synchronisation; median, minimum,
maximum over --reps after --warmup.  Kernel time (gpf_kernel_timing, GPF_K_STEP): the call's one launch; the twin's k_init + k_block_series.

    python tools/block_pmmh_bench.py [--reps 5] [--warmup 1] [--cases 0,1] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from block_smooth_bench import data, model_of, stats

CASES = [("lgssm2", 10_000, 100, 100, "residual"), ("lgssm2", 64, 2048, 32, "residual")]     # (model, n_blocks, block_size, T, method)
K_STEP = 0
INF = float("inf")


def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def case(g, name, B, bs, T, method, reps, warmup, out):
    m = model_of(g, name)
    n, seed = B * bs, 1009
    ys = np.ascontiguousarray(data(g, m, B, T))
    y0, yrun = np.ascontiguousarray(ys[:, 0]), np.ascontiguousarray(ys[:, 1:])
    rows = g.block_params_rows(m, [m] * B, n, bs)
    prop = rows.copy(); prop[:, 4] *= 1.0 + 0.05 * np.sin(np.arange(B))       # (lgssm2: sq; the default proposal reads no constant derived from it)
    st = g.pf_initialize_blocks(m, (1,), y0, n, bs, seed=3, params=rows)
    g.pf_run_blocks(st, yrun, bs, method)
    tw = g.pf_initialize_blocks(m, (1,), y0, n, bs, seed=seed, params=prop)
    L, mid, n_obs = st._L, g.api.RESAMPLE_METHODS[method], y0.shape[1]
    pilot = g.pf_pmmh_blocks(st, ys, prop, np.full(B, INF), bs, method, seed=seed).lml

    def loop(thr):
        twin = g.pf_initialize_blocks(m, (), y0, n, bs, seed=seed, params=prop)
        g.pf_run_blocks(twin, yrun, bs, method)
        Lp, Ls = g.block_stats(twin, bs)[1], g.block_stats(st, bs)[1]
        acc = Lp > thr
        sel = np.repeat(acc, bs)
        r, w = g.get_traces(st), st.log_weights
        r[sel] = g.get_traces(twin)[sel]
        w[sel] = (twin.log_weights + np.repeat(Ls - Lp, bs))[sel]
        p = g.get_block_params(st); p[acc] = prop[acc]
        st.traces, st.log_weights = r, w
        g.set_block_params(st, p, bs)
        twin.close()
        st.synchronize()

    def loop_c(thr):
        tw._check(L.gpf_set_block_params(tw._h, pd(prop), prop.shape[1], bs))
        tw._check(L.gpf_initialize_blocks(tw._h, pd(y0), n_obs, bs))
        tw._check(L.gpf_run_blocks(tw._h, pd(yrun), n_obs, T - 1, 0, bs, mid, 1, 0.5, None, None, None, None))
        tw.synchronize()

    def call(thr):
        return g.pf_pmmh_blocks(st, ys, prop, thr, bs, method, seed=seed)

    for share, thr in ((0.0, np.full(B, INF)), (0.25, np.full(B, np.quantile(pilot, 0.75))), (1.0, np.full(B, -INF))):
        row = dict(model=name, n_blocks=B, block_size=bs, T=T, method=method, share_asked=share)
        calls = (("loop", loop, None), ("loop_c", loop_c, tw), ("call", call, st))
        times = {c: [] for c, _, _ in calls}
        for r in range(warmup + reps):                                        # (alternating: the three see the same machine)
            for c, f, _ in calls:
                t0 = time.perf_counter()
                res = f(thr)
                dt = time.perf_counter() - t0
                if r >= warmup:
                    times[c].append(dt)
        row["share"] = float(res.accepted.mean())
        for c, f, hk in calls:
            row[c] = stats(times[c])
            if hk is not None:
                hk.kernel_timing(K_STEP, True)
                f(thr)
                row[c]["kernel_ms"], row[c]["launches"] = hk.kernel_time(K_STEP)
                hk.kernel_timing(K_STEP, False)
        row["call_over_loop"] = row["call"]["median_ms"] / row["loop"]["median_ms"]
        row["call_over_loop_c"] = row["call"]["median_ms"] / row["loop_c"]["median_ms"]
        print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()
    st.close(); tw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default=",".join(str(k) for k in range(len(CASES))))
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "a") as out:
        for k in (int(c) for c in a.cases.split(",")):
            case(g, *CASES[k], a.reps, a.warmup, out)


if __name__ == "__main__":
    main()
