"""Particle Gibbs with backward simulation per block in one launch (gpf.h gpf_sweep_blocks_backward) next to the loop of calls it stands for, alternating:
    loop       tools/block_sweep_bench.py's loop on a twin with history = T + 1, history_weights = True, then block_backward_trajectories(tw, bs, 1,
               return_indices=True)                                                                     the package's 2 T + 1 calls
    loop_c     the same calls through the C ABI with nothing read back but the path and its indices
    backward   pf_sweep_blocks_backward(st, ys, ref, bs, ancestor_sampling=..., ess_frac=0.5)           one call, all five outputs read back
    sweep      pf_sweep_blocks(st, ...): the ancestral draw, for scale
Before every timed call the state is initialised again (not timed); wall time around each call, ending in a synchronisation; median, minimum, maximum
over --reps after --warmup.  Kernel time (gpf_kernel_timing) from --kreps further calls: GPF_K_STEP + GPF_K_SEARCH -- the one kernel of the two calls;
of the loop its block resample and k_step only (its staging, snapshot / record, compose and backward kernels carry no timer).  same_results: two fresh
twins, the loop on one and the call on the other, agree bit for bit.  --renewal: the invariance experiment of tests/block_ancestor_spec.py (T = 8, 4096
blocks of 8), the share of blocks whose drawn x_1 is not the retained one, per draw and setting of ancestor_sampling.

    python tools/block_sweep_backward_bench.py [--reps 7] [--warmup 2] [--kreps 2] [--cases 0,1,2,3] [--renewal] [--out FILE.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from block_smooth_bench import data, model_of, stats
from block_sweep_bench import CASES, K_SEARCH, K_STEP, MULTINOMIAL, pd


def case(g, name, n_blocks, nb, T, anc, reps, warmup, kreps, out):
    m = model_of(g, name)
    ys = np.ascontiguousarray(data(g, m, n_blocks, T + 1))
    ref = np.ascontiguousarray(np.random.default_rng(5).standard_normal((n_blocks, T + 1, m.dim)))
    y0, r0, yrun, rrun = (np.ascontiguousarray(x) for x in (ys[:, 0], ref[:, 0], ys[:, 1:], ref[:, 1:]))
    ysteps, rsteps = [np.ascontiguousarray(yrun[:, t]) for t in range(T)], [np.ascontiguousarray(rrun[:, t]) for t in range(T)]
    n, n_obs, d = n_blocks * nb, y0.shape[1], m.dim
    make = lambda **kw: g.pf_initialize_blocks(m, (1,), y0, n, nb, seed=3, reference=r0, **kw)
    st, tw = make(), make(history=T + 1, history_weights=True)
    L = st._L
    path, idx = np.empty((n_blocks, 1, T + 1, d)), np.empty((n_blocks, 1, T + 1), np.int64)

    def reset(s):
        s._check(L.gpf_initialize_blocks_ref(s._h, pd(y0), n_obs, nb, pd(r0), d))
        s.synchronize()

    def loop(s=tw):
        for t in range(T):
            kw = dict(reference=rsteps[t], observations=ysteps[t]) if anc else {}
            g.pf_resample_blocks(s, nb, "multinomial", conditional=True, ess_frac=0.5, check=False, **kw)
            g.pf_update_blocks(s, (), (), ysteps[t], nb, reference=rsteps[t])
        r = g.block_backward_trajectories(s, nb, 1, return_indices=True)
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
        tw._check(L.gpf_block_backward_sample(h, nb, 1, 1, T + 1, pd(path), idx.ctypes.data_as(C.POINTER(C.c_int64))))
        tw.synchronize()

    backward = lambda s=st: g.pf_sweep_blocks_backward(s, yrun, rrun, nb, ancestor_sampling=anc, ess_frac=0.5)
    sweep = lambda s=st: g.pf_sweep_blocks(s, yrun, rrun, nb, ancestor_sampling=anc, ess_frac=0.5)
    calls = {"loop": (loop, tw), "loop_c": (loop_c, tw), "backward": (backward, st), "sweep": (sweep, st)}
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
    p, q = make(history=T + 1, history_weights=True), make()
    (tp, ti), r = loop(p), backward(q)
    same = bool(np.array_equal(tp[:, 0], r.path) and np.array_equal(ti[:, 0], r.indices) and np.array_equal(p.log_weights, q.log_weights)
                and np.array_equal(p.traces, q.traces) and np.array_equal(p.parents, q.parents) and np.array_equal(g.block_stats(p, nb)[1], r.lml[:, -1]))
    p.close(); q.close()
    row = dict(model=name, n_blocks=n_blocks, block_size=nb, T=T, ancestor_sampling=anc, ess_frac=0.5)
    for c in calls:
        row[c] = dict(stats(times[c]), **kernel[c])
    row["same_results"] = same
    row["backward_median_below_loop_c_min"] = bool(row["backward"]["median_ms"] < row["loop_c"]["min_ms"])
    print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()
    st.close(); tw.close()


def renewal(g, out):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import block_ancestor_spec as asp
    import block_conditional_spec as cs
    m, ys, ref, _, _ = asp.invariance_setup(g.models)
    for anc in (True, False):
        row = dict(experiment="x1 renewed", blocks=cs.INV_B, block_size=cs.INV_N, T=ys.shape[0] - 1, ancestor_sampling=anc)
        for name, f in (("ancestral", g.pf_sweep_blocks), ("backward", g.pf_sweep_blocks_backward)):
            st = g.pf_initialize_blocks(m, (1,), np.tile(ys[0], (cs.INV_B, 1)), cs.INV_B * cs.INV_N, cs.INV_N, seed=cs.INV_SEED, reference=ref[:, 0])
            r = f(st, np.ascontiguousarray(ys[1:]), np.ascontiguousarray(ref[:, 1:]), cs.INV_N, ancestor_sampling=anc, ess_frac=None)
            row[name] = float((r.path[:, 0] != ref[:, 0]).any(axis=1).mean())
            st.close()
        print(json.dumps(row), flush=True); out.write(json.dumps(row) + "\n"); out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kreps", type=int, default=2)
    ap.add_argument("--cases", default="0,1,2,3")
    ap.add_argument("--renewal", action="store_true")
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpf_amd as g
    with open(a.out, "a") as out:
        if a.renewal:
            renewal(g, out)
        for k in (int(c) for c in a.cases.split(",") if c != ""):
            case(g, *CASES[k], a.reps, a.warmup, a.kreps, out)


if __name__ == "__main__":
    main()
