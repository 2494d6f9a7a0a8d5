"""Wall time of pf_coalesce / pf_introduce on one GPU (gpf.h gpf_coalesce, gpf_introduce).

Both calls return after a stream synchronisation, so the host wall clock around one call is what a user waits for: the kernels, the
one host read of the group count (coalesce), the reallocation of the particle buffers.  Every repetition starts from the same state
(checkpoint / restore outside the timed region).  Prints one JSON line per case.

    python tools/coalesce_introduce_bench.py [--n 1000000] [--reps 20] [--out file.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, setup=None):
    ts = []
    for _ in range(reps + 2):                     # two warm-up calls
        if setup:
            setup()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts = ts[2:]
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10 ** 6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gpf_amd as g
    N, R = a.n, a.reps
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def coalesce_case(name, st, by, n_fixed):
        blob = st.checkpoint()
        groups = {}
        fresh = {"st": st}

        def setup2():
            fresh["st"] = None
            s = g.DeviceParticleFilterState(st.model, n_fixed, seed=st.seed, keep_prev=st.keep_prev)
            s.restore(blob)
            fresh["st"] = s

        def run2():
            g.pf_coalesce(fresh["st"], by=by)
            groups["n"] = fresh["st"].n_particles

        r = timed(run2, R, setup2)
        emit(dict(case=name, op="pf_coalesce", n_old=n_fixed, n_new=groups["n"], distinct_frac=groups["n"] / n_fixed, **r))

    ys = g.models.simulate(g.models.lgssm2(), 4)
    m = g.models.lgssm2()
    st = g.pf_initialize(m, (1,), ys[0], N, seed=7)
    g.pf_update(st, (2,), (None,), ys[1])
    g.pf_resample(st, "multinomial", check=False)
    g.pf_update(st, (3,), (None,), ys[2])
    g.pf_resample(st, "multinomial", check=False)
    g.get_ess(st)
    coalesce_case("lgssm2_after_multinomial_resample", st, None, N)

    om = g.models.object_motion()
    yo = g.models.simulate(om, 3)
    so = g.pf_initialize(om, (1,), yo[0], N, seed=7)
    g.pf_update(so, (2,), (None,), yo[1])
    rows = so.traces
    col = [c for c in range(2) if len(set(rows[:4096, c].tolist())) <= 2][0]
    coalesce_case("object_motion_by_moving", so, col, N)

    sd = g.pf_initialize(m, (1,), ys[0], N, seed=7)
    coalesce_case("lgssm2_all_distinct", sd, None, N)

    # pf_introduce of N particles into a small filter, t = 1 and t = 100, against pf_initialize + (t - 1) pf_update of N particles
    T = 100
    yl = g.models.simulate(m, T)
    for t in (1, T):
        base = g.pf_initialize(m, (1,), yl[0], 1000, seed=3)
        blob = base.checkpoint()
        holder = {}

        def setup():
            holder["st"] = None
            s = g.DeviceParticleFilterState(m, 1000, seed=3)
            s.restore(blob)
            holder["st"] = s

        def run():
            g.pf_introduce(holder["st"], yl[:t], N)

        r = timed(run, max(3, R // 4) if t > 1 else R, setup)
        emit(dict(case=f"lgssm2_introduce_t{t}", op="pf_introduce", n_old=1000, n_add=N, t=t, **r))

        def setup_path():                          # (handle creation outside the timed region, as for pf_introduce)
            holder["p"] = None
            holder["p"] = g.DeviceParticleFilterState(m, N, seed=3)

        def run_path():
            s = holder["p"]
            y0 = np.ascontiguousarray(yl[0])
            s._check(s._L.gpf_initialize(s._h, y0.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), y0.size))
            for e in range(1, t):
                g.pf_update(s, (e + 1,), (None,), yl[e])
            s.synchronize()

        r = timed(run_path, max(3, R // 4) if t > 1 else R, setup_path)
        emit(dict(case=f"lgssm2_init_plus_{t - 1}_updates", op="pf_initialize + pf_update x (t-1)", n=N, t=t, **r))

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
