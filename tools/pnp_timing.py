"""Per-call time of the device PnP RANSAC (drfe_pnp_ransac_batch) next to the host entry (drfe_pnp_ransac_host, one CPU thread) on
the same planted scenes (tests/pnp_numpy.py: 30 % outliers, SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), tail 5): 1, 4, 16, 64
and 512 solvers of 30, 100 and 1 000 correspondences.  The clock is around the C entry alone (the records are packed once, outside
it); the device call returns with the table in host memory, so wall time is its cost, staging and both copies included.  Every
timed shape is called once before it is timed, and a configuration is repeated until at least --seconds have been timed.  Device ==
host is checked.  Prints one JSON line per configuration and writes them to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, seconds, max_reps):
    fn()
    ts = []
    while (sum(ts) < seconds and len(ts) < max_reps) or len(ts) < 3:
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts)), len(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--max-reps", type=int, default=200)
    ap.add_argument("--solvers", type=int, nargs="*", default=[1, 4, 16, 64, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_timing.jsonl"))
    args = ap.parse_args()
    import pnp_numpy as pn
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows = []
    try:
        for N in (30, 100, 1000):
            rng = np.random.default_rng(N)
            pool = [pn.random_solver(rng, N, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991, tail=5, seed=i + 1,
                                     outlier_frac=0.3, noise=0.3)[0] for i in range(max(args.solvers))]
            for n in args.solvers:
                problems = pn.pack(pool[:n])
                Pd, od, rd, keep_d = lib._pnp_pack(problems)
                Ph, oh, rh, keep_h = lib._pnp_pack(problems)

                def dev():
                    if L.drfe_pnp_ransac_batch(ctx.h, C.byref(Pd), C.byref(od), None) != 0:
                        raise RuntimeError("drfe_pnp_ransac_batch failed")

                def host():
                    if L.drfe_pnp_ransac_host(C.byref(Ph), C.byref(oh)) != 0:
                        raise RuntimeError("drfe_pnp_ransac_host failed")
                dm, dmin, dmax, dreps = timed(dev, args.seconds, args.max_reps)
                hm, hmin, hmax, hreps = timed(host, args.seconds, args.max_reps)
                assert not pn.tables_equal(rd, rh), (N, n)
                row = dict(solvers=n, correspondences=N, hypotheses=int(rh["hypotheses"].sum()), refines=int(rh["refines"].sum()),
                           device_ms=round(dm, 4), device_min_ms=round(dmin, 4), device_max_ms=round(dmax, 4), device_reps=dreps,
                           host_ms=round(hm, 4), host_min_ms=round(hmin, 4), host_max_ms=round(hmax, 4), host_reps=hreps,
                           speedup=round(hm / dm, 2))
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
