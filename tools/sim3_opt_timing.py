"""Per-call time of the device OptimizeSim3 (drfe_sim3_opt_batch) next to its host entry (drfe_sim3_opt_host, one CPU thread) on
the same planted fixed-scale problems (tests/sim3_opt_numpy.py: 20 % gross outliers): 1, 2, 4, 8, 16, 64 and 512 problems of 50,
150 and 500 matches.
The clock is around the C entry alone (the records are packed once, outside it); the device call returns with the outputs in host
memory, so wall time is its cost, staging and both copies included.  Every timed shape is called once before it is timed; the two
entries are then called in turn until each has at least --seconds (default 1) of timed calls and at least five; the row holds the
median and the spread (max - min) of both entries.  Device == host is checked at every size (--keep-going records the verdict and
goes on).  The reference's own function cannot be built next to this library, and the entry is new, so the table compares this
library's two entries only.  Prints one JSON line per configuration and writes them to --out (profiles/sim3_opt_timing.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--problems", type=int, nargs="*", default=[1, 2, 4, 8, 16, 64, 512])
    ap.add_argument("--matches", type=int, nargs="*", default=[50, 150, 500])
    ap.add_argument("--keep-going", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_opt_timing.jsonl"))
    args = ap.parse_args()
    import sim3_opt_numpy as sn
    from dr_slam_amd import lib
    from pose_opt_timing import timed_pair
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows = []
    try:
        for N in args.matches:
            rng = np.random.default_rng(N)
            pool = [sn.problem(rng, N, outlier_frac=0.2) for _ in range(max(args.problems))]
            for n in args.problems:
                problems = sn.pack(pool[:n])
                Pd, od, rd, keep_d = lib._sim3_opt_pack(problems)
                Ph, oh, rh, keep_h = lib._sim3_opt_pack(problems)

                def dev():
                    if L.drfe_sim3_opt_batch(ctx.h, C.byref(Pd), C.byref(od), None) != 0:
                        raise RuntimeError("drfe_sim3_opt_batch failed")

                def host():
                    if L.drfe_sim3_opt_host(C.byref(Ph), C.byref(oh)) != 0:
                        raise RuntimeError("drfe_sim3_opt_host failed")
                (dm, dmin, dmax, dreps), (hm, hmin, hmax, hreps) = timed_pair(dev, host, args.seconds, args.max_reps)
                differ = sn.tables_equal(rd, rh)
                assert args.keep_going or not differ, (N, n, differ)
                row = dict(problems=n, matches=N, iterations=int(rh["iterations"].sum()), trials=int(rh["trials"].sum()),
                           device_ms=round(dm, 4), device_spread_ms=round(dmax - dmin, 4), device_reps=dreps,
                           host_ms=round(hm, 4), host_spread_ms=round(hmax - hmin, 4), host_reps=hreps,
                           speedup=round(hm / dm, 2), equal=not differ,
                           device_wins=bool(hm - dm > max(dmax - dmin, hmax - hmin)))
                print(json.dumps(row), flush=True)
                rows.append(row)
        rows.append(dict(handed_back=ctx.sim3_opt_stats()["handed_back"]))
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
