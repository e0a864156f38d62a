"""Per-call time of the device PoseOptimization (drfe_pose_opt_batch) next to its host entry (drfe_pose_opt_host, one CPU thread) on
the same planted frames (tests/pose_opt_numpy.py: 20 % gross outliers, alternating mono / stereo points): 1, 4, 16, 64 and 512
frames of 100, 300 and 1 000 point edges, without and with 30 lines and 3 plane slots (matched, parallel and vertical map plane
each, bStruct on).
The clock is around the C entry alone (the records are packed once, outside it); the device call returns with the outputs in host
memory, so wall time is its cost, staging and both copies included.  Every timed shape is called once before it is timed; the two entries are then
called in turn until each has at least --seconds (default 1) of timed calls and at least five; the row holds the median and the
spread (max - min) of both entries.  Device == host is checked at every size.  Prints one JSON line per configuration and writes them to
--out (profiles/pose_opt_timing.jsonl)."""
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


def timed_pair(fa, fb, seconds, max_reps):
    """fa and fb called in turn (a b a b ..), each once before the clock starts, until each has at least five timed calls and
    `seconds` of them (or max_reps): per function (median ms, min ms, max ms, calls).  Alternating puts a drift of the machine -
    clocks, other tenants - into both columns alike."""
    fa()
    fb()
    ta, tb = [], []

    def more(ts):
        return (sum(ts) < seconds and len(ts) < max_reps) or len(ts) < 5
    while more(ta) or more(tb):
        for fn, ts in ((fa, ta), (fb, tb)):
            if more(ts):
                t = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t)
    return [(1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts)), len(ts)) for ts in (ta, tb)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 4, 16, 64, 512])
    ap.add_argument("--points", type=int, nargs="*", default=[100, 300, 1000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_opt_timing.jsonl"))
    args = ap.parse_args()
    import pose_opt_numpy as pn
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows = []
    try:
        for N in args.points:
            for extras in (False, True):
                rng = np.random.default_rng(N + extras)
                pool = [pn.frame(rng, N, 30 if extras else 0, planes=(7, 7, 7) if extras else (), b_struct=int(extras), outlier_frac=0.2)
                        for _ in range(max(args.frames))]
                for n in args.frames:
                    problems = pn.pack(pool[:n])
                    Pd, od, rd, keep_d = lib._pose_opt_pack(problems)
                    Ph, oh, rh, keep_h = lib._pose_opt_pack(problems)

                    def dev():
                        if L.drfe_pose_opt_batch(ctx.h, C.byref(Pd), C.byref(od), None) != 0:
                            raise RuntimeError("drfe_pose_opt_batch failed")

                    def host():
                        if L.drfe_pose_opt_host(C.byref(Ph), C.byref(oh)) != 0:
                            raise RuntimeError("drfe_pose_opt_host failed")
                    (dm, dmin, dmax, dreps), (hm, hmin, hmax, hreps) = timed_pair(dev, host, args.seconds, args.max_reps)
                    assert not pn.tables_equal(rd, rh), (N, extras, n)
                    row = dict(frames=n, points=N, lines=30 if extras else 0, plane_slots=3 if extras else 0,
                               iterations=int(rh["iterations"].sum()), trials=int(rh["trials"].sum()),
                               device_ms=round(dm, 4), device_spread_ms=round(dmax - dmin, 4), device_reps=dreps,
                               host_ms=round(hm, 4), host_spread_ms=round(hmax - hmin, 4), host_reps=hreps,
                               speedup=round(hm / dm, 2),
                               device_wins=bool(hm - dm > max(dmax - dmin, hmax - hmin)))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
        rows.append(dict(handed_back=ctx.pose_opt_stats()["handed_back"]))
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
