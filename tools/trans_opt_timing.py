"""Per-call time of the device TranslationOptimization (drfe_trans_opt_batch) next to its host entry (drfe_trans_opt_host, one CPU
thread) and next to the device PoseOptimization (drfe_pose_opt_batch) on the same planted frames (tests/trans_opt_numpy.py: the
start rotation the planted one, 20 % gross outliers, alternating mono / stereo points): 1, 4, 16, 64 and 512 frames of (100 points),
(300 points, 30 lines, 3 plane slots) and (1 000 points, 30 lines, 3 plane slots); a plane slot holds a matched, a parallel and a
vertical map plane, bStruct on.
The protocol is tools/pose_opt_timing.py's: the clock is around the C entry alone (the records are packed once, outside it); a
device call returns with the outputs in host memory, so wall time is its cost, staging and both copies included.  Every timed
shape is called once before it is timed; the entries are then called in turn until each has at least --seconds (default 1) of
timed calls and at least five; the row holds the median and the spread (max - min) of each entry, and each device entry's time
per Levenberg trial (call time over its own iterations + trials summed over the frames).  trans device == trans host is checked
at every size.  Prints one JSON line per configuration and writes them to --out (profiles/trans_opt_timing.jsonl)."""
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


def timed_in_turn(fns, seconds, max_reps):
    """the functions called in turn (a b c a b c ..), each once before the clock starts, until each has at least five timed calls
    and `seconds` of them (or max_reps): per function (median ms, min ms, max ms, calls).  Taking turns puts a drift of the machine
    - clocks, other tenants - into every column alike."""
    for fn in fns:
        fn()
    times = [[] for _ in fns]

    def more(ts):
        return (sum(ts) < seconds and len(ts) < max_reps) or len(ts) < 5
    while any(more(ts) for ts in times):
        for fn, ts in zip(fns, times):
            if more(ts):
                t = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t)
    return [(1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts)), len(ts)) for ts in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 4, 16, 64, 512])
    ap.add_argument("--shapes", type=int, nargs="*", default=[100, 0, 0, 300, 30, 3, 1000, 30, 3], help="points lines plane_slots, repeated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trans_opt_timing.jsonl"))
    args = ap.parse_args()
    import trans_opt_numpy as tn
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows = []
    try:
        for N, NL, S in zip(args.shapes[0::3], args.shapes[1::3], args.shapes[2::3]):
            rng = np.random.default_rng(N + NL + S)
            pool = [tn.tframe(rng, N, NL, planes=(7,) * S, b_struct=int(S > 0), outlier_frac=0.2) for _ in range(max(args.frames))]
            for n in args.frames:
                problems = tn.pack(pool[:n])
                packs = [lib._pose_opt_pack(problems) for _ in range(3)]
                (Pd, od, rd, _k0), (Ph, oh, rh, _k1), (Pp, op, rp, _k2) = packs

                def dev():
                    if L.drfe_trans_opt_batch(ctx.h, C.byref(Pd), C.byref(od), None) != 0:
                        raise RuntimeError("drfe_trans_opt_batch failed")

                def host():
                    if L.drfe_trans_opt_host(C.byref(Ph), C.byref(oh)) != 0:
                        raise RuntimeError("drfe_trans_opt_host failed")

                def pose():
                    if L.drfe_pose_opt_batch(ctx.h, C.byref(Pp), C.byref(op), None) != 0:
                        raise RuntimeError("drfe_pose_opt_batch failed")
                (dm, dmin, dmax, dreps), (hm, hmin, hmax, hreps), (pm, pmin, pmax, preps) = timed_in_turn((dev, host, pose), args.seconds, args.max_reps)
                assert not tn.tables_equal(rd, rh), (N, NL, S, n)
                steps = int(rd["iterations"].sum()) + int(rd["trials"].sum())
                pose_steps = int(rp["iterations"].sum()) + int(rp["trials"].sum())
                row = dict(frames=n, points=N, lines=NL, plane_slots=S, iterations=int(rd["iterations"].sum()), trials=int(rd["trials"].sum()),
                           device_ms=round(dm, 4), device_spread_ms=round(dmax - dmin, 4), device_reps=dreps,
                           host_ms=round(hm, 4), host_spread_ms=round(hmax - hmin, 4), host_reps=hreps,
                           speedup=round(hm / dm, 2), device_wins=bool(hm - dm > max(dmax - dmin, hmax - hmin)),
                           pose_opt_ms=round(pm, 4), pose_opt_spread_ms=round(pmax - pmin, 4), pose_opt_reps=preps,
                           pose_opt_iterations=int(rp["iterations"].sum()), pose_opt_trials=int(rp["trials"].sum()),
                           device_us_per_step=round(1e3 * dm / max(steps, 1), 4), pose_opt_us_per_step=round(1e3 * pm / max(pose_steps, 1), 4),
                           # not slower per Levenberg trial than PoseOptimization's device entry, by more than the larger spread
                           per_step_ok=bool(dm / max(steps, 1) - pm / max(pose_steps, 1) <=
                                            max((dmax - dmin) / max(steps, 1), (pmax - pmin) / max(pose_steps, 1))))
                print(json.dumps(row), flush=True)
                rows.append(row)
        rows.append(dict(handed_back=ctx.trans_opt_stats()["handed_back"], pose_opt_handed_back=ctx.pose_opt_stats()["handed_back"]))
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
