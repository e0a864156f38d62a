"""Per-call time of LocalMapping::MapPlaneCulling's device entry (drfe_plane_map_cull_batch, device forced) next to its host entry
(drfe_plane_map_cull_host, one CPU thread: the reference's own walk restated) on the same map: Manhattan-style maps of 16, 64 and
256 planes in three families of parallel walls half a metre apart (a third of the pairs pass the angle gate, none is near
enough to merge), clouds of 500 and 4000 points, every plane seen from three key frames.  "with_events" 1 moves one plane in
sixteen onto the wall of the plane six further on, so that it is merged, its survivor rebuilt and the survivor's column read
again by the row between them.

The clock is around the C entry alone, inputs packed and output arrays allocated once; a device call returns with the results in
host memory and the map committed, so wall time is its cost, all copies, rebuild rounds and column recomputes included.  A call
with events changes the resident map, so every timed device call follows a fresh (untimed) upload, in all shapes alike.  One
untimed pair of calls warms up, then --reps (default 9) calls per side.  The row holds the median and the interquartile range
of both, the same for the device entry with one row per tile (a per-pair work list: every pair loads its cloud again), and the
call's counters: pairs and cloud points scanned, rebuilds, stale columns.  The device entry wins a row when the host's median
exceeds its median by more than the larger of the two interquartile ranges.  Device == host is checked on every shape.  Prints
one JSON line per shape, then device_from: the smallest plane count from which the device entry wins at every cloud size and in
both variants (null: at none), and writes them to --out (profiles/plane_cull_timing.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

f32 = np.float32


def make_scene(n_planes, cloud_points, with_events, seed=0):
    rng = np.random.default_rng(seed + 1000 * n_planes + cloud_points)
    n_kfs = 12
    Twc = np.stack([np.eye(4, dtype=f32)] * n_kfs)
    for k in range(n_kfs):
        Twc[k, :3, 3] = (0.25 * k, -0.125 * k, 0.0625 * k)
    offset = [0.5 * (p // 3) for p in range(n_planes)]
    if with_events:
        for p in range(0, n_planes - 6, 16):
            offset[p] = offset[p + 6] + 0.01
    s = dict(coefs=np.zeros((n_planes, 4), f32), bad=np.zeros(n_planes, np.uint8), clouds=[], found=np.full(n_planes, 10, np.int32),
             visible=np.full(n_planes, 12, np.int32), n_obs=np.full(n_planes, 3, np.int32), first_kf_id=np.full(n_planes, 40, np.int32),
             obs=[], kf_clouds=[[] for _ in range(n_kfs)], Twc=Twc, dTh=0.1, aTh=0.985, current_kf_id=50,
             recent=list(range(max(n_planes - 8, 0), n_planes)))

    def cloud(axis, h, n):
        p = np.empty((n, 3), f32)
        others = [a for a in range(3) if a != axis]
        p[:, others[0]] = rng.uniform(-1, 1, n)
        p[:, others[1]] = rng.uniform(-1, 1, n)
        p[:, axis] = h + rng.normal(0, 0.003, n)
        return p

    for p in range(n_planes):
        axis = p % 3
        s["coefs"][p, axis] = 1
        s["coefs"][p, 3] = -offset[p]
        s["clouds"].append(cloud(axis, offset[p], cloud_points))
        o = []
        for kf in sorted(rng.choice(n_kfs, 3, replace=False).tolist()):
            s["kf_clouds"][kf].append((cloud(axis, offset[p], cloud_points // 3) - Twc[kf, :3, 3]).astype(f32))
            o.append((kf, len(s["kf_clouds"][kf]) - 1))
        s["obs"].append(o)
    return s


def quartiles(ts):
    q1, med, q3 = (1e3 * float(x) for x in np.percentile(ts, [25, 50, 75]))
    return round(med, 4), round(q3 - q1, 4), len(ts)


def equal(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in ("events", "bad", "n_obs", "found", "visible", "verdicts")) and a["rebuilt"] == b["rebuilt"]
            and a["counters"] == b["counters"] and all(a["clouds"][j].tobytes() == b["clouds"][j].tobytes() for j in a["rebuilt"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--planes", type=int, nargs="*", default=[16, 64, 256])
    ap.add_argument("--cloud-points", type=int, nargs="*", default=[500, 4000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_cull_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows, wins = [], {}
    try:
        for P in args.planes:
            for n in args.cloud_points:
                for ev in (0, 1):
                    s = make_scene(P, n, ev)
                    mp = dict(coefs=s["coefs"], bad=s["bad"], clouds=s["clouds"], points=np.zeros((0, 3), f32))
                    cin, cout, keep, o = lib._plane_cull_pack(s)
                    coefs, bad = np.ascontiguousarray(s["coefs"], f32), np.ascontiguousarray(s["bad"], np.uint8)
                    coff, xyz = lib._clouds_csr(list(s["clouds"]))

                    def host():
                        t = time.perf_counter()
                        rc = L.drfe_plane_map_cull_host(C.byref(cin), lib._p(coefs), lib._p(bad), lib._p(coff), lib._p(xyz), C.byref(cout))
                        dt = time.perf_counter() - t
                        assert rc == 0, rc
                        return dt, lib._plane_cull_result(cin, cout, o)

                    def device(mode):
                        ctx.plane_map_upload([mp])
                        t = time.perf_counter()
                        rc = L.drfe_plane_map_cull_batch(ctx.h, 0, C.byref(cin), mode, C.byref(cout), None)
                        dt = time.perf_counter() - t
                        assert rc == 0, L.drfe_last_error(ctx.h).decode()
                        return dt, lib._plane_cull_result(cin, cout, o)

                    times = {"host": [], "device": [], "per_pair": []}
                    same = True
                    for rep in range(args.reps + 1):
                        th, rh = host()
                        td, rd = device(lib.PLANE_CULL_DEVICE)
                        tp, rp = device(lib.PLANE_CULL_DEVICE_PER_PAIR)
                        same = same and equal(rh, rd) and equal(rh, rp)
                        if rep:                                  # the first round is the warm-up
                            times["host"].append(th)
                            times["device"].append(td)
                            times["per_pair"].append(tp)
                    (hm, hiqr, hreps), (dm, diqr, dreps), (pm, piqr, _) = (quartiles(times[k]) for k in ("host", "device", "per_pair"))
                    row = dict(planes=P, cloud_points=n, with_events=ev, events=int(len(rh["events"])), **rh["counters"],
                               device_ms=dm, device_iqr_ms=diqr, device_reps=dreps, host_ms=hm, host_iqr_ms=hiqr, host_reps=hreps,
                               per_pair_ms=pm, per_pair_iqr_ms=piqr, speedup=round(hm / dm, 2), equal=bool(same),
                               device_wins=bool(hm - dm > max(diqr, hiqr)))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                    wins.setdefault(P, []).append(row["device_wins"])
        device_from = None
        for P in sorted(wins, reverse=True):
            if not all(wins[P]):
                break
            device_from = P
        rows.append(dict(device_from=device_from))
        print(json.dumps(rows[-1]), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
