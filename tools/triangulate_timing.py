"""Per-call time of device map-point / map-line triangulation (drfe_triangulate_points_batch / drfe_triangulate_lines_batch)
next to the host entries (drfe_triangulate_points_host / _lines_host, one CPU thread) on the same synthetic matches
(tests/triangulate_numpy.py's scenes: RGB-D keyframes around a room, 40 % monocular keypoints, 15 % wrong matches).
Configurations: one pair of a few hundred matches; one keyframe's ten neighbour pairs as ten calls (CreateNewMapPoints' loop);
a batch of 640 independent pairs in one call (many keyframes or sequences at once).  The device call returns with the results in
host memory, so wall time is its cost (staging and both copies included).  Device == host is checked.  Prints one JSON line per
configuration and writes them to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def one_pair(scene, p):
    s = dict(scene)
    a, b = int(scene["match_offsets"][p]), int(scene["match_offsets"][p + 1])
    s.update(kf1=scene["kf1"][p:p + 1], kf2=scene["kf2"][p:p + 1], match_offsets=np.int32([0, b - a]), matches=scene["matches"][a:b])
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_timing.jsonl"))
    args = ap.parse_args()
    import triangulate_numpy as TN
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)
    rows = []
    try:
        for line in (False, True):
            rng = np.random.default_rng(21 + line)
            one = TN.random_scene(rng, n_kf=2, n_feat=600, n_pairs=1, line=line, per_pair=(300, 301))
            ten = TN.random_scene(rng, n_kf=12, n_feat=600, n_pairs=10, line=line, per_pair=(200, 400), one_kf1=True)
            big = TN.random_scene(rng, n_kf=64, n_feat=600, n_pairs=640, line=line, per_pair=(200, 400))
            host_fn = lib.triangulate_lines_host if line else lib.triangulate_points_host
            dev_fn = ctx.triangulate_lines_batch if line else ctx.triangulate_points_batch
            for name, calls in (("one pair", [one]), ("one keyframe: 10 pairs as 10 calls", [one_pair(ten, p) for p in range(10)]),
                                ("640 pairs in one call", [big])):
                for s in calls:
                    h, d = host_fn(s), dev_fn(s)
                    for k in h:
                        assert h[k].tobytes() == d[k].tobytes(), (name, k)
                dm, dmin = timed(lambda: [dev_fn(s) for s in calls], args.reps)
                hm, _ = timed(lambda: [host_fn(s) for s in calls], max(3, args.reps // 2))
                st = np.concatenate([host_fn(s)["branch"] for s in calls])
                row = dict(kind="lines" if line else "points", config=name, calls=len(calls),
                           matches=int(sum(len(s["matches"]) for s in calls)), svd_frac=round(float((st == 1).mean()), 3),
                           device_ms=round(dm, 4), device_min_ms=round(dmin, 4), host_ms=round(hm, 4), speedup=round(hm / dm, 2))
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
