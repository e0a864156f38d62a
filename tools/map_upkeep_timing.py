"""Per-call time of device map-point / map-line upkeep (drfe_map_point_upkeep_batch + drfe_map_line_upkeep_batch: descriptor,
normal and distance band of every item) next to the host entries (drfe_map_point_upkeep_host / drfe_map_line_upkeep_host, one
CPU thread) on the same items.  Configurations: one keyframe's worth (1 000 points with 2-10 observations and 100 lines, as
LocalMapping::ProcessNewKeyFrame touches) and a map-wide sweep (50 000 points whose observation counts have a heavy tail up
to 600, plus 5 000 lines, as loop correction or a map load).  The device call returns with the results in host memory, so wall
time is its cost (staging and both copies included).  Device == host is checked.  Prints one JSON line per configuration and
writes them to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def counts_for(rng, n, heavy):
    """2-10 observations; with `heavy`, 8 % of the items long-lived (Pareto tail from 11 to 600)"""
    c = rng.integers(2, 11, n)
    if heavy:
        k = rng.random(n) < 0.08
        c[k] = np.minimum(600, 11 + (rng.pareto(1.2, int(k.sum())) * 20).astype(np.int64))
    return c


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, float(np.median(ts)), float(np.min(ts))


def main():
    import map_upkeep_numpy as MU
    from dr_slam_amd import lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_upkeep_timing.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = lib.Context(max_batch=1)
    rows = []
    try:
        for name, npts, nlines, heavy in (("keyframe", 1000, 100, False), ("map_sweep", 50000, 5000, True)):
            ps = MU.random_scene(rng, counts_for(rng, npts, heavy), n_kf=2000, flips=(0, 20))
            ls = MU.random_scene(rng, counts_for(rng, nlines, heavy), line=True, n_kf=2000, flips=(0, 20))

            def dev():
                return ctx.map_point_upkeep_batch(ps), ctx.map_line_upkeep_batch(ls)

            def host():
                return lib.map_point_upkeep_host(ps), lib.map_line_upkeep_host(ls)
            dev()                                                     # warm-up: buffers, code objects
            before = ctx.map_upkeep_stats()
            (dp, dl), dmed, dmin = timed(dev, a.reps)
            after = ctx.map_upkeep_stats()
            (hp, hl), hmed, hmin = timed(host, max(1, a.reps // 2))
            same = all(dp[k].tobytes() == hp[k].tobytes() and dl[k].tobytes() == hl[k].tobytes() for k in dp)
            obs = int(ps["obs_offsets"][-1] + ls["obs_offsets"][-1])
            row = dict(config=name, points=npts, lines=nlines, observations=obs,
                       max_obs=int(max(np.diff(ps["obs_offsets"]).max(), np.diff(ls["obs_offsets"]).max())),
                       device_ms_median=round(dmed, 3), device_ms_min=round(dmin, 3), host_ms_median=round(hmed, 3),
                       host_ms_min=round(hmin, 3), speedup=round(hmed / dmed, 2), equal=bool(same),
                       stats_per_call={k: (after[k] - before[k]) // a.reps for k in after})
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
