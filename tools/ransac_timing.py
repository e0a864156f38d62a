"""Per-call time of a device RANSAC (drfe_sim3_ransac_batch, drfe_pnp_ransac_batch, drfe_init_ransac_batch) next to its host entry
(drfe_*_ransac_host, one CPU thread) on the same planted scenes, 30 % outliers (init: 20 %): 1, 4, 16, 64 and 512 solvers,
  --solver sim3  of 100 and of 1 000 correspondences (tests/sim3_numpy.py: min_inliers 20, 300 iterations each),
  --solver pnp   of 30, 100 and 1 000 (tests/pnp_numpy.py: SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), tail 5),
  --solver init  of 100, 300 and 1 000 matches (tests/initializer_numpy.py: sigma 1.0, 200 iterations, general and planar scenes
                 in turn, a tenth more keys than matches in each frame).
The clock is around the C entry alone (the records are packed once, outside it); the device call returns with the table in host
memory, so wall time is its cost, staging and both copies included.  Every timed shape is called once before it is timed, and a
configuration is repeated until at least --seconds have been timed.  Device == host is checked.  Prints one JSON line per
configuration and writes them to --out (profiles/sim3_timing.jsonl, profiles/pnp_timing.jsonl, profiles/initializer_timing.jsonl)."""
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


def sim3_scene(sn, rng, N, i):
    return sn.random_solver(rng, N, fix_scale=bool(i & 1), min_inliers=20, max_iterations=300, seed=i + 1, outlier_frac=0.3,
                            scale=1.2, noise=0.001)[0]


def pnp_scene(pn, rng, N, i):
    return pn.random_solver(rng, N, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991, tail=5, seed=i + 1,
                            outlier_frac=0.3, noise=0.3)[0]


def init_scene(sn, rng, N, i):
    return sn.planted(rng, N, planar=bool(i & 1) and sn.PLANAR["planar"], baseline=sn.PLANAR["baseline"] if i & 1 else 0.35,
                      extra1=N // 10, extra2=N // 10, max_iterations=200, seed=i)


# module of scenes, correspondences per solver, scene, the row's fields after `correspondences` from the host table
SOLVERS = {
    "sim3": ("sim3_numpy", (100, 1000), sim3_scene, lambda t: dict(iterations=300, hypotheses=int(t["hypotheses"].sum()))),
    "pnp": ("pnp_numpy", (30, 100, 1000), pnp_scene,
            lambda t: dict(hypotheses=int(t["hypotheses"].sum()), refines=int(t["refines"].sum()))),
    "init": ("initializer_numpy", (100, 300, 1000), init_scene,
             lambda t: dict(hypotheses=int(t["hypotheses"].sum()), branch_h=int((t["branch"] == 1).sum()), ok=int(t["ok"].sum()))),
}


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
    ap.add_argument("--solver", choices=sorted(SOLVERS), required=True)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--max-reps", type=int, default=200)
    ap.add_argument("--solvers", type=int, nargs="*", default=[1, 4, 16, 64, 512])
    ap.add_argument("--out")
    args = ap.parse_args()
    name = args.solver
    out = args.out or os.path.join(ROOT, "profiles", ("initializer" if name == "init" else name) + "_timing.jsonl")
    module, sizes, scene, extra = SOLVERS[name]
    sn = __import__(module)
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    pack = getattr(lib, "_%s_pack" % name)
    batch, host_entry = getattr(L, "drfe_%s_ransac_batch" % name), getattr(L, "drfe_%s_ransac_host" % name)
    rows = []
    try:
        for N in sizes:
            rng = np.random.default_rng(N)
            pool = [scene(sn, rng, N, i) for i in range(max(args.solvers))]
            for n in args.solvers:
                problems = sn.pack(pool[:n])
                Pd, od, rd, keep_d = pack(problems)
                Ph, oh, rh, keep_h = pack(problems)

                def dev():
                    if batch(ctx.h, C.byref(Pd), C.byref(od), None) != 0:
                        raise RuntimeError("drfe_%s_ransac_batch failed" % name)

                def host():
                    if host_entry(C.byref(Ph), C.byref(oh)) != 0:
                        raise RuntimeError("drfe_%s_ransac_host failed" % name)
                dm, dmin, dmax, dreps = timed(dev, args.seconds, args.max_reps)
                hm, hmin, hmax, hreps = timed(host, args.seconds, args.max_reps)
                assert not sn.tables_equal(rd, rh), (N, n)
                row = dict(solvers=n, correspondences=N, **extra(rh),
                           device_ms=round(dm, 4), device_min_ms=round(dmin, 4), device_max_ms=round(dmax, 4), device_reps=dreps,
                           host_ms=round(hm, 4), host_min_ms=round(hmin, 4), host_max_ms=round(hmax, 4), host_reps=hreps,
                           speedup=round(hm / dm, 2))
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
