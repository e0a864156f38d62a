"""Per-call time of the device entry of CorrectLoop's Sim3 propagation (drfe_lmap_correct_device) next to its host entry
(drfe_lmap_correct_host, one CPU thread: the baseline, since the entry is new) on the same store: the graphs of
tools/lmap_timing.py - 100, 1000 and 4000 key frames of about 1000 map points each, every point observed by 8 key frames drawn
from a window of 64 consecutive ones - with random poses, positions and octaves, the first observer as reference key frame, and
calls of 1, 4, 16, 64 and 256 distinct key frames drawn at random (a store of 100 key frames gives a call at most 100; the row
keeps the size asked for under "called" and the size run under "named").
Two stores with the same content take the same kind of calls in turn, one created with a context and one without.  The clock is
around the C entry alone, output arrays allocated once; a device call returns with the records in host memory and committed, so
wall time is its cost, all copies included.  A call commits, so the next one reads the poses and positions it left: Scw is a small
rotation with scale 1, and the current key frame alternates between the first two called ones, so that every call finds the
stamps of the one before and moves every point again.  A call of one key frame cannot alternate: after its first call the stamps
hold and it measures the poses and the walk alone, on both sides.  The device's image is kept current by the calls themselves, so
no upload is in the timed calls; the host's is its own memory.  Every timed shape is called once before it is timed; the two
entries are then called in turn until each has at least --seconds (default 0.5) of timed calls and at least five; the row holds
the median, the interquartile range and the spread (max - min) of both.  The device entry wins a row when the host's median exceeds
its median by more than the larger of the two interquartile ranges.  Device == host is checked on every shape's first call, and
again on one more call after both stores were given the same geometry anew (the timed calls leave them after different numbers
of calls).  Prints one JSON line per shape, then device_from: the smallest call size from which the device entry wins at every
measured store size (null: at none), and writes them to --out (profiles/loop_correct_timing.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lmap_timing import fill, make_graph, timed_pair_quartiles  # noqa: E402

LEVELS = 8


def random_poses(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    x, y, z, w = q.T
    T = np.zeros((n, 4, 4), np.float32)
    T[:, 0, :3] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1)
    T[:, 1, :3] = np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1)
    T[:, 2, :3] = np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)
    T[:, :3, 3] = rng.uniform(-10, 10, (n, 3))
    T[:, 3, 3] = 1
    return T


def make_geometry(rng, g):
    return dict(poses=random_poses(rng, g["n_kf"]), world=rng.uniform(-20, 20, (g["n_mp"], 3)).astype(np.float32),
                ref=np.ascontiguousarray(g["obs"][g["obs_off"][:-1]]), level=rng.integers(0, LEVELS, g["n_mp"]).astype(np.int32),
                scales=(np.float32(1.2) ** np.arange(LEVELS)).astype(np.float32))


def fill_geometry(lib, L, db, g, geo):
    p = lib._p
    db.set_scales(geo["scales"])
    db.set_poses(g["handle"], geo["poses"])
    G = lib.LmapPointGeometry(g["n_mp"], 0, p(g["mp_handle"]), p(geo["world"]), p(geo["ref"]), p(geo["level"]), None, None)
    db._chk(L.drfe_lmap_set_point_geometry(db.h, C.byref(G)), "set_point_geometry")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--called", type=int, nargs="*", default=[1, 4, 16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_correct_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    half = 0.01
    Scw = np.array([np.sin(half), 0.0, 0.0, np.cos(half), 0.01, -0.02, 0.015, 1.0], np.float64)
    rows, wins = [], {}
    try:
        for n_kf in args.keyframes:
            g = make_graph(np.random.default_rng(n_kf), n_kf)
            geo = make_geometry(np.random.default_rng(n_kf + 1), g)
            dbs = {"device": lib.LocalMap(ctx), "host": lib.LocalMap()}
            for db in dbs.values():
                fill(lib, L, db, g)
                fill_geometry(lib, L, db, g, geo)
            order = np.random.default_rng(n_kf + 2).permutation(n_kf).astype(np.int32)
            for asked in args.called:
                n = min(asked, n_kf)
                hs = np.ascontiguousarray(order[:n])
                cap = int(sum(g["pt_off"][h + 1] - g["pt_off"][h] for h in hs))
                state = {}
                for mode in ("device", "host"):
                    r = {"walk_pos": np.zeros(n, np.int32), "corrected": np.zeros((n, 8), np.float64),
                         "non_corrected": np.zeros((n, 8), np.float64), "Tiw": np.zeros((n, 16), np.float32),
                         "n_points": np.zeros(1, np.int32), "points": np.zeros(cap, np.int32), "claimed_by": np.zeros(cap, np.int32),
                         "world": np.zeros((cap, 3), np.float32), "normal": np.zeros((cap, 3), np.float32),
                         "max_distance": np.zeros(cap, np.float32), "min_distance": np.zeros(cap, np.float32),
                         "status": np.zeros(cap, np.uint8)}
                    out = lib.LmapCorrectOut(cap, 0, *[lib._p(r[k]) for k in lib.LMAP_CORRECT_OUT_FIELDS])
                    state[mode] = dict(out=out, r=r, db=dbs[mode], calls=0)

                def call(mode):
                    S = state[mode]
                    fn = getattr(L, f"drfe_lmap_correct_{mode}")
                    cur = int(hs[S["calls"] % min(n, 2)])
                    S["calls"] += 1
                    a = (S["db"].h, cur, lib._p(Scw), n, lib._p(hs), C.byref(S["out"])) + ((None,) if mode == "device" else ())
                    if fn(*a) != 0:
                        raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(S["db"].h).decode())

                def equal():
                    d, h = state["device"]["r"], state["host"]["r"]
                    m = int(h["n_points"][0])
                    return all(d[k][:(m if len(d[k]) == cap else n)].tobytes() == h[k][:(m if len(h[k]) == cap else n)].tobytes()
                               for k in d if k != "n_points") and int(d["n_points"][0]) == m, m

                def again():
                    for S in state.values():
                        fill_geometry(lib, L, S["db"], g, geo)
                        S["calls"] = 0
                again()
                call("device")
                call("host")
                first_equal, moved_first = equal()
                assert first_equal, (n_kf, n)
                (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = timed_pair_quartiles(
                    lambda: call("device"), lambda: call("host"), args.seconds, args.max_reps)
                moved_steady = int(state["host"]["r"]["n_points"][0])
                again()
                call("device")
                call("host")
                last_equal, _ = equal()
                assert last_equal, (n_kf, n)
                dm, diqr, hm, hiqr = round(dm, 4), round(diqr, 4), round(hm, 4), round(hiqr, 4)      # the file's digits decide
                row = dict(keyframes=n_kf, points=g["n_mp"], called=asked, named=n, row_entries=cap, moved_first_call=moved_first,
                           moved_per_timed_call=moved_steady, device_ms=dm, device_iqr_ms=diqr, device_spread_ms=round(dspread, 4),
                           device_reps=dreps, host_ms=hm, host_iqr_ms=hiqr, host_spread_ms=round(hspread, 4), host_reps=hreps,
                           speedup=round(hm / dm, 2), equal=bool(first_equal and last_equal), device_wins=bool(hm - dm > max(diqr, hiqr)))
                print(json.dumps(row), flush=True)
                rows.append(row)
                wins.setdefault(asked, []).append(row["device_wins"])
            for db in dbs.values():
                db.close()
        device_from = None
        for n in sorted(wins, reverse=True):
            if not all(wins[n]):
                break
            device_from = n
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
