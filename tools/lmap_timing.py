"""Per-call time of Tracking::UpdateLocalMap's device entry (drfe_lmap_update_device) next to its host entry (drfe_lmap_update_host,
one CPU thread) on the same store and frames: 100, 1000 and 4000 key frames of about 1000 map points each, every point observed
by 8 key frames drawn from a window of 64 consecutive ones (so a frame of about 1000 points from one place votes for about 80
key frames and its gathers walk about 10^5 entries), neighbours, children and parents among the adjacent key frames, a map line
per 10 points; 1, 4, 16, 64 and 256 frames a call.
Two stores with the same content take the same calls in turn, one created with a context and one without.  The clock is around
the C entry alone (the query arrays are packed once; only the frame ids are raised between calls, as the entry requires); a
device call returns with the lists in host memory, so wall time is its cost, all copies included.  The image is on the device
before the clock starts (the first call sends it).  Every timed shape is called once before it is timed; the two entries are then
called in turn until each has at least --seconds (default 0.5) of timed calls and at least five; the row holds the median, the
interquartile range and the spread (max - min) of both.  The device entry wins a row when the host's median exceeds its median by
more than the larger of the two interquartile ranges.  Device == host is checked on every shape's first call.  The reference's
Tracking cannot be built next to this library, so the table compares this library's two entries only.  Prints one JSON line per
shape, then device_from: the smallest query count from which the device entry wins at every measured store size (null: at none),
and writes them to --out (profiles/lmap_timing.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS_PER_KF = 1000
OBS = 8
WINDOW = 64


def timed_pair_quartiles(fa, fb, seconds, max_reps):
    """a b a b .., each called once before the clock starts; per function (median, interquartile range, max - min, calls), in ms"""
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
    out = []
    for ts in (ta, tb):
        q1, med, q3 = (1e3 * float(x) for x in np.percentile(ts, [25, 50, 75]))
        out.append((med, q3 - q1, 1e3 * float(np.max(ts) - np.min(ts)), len(ts)))
    return out


def make_graph(rng, n_kf):
    """the arrays of drfe_lmap_set_keyframes / _set_points / _set_lines"""
    n_mp = n_kf * POINTS_PER_KF // OBS
    n_ml = (n_mp + 9) // 10
    win = min(WINDOW, n_kf)
    base = np.clip(np.arange(n_mp) * OBS // POINTS_PER_KF - win // 2, 0, n_kf - win)
    keys = rng.random((n_mp, win)).argsort(axis=1)[:, :min(OBS, win)]          # distinct key frames of the window
    obs = (base[:, None] + keys).astype(np.int32)
    obs_off = (np.arange(n_mp + 1) * obs.shape[1]).astype(np.int32)
    # a key frame's match row: the points that observe it, in random order, one entry in ten null
    kf_of, pt_of = obs.reshape(-1), np.repeat(np.arange(n_mp, dtype=np.int32), obs.shape[1])
    order = np.lexsort((rng.random(len(kf_of)), kf_of))
    rows = pt_of[order].copy()
    rows[rng.random(len(rows)) < 0.1] = -1
    pt_off = np.concatenate([[0], np.cumsum(np.bincount(kf_of, minlength=n_kf))]).astype(np.int32)
    lines = np.where(rows >= 0, rows // 10, -1).astype(np.int32)[::4].copy()   # a quarter as many line matches
    ln_off = ((pt_off + 3) // 4).astype(np.int32)
    k = np.arange(n_kf, dtype=np.int32)
    nbr = np.clip(k[:, None] + np.array([1, -1, 2, -2, 3, -3, 4, -4, 5, -5], np.int32), 0, n_kf - 1).astype(np.int32)
    nbr[nbr == k[:, None]] = -1
    parent = (k - 1).astype(np.int32)
    child_off = np.minimum(np.arange(n_kf + 1), n_kf - 1).astype(np.int32)      # key frame k has the child k + 1
    children = np.arange(1, n_kf, dtype=np.int32)
    rank = (rng.permutation(n_kf).astype(np.uint64) + 1) * 4096
    return dict(n_kf=n_kf, n_mp=n_mp, n_ml=n_ml, handle=k, rank=rank, kf_bad=(rng.random(n_kf) < 0.02).astype(np.uint8),
                parent=parent, nbr=np.ascontiguousarray(nbr), child_off=child_off, children=children, pt_off=pt_off,
                rows=np.ascontiguousarray(rows), ln_off=ln_off, lines=np.ascontiguousarray(lines[:ln_off[-1]]),
                mp_handle=np.arange(n_mp, dtype=np.int32), mp_bad=(rng.random(n_mp) < 0.02).astype(np.uint8), obs_off=obs_off,
                obs=np.ascontiguousarray(obs.reshape(-1)), ml_handle=np.arange(n_ml, dtype=np.int32), ml_bad=np.zeros(n_ml, np.uint8))


def fill(lib, L, db, g):
    p = lib._p
    K = lib.LmapKeyframes(g["n_kf"], 0, p(g["handle"]), p(g["rank"]), p(g["kf_bad"]), p(g["parent"]), p(g["nbr"]), p(g["child_off"]),
                          p(g["children"]), p(g["pt_off"]), p(g["rows"]), p(g["ln_off"]), p(g["lines"]))
    db._chk(L.drfe_lmap_set_keyframes(db.h, C.byref(K)), "set_keyframes")
    db._chk(L.drfe_lmap_set_points(db.h, g["n_mp"], p(g["mp_handle"]), p(g["mp_bad"]), p(g["obs_off"]), p(g["obs"])), "set_points")
    db._chk(L.drfe_lmap_set_lines(db.h, g["n_ml"], p(g["ml_handle"]), p(g["ml_bad"])), "set_lines")


def make_frames(rng, g, n):
    """n frames of POINTS_PER_KF keypoints: the points around a random key frame, one in ten null"""
    pts = np.empty((n, POINTS_PER_KF), np.int32)
    for i in range(n):
        c = int(rng.integers(0, g["n_kf"])) * POINTS_PER_KF // OBS
        lo, hi = max(0, c - 4 * POINTS_PER_KF // OBS), min(g["n_mp"], c + 4 * POINTS_PER_KF // OBS)
        pts[i] = rng.integers(lo, hi, POINTS_PER_KF)
    pts[rng.random(pts.shape) < 0.1] = -1
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 4, 16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmap_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows, wins = [], {}
    try:
        for n_kf in args.keyframes:
            g = make_graph(np.random.default_rng(n_kf), n_kf)
            dbs = {"device": lib.LocalMap(ctx), "host": lib.LocalMap()}
            for db in dbs.values():
                fill(lib, L, db, g)
            next_id = {"device": 1, "host": 1}
            frames = make_frames(np.random.default_rng(n_kf + 1), g, max(args.queries))
            for n in args.queries:
                pts = np.ascontiguousarray(frames[:n].reshape(-1))
                off = (np.arange(n + 1) * POINTS_PER_KF).astype(np.int32)
                lns = np.ascontiguousarray(np.where(pts >= 0, pts // 10, -1)[::10].astype(np.int32))
                loff = (np.arange(n + 1) * (POINTS_PER_KF // 10)).astype(np.int32)
                caps = (n * n_kf, min(n * g["n_mp"], n * 400 * POINTS_PER_KF), min(n * g["n_ml"], n * 40 * POINTS_PER_KF), len(pts))
                state = {}
                for mode in ("device", "host"):
                    ident = np.zeros(n, np.int64)
                    r = {"kf_offsets": np.zeros(n + 1, np.int32), "kfs": np.zeros(caps[0], np.int32), "ref_kf": np.zeros(n, np.int32),
                         "mp_offsets": np.zeros(n + 1, np.int32), "mps": np.zeros(caps[1], np.int32),
                         "mp_in_frame": np.zeros(caps[1], np.uint8), "ml_offsets": np.zeros(n + 1, np.int32),
                         "mls": np.zeros(caps[2], np.int32), "ml_in_frame": np.zeros(caps[2], np.uint8),
                         "nulled_offsets": np.zeros(n + 1, np.int32), "nulled": np.zeros(caps[3], np.int32),
                         "record": np.zeros((n, 4), np.int32)}
                    Q = lib.LmapQueries(n, 0, lib._p(ident), lib._p(off), lib._p(pts), lib._p(loff), lib._p(lns), None, None)
                    out = lib.LmapOut(*caps, *[lib._p(r[k]) for k in lib.LMAP_OUT_FIELDS])
                    state[mode] = dict(Q=Q, out=out, r=r, ident=ident, db=dbs[mode])

                def call(mode):
                    S = state[mode]
                    S["ident"][:] = next_id[mode] + np.arange(n)            # above every id this store has seen
                    next_id[mode] += n
                    fn = getattr(L, f"drfe_lmap_update_{mode}")
                    a = (S["db"].h, C.byref(S["Q"]), C.byref(S["out"])) + ((None,) if mode == "device" else ())
                    if fn(*a) != 0:
                        raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(S["db"].h).decode())
                call("device")
                call("host")
                d, h = state["device"]["r"], state["host"]["r"]
                used = {"kfs": h["kf_offsets"][n], "mps": h["mp_offsets"][n], "mp_in_frame": h["mp_offsets"][n],
                        "mls": h["ml_offsets"][n], "ml_in_frame": h["ml_offsets"][n], "nulled": h["nulled_offsets"][n]}
                equal = all(d[k][:used.get(k, len(d[k]))].tobytes() == h[k][:used.get(k, len(h[k]))].tobytes() for k in d)
                assert equal, (n_kf, n)
                (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = timed_pair_quartiles(
                    lambda: call("device"), lambda: call("host"), args.seconds, args.max_reps)
                row = dict(keyframes=n_kf, points=g["n_mp"], queries=n, local_kfs_per_query=round(float(used["kfs"]) / n, 1),
                           local_points_per_query=round(float(used["mps"]) / n, 1), device_ms=round(dm, 4),
                           device_iqr_ms=round(diqr, 4), device_spread_ms=round(dspread, 4), device_reps=dreps,
                           host_ms=round(hm, 4), host_iqr_ms=round(hiqr, 4), host_spread_ms=round(hspread, 4), host_reps=hreps,
                           speedup=round(hm / dm, 2), equal=equal, device_wins=bool(hm - dm > max(diqr, hiqr)))
                print(json.dumps(row), flush=True)
                rows.append(row)
                wins.setdefault(n, []).append(row["device_wins"])
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
