"""Per-call time of the device entry of the map update after a global bundle adjustment (drfe_lmap_gba_device) next to its host
entry (drfe_lmap_gba_host, one CPU thread: the only baseline there is, since the entry is new) on the same store: the graphs of
tools/lmap_timing.py - 100, 1000 and 4000 key frames of about 1000 map points each - with random poses and positions, the first
observer as reference key frame, and a spanning tree formed from the first observer: the parent of key frame k is the first
observer of the first point of its match row whose first observer is an earlier key frame (k - 1 when there is none), so that
key frame 0 is the one origin.  Three stamp mixes: everything adjusted; the newest 2 % of the key frames, and the points whose
reference key frame they are, made while the adjustment ran (no stamp); a random tenth.
Two stores with the same content take the same calls in turn, one created with a context and one without.  A real call always
follows a fresh adjustment, so the clock is around drfe_lmap_set_gba_keyframes, drfe_lmap_set_gba_points and the entry together, on
both sides: the upload of the state block is part of the device's cost, and so is the copy of the records back - a device call
returns with them in host memory and committed.  nLoopKF goes up by one per call, so that the items left out keep an older stamp
and are composed, or moved through their reference key frame, every time.  Every shape is called once before it is timed; the two
entries are then called in turn until each has at least --seconds (default 0.5) of timed calls and at least five; the row holds the
median, the interquartile range and the spread (max - min) of both.  The device entry wins a row when the host's median exceeds its
median by more than the larger of the two interquartile ranges.  Device == host is checked on every shape's first call, and again
on one more call after both stores were given the same geometry and state anew.  Prints one JSON line per shape, then device_from:
the smallest number of stored points from which the device entry wins at every stamp mix and at every larger measured store (null:
at none), and writes them to --out (profiles/gba_propagate_timing.jsonl)."""
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
from loop_correct_timing import fill_geometry, make_geometry, random_poses  # noqa: E402

MIXES = ("all_adjusted", "newest_2_percent_new", "a_tenth_new")


def spanning_tree(g):
    """parent, child_off and children from the first observers"""
    n = g["n_kf"]
    first = g["obs"][g["obs_off"][:-1]]
    parent = np.full(n, -1, np.int32)
    for k in range(1, n):
        row = g["rows"][g["pt_off"][k]:g["pt_off"][k + 1]]
        cand = first[row[row >= 0]]
        cand = cand[cand < k]
        parent[k] = cand[0] if len(cand) else k - 1
    order = np.argsort(parent[1:], kind="stable") + 1
    g["parent"] = parent
    g["children"] = order.astype(np.int32)
    g["child_off"] = np.concatenate([[0], np.cumsum(np.bincount(parent[1:], minlength=n))]).astype(np.int32)


def new_keyframes(rng, n, mix):
    """the key frames made while the adjustment ran: never the origin"""
    new = np.zeros(n, bool)
    if mix == "newest_2_percent_new":
        new[n - max(1, n // 50):] = True
    elif mix == "a_tenth_new":
        new[1 + rng.permutation(n - 1)[:n // 10]] = True
    new[0] = False
    return new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gba_propagate_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    p = lib._p
    rows, wins = [], {}
    try:
        for n_kf in args.keyframes:
            g = make_graph(np.random.default_rng(n_kf), n_kf)
            spanning_tree(g)
            geo = make_geometry(np.random.default_rng(n_kf + 1), g)
            rng = np.random.default_rng(n_kf + 2)
            T_all = random_poses(rng, n_kf).reshape(n_kf, 16)
            X_all = rng.uniform(-20, 20, (g["n_mp"], 3)).astype(np.float32)
            for mix in MIXES:
                new = new_keyframes(rng, n_kf, mix)
                kf_h = np.ascontiguousarray(g["handle"][~new])
                kf_T = np.ascontiguousarray(T_all[~new])
                mp_sel = ~new[geo["ref"]]
                mp_h = np.ascontiguousarray(g["mp_handle"][mp_sel])
                mp_X = np.ascontiguousarray(X_all[mp_sel])
                kf_s, mp_s = np.zeros(len(kf_h), np.int32), np.zeros(len(mp_h), np.int32)
                origin = np.zeros(1, np.int32)
                capK, capP = n_kf, g["n_mp"]
                dbs = {"device": lib.LocalMap(ctx), "host": lib.LocalMap()}
                state = {}
                for mode, db in dbs.items():
                    fill(lib, L, db, g)
                    r = {"n_keyframes": np.zeros(1, np.int32), "keyframes": np.zeros(capK, np.int32), "Tcw": np.zeros((capK, 16), np.float32),
                         "TcwBef": np.zeros((capK, 16), np.float32), "composed": np.zeros(capK, np.uint8),
                         "n_points": np.zeros(1, np.int32), "points": np.zeros(capP, np.int32), "world": np.zeros((capP, 3), np.float32),
                         "kind": np.zeros(capP, np.uint8)}
                    out = lib.LmapGbaOut(capK, capP, *[p(r[k]) for k in lib.LMAP_GBA_OUT_FIELDS])
                    state[mode] = dict(out=out, r=r, db=db, loop=0)

                def call(mode):
                    S = state[mode]
                    S["loop"] += 1
                    kf_s[:] = S["loop"]
                    mp_s[:] = S["loop"]
                    h = S["db"].h
                    fn = getattr(L, f"drfe_lmap_gba_{mode}")
                    rc = L.drfe_lmap_set_gba_keyframes(h, len(kf_h), p(kf_h), p(kf_T), p(kf_s))
                    rc = rc or L.drfe_lmap_set_gba_points(h, len(mp_h), p(mp_h), p(mp_X), p(mp_s))
                    rc = rc or fn(*((h, S["loop"], 1, p(origin), C.byref(S["out"])) + ((None,) if mode == "device" else ())))
                    if rc != 0:
                        raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(h).decode())

                def equal():
                    d, h = state["device"]["r"], state["host"]["r"]
                    v, m = int(h["n_keyframes"][0]), int(h["n_points"][0])
                    same = int(d["n_keyframes"][0]) == v and int(d["n_points"][0]) == m
                    for k in ("keyframes", "Tcw", "TcwBef", "composed"):
                        same = same and d[k][:v].tobytes() == h[k][:v].tobytes()
                    for k in ("points", "world", "kind"):
                        same = same and d[k][:m].tobytes() == h[k][:m].tobytes()
                    return same

                def again(loop):
                    for S in state.values():
                        fill_geometry(lib, L, S["db"], g, geo)
                        S["loop"] = loop
                again(0)
                call("device")
                call("host")
                first_equal = equal()
                assert first_equal, (n_kf, mix)
                (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = timed_pair_quartiles(
                    lambda: call("device"), lambda: call("host"), args.seconds, args.max_reps)
                R = state["host"]["r"]
                v, m = int(R["n_keyframes"][0]), int(R["n_points"][0])
                composed, kind_ref = int(R["composed"][:v].sum()), int((R["kind"][:m] == 2).sum())
                st = dbs["host"].gba_stats()
                again(10 ** 6)
                call("device")
                call("host")
                last_equal = equal()
                assert last_equal, (n_kf, mix)
                dm, diqr, hm, hiqr = round(dm, 4), round(diqr, 4), round(hm, 4), round(hiqr, 4)      # the file's digits decide
                row = dict(keyframes=n_kf, points=g["n_mp"], mix=mix, visited=v, composed=composed, deepest_chain=st["deepest_chain"],
                           moved=m, moved_through_ref=kind_ref, device_ms=dm, device_iqr_ms=diqr, device_spread_ms=round(dspread, 4),
                           device_reps=dreps, host_ms=hm, host_iqr_ms=hiqr, host_spread_ms=round(hspread, 4), host_reps=hreps,
                           speedup=round(hm / dm, 2), equal=bool(first_equal and last_equal), device_wins=bool(hm - dm > max(diqr, hiqr)))
                print(json.dumps(row), flush=True)
                rows.append(row)
                wins.setdefault(g["n_mp"], []).append(row["device_wins"])
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
