"""Per-call time of the device entry of LocalMapping::MapPointCulling and MapLineCulling (drfe_lmap_recent_cull_device) next to its
host entry (drfe_lmap_recent_cull_host, one CPU thread) on the same store: the graphs of tools/lmap_timing.py at 100, 400 and 1600
key frames of about 1000 map points each, every point observed by 8 key frames, a tenth as many map lines observed where they
stand in the line rows; and recent lists of 64, 512, 4096 and 32768 entries, seven eighths of them points (a store that holds
fewer distinct items gives a shorter list; the row keeps the length asked for under "entries" and the length run under "named").

"culled_tenth" 0 lists items that stay (found == visible, first seen by the current key frame); 1 makes every tenth entry an item
with found / visible = 1 / 5, which gets SetBadFlag and nulls its 8 observers' entries.

Two stores with the same content take the same calls in turn, one created with a context and one without.  The clock is around the
C entry alone, output arrays allocated once; a device call returns with the results in host memory and committed, so wall time is
its cost, all copies included.  A call that culls changes the store, so with culled_tenth 1 both stores are filled again before
every timed call and one untimed call of a single item that stays rebuilds the image and sends it to the device, as a caller with
a resident store would meet it; those shapes get --cull-reps calls each (default 7).  Without culls nothing changes and the two
entries are called in turn until each has at least --seconds (default 0.5) of timed calls and at least five.  The row holds the
median, the interquartile range and the spread (max - min) of both.  The device entry wins a row when the host's median exceeds its
median by more than the larger of the two interquartile ranges.  Device == host is checked on every shape.  Prints one JSON line
per shape, then device_from: the smallest list length from which the device entry wins at every measured store size and in both
variants (null: at none), and writes them to --out (profiles/recent_cull_timing.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lmap_timing import fill, make_graph, timed_pair_quartiles  # noqa: E402

CURRENT = 100000
FIELDS = ("action", "n_kept", "kept", "n_culled", "culled", "erased_offsets", "erased_kf", "erased_index")


def quartiles(ts):
    q1, med, q3 = (1e3 * float(x) for x in np.percentile(ts, [25, 50, 75]))
    return med, q3 - q1, 1e3 * float(np.max(ts) - np.min(ts)), len(ts)


def attributes(g):
    """the point part of drfe_lmap_set_cull_attributes and the arrays of drfe_lmap_set_recent_attributes for a graph of make_graph;
    every item stays until a shape says otherwise"""
    n_kf, n_mp, n_ml = g["n_kf"], g["n_mp"], g["n_ml"]
    rows, pt_off, obs, obs_off = g["rows"], g["pt_off"], g["obs"], g["obs_off"]
    kf_of = np.repeat(np.arange(n_kf, dtype=np.int64), np.diff(pt_off))
    # the index of each observation in its observer's row; a null entry hid some points from their observer's row: those
    # observations name the row's first entry (whatever stands there), as a stale index would
    e = np.flatnonzero(rows >= 0)
    key = kf_of[e] * n_mp + rows[e]
    order = np.argsort(key, kind="stable")
    key, e = key[order], e[order]
    pt_of = np.repeat(np.arange(n_mp, dtype=np.int64), np.diff(obs_off))
    want = obs.astype(np.int64) * n_mp + pt_of
    at = np.minimum(np.searchsorted(key, want), len(key) - 1)
    idx = np.where(key[at] == want, e[at] - pt_off[obs], 0).astype(np.int32)
    # a line is observed by the key frames in whose line row it stands, at its first place there
    lines, ln_off = g["lines"], g["ln_off"]
    lkf = np.repeat(np.arange(n_kf, dtype=np.int64), np.diff(ln_off))
    le = np.flatnonzero(lines >= 0)
    lkey = lines[le].astype(np.int64) * n_kf + lkf[le]
    lkey, first = np.unique(lkey, return_index=True)
    le = le[first]
    l_of = (lkey // n_kf).astype(np.int32)
    l_obs = (lkey % n_kf).astype(np.int32)
    l_idx = (le - ln_off[l_obs]).astype(np.int32)
    l_off = np.concatenate([[0], np.cumsum(np.bincount(l_of, minlength=n_ml))]).astype(np.int32)
    cull = dict(kf_handle=np.zeros(0, np.int32), th_depth=np.zeros(0, np.float32), kf_flags=np.zeros(0, np.uint8), row_offsets=np.zeros(1, np.int32),
                octave=np.zeros(0, np.int32), depth=np.zeros(0, np.float32), stereo=np.zeros(0, np.uint8), point_handle=g["mp_handle"],
                n_obs=np.diff(obs_off).astype(np.int32), obs_offsets=obs_off, obs_index=idx)
    recent = dict(point_handle=g["mp_handle"], point_found=np.full(n_mp, 4, np.int32), point_visible=np.full(n_mp, 4, np.int32),
                  point_first_kf=np.full(n_mp, CURRENT, np.int64), line_handle=g["ml_handle"], line_found=np.full(n_ml, 4, np.int32),
                  line_visible=np.full(n_ml, 4, np.int32), line_first_kf=np.full(n_ml, CURRENT, np.int64),
                  line_n_obs=np.diff(l_off).astype(np.int32), line_obs_offsets=l_off, line_obs=np.ascontiguousarray(l_obs),
                  line_obs_index=np.ascontiguousarray(l_idx))
    return cull, recent


def set_attributes(lib, L, db, cull, recent):
    p = lib._p
    A = lib.LmapCullAttributes(0, len(cull["point_handle"]), *[p(cull[k]) for k in lib.LMAP_CULL_ATTR_FIELDS])
    db._chk(L.drfe_lmap_set_cull_attributes(db.h, C.byref(A)), "set_cull_attributes")
    R = lib.LmapRecentAttributes(len(recent["point_handle"]), len(recent["line_handle"]), *[p(recent[k]) for k in lib.LMAP_RECENT_ATTR_FIELDS])
    db._chk(L.drfe_lmap_set_recent_attributes(db.h, C.byref(R)), "set_recent_attributes")


def out_lists(lib, handles, caps):
    """the two drfe_lmap_recent_list of a call and the arrays they point to"""
    arrs, lists = [], []
    for hs, cap in zip(handles, caps):
        n = len(hs)
        a = {"handles": hs, "action": np.zeros(max(1, n), np.uint8), "n_kept": np.zeros(1, np.int32), "kept": np.zeros(max(1, n), np.int32),
             "n_culled": np.zeros(1, np.int32), "culled": np.zeros(max(1, n), np.int32), "erased_offsets": np.zeros(n + 1, np.int32),
             "erased_kf": np.zeros(max(1, cap), np.int32), "erased_index": np.zeros(max(1, cap), np.int32)}
        arrs.append(a)
        lists.append(lib.LmapRecentList(n, lib._p(hs), cap, *[lib._p(a[f]) for f in FIELDS]))
    return arrs, lists


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--cull-reps", type=int, default=7)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 400, 1600])
    ap.add_argument("--entries", type=int, nargs="*", default=[64, 512, 4096, 32768])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recent_cull_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows, wins = [], {}
    try:
        for n_kf in args.keyframes:
            g = make_graph(np.random.default_rng(n_kf), n_kf)
            g["kf_bad"][:] = 0
            g["mp_bad"][:] = 0
            cull, recent = attributes(g)
            dbs = {"device": lib.LocalMap(ctx), "host": lib.LocalMap()}
            rng = np.random.default_rng(n_kf + 2)
            p_order, l_order = rng.permutation(g["n_mp"]).astype(np.int32), rng.permutation(g["n_ml"]).astype(np.int32)
            for tenth in (0, 1):
                for asked in args.entries:
                    n_l = min(asked // 8, g["n_ml"] - 1)
                    n_p = min(asked - asked // 8, g["n_mp"] - 1)
                    hs = [np.ascontiguousarray(p_order[:n_p]), np.ascontiguousarray(l_order[:n_l])]
                    stay = [np.ascontiguousarray(p_order[-1:]), np.zeros(0, np.int32)]
                    shaped = {k: v.copy() for k, v in recent.items()}
                    if tenth:
                        for kind, name in ((0, "point"), (1, "line")):
                            doomed = hs[kind][::10]
                            shaped[name + "_found"][doomed] = 1
                            shaped[name + "_visible"][doomed] = 5
                    caps = [8 * n_p + 64, int(recent["line_n_obs"][hs[1]].sum()) + 64]
                    state = {m: out_lists(lib, hs, caps) for m in dbs}
                    warm = {m: out_lists(lib, stay, [64, 64]) for m in dbs}

                    def refill():
                        for db in dbs.values():
                            fill(lib, L, db, g)
                            set_attributes(lib, L, db, cull, shaped)

                    def call(mode, S=None):
                        _, lists = S or state[mode]
                        fn = getattr(L, f"drfe_lmap_recent_cull_{mode}")
                        a = (dbs[mode].h, CURRENT, 0, C.byref(lists[0]), C.byref(lists[1])) + ((None,) if mode == "device" else ())
                        if fn(*a) != 0:
                            raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(dbs[mode].h).decode())

                    def equal():
                        ok, culled, erased = True, 0, 0
                        for d, h in zip(state["device"][0], state["host"][0]):
                            nk, nc = int(h["n_kept"][0]), int(h["n_culled"][0])
                            ne = int(h["erased_offsets"][nc])
                            ok = ok and all(d[k].tobytes() == h[k].tobytes() for k in ("action", "n_kept", "n_culled"))
                            for k, m in (("kept", nk), ("culled", nc), ("erased_offsets", nc + 1), ("erased_kf", ne), ("erased_index", ne)):
                                ok = ok and d[k][:m].tobytes() == h[k][:m].tobytes()
                            culled += nc
                            erased += ne
                        return ok, culled, erased

                    refill()
                    if tenth:
                        times = {"device": [], "host": []}
                        for rep in range(args.cull_reps + 1):
                            if rep:
                                refill()
                            for mode in dbs:
                                call(mode, warm[mode])                  # the image again, and on the device
                                t = time.perf_counter()
                                call(mode)
                                if rep:                                  # the first pair is the warm-up
                                    times[mode].append(time.perf_counter() - t)
                            same, nc, ne = equal()
                            assert same and nc > 0, (n_kf, asked, "culled")
                        (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = quartiles(times["device"]), quartiles(times["host"])
                    else:
                        call("device")
                        call("host")
                        same, nc, ne = equal()
                        assert same and nc == 0, (n_kf, asked)
                        (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = timed_pair_quartiles(
                            lambda: call("device"), lambda: call("host"), args.seconds, args.max_reps)
                        same = same and equal()[0]
                    dm, diqr, hm, hiqr = round(dm, 4), round(diqr, 4), round(hm, 4), round(hiqr, 4)      # the file's digits decide
                    row = dict(keyframes=n_kf, points=g["n_mp"], lines=g["n_ml"], entries=asked, named=n_p + n_l, culled_tenth=tenth, culled=nc,
                               erased=ne, device_ms=dm, device_iqr_ms=diqr, device_spread_ms=round(dspread, 4), device_reps=dreps,
                               host_ms=hm, host_iqr_ms=hiqr, host_spread_ms=round(hspread, 4), host_reps=hreps, speedup=round(hm / dm, 2),
                               equal=bool(same), device_wins=bool(hm - dm > max(diqr, hiqr)))
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
