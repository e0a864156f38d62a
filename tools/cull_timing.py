"""Per-call time of LocalMapping::KeyFrameCulling's device entry (drfe_lmap_cull_device) next to its host entry (drfe_lmap_cull_host,
one CPU thread: the reference's own walk restated) on the same store: the graphs of tools/lmap_timing.py at 100, 400 and 1600 key
frames of about 1000 map points each, every point observed by 8 key frames drawn from a window of 64 consecutive ones, and calls of
1, 4, 16, 64 and 256 distinct key frames (a store of 100 key frames gives a call at most 99; the row keeps the size asked for under
"called" and the size run under "named").

The attributes are laid out so that the walk is as long as it gets and the verdicts are known.  The first two observers of a point see
it at octave 0 and the others at octave 2, so for six of eight entries of an ordinary key frame three observers count, found
after a walk through the list, and the other two have one: 0.75 < 0.9, kept.  Every tenth key frame sees all its points at octave 5:
every entry is redundant, culled.  "culled_tenth" 0 calls ordinary key frames only; 1 puts one such key frame in every ten.

Two stores with the same content take the same calls in turn, one created with a context and one without.  The clock is around the
C entry alone, output arrays allocated once; a device call returns with the results in host memory and committed, so wall time is
its cost, all copies included.  A call that culls changes the store, so with culled_tenth 1 both stores are filled again before
every timed call and one untimed call of a key frame that stays rebuilds the image and sends it to the device, as a caller with a
resident store would meet it; those shapes get --cull-reps calls each (default 7).  Without culls nothing changes and the two
entries are called in turn until each has at least --seconds (default 0.5) of timed calls and at least five.  The row holds the
median, the interquartile range and the spread (max - min) of both.  The device entry wins a row when the host's median exceeds its
median by more than the larger of the two interquartile ranges.  Device == host is checked on every shape.  Prints one JSON line
per shape, then device_from: the smallest call size from which the device entry wins at every measured store size and in both
variants (null: at none), and writes them to --out (profiles/cull_timing.jsonl)."""
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


def attributes(rng, g):
    """the arrays of drfe_lmap_set_cull_attributes for a graph of make_graph"""
    n_kf, n_mp = g["n_kf"], g["n_mp"]
    rows, pt_off, obs, obs_off = g["rows"], g["pt_off"], g["obs"], g["obs_off"]
    kf_of = np.repeat(np.arange(n_kf, dtype=np.int32), np.diff(pt_off))
    culled = (np.arange(n_kf) % 10) == 5
    first, second = obs[obs_off[:-1]], obs[obs_off[:-1] + 1]
    at = np.maximum(rows, 0)
    octave = np.where((rows >= 0) & (first[at] != kf_of) & (second[at] != kf_of), 2, 0).astype(np.int32)
    octave[culled[kf_of]] = 5
    stereo = (rng.random(len(rows)) < 0.3).astype(np.uint8)
    depth = np.ones(len(rows), np.float32)
    # the index of each observation in its observer's row: a null entry hid some points from their observer's row, those
    # observations name the row's first entry (whatever stands there), as a stale index would
    idx = np.zeros(len(obs), np.int32)
    where = {}
    for e in np.flatnonzero(rows >= 0):
        where[(int(kf_of[e]), int(rows[e]))] = int(e - pt_off[kf_of[e]])
    pt_of = np.repeat(np.arange(n_mp, dtype=np.int32), np.diff(obs_off))
    for o in range(len(obs)):
        idx[o] = where.get((int(obs[o]), int(pt_of[o])), 0)
    n_obs = np.zeros(n_mp, np.int32)
    np.add.at(n_obs, pt_of, 1 + stereo[pt_off[obs] + idx])
    flags = np.zeros(n_kf, np.uint8)
    flags[0] = 2                                                # key frame 0 has no parent: the origin
    return dict(kf_handle=g["handle"], th_depth=np.full(n_kf, 40.0, np.float32), kf_flags=flags, row_offsets=pt_off, octave=octave,
                depth=depth, stereo=stereo, point_handle=g["mp_handle"], n_obs=n_obs, obs_offsets=obs_off, obs_index=idx, culled=culled)


def set_attributes(lib, L, db, a):
    p = lib._p
    A = lib.LmapCullAttributes(len(a["kf_handle"]), len(a["point_handle"]), *[p(a[k]) for k in lib.LMAP_CULL_ATTR_FIELDS])
    db._chk(L.drfe_lmap_set_cull_attributes(db.h, C.byref(A)), "set_cull_attributes")


def out_arrays(lib, n, n_kf, n_rows):
    ct, cw, cch, cnu, cp, cob = n_kf, 1 << 16, 2 * n_kf + 64, n_rows + 64, n_rows + 64, 8 * n_rows + 64
    r, rows = lib.LocalMap._conn_rows(ct, cw, cw)
    c = {"record": np.zeros((n, 4), np.int32), "Tcp": np.zeros((n, 16), np.float32), "has_Tcp": np.zeros(n, np.uint8),
         "n_culled": np.zeros(1, np.int32), "culled": np.zeros(n, np.int32), "n_touched": np.zeros(1, np.int32),
         "touched": np.zeros(ct, np.int32), "flags": np.zeros(ct, np.uint8), "children_offsets": np.zeros(ct + 1, np.int32),
         "children": np.zeros(cch, np.int32), "nulled_offsets": np.zeros(ct + 1, np.int32), "nulled": np.zeros(cnu, np.int32),
         "n_points": np.zeros(1, np.int32), "points": np.zeros(cp, np.int32), "point_n_obs": np.zeros(cp, np.int32),
         "point_ref": np.zeros(cp, np.int32), "point_bad": np.zeros(cp, np.uint8), "obs_offsets": np.zeros(cp + 1, np.int32),
         "obs": np.zeros(cob, np.int32), "obs_index": np.zeros(cob, np.int32)}
    p = lib._p
    out = lib.LmapCullOut(ct, cch, cnu, cp, cob, 0, p(c["record"]), p(c["Tcp"]), p(c["has_Tcp"]), p(c["n_culled"]), p(c["culled"]),
                          p(c["n_touched"]), p(c["touched"]), rows, p(c["flags"]), p(c["children_offsets"]), p(c["children"]),
                          p(c["nulled_offsets"]), p(c["nulled"]), p(c["n_points"]), p(c["points"]), p(c["point_n_obs"]),
                          p(c["point_ref"]), p(c["point_bad"]), p(c["obs_offsets"]), p(c["obs"]), p(c["obs_index"]))
    return dict(out=out, r=r, c=c)


def quartiles(ts):
    q1, med, q3 = (1e3 * float(x) for x in np.percentile(ts, [25, 50, 75]))
    return med, q3 - q1, 1e3 * float(np.max(ts) - np.min(ts)), len(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--cull-reps", type=int, default=7)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 400, 1600])
    ap.add_argument("--called", type=int, nargs="*", default=[1, 4, 16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows, wins = [], {}
    try:
        for n_kf in args.keyframes:
            g = make_graph(np.random.default_rng(n_kf), n_kf)
            g["kf_bad"][:] = 0
            a = attributes(np.random.default_rng(n_kf + 1), g)
            dbs = {"device": lib.LocalMap(ctx), "host": lib.LocalMap()}
            stay = np.array([1 if n_kf > 1 else 0], np.int32)   # an ordinary key frame: the untimed call after a refill

            def refill():
                for db in dbs.values():
                    fill(lib, L, db, g)
                    set_attributes(lib, L, db, a)

            refill()
            order = np.random.default_rng(n_kf + 2).permutation(np.arange(1, n_kf))
            plain, doomed = [h for h in order if not a["culled"][h]], [h for h in order if a["culled"][h]]
            for tenth in (0, 1):
                for asked in args.called:
                    n = min(asked, len(plain))
                    hs = list(plain[:n])
                    if tenth:
                        for i, h in zip(range(0, n, 10), doomed):
                            hs[i] = h
                    hs = np.ascontiguousarray(hs, np.int32)
                    n_rows = int(sum(g["pt_off"][h + 1] - g["pt_off"][h] for h in hs))
                    state = {m: dict(out_arrays(lib, max(n, 1), n_kf, n_rows), db=dbs[m]) for m in dbs}
                    warm = {m: dict(out_arrays(lib, 1, n_kf, 2048), db=dbs[m]) for m in dbs}

                    def call(mode, S=None, handles=None):
                        S = S or state[mode]
                        handles = hs if handles is None else handles
                        fn = getattr(L, f"drfe_lmap_cull_{mode}")
                        args_ = (S["db"].h, len(handles), lib._p(handles), 0, C.byref(S["out"])) + ((None,) if mode == "device" else ())
                        if fn(*args_) != 0:
                            raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(S["db"].h).decode())

                    def equal():
                        d, h = state["device"], state["host"]
                        nt, npt, nc = int(h["c"]["n_touched"][0]), int(h["c"]["n_points"][0]), int(h["c"]["n_culled"][0])
                        ok = all(d["c"][k].tobytes() == h["c"][k].tobytes() for k in ("record", "Tcp", "has_Tcp", "n_culled", "n_touched", "n_points"))
                        for k, m in (("culled", nc), ("touched", nt), ("flags", nt), ("children_offsets", nt + 1), ("nulled_offsets", nt + 1),
                                     ("points", npt), ("point_n_obs", npt), ("point_bad", npt), ("obs_offsets", npt + 1),
                                     ("obs", h["c"]["obs_offsets"][npt]), ("obs_index", h["c"]["obs_offsets"][npt]),
                                     ("children", h["c"]["children_offsets"][nt]), ("nulled", h["c"]["nulled_offsets"][nt])):
                            ok = ok and d["c"][k][:m].tobytes() == h["c"][k][:m].tobytes()
                        for k, m in (("parent", nt), ("weight_offsets", nt + 1), ("ordered_offsets", nt + 1)):
                            ok = ok and d["r"][k][:m].tobytes() == h["r"][k][:m].tobytes()
                        return ok, nc, npt

                    if tenth:
                        times = {"device": [], "host": []}
                        for rep in range(args.cull_reps + 1):
                            refill()
                            for mode in dbs:
                                call(mode, warm[mode], stay)            # the image again, and on the device
                                t = time.perf_counter()
                                call(mode)
                                if rep:                                  # the first pair is the warm-up
                                    times[mode].append(time.perf_counter() - t)
                            same, nc, npt = equal()
                            assert same, (n_kf, n, "culled")
                        (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = quartiles(times["device"]), quartiles(times["host"])
                        refill()
                    else:
                        call("device")
                        call("host")
                        same, nc, npt = equal()
                        assert same and nc == 0, (n_kf, n)
                        (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = timed_pair_quartiles(
                            lambda: call("device"), lambda: call("host"), args.seconds, args.max_reps)
                        same = same and equal()[0]
                    dm, diqr, hm, hiqr = round(dm, 4), round(diqr, 4), round(hm, 4), round(hiqr, 4)      # the file's digits decide
                    row = dict(keyframes=n_kf, points=g["n_mp"], called=asked, named=n, culled_tenth=tenth, culled=nc, touched_points=npt,
                               row_entries=n_rows, device_ms=dm, device_iqr_ms=diqr, device_spread_ms=round(dspread, 4), device_reps=dreps,
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
