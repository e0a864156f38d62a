"""Per-call time of KeyFrame::UpdateConnections' device entry (drfe_lmap_connect_device) next to its host entry
(drfe_lmap_connect_host, one CPU thread: the baseline, since the entry is new) on the same store: the graphs of
tools/lmap_timing.py - 100, 1000 and 4000 key frames of about 1000 map points each, every point observed by 8 key frames drawn
from a window of 64 consecutive ones, so a key frame's counter has about 64 entries and most of them pass the threshold - and calls
of 1, 4, 16, 64 and 256 distinct key frames drawn at random (a store of 100 key frames gives a call at most 100; the row keeps
the size asked for under "called" and the size run under "named").
Two stores with the same content take the same calls in turn, one created with a context and one without.  The clock is around
the C entry alone, output arrays allocated once; a device call returns with the rows in host memory and committed, so wall time
is its cost, all copies included.  Each call commits, so the next one sends the graph block of the image again (parents,
neighbours, children, connection rows; not the match rows): that is in the device's time, as it is for a caller.  After the
first call of a shape the store holds the call's own result, so every later call meets its own weights (no AddConnection
changes anything); the vote, the edges and the rows are computed in full all the same.  Every timed shape is called once before
it is timed; the two entries are then called in turn until each has at least --seconds (default 0.5) of timed calls and at least
five; the row holds the median, the interquartile range and the spread (max - min) of both.  The device entry wins a row when the
host's median exceeds its median by more than the larger of the two interquartile ranges.  Device == host is checked on every
shape's first and last call.  Prints one JSON line per shape, then device_from: the smallest call size from which the device
entry wins at every measured store size (null: at none), and writes them to --out (profiles/conn_timing.jsonl)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--called", type=int, nargs="*", default=[1, 4, 16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conn_timing.jsonl"))
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
                db.set_connections([dict(handle=h, first=1) for h in range(1, n_kf)])
            order = np.random.default_rng(n_kf + 2).permutation(n_kf).astype(np.int32)
            for asked in args.called:
                n = min(asked, n_kf)
                hs = np.ascontiguousarray(order[:n])
                cc, ct, cw = n * (n_kf - 1), n_kf, min(n_kf * (n_kf - 1), (n + 2) * 64 * 130 + 4096)
                state = {}
                for mode in ("device", "host"):
                    r, conn_rows = lib.LocalMap._conn_rows(ct, cw, cw)
                    c = {"counter_offsets": np.zeros(n + 1, np.int32), "counter_kfs": np.zeros(cc, np.int32),
                         "counter_votes": np.zeros(cc, np.int32), "record": np.zeros((n, 4), np.int32), "new_parent": np.zeros(n, np.int32),
                         "n_touched": np.zeros(1, np.int32), "touched": np.zeros(ct, np.int32), "flags": np.zeros(ct, np.uint8)}
                    out = lib.LmapConnectOut(cc, ct, lib._p(c["counter_offsets"]), lib._p(c["counter_kfs"]), lib._p(c["counter_votes"]),
                                             lib._p(c["record"]), lib._p(c["new_parent"]), lib._p(c["n_touched"]), lib._p(c["touched"]),
                                             conn_rows, lib._p(c["flags"]))
                    state[mode] = dict(out=out, r=r, c=c, db=dbs[mode])

                def call(mode):
                    S = state[mode]
                    fn = getattr(L, f"drfe_lmap_connect_{mode}")
                    a = (S["db"].h, n, lib._p(hs), C.byref(S["out"])) + ((None,) if mode == "device" else ())
                    if fn(*a) != 0:
                        raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(S["db"].h).decode())

                def equal():
                    d, h = state["device"], state["host"]
                    nt = int(h["c"]["n_touched"][0])
                    used = {"counter_kfs": h["c"]["counter_offsets"][n], "counter_votes": h["c"]["counter_offsets"][n], "touched": nt,
                            "flags": nt, "weight_offsets": nt + 1, "ordered_offsets": nt + 1, "parent": nt, "first_connection": nt,
                            "weight_kfs": h["r"]["weight_offsets"][nt], "weight_w": h["r"]["weight_offsets"][nt],
                            "ordered_kfs": h["r"]["ordered_offsets"][nt], "ordered_w": h["r"]["ordered_offsets"][nt]}
                    return all(d[w][k][:used.get(k, len(d[w][k]))].tobytes() == h[w][k][:used.get(k, len(h[w][k]))].tobytes()
                               for w in ("c", "r") for k in d[w]), nt, used
                call("device")
                call("host")
                first_equal, nt, used = equal()
                assert first_equal, (n_kf, n)
                changed_first = int((state["host"]["c"]["flags"][:nt] != 0).sum())
                (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = timed_pair_quartiles(
                    lambda: call("device"), lambda: call("host"), args.seconds, args.max_reps)
                last_equal, nt, used = equal()
                assert last_equal, (n_kf, n)
                dm, diqr, hm, hiqr = round(dm, 4), round(diqr, 4), round(hm, 4), round(hiqr, 4)      # the file's digits decide
                row = dict(keyframes=n_kf, points=g["n_mp"], called=asked, named=n, touched=nt,
                           counter_per_called=round(float(used["counter_kfs"]) / n, 1), weights=int(used["weight_kfs"]),
                           changed_rows_first_call=changed_first, device_ms=round(dm, 4), device_iqr_ms=round(diqr, 4),
                           device_spread_ms=round(dspread, 4), device_reps=dreps, host_ms=round(hm, 4), host_iqr_ms=round(hiqr, 4),
                           host_spread_ms=round(hspread, 4), host_reps=hreps, speedup=round(hm / dm, 2), equal=bool(first_equal and last_equal),
                           device_wins=bool(hm - dm > max(diqr, hiqr)))
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
