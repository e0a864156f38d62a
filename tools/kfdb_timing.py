"""Per-call time of KeyFrameDatabase's device entries (drfe_kfdb_reloc_queries_device, drfe_kfdb_loop_queries_device) next to
their host entries (one CPU thread) on the same database and queries: 100, 1000 and 4000 visible key frames of about 250 words
each (a walk over places in a vocabulary of 50 000 words, every key frame with up to ten neighbours), 1, 2, 4, 8, 16, 64 and 200
queries a call.
Two databases with the same content take the same calls in turn, one created with a context and one without.  The clock is around
the C entry alone (the query arrays are packed once; only the ids are raised between calls, as the entries require); a device call
returns with the candidates in host memory, so wall time is its cost, both copies included.  The database image is on the device
before the clock starts (the first call sends it).  Every timed shape is called once before it is timed; the two entries are then
called in turn until each has at least --seconds (default 0.5) of timed calls and at least five; the row holds the median, the
interquartile range and the spread (max - min) of both.  The device entry wins a row when the host's median exceeds its median
by more than the larger of the two interquartile ranges (max - min of hundreds of calls on a shared host is its worst outlier).  Device == host is checked on every shape's first call.  The reference's own class cannot be built
next to this library, so the table compares this library's two entries only.  Prints one JSON line per configuration, then
device_from: the smallest query count from which the device entry wins at every measured database size and kind, and writes them
to --out (profiles/kfdb_timing.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PLACES = 200


def timed_pair_quartiles(fa, fb, seconds, max_reps):
    """pose_opt_timing.timed_pair's schedule (a b a b .., each called once before the clock starts), returning per function
    (median, interquartile range, max - min, calls), in ms"""
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


def make_vectors(rng, n):
    places = [np.sort(rng.choice(np.arange(p * 240, p * 240 + 1200), size=300, replace=False)) for p in range(N_PLACES)]
    out = []
    for i in range(n):
        ids = places[(i // 5) % N_PLACES]
        ids = ids[rng.random(len(ids)) < 0.85]
        w = rng.random(len(ids)) + 0.2
        out.append((ids.astype(np.int32), w / w.sum()))
    return out


def fill(db, vectors, rng):
    handles = np.arange(len(vectors), dtype=np.int32)
    for h, (ids, vals) in zip(handles, vectors):
        db.put(int(h), ids, vals)
        db.add(int(h))
    rows = [[int(x) for x in np.clip(h + rng.integers(-12, 13, size=10), 0, len(vectors) - 1) if x != h] for h in handles]
    db.set_neighbours(handles, rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 2, 4, 8, 16, 64, 200])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    rows = []
    wins = {}
    try:
        for n_kf in args.keyframes:
            vectors = make_vectors(np.random.default_rng(n_kf), n_kf + max(args.queries))
            stored, lost = vectors[:n_kf], vectors[n_kf:]
            dbs = {}
            next_id = {(m, k): 1 for m in ("device", "host") for k in ("reloc", "loop")}
            for mode in ("device", "host"):
                dbs[mode] = lib.KeyFrameDatabase(ctx if mode == "device" else None)
                fill(dbs[mode], stored, np.random.default_rng(1))
                for k, (ids, vals) in enumerate(lost):               # the loop queries' key frames: stored, never added
                    dbs[mode].put(n_kf + k, ids, vals)
            for kind in ("reloc", "loop"):
                for n in args.queries:
                    cap = n * n_kf
                    state = {}
                    for mode in ("device", "host"):
                        ident = np.arange(1, n + 1, dtype=np.int64)
                        off, ids = lib._csr_i32([v[0] for v in lost[:n]])
                        vals = np.ascontiguousarray(np.concatenate([v[1] for v in lost[:n]]), np.float64)
                        handle = np.arange(n_kf, n_kf + n, dtype=np.int32)
                        zero = np.zeros(n + 1, np.int32)
                        ms = np.full(n, 0.05, np.float32)
                        r = {"cand_offsets": np.zeros(n + 1, np.int32), "candidates": np.zeros(cap, np.int32),
                             "record": np.zeros((n, 4), np.int32), "min_score": np.zeros(n, np.float32),
                             "uninit_reads": np.zeros(n, np.int32)}
                        out = lib.KfdbOut(cap, 0, *[lib._p(r[k]) for k in ("cand_offsets", "candidates", "record", "min_score",
                                                                           "uninit_reads")])
                        if kind == "reloc":
                            Q = lib.KfdbRelocQueries(n, 0, lib._p(ident), lib._p(off), lib._p(ids), lib._p(vals))
                        else:
                            Q = lib.KfdbLoopQueries(n, 0, lib._p(handle), lib._p(ident), lib._p(zero), None, lib._p(ms), None, None,
                                                    None)
                        state[mode] = dict(Q=Q, out=out, r=r, ident=ident, keep=(off, ids, vals, handle, zero, ms), db=dbs[mode])

                    def call(mode):
                        S = state[mode]
                        S["ident"][:] = next_id[mode, kind] + np.arange(n)      # above every id this database has seen
                        next_id[mode, kind] += n
                        fn = getattr(L, f"drfe_kfdb_{kind}_queries_{mode}")
                        a = (S["db"].h, C.byref(S["Q"]), C.byref(S["out"])) + ((None,) if mode == "device" else ())
                        if fn(*a) != 0:
                            raise RuntimeError(f"{kind} {mode}: " + L.drfe_kfdb_last_error(S["db"].h).decode())
                    call("device")
                    call("host")
                    d, h = state["device"]["r"], state["host"]["r"]
                    equal = all(d[k].tobytes() == h[k].tobytes() for k in d)
                    assert equal, (kind, n_kf, n)
                    (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = timed_pair_quartiles(
                        lambda: call("device"), lambda: call("host"), args.seconds, args.max_reps)
                    row = dict(kind=kind, keyframes=n_kf, queries=n, candidates=int(h["cand_offsets"][n]),
                               device_ms=round(dm, 4), device_iqr_ms=round(diqr, 4), device_spread_ms=round(dspread, 4),
                               device_reps=dreps, host_ms=round(hm, 4), host_iqr_ms=round(hiqr, 4),
                               host_spread_ms=round(hspread, 4), host_reps=hreps, speedup=round(hm / dm, 2), equal=equal,
                               device_wins=bool(hm - dm > max(diqr, hiqr)))
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
