"""Per-call time of the device entries of what surrounds the solver of Optimizer::OptimizeEssentialGraph
(drfe_lmap_essential_edges_device, drfe_lmap_essential_commit_device) next to their host entries (one CPU thread: the only baseline
there is, since the entries are new) on the same store: the graphs of tools/lmap_timing.py - 100, 1000 and 4000 key frames of
about 1000 map points each, that is 12 500, 125 000 and 500 000 points - with the geometry of tools/loop_correct_timing.py, a
spanning tree that steps over the bad key frames, connection rows to the sixteen nearest key frames with weights on both sides of
100, and a loop edge at every fiftieth key frame.  A call closes a loop between key frame 0 and the newest one; its loop
connections tie the twenty newest key frames to the twenty oldest.
Three mixes per call.  Edges: no Sim3 table; a table of the twenty newest key frames; the same after drfe_lmap_set_poses of twenty
key frames (the geometry block goes up again).  Commit: every point through its reference key frame; a third of the points stamped
by the current key frame; the first after drfe_lmap_set_poses of twenty key frames.  Two stores with the same content take the
same calls in turn, one created with a context and one without; the clock is around the setters that precede a call
(drfe_lmap_set_loop_edges of the two ends of the last loop, and the pose edit where the mix has one) and the entry together, on
both sides, and a device call returns with its records in host memory and committed.  Every shape is called once before it is
timed; the two entries are then called in turn until each has at least --seconds (default 0.5) of timed calls and at least five;
the row holds the median, the interquartile range and the spread of both.  The device entry wins a row when the host's median
exceeds its median by more than the larger of the two interquartile ranges.  Device == host is checked on every shape's first
call and on one more call after both stores were given the same poses and positions anew.  Prints one JSON line per shape,
then edges_device_from (stored key frames) and commit_device_from (stored points): the smallest measured shape from which the
device entry wins at every mix and at every larger measured shape (null: at none), and writes them to --out
(profiles/essential_timing.jsonl)."""
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

EDGE_MIXES = ("no_table", "table_of_20", "table_of_20_after_pose_edit")
COMMIT_MIXES = ("by_reference", "a_third_by_cur", "by_reference_after_pose_edit")
NEAR = 16


def spanning_tree(g):
    """the parent of key frame k is the nearest earlier one that is not bad; key frame 0 is not bad"""
    n = g["n_kf"]
    g["kf_bad"][0] = 0
    parent = np.full(n, -1, np.int32)
    last = 0
    for k in range(1, n):
        parent[k] = last
        if not g["kf_bad"][k]:
            last = k
    order = np.argsort(parent[1:], kind="stable") + 1
    g["parent"] = parent
    g["children"] = order.astype(np.int32)
    g["child_off"] = np.concatenate([[0], np.cumsum(np.bincount(parent[1:], minlength=n))]).astype(np.int32)


def connection_rows(rng, n):
    rows = []
    for k in range(n):
        near = [o for o in range(k - NEAR // 2, k + NEAR // 2 + 1) if 0 <= o < n and o != k]
        w = sorted(((int(170 - 18 * abs(o - k) + rng.integers(0, 30)), o) for o in near), reverse=True)
        rows.append(dict(handle=k, first=0, weights=[(o, x) for x, o in w], ordered=[(o, x) for x, o in w]))
    return rows


def small_sim3(rng, n):
    S = np.zeros((n, 8))
    S[:, :3] = rng.normal(0, 0.01, (n, 3))
    S[:, 3] = 1.0
    S[:, 4:7] = rng.normal(0, 0.05, (n, 3))
    S[:, 7] = 1.0 + rng.normal(0, 0.01, n)
    return S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-reps", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    p = lib._p
    rows, wins = [], {"edges": {}, "commit": {}}
    try:
        for n_kf in args.keyframes:
            g = make_graph(np.random.default_rng(n_kf), n_kf)
            spanning_tree(g)
            geo = make_geometry(np.random.default_rng(n_kf + 1), g)
            rng = np.random.default_rng(n_kf + 2)
            conns = connection_rows(rng, n_kf)
            good = np.flatnonzero(g["kf_bad"] == 0).astype(np.int32)
            cur, loop = int(good[-1]), 0
            newest, oldest = good[-20:], good[:20]
            loop_rows = [(int(k), [int(k) - 50]) for k in good if k >= 50 and k % 50 == 0 and not g["kf_bad"][k - 50]]
            last_loop = [(cur, [loop]), (loop, [cur])]
            lc_h = np.ascontiguousarray(newest)
            lc_off = (np.arange(len(newest) + 1) * len(oldest)).astype(np.int32)
            lc_kfs = np.ascontiguousarray(np.tile(oldest, len(newest)))
            tab_h = np.ascontiguousarray(newest)
            tab_c, tab_n = small_sim3(rng, len(newest)), small_sim3(rng, len(newest))
            edit_h = np.ascontiguousarray(newest)
            edit_T = random_poses(rng, len(newest)).reshape(len(newest), 16)
            by_cur = np.where(np.arange(g["n_mp"]) % 3 == 0, cur, 0).astype(np.int32)
            by_ref = np.ascontiguousarray(geo["ref"]).astype(np.int32)
            n_good = len(good)
            bound = 0
            dbs = {"device": lib.LocalMap(ctx), "host": lib.LocalMap()}
            state = {}
            for mode, db in dbs.items():
                fill(lib, L, db, g)
                fill_geometry(lib, L, db, g, geo)
                db.set_connections(conns)
                db.set_loop_edges(loop_rows)
                bound = db.essential_scratch(len(lc_kfs))["edge_bound"] + 2
                e = {"n_vertices": np.zeros(1, np.int32), "vertices": np.zeros(n_kf, np.int32), "Scw": np.zeros((n_kf, 8)),
                     "fixed": np.zeros(n_kf, np.uint8), "n_edges": np.zeros(1, np.int32), "from": np.zeros(bound, np.int32),
                     "to": np.zeros(bound, np.int32), "measurement": np.zeros((bound, 8)), "kind": np.zeros(bound, np.uint8)}
                c = {"Tiw": np.zeros((n_kf, 16), np.float32), "Swc": np.zeros((n_kf, 8)), "n_points": np.zeros(1, np.int32),
                     "points": np.zeros(g["n_mp"], np.int32), "ref": np.zeros(g["n_mp"], np.int32),
                     "world": np.zeros((g["n_mp"], 3), np.float32), "normal": np.zeros((g["n_mp"], 3), np.float32),
                     "max_distance": np.zeros(g["n_mp"], np.float32), "min_distance": np.zeros(g["n_mp"], np.float32),
                     "status": np.zeros(g["n_mp"], np.uint8)}
                state[mode] = dict(db=db, e=e, c=c)

            def setters(S, edit):
                S["db"].set_loop_edges(last_loop)
                if edit:
                    S["db"]._chk(L.drfe_lmap_set_poses(S["db"].h, len(edit_h), p(edit_h), p(edit_T)), "set_poses")

            def edges_call(mode, mix):
                S = state[mode]
                setters(S, mix.endswith("pose_edit"))
                nt = 0 if mix == "no_table" else len(tab_h)
                call = lib.LmapEssentialEdgesCall(loop, cur, nt, len(lc_h), p(tab_h) if nt else None, p(tab_c) if nt else None,
                                                  p(tab_n) if nt else None, p(lc_h), p(lc_off), p(lc_kfs), n_kf, bound,
                                                  *[p(S["e"][k]) for k in lib.LMAP_ESSENTIAL_EDGES_OUT])
                fn = getattr(L, f"drfe_lmap_essential_edges_{mode}")
                if fn(*((S["db"].h, C.byref(call)) + ((None,) if mode == "device" else ()))) != 0:
                    raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(S["db"].h).decode())

            def commit_call(mode, mix):
                S = state[mode]
                setters(S, mix.endswith("pose_edit"))
                e = S["e"]
                nv = int(e["n_vertices"][0])
                opt = e["Scw"][:nv] * nudge[:nv]
                call = lib.LmapEssentialCommitCall(cur, nv, p(e["vertices"]), p(e["Scw"]), p(opt), g["n_mp"], 0,
                                                   *[p(S["c"][k]) for k in lib.LMAP_ESSENTIAL_COMMIT_OUT])
                fn = getattr(L, f"drfe_lmap_essential_commit_{mode}")
                if fn(*((S["db"].h, C.byref(call)) + ((None,) if mode == "device" else ()))) != 0:
                    raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(S["db"].h).decode())

            nudge = np.ones((n_kf, 8))
            nudge[:, 4:7] = 1.001
            nudge[:, 7] = 1.0005

            def equal(which, counts, arrays):
                d, h = state["device"][which], state["host"][which]
                same = True
                for cnt, keys in zip(counts, arrays):
                    m = int(h[cnt][0]) if isinstance(cnt, str) else cnt
                    same = same and (not isinstance(cnt, str) or int(d[cnt][0]) == m)
                    for k in keys:
                        same = same and d[k][:m].tobytes() == h[k][:m].tobytes()
                return same

            def stamps(by):
                """both stores back to the same poses and positions (the two entries are timed for different numbers of calls, and
                every commit moves the map), with the stamps of the mix"""
                for S in state.values():
                    S["db"].set_poses(g["handle"], geo["poses"])
                    G = lib.LmapPointGeometry(g["n_mp"], 0, p(g["mp_handle"]), p(geo["world"]), p(geo["ref"]), p(geo["level"]), p(by), p(by_ref))
                    S["db"]._chk(L.drfe_lmap_set_point_geometry(S["db"].h, C.byref(G)), "set_point_geometry")

            for call, mixes in (("edges", EDGE_MIXES), ("commit", COMMIT_MIXES)):
                for mix in mixes:
                    def start():
                        if call == "commit":
                            stamps(by_cur if mix == "a_third_by_cur" else np.zeros(g["n_mp"], np.int32))
                            edges_call("device", "no_table")
                            edges_call("host", "no_table")
                    start()
                    fn = edges_call if call == "edges" else commit_call
                    eq = (lambda: equal("e", ("n_vertices", "n_edges"), (("vertices", "Scw", "fixed"), ("from", "to", "measurement", "kind")))) \
                        if call == "edges" else \
                        (lambda: equal("c", (n_good, "n_points"), (("Tiw", "Swc"), lib.LMAP_ESSENTIAL_COMMIT_OUT[3:])))
                    fn("device", mix)
                    fn("host", mix)
                    first_equal = eq()
                    assert first_equal, (call, n_kf, mix)
                    (dm, diqr, dspread, dreps), (hm, hiqr, hspread, hreps) = timed_pair_quartiles(
                        lambda: fn("device", mix), lambda: fn("host", mix), args.seconds, args.max_reps)
                    start()
                    fn("device", mix)
                    fn("host", mix)
                    last_equal = eq()
                    assert last_equal, (call, n_kf, mix)
                    dm, diqr, hm, hiqr = round(dm, 4), round(diqr, 4), round(hm, 4), round(hiqr, 4)      # the file's digits decide
                    R = state["host"]
                    row = dict(call=call, keyframes=n_kf, points=g["n_mp"], mix=mix, vertices=int(R["e"]["n_vertices"][0]),
                               edges=int(R["e"]["n_edges"][0]), moved=int(R["c"]["n_points"][0]), device_ms=dm, device_iqr_ms=diqr,
                               device_spread_ms=round(dspread, 4), device_reps=dreps, host_ms=hm, host_iqr_ms=hiqr,
                               host_spread_ms=round(hspread, 4), host_reps=hreps, speedup=round(hm / dm, 2),
                               equal=bool(first_equal and last_equal), device_wins=bool(hm - dm > max(diqr, hiqr)))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                    wins[call].setdefault(n_kf if call == "edges" else g["n_mp"], []).append(row["device_wins"])
            for db in dbs.values():
                db.close()
        last = {}
        for call in ("edges", "commit"):
            device_from = None
            for n in sorted(wins[call], reverse=True):
                if not all(wins[call][n]):
                    break
                device_from = n
            last[call + "_device_from"] = device_from
        rows.append(last)
        print(json.dumps(last), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
