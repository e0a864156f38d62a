"""Per-call time of the fuse commit's device entry (drfe_lmap_fuse_device) next to its host entry (drfe_lmap_fuse_host, one CPU
thread) and next to what a caller that keeps a store has to do for the same fusion without this operation: the graphs of
tools/lmap_timing.py at 100, 400 and 1600 key frames of about 1000 map points each, every point observed by 8 key frames.

Two call shapes.  "neighbours" is SearchInNeighbors': 20 NEIGHBOURS steps of 1000 candidates on 20 key frames plus one of 10000
(31 000 candidates).  "loop" is SearchAndFuse's: 30 LOOP steps of 4000 (120 000 candidates).  A twentieth, then a fifth, of
the candidates carry an answer of the search; the rest have best_idx -1.  Of the answered candidates of a NEIGHBOURS step a
third is sent to an empty entry of the row (an addition, while the row has empty entries left: a row has about a hundred), a
third has nObs 7 and is sent to an occupant with 8 (the candidate is replaced), a third has 8 and meets an occupant it ties
with or beats (the occupant is replaced); in a LOOP step an occupant that is not bad is always replaced.  Candidates are
drawn at random, so a few already observe the key frame and are skipped: every row reports the actions actually taken.

Three columns, wall time of the C entry, output arrays allocated once and at the bounds that always suffice (so the device entry
never pre-walks on the host).  A call changes the store, so both stores are filled again before every timed call and one untimed
call without an answer rebuilds the image and sends it to the device, as a caller with a resident store meets it; every shape
gets --reps timed calls (default 5) after one warm-up.  "baseline" is the third column: on a resident store the caller runs the
fusion on its objects and then pushes every touched key frame through drfe_lmap_set_keyframes and every touched point through
drfe_lmap_set_points, _set_cull_attributes and _set_recent_attributes (arrays packed beforehand, not timed), and the next
device call (an update of one small frame) pays the rebuild of the image and its upload; the time of that small update on an
unchanged store is subtracted.  Medians with the interquartile range.  The device entry wins a row when the host's median exceeds
its median by more than the larger of the two interquartile ranges.  Device == host is checked on every shape.  Prints one JSON
line per shape, then device_from: the smallest number of candidates per call from which the device entry wins at every measured
store size in both answered shares (null: at none), and writes them to --out (profiles/fuse_timing.jsonl)."""
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

from lmap_timing import fill, make_graph  # noqa: E402
from recent_cull_timing import attributes, quartiles, set_attributes  # noqa: E402

POINT = 1
SHAPES = {"neighbours": [(0, 1000)] * 20 + [(0, 10000)], "loop": [(1, 4000)] * 30}
CALL_FIELDS = ("n_replaced", "replaced_kind", "loser", "winner", "record_offsets", "record_kf", "record_index", "record_moved",
               "n_touched", "touched_points", "touched_lines")


def with_keyframe_attributes(g, cull, rng):
    """the key-frame part of drfe_lmap_set_cull_attributes (the fuse commit reads the stereo flags), and nObs 7 for even points"""
    n = len(g["rows"])
    cull = dict(cull, kf_handle=g["handle"], th_depth=np.full(g["n_kf"], 40.0, np.float32), kf_flags=np.zeros(g["n_kf"], np.uint8),
                row_offsets=g["pt_off"], octave=np.zeros(n, np.int32), depth=np.ones(n, np.float32),
                stereo=(rng.random(n) < 0.5).astype(np.uint8))
    cull["n_obs"] = np.where(g["mp_handle"] % 2 == 0, 7, 8).astype(np.int32)
    return cull


def make_steps(rng, g, shape, share):
    steps = []
    kfs = rng.choice(g["n_kf"], len(SHAPES[shape]), replace=False)
    for (form, n), kf in zip(SHAPES[shape], kfs):
        row = g["rows"][g["pt_off"][kf]:g["pt_off"][kf + 1]]
        empty, odd = np.flatnonzero(row < 0), np.flatnonzero((row >= 0) & (row % 2 == 1))
        full = np.flatnonzero(row >= 0)
        cand = rng.integers(0, g["n_mp"], n).astype(np.int32)
        best = np.full(n, -1, np.int32)
        answered = rng.choice(n, max(1, int(n * share)), replace=False)
        for j, i in enumerate(answered):
            if j % 3 == 0:
                best[i] = empty[(j // 3) % len(empty)] if len(empty) else full[j % len(full)]
            elif j % 3 == 1:
                cand[i] -= cand[i] % 2                                   # nObs 7 against an occupant with 8
                best[i] = odd[rng.integers(len(odd))]
            else:
                cand[i] |= 1
                best[i] = full[rng.integers(len(full))]
        steps.append(dict(keyframe=int(kf), kind=POINT, form=form, candidates=np.minimum(cand, g["n_mp"] - 1), best_idx=best))
    return steps


def pack(lib, steps, n_kf):
    """the drfe_lmap_fuse_call of the steps with arrays at the bounds that always suffice"""
    S = (lib.LmapFuseStep * len(steps))()
    keep, live = [], 0
    for i, st in enumerate(steps):
        m = len(st["candidates"])
        a = dict(action=np.zeros(m, np.uint8), n_fused=np.zeros(1, np.int32), replace=np.zeros(m, np.int32))
        keep.append(a)
        live += int(np.count_nonzero(st["best_idx"] >= 0))
        S[i] = lib.LmapFuseStep(st["keyframe"], st["kind"], st["form"], m, lib._p(st["candidates"]), lib._p(st["best_idx"]),
                                lib._p(a["action"]), lib._p(a["n_fused"]), lib._p(a["replace"]))
    rec = live * n_kf
    r = {"n_replaced": np.zeros(1, np.int32), "replaced_kind": np.zeros(live, np.int32), "loser": np.zeros(live, np.int32),
         "winner": np.zeros(live, np.int32), "record_offsets": np.zeros(live + 1, np.int32), "record_kf": np.zeros(rec, np.int32),
         "record_index": np.zeros(rec, np.int32), "record_moved": np.zeros(rec, np.uint8), "n_touched": np.zeros(2, np.int32),
         "touched_points": np.zeros(live, np.int32), "touched_lines": np.zeros(live, np.int32)}
    call = lib.LmapFuseCall(len(steps), C.cast(S, C.c_void_p), live, rec, live, *[lib._p(r[k]) for k in CALL_FIELDS])
    return dict(call=call, S=S, keep=keep, r=r, live=live)


def baseline_arrays(lib, g, db, P, steps, cull, recent):
    """what the caller pushes back after the fusion P left in db: the rows of every touched key frame, and the observations,
    attributes and counters of every touched point, packed for the four setters"""
    r = P["r"]
    n_rep = int(r["n_replaced"][0])
    n_rec = int(r["record_offsets"][n_rep])
    kfs = np.unique(np.concatenate([[s["keyframe"] for s in steps], r["record_kf"][:n_rec]])).astype(np.int32)
    acted = [s["candidates"][a["action"] >= 2] for s, a in zip(steps, P["keep"])]
    pts = np.unique(np.concatenate(acted + [r["loser"][:n_rep], r["winner"][:n_rep]])).astype(np.int32)
    rows = [db.get_match_row(POINT, int(k)) for k in kfs]
    lrows = [g["lines"][g["ln_off"][k]:g["ln_off"][k + 1]] for k in kfs]
    csr = lambda parts: (np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int32),  # noqa: E731
                         np.ascontiguousarray(np.concatenate(parts) if parts else [], np.int32))
    poff, pflat = csr(rows)
    loff, lflat = csr(lrows)
    coff, cflat = csr([g["children"][g["child_off"][k]:g["child_off"][k + 1]] for k in kfs])
    K = dict(handle=kfs, rank=np.ascontiguousarray(g["rank"][kfs]), bad=np.ascontiguousarray(g["kf_bad"][kfs]),
             parent=np.ascontiguousarray(g["parent"][kfs]), nbr=np.ascontiguousarray(g["nbr"][kfs]), coff=coff, children=cflat,
             poff=poff, points=pflat, loff=loff, lines=lflat)
    obs = [db.get_observers(POINT, int(p)) for p in pts]
    ooff, oflat = csr([o[1] for o in obs])
    ca = db.get_cull_attributes(point_handles=pts)["points"]
    _, iflat = csr([c["obs_index"] for c in ca])
    ra = db.get_recent_attributes(point_handles=pts)["points"]
    Pn = dict(handle=pts, bad=np.array([o[0] for o in obs], np.uint8), ooff=ooff, obs=oflat,
              n_obs=np.array([c["n_obs"] for c in ca], np.int32), idx=iflat, found=np.array([x["found"] for x in ra], np.int32),
              visible=np.array([x["visible"] for x in ra], np.int32), first=np.array([x["first_kf"] for x in ra], np.int64))
    p = lib._p
    Ks = lib.LmapKeyframes(len(kfs), 0, p(K["handle"]), p(K["rank"]), p(K["bad"]), p(K["parent"]), p(K["nbr"]), p(K["coff"]), p(K["children"]),
                           p(K["poff"]), p(K["points"]), p(K["loff"]), p(K["lines"]))
    z32, zf, z8 = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.uint8)
    As = lib.LmapCullAttributes(0, len(pts), p(z32), p(zf), p(z8), p(z32), p(z32), p(zf), p(z8), p(Pn["handle"]), p(Pn["n_obs"]), p(Pn["ooff"]), p(Pn["idx"]))
    Rs = lib.LmapRecentAttributes(len(pts), 0, p(Pn["handle"]), p(Pn["found"]), p(Pn["visible"]), p(Pn["first"]), *([None] * 8))
    return dict(K=K, P=Pn, Ks=Ks, As=As, Rs=Rs, keep=(z32, zf, z8), n_kfs=len(kfs), n_points=len(pts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 400, 1600])
    ap.add_argument("--host-only", action="store_true", help="no GPU: the device column runs the host entry too; for trying the tool out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_timing.jsonl"))
    args = ap.parse_args()
    from dr_slam_amd import lib
    ctx = None if args.host_only else lib.Context(max_batch=1)   # fails without a GPU: there is no other way to measure the device
    entry = {"device": "host" if args.host_only else "device", "host": "host"}
    L = lib.load()
    rows, wins = [], {}
    frame_id = iter(range(1, 1 << 30))
    for n_kf in args.keyframes:
        g = make_graph(np.random.default_rng(n_kf), n_kf)
        g["kf_bad"][:] = 0
        g["mp_bad"][:] = 0
        cull, recent = attributes(g)
        cull = with_keyframe_attributes(g, cull, np.random.default_rng(n_kf + 1))
        dbs = {"device": lib.LocalMap(ctx), "host": lib.LocalMap(), "baseline": lib.LocalMap(ctx)}
        small = [dict(frame_id=0, points=g["rows"][:64])]

        def refill(names):
            for m in names:
                fill(lib, L, dbs[m], g)
                p = lib._p
                A = lib.LmapCullAttributes(g["n_kf"], g["n_mp"], *[p(cull[k]) for k in lib.LMAP_CULL_ATTR_FIELDS])
                dbs[m]._chk(L.drfe_lmap_set_cull_attributes(dbs[m].h, C.byref(A)), "set_cull_attributes")
                set_attributes(lib, L, dbs[m], dict(cull, point_handle=np.zeros(0, np.int32)), recent)

        def small_update(db):
            small[0]["frame_id"] = next(frame_id)
            t = time.perf_counter()
            db.update(small, mode=entry["device"])
            return time.perf_counter() - t

        for shape in SHAPES:
            for share in (0.05, 0.2):
                steps = make_steps(np.random.default_rng(n_kf * 7 + int(share * 100)), g, shape, share)
                n_cand = sum(len(s["candidates"]) for s in steps)
                warm_steps = [dict(keyframe=0, kind=POINT, form=0, candidates=np.zeros(1, np.int32), best_idx=np.full(1, -1, np.int32))]
                packed = {m: pack(lib, steps, n_kf) for m in ("device", "host")}
                warm = {m: pack(lib, warm_steps, n_kf) for m in ("device", "host")}

                def call(mode, P):
                    fn = getattr(L, f"drfe_lmap_fuse_{entry[mode]}")
                    a = (dbs[mode].h, C.byref(P["call"])) + ((None,) if entry[mode] == "device" else ())
                    t = time.perf_counter()
                    rc = fn(*a)
                    dt = time.perf_counter() - t
                    if rc != 0:
                        raise RuntimeError(f"{mode}: " + L.drfe_lmap_last_error(dbs[mode].h).decode())
                    return dt

                times = {"device": [], "host": [], "baseline": []}
                same, handed = True, 0
                for rep in range(args.reps + 1):
                    refill(("device", "host", "baseline"))
                    before = dbs["device"].fuse_stats()["handed_back"]
                    for mode in ("device", "host"):
                        call(mode, warm[mode])                          # the image again, and on the device
                        dt = call(mode, packed[mode])
                        if rep:                                          # the first round is the warm-up
                            times[mode].append(dt)
                    handed = dbs["device"].fuse_stats()["handed_back"] - before
                    d, h = packed["device"], packed["host"]
                    n_rep = int(h["r"]["n_replaced"][0])
                    n_rec = int(h["r"]["record_offsets"][n_rep])
                    same = same and all(x["action"].tobytes() == y["action"].tobytes() for x, y in zip(d["keep"], h["keep"]))
                    same = same and int(d["r"]["n_replaced"][0]) == n_rep and all(
                        d["r"][k][:m].tobytes() == h["r"][k][:m].tobytes() for k, m in (("loser", n_rep), ("winner", n_rep), ("record_kf", n_rec),
                                                                                      ("record_index", n_rec), ("record_moved", n_rec)))
                    # the third column: the same fusion pushed back through the setters of a resident store
                    B = baseline_arrays(lib, g, dbs["host"], h, steps, cull, recent)
                    db = dbs["baseline"]
                    small_update(db)
                    idle = small_update(db)
                    t = time.perf_counter()
                    rc = L.drfe_lmap_set_keyframes(db.h, C.byref(B["Ks"]))
                    rc |= L.drfe_lmap_set_points(db.h, B["n_points"], lib._p(B["P"]["handle"]), lib._p(B["P"]["bad"]), lib._p(B["P"]["ooff"]), lib._p(B["P"]["obs"]))
                    rc |= L.drfe_lmap_set_cull_attributes(db.h, C.byref(B["As"]))
                    rc |= L.drfe_lmap_set_recent_attributes(db.h, C.byref(B["Rs"]))
                    dt = time.perf_counter() - t
                    if rc != 0:
                        raise RuntimeError("baseline: " + L.drfe_lmap_last_error(db.h).decode())
                    dt += small_update(db) - idle
                    if rep:
                        times["baseline"].append(dt)
                actions = np.concatenate([a["action"] for a in packed["host"]["keep"]])
                q = {m: quartiles(times[m]) for m in times}
                dm, diqr, hm, hiqr, bm, biqr = (round(v, 4) for v in (q["device"][0], q["device"][1], q["host"][0], q["host"][1],
                                                                      q["baseline"][0], q["baseline"][1]))
                row = dict(keyframes=n_kf, points=g["n_mp"], shape=shape, candidates=n_cand, answered_share=share, live=packed["host"]["live"],
                           added=int(np.count_nonzero((actions == 2) | (actions == 3))), skipped=int(np.count_nonzero(actions == 1)),
                           candidate_replaced=int(np.count_nonzero(actions == 5)), occupant_replaced=int(np.count_nonzero(actions == 6)),
                           recorded=int(np.count_nonzero(actions == 8)), replaced=int(packed["host"]["r"]["n_replaced"][0]),
                           touched_kfs=B["n_kfs"], touched_points=B["n_points"], handed_back=int(handed), reps=args.reps,
                           device_ms=dm, device_iqr_ms=diqr, host_ms=hm, host_iqr_ms=hiqr, baseline_ms=bm, baseline_iqr_ms=biqr,
                           host_over_device=round(hm / dm, 3), baseline_over_host=round(bm / hm, 2), baseline_over_device=round(bm / dm, 2),
                           equal=bool(same), device_wins=bool(hm - dm > max(diqr, hiqr)))
                print(json.dumps(row), flush=True)
                rows.append(row)
                wins.setdefault(n_cand, []).append(row["device_wins"])
        for db in dbs.values():
            db.close()
    device_from = None
    for n in sorted(wins, reverse=True):
        if not all(wins[n]):
            break
        device_from = n
    last = dict(device_from=device_from, rule="the smallest number of candidates per call from which the device entry wins at every "
                "measured store size in both answered shares; null: at none")
    print(json.dumps(last), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows + [last]:
            f.write(json.dumps(r) + "\n")
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()
