"""Times the item loops of ProcessNewKeyFrame on the local-map store and writes
profiles/insert_timing.jsonl: per shape the device entry, the host entry and a baseline.

Shapes: stores of 100, 1 000 and 4 000 key frames with rows of 1 000 points and 100 lines (every stored item has four
observers), calls of 1, 4, 16 and 64 new key frames, a tenth and nine tenths of whose entries are ADDED (the rest are RECENT).
Every repetition calls key frames that no call has named before, so nothing is restored in between.  The timed region holds what
precedes a call in a running system: the new key frames' rows and culling attributes pushed through the setters (which makes the
image stale), then the call.  Medians of REPS repetitions after one warm-up, per entry on a store of its own.

The baseline is what the store offered before this entry for the same effect on the store: the same setters, then every touched
point and line pushed back through drfe_lmap_set_points / _set_cull_attributes / _set_recent_attributes with its new observer,
then an empty drfe_lmap_recent_cull_host, which rebuilds the images the setters made stale as the entries' own call does.  It
leaves out the drfe_map_point_upkeep_host call that the normals would need on top, so it is a lower bound on that path; like the
entries it pays the Python binding's packing of its arguments.

    python tools/insert_timing.py [--stores 100,1000,4000] [--calls 1,4,16,64] [--entries device,host,baseline]
                                  [--out profiles/insert_timing.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dr_slam_amd import lib  # noqa: E402

POINT, LINE = lib.LMAP_POINT, lib.LMAP_LINE
ROW, LROW, SEEN = 1000, 100, 4
REPS = 5


def build(K, new, share, rng):
    """the rows of a world: K stored key frames (handles 1 .. K), `new` new ones behind them"""
    bp, bl = ROW // SEEN, LROW // SEEN
    nP, nL = K * bp, K * bl
    kf_rows = {}
    pobs = [[] for _ in range(nP)]
    lobs = [[] for _ in range(nL)]
    for k in range(K):
        pr = [((k + i // bp) % K) * bp + i % bp for i in range(ROW)]
        lr = [((k + i // bl) % K) * bl + i % bl for i in range(LROW)]
        kf_rows[k + 1] = (pr, lr)
    for p in range(nP):
        b = p // bp
        pobs[p] = sorted(((b - d) % K + 1, d * bp + p % bp) for d in range(SEEN))
    for l in range(nL):
        b = l // bl
        lobs[l] = sorted(((b - d) % K + 1, d * bl + l % bl) for d in range(SEEN))
    added = {}
    for m in range(new):
        h = K + 1 + m
        pr = [int(v) for v in rng.choice(nP, ROW, replace=False)]
        lr = [int(v) for v in rng.choice(nL, LROW, replace=False)]
        kf_rows[h] = (pr, lr)
        addp = rng.random(ROW) < share
        addl = rng.random(LROW) < share
        for i, p in enumerate(pr):
            if not addp[i]:
                pobs[p].append((h, i))
        for i, l in enumerate(lr):
            if not addl[i]:
                lobs[l].append((h, i))
        added[h] = ([(p, i) for i, p in enumerate(pr) if addp[i]], [(l, i) for i, l in enumerate(lr) if addl[i]])
    return dict(K=K, new=new, kf_rows=kf_rows, pobs=pobs, lobs=lobs, added=added)


def kf_dicts(W, handles):
    return [dict(handle=h, rank=h, bad=0, points=W["kf_rows"][h][0], lines=W["kf_rows"][h][1], parent=-1 if h == 1 else 1,
                 children=[]) for h in handles]


def cull_dicts(W, handles):
    return [dict(handle=h, th_depth=40.0, flags=2 if h == 1 else 0, octave=[0] * ROW, depth=[1.0] * ROW,
                 stereo=[i % 2 for i in range(ROW)]) for h in handles]


def point_dicts(W, pts):
    obs = W["pobs"]
    return ([dict(handle=p, bad=0, obs=[k for k, _ in obs[p]]) for p in pts],
            [dict(handle=p, n_obs=len(obs[p]), obs_index=[i for _, i in obs[p]]) for p in pts],
            [dict(handle=p, found=1, visible=1, first_kf=0) for p in pts])


def line_dicts(W, lns):
    obs = W["lobs"]
    return [dict(handle=l, found=1, visible=1, first_kf=0, n_obs=len(obs[l]), obs=[k for k, _ in obs[l]],
                 obs_index=[i for _, i in obs[l]]) for l in lns]


def store_of(W, ctx):
    lm = lib.LocalMap(ctx)
    handles = sorted(W["kf_rows"])
    lm.set_keyframes(kf_dicts(W, handles))
    pts, lns = range(len(W["pobs"])), range(len(W["lobs"]))
    rows, cull, rec = point_dicts(W, pts)
    lm.set_points(rows)
    lm.set_lines(list(lns), [0] * len(lns))
    lm.set_cull_attributes(kfs=cull_dicts(W, handles), points=cull)
    lm.set_recent_attributes(points=rec, lines=line_dicts(W, lns))
    lm.set_scales([1.2 ** i for i in range(8)])
    T = np.tile(np.eye(4, dtype=np.float32), (len(handles), 1, 1))
    T[:, 0, 3] = -0.01 * np.arange(len(handles), dtype=np.float32)
    lm.set_poses(handles, T)
    bp = ROW // SEEN
    lm.set_point_geometry([dict(handle=p, world=(0.01 * (p // bp), 0.01 * (p % bp), 3.0), ref_kf=W["pobs"][p][0][0]) for p in pts])
    return lm


def one(lm, W, called, entry):
    t0 = time.perf_counter()
    lm.set_keyframes(kf_dicts(W, called))
    lm.set_cull_attributes(kfs=cull_dicts(W, called), points=[])
    if entry == "baseline":
        pts, lns = {}, {}
        for h in called:
            for p, i in W["added"][h][0]:
                pts.setdefault(p, []).append((h, i))
            for l, i in W["added"][h][1]:
                lns.setdefault(l, []).append((h, i))
        for p, more in pts.items():
            W["pobs"][p] = W["pobs"][p] + more
        for l, more in lns.items():
            W["lobs"][l] = W["lobs"][l] + more
        rows, cull, rec = point_dicts(W, sorted(pts))
        lm.set_points(rows)
        lm.set_cull_attributes(kfs=[], points=cull)
        lm.set_recent_attributes(points=rec, lines=line_dicts(W, sorted(lns)))
        lm.recent_cull(0, [], [], mode="host")
        n = sum(len(v) for v in pts.values())
    else:
        r = lm.insert(called, mode=entry, capacity=(len(called) * ROW, len(called) * ROW, len(called) * ROW))
        n = len(r["added_points"])
    return time.perf_counter() - t0, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stores", default="100,1000,4000")
    ap.add_argument("--calls", default="1,4,16,64")
    ap.add_argument("--entries", default="device,host,baseline")
    ap.add_argument("--out", default=os.path.join("profiles", "insert_timing.jsonl"))
    a = ap.parse_args()
    calls = [int(v) for v in a.calls.split(",")]
    entries = a.entries.split(",")
    ctx = lib.Context() if "device" in entries else None
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for K in (int(v) for v in a.stores.split(",")):
            for share in (0.1, 0.9):
                new = sum(calls) * (REPS + 1)
                times = {}
                for entry in entries:
                    W = build(K, new, share, np.random.default_rng(K))
                    lm = store_of(W, ctx if entry == "device" else None)
                    at = K + 1
                    for n in calls:
                        ts = []
                        for rep in range(REPS + 1):
                            t, added = one(lm, W, list(range(at, at + n)), entry)
                            at += n
                            if rep:
                                ts.append(t)
                        times[(entry, n)] = (statistics.median(ts), added)
                    del lm
                for n in calls:
                    rec = dict(keyframes=K, called=n, share=share, entries=n * (ROW + LROW), points_added=times[(entries[0], n)][1])
                    rec.update({e + "_ms": round(1e3 * times[(e, n)][0], 3) for e in entries})
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
    if ctx:
        ctx.close()


if __name__ == "__main__":
    main()
