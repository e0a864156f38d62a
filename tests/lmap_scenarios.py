"""Hand-built graphs for Tracking::UpdateLocalMap, one per rule kept from the reference (src/Tracking.cc:3396-3541), each with the
lists it must leave written out by hand, and seeded random scripts.  Pure numpy: nothing here imports the library.

A script is a list of operations that play() runs on lib.LocalMap or on lmap_numpy.Store:
    ("kfs", rows) ("points", rows) ("lines", handles, bad) ("bad", kind, handles, flags) ("remove", kind, handle)
    ("update", queries)
A scenario returns (script, expect, votes): expect has, per update and per query, the hand-written kfs, ref_kf, record, mps,
mp_in_frame, mls, ml_in_frame and nulled (a key that is left out is not compared); votes is the keyframeCounter the scenario
means its first query to have, by key-frame handle, which votes_of() recomputes from the script to check the premise."""
import numpy as np

KEYFRAME, POINT, LINE = range(3)


def kf(h, rank, bad=0, parent=-1, nb=(), ch=(), pts=(), lns=()):
    return dict(handle=h, rank=rank, bad=bad, parent=parent, neighbours=list(nb), children=list(ch), points=list(pts), lines=list(lns))


def mp(h, obs=(), bad=0):
    return dict(handle=h, obs=list(obs), bad=bad)


def snap(row):
    """a copy of a row that later edits of the generator's graph do not reach"""
    return {k: (list(v) if isinstance(v, list) else v) for k, v in row.items()}


def play(ops, store, mode="host"):
    out = []
    for op in ops:
        if op[0] == "kfs":
            store.set_keyframes(op[1])
        elif op[0] == "points":
            store.set_points(op[1])
        elif op[0] == "lines":
            store.set_lines(op[1], op[2])
        elif op[0] == "bad":
            store.set_bad(op[1], op[2], op[3])
        elif op[0] == "remove":
            store.remove(op[1], op[2])
        elif op[0] == "update":
            out.append(store.update(op[1], mode=mode))
        else:
            raise ValueError(op[0])
    return out


def votes_of(ops):
    """keyframeCounter of the first query of the first update, from the script's rows alone"""
    points = {}
    for op in ops:
        if op[0] == "points":
            for r in op[1]:
                points[r["handle"]] = r
        elif op[0] == "bad" and op[1] == POINT:
            for h, f in zip(op[2], op[3]):
                points[h]["bad"] = f
        elif op[0] == "update":
            votes = {}
            for h in op[1][0].get("points", ()):
                if h != -1 and not points[h]["bad"]:
                    for k in points[h]["obs"]:
                        votes[k] = votes.get(k, 0) + 1
            return votes
    return {}


def check(results, expect):
    """the hand-written expectations against what update() returned"""
    assert len(results) == len(expect)
    for r, e in zip(results, expect):
        for k, want in e.items():
            if k == "ref_kf":
                assert r[k].tolist() == want, (k, r[k].tolist(), want)
            elif k == "record":
                assert r[k].tolist() == want, (k, r[k].tolist(), want)
            else:
                got = [[int(v) for v in a] for a in r[k]]
                assert got == want, (k, got, want)


def vote_tie():
    """key frames 1 and 2 both get two votes; 2 has the lower rank, so it is met first and strict > keeps it.  Ranks (30, 10, 20)
    run against the handles (1, 2, 3) and against the order of the rows: the list is in rank order."""
    ops = [("kfs", [kf(1, 30, pts=[101, 103]), kf(3, 20, pts=[102, 100]), kf(2, 10, pts=[100, -1, 101])]),
           ("points", [mp(100, [1, 2]), mp(101, [2, 1]), mp(102, [3]), mp(103)]),
           ("update", [dict(frame_id=5, points=[100, 101, 102])])]
    expect = [dict(kfs=[[2, 3, 1]], ref_kf=[2], record=[[3, 3, 0, 2]], mps=[[100, 101, 102, 103]], mp_in_frame=[[1, 1, 1, 0]],
                   mls=[[]], nulled=[[]])]
    return ops, expect, {1: 2, 2: 2, 3: 1}


def best_bad():
    """the key frame with most votes is bad: counted, not listed, never pKFmax"""
    ops = [("kfs", [kf(1, 1, bad=1, pts=[100]), kf(2, 2, pts=[101]), kf(3, 3, pts=[102])]),
           ("points", [mp(100, [1, 2, 3]), mp(101, [1, 2]), mp(102, [1])]),
           ("update", [dict(frame_id=1, points=[100, 101, 102])])]
    expect = [dict(kfs=[[2, 3]], ref_kf=[2], record=[[3, 2, 0, 2]], mps=[[101, 102]], mp_in_frame=[[1, 1]], nulled=[[]])]
    return ops, expect, {1: 3, 2: 2, 3: 1}


def all_bad():
    """a counter that is not empty but holds only bad key frames: an empty list (prev_kfs is not kept), no reference key frame"""
    ops = [("kfs", [kf(1, 1, bad=1, pts=[100]), kf(2, 2, bad=1, pts=[100]), kf(3, 3, pts=[100])]),
           ("points", [mp(100, [1, 2])]),
           ("update", [dict(frame_id=1, points=[100], prev_kfs=[3])])]
    expect = [dict(kfs=[[]], ref_kf=[-1], record=[[2, 0, 0, 0]], mps=[[]], mls=[[]], nulled=[[]])]
    return ops, expect, {1: 1, 2: 1}


def empty_counter():
    """no vote at all (a null, a bad point, a point nobody observes): the early return.  The list stays what the previous frame
    left, the gathers run on it, the bad point is still reported; without prev_kfs everything but the nulled list is empty."""
    ops = [("kfs", [kf(1, 1, pts=[101, 102], lns=[300]), kf(3, 3, pts=[102, 100, 103], nb=[1])]),
           ("points", [mp(100, [1], bad=1), mp(101), mp(102), mp(103)]),
           ("lines", [300], [0]),
           ("update", [dict(frame_id=1, points=[-1, 100, 101], prev_kfs=[3, 1]), dict(frame_id=2, points=[-1, 100, 101])])]
    expect = [dict(kfs=[[3, 1], []], ref_kf=[-1, -1], record=[[0, 0, 0, 0], [0, 0, 0, 0]], mps=[[102, 103, 101], []],
                   mp_in_frame=[[0, 0, 1], []], mls=[[300], []], ml_in_frame=[[0], []], nulled=[[1], [1]])]
    return ops, expect, {}


def double_vote():
    """a point that is in the frame twice votes twice"""
    ops = [("kfs", [kf(1, 2, pts=[100]), kf(2, 1, pts=[101])]),
           ("points", [mp(100, [1]), mp(101, [2])]),
           ("update", [dict(frame_id=9, points=[100, 101, 100])])]
    expect = [dict(kfs=[[2, 1]], ref_kf=[1], record=[[2, 2, 0, 2]], mps=[[101, 100]], mp_in_frame=[[1, 1]])]
    return ops, expect, {1: 2, 2: 1}


def limit_80(listed):
    """`listed` voted key frames 0 .. listed - 1 (rank = handle), each with the neighbour 1000 + h and the child 2000 + h.
    80: size() > 80 is false, key frame 0 pushes 1000 and 2000, then 82 > 80 ends it.  81: nothing is pushed.  78: key frame 0
    makes it 80, which still expands: key frame 1 pushes too, then 82 > 80."""
    rows = [kf(h, h, nb=[1000 + h], ch=[2000 + h], pts=[h]) for h in range(listed)]
    rows += [kf(1000 + h, 1000 + h) for h in range(listed)] + [kf(2000 + h, 2000 + h) for h in range(listed)]
    ops = [("kfs", rows), ("points", [mp(7, list(range(listed)))] + [mp(h) for h in range(listed) if h != 7]),
           ("update", [dict(frame_id=1, points=[7])])]
    base = list(range(listed))
    tail = {80: [1000, 2000], 81: [], 78: [1000, 2000, 1001, 2001]}[listed]
    expect = [dict(kfs=[base + tail], ref_kf=[0], record=[[listed, listed, len(tail), 1]], mps=[base])]
    return ops, expect, {h: 1 for h in range(listed)}


def neighbour_choice():
    """key frame 1's neighbours: a hole, a bad one, a listed one, then 4 (taken; 5 is not looked at).  Key frame 3's: 4, by now
    listed, then 5.  Key frame 1's parent is 3, listed already: no push and no break, so key frame 3 is still expanded."""
    ops = [("kfs", [kf(1, 1, nb=[-1, 2, 3, 4, 5], parent=3), kf(2, 2, bad=1), kf(3, 3, nb=[4, 5]), kf(4, 4), kf(5, 5)]),
           ("points", [mp(100, [1, 3])]),
           ("update", [dict(frame_id=1, points=[100])])]
    expect = [dict(kfs=[[1, 3, 4, 5]], ref_kf=[1], record=[[2, 2, 2, 1]])]
    return ops, expect, {1: 1, 3: 1}


def children_by_rank():
    """children are walked in rank order whatever order they are given in: 6 (rank 20, bad), 7 (rank 30, taken), 5 (rank 50)"""
    ops = [("kfs", [kf(1, 1, ch=[5, 7, 6]), kf(5, 50), kf(6, 20, bad=1), kf(7, 30)]),
           ("points", [mp(100, [1])]),
           ("update", [dict(frame_id=1, points=[100])])]
    expect = [dict(kfs=[[1, 7]], ref_kf=[1], record=[[1, 1, 1, 1]])]
    return ops, expect, {1: 1}


def parent_break():
    """key frame 1 contributes neighbour, child and parent; the parent's break leaves the outer loop: key frame 2's neighbour 6
    is never taken"""
    ops = [("kfs", [kf(1, 1, nb=[3], ch=[4], parent=5), kf(2, 2, nb=[6]), kf(3, 3), kf(4, 4), kf(5, 5), kf(6, 6)]),
           ("points", [mp(100, [1, 2])]),
           ("update", [dict(frame_id=1, points=[100])])]
    expect = [dict(kfs=[[1, 2, 3, 4, 5]], ref_kf=[1], record=[[2, 2, 3, 1]])]
    return ops, expect, {1: 1, 2: 1}


def bad_parent():
    """the parent is pushed with no bad test, and UpdateLocalPoints walks it like any other: its point 200 is listed"""
    ops = [("kfs", [kf(1, 1, parent=9, pts=[100]), kf(9, 9, bad=1, pts=[200])]),
           ("points", [mp(100, [1]), mp(200)]),
           ("update", [dict(frame_id=1, points=[100])])]
    expect = [dict(kfs=[[1, 9]], ref_kf=[1], record=[[1, 1, 1, 1]], mps=[[100, 200]], mp_in_frame=[[1, 0]])]
    return ops, expect, {1: 1}


def pushed_not_expanded():
    """the expansion walks only what the vote loop listed: pushed key frame 2 does not bring its neighbour 3"""
    ops = [("kfs", [kf(1, 1, nb=[2]), kf(2, 2, nb=[3]), kf(3, 3)]),
           ("points", [mp(100, [1])]),
           ("update", [dict(frame_id=1, points=[100])])]
    expect = [dict(kfs=[[1, 2]], ref_kf=[1], record=[[1, 1, 1, 1]])]
    return ops, expect, {1: 1}


def gathers():
    """duplicates across key frames are listed where first met; bad point 102 and bad line 302 are in both rows, are never
    stamped and never listed; the frame's bad point 102 is nulled; in_frame marks the frame's remaining points and its lines"""
    ops = [("kfs", [kf(1, 1, pts=[100, 101, -1, 102], lns=[300, -1, 301, 302]), kf(2, 2, pts=[101, 103, 102, 100, 104], lns=[301, 302, 303])]),
           ("points", [mp(100, [1]), mp(101), mp(102, [1, 2], bad=1), mp(103), mp(104, [2])]),
           ("lines", [300, 301, 302, 303], [0, 0, 1, 0]),
           ("update", [dict(frame_id=3, points=[100, 104, 102], lines=[303, -1, 302])])]
    expect = [dict(kfs=[[1, 2]], ref_kf=[1], record=[[2, 2, 0, 1]], mps=[[100, 101, 103, 104]], mp_in_frame=[[1, 0, 0, 1]],
                   mls=[[300, 301, 303]], ml_in_frame=[[0, 0, 1]], nulled=[[2]])]
    return ops, expect, {1: 1, 2: 1}


HAND = {
    "vote_tie": vote_tie, "best_bad": best_bad, "all_bad": all_bad, "empty_counter": empty_counter, "double_vote": double_vote,
    "limit_80": lambda: limit_80(80), "limit_81": lambda: limit_80(81), "limit_crossing": lambda: limit_80(78),
    "neighbour_choice": neighbour_choice, "children_by_rank": children_by_rank, "parent_break": parent_break,
    "bad_parent": bad_parent, "pushed_not_expanded": pushed_not_expanded, "gathers": gathers,
}


def random_script(seed, n_kf=40, n_mp=300, n_ml=60, row=30, obs=6, calls=8, per_call=8, frame_points=60, edits=True):
    """a seeded graph, `calls` updates of `per_call` frames each, and between them edits that keep every reference known: bad flags
    set and cleared, rows replaced, key frames / points / lines removed together with every mention of them"""
    rng = np.random.default_rng(seed)
    kf_h = [int(h) for h in rng.permutation(4 * n_kf)[:n_kf]]
    ranks = [int(r) for r in rng.integers(1, 2 ** 63, n_kf, dtype=np.uint64) * 2 + rng.integers(0, 2, n_kf, dtype=np.uint64)]
    assert len(set(ranks)) == n_kf
    mp_h = [int(h) for h in rng.permutation(3 * n_mp)[:n_mp]]
    ml_h = [int(h) for h in rng.permutation(3 * n_ml)[:n_ml]]
    G = dict(kf={}, mp={}, ml={})

    def pick(pool, k, holes=0.0):
        if not pool or k <= 0:
            return []
        out = [int(pool[i]) for i in rng.integers(0, len(pool), k)]
        return [-1 if rng.random() < holes else h for h in out]

    def kf_row(h, rank):
        others = [x for x in kf_h if x != h]
        return kf(h, rank, bad=int(rng.random() < 0.15), parent=pick(others, 1)[0] if rng.random() < 0.7 and others else -1,
                  nb=list(dict.fromkeys(pick(others, int(rng.integers(0, 11)), 0.1)))[:10],
                  ch=[x for x in dict.fromkeys(pick(others, int(rng.integers(0, 4))))],
                  pts=pick(mp_h, int(rng.integers(0, row + 1)), 0.2), lns=pick(ml_h, int(rng.integers(0, row // 3 + 1)), 0.2))

    def mp_row(h):
        return mp(h, obs=list(dict.fromkeys(pick(kf_h, int(rng.integers(0, obs + 1))))), bad=int(rng.random() < 0.1))

    for h, r in zip(kf_h, ranks):
        G["kf"][h] = kf_row(h, r)
    for h in mp_h:
        G["mp"][h] = mp_row(h)
    for h in ml_h:
        G["ml"][h] = int(rng.random() < 0.1)
    ops = [("kfs", [snap(r) for r in G["kf"].values()]), ("points", [snap(r) for r in G["mp"].values()]), ("lines", list(ml_h), [G["ml"][h] for h in ml_h])]
    fid = int(rng.integers(1, 100))
    prev = []
    for _ in range(calls):
        qs = []
        for _ in range(per_call):
            q = dict(frame_id=fid, points=pick(mp_h, int(rng.integers(0, frame_points + 1)) if rng.random() < 0.9 else 0, 0.3))
            fid += int(rng.integers(1, 4))
            if rng.random() < 0.6:
                q["lines"] = pick(ml_h, int(rng.integers(0, 12)), 0.3)
            if rng.random() < 0.5:
                q["prev_kfs"] = pick(kf_h, int(rng.integers(0, 12)))
            qs.append(q)
        ops.append(("update", qs))
        if not edits:
            continue
        for _ in range(int(rng.integers(0, 4))):
            what = int(rng.integers(0, 6))
            if what == 0 and kf_h:
                hs = pick(kf_h, 3)
                fl = [int(rng.random() < 0.5) for _ in hs]
                for h, f in zip(hs, fl):
                    G["kf"][h]["bad"] = f
                ops.append(("bad", KEYFRAME, hs, fl))
            elif what == 1 and mp_h:
                hs = pick(mp_h, 5)
                fl = [int(rng.random() < 0.5) for _ in hs]
                for h, f in zip(hs, fl):
                    G["mp"][h]["bad"] = f
                ops.append(("bad", POINT, hs, fl))
            elif what == 2 and ml_h:
                hs = pick(ml_h, 3)
                fl = [int(rng.random() < 0.5) for _ in hs]
                for h, f in zip(hs, fl):
                    G["ml"][h] = f
                ops.append(("bad", LINE, hs, fl))
            elif what == 3 and kf_h:
                h = pick(kf_h, 1)[0]
                G["kf"][h] = kf_row(h, G["kf"][h]["rank"])
                hp = pick(mp_h, 1)[0]
                G["mp"][hp] = mp_row(hp)
                ops += [("kfs", [snap(G["kf"][h])]), ("points", [snap(G["mp"][hp])])]
            elif what == 4 and len(kf_h) > 3:
                h = pick(kf_h, 1)[0]
                kf_h.remove(h)
                del G["kf"][h]
                for r in G["kf"].values():
                    r["parent"] = -1 if r["parent"] == h else r["parent"]
                    r["neighbours"] = [-1 if x == h else x for x in r["neighbours"]]
                    r["children"] = [x for x in r["children"] if x != h]
                for r in G["mp"].values():
                    r["obs"] = [x for x in r["obs"] if x != h]
                ops += [("remove", KEYFRAME, h), ("kfs", [snap(r) for r in G["kf"].values()]), ("points", [snap(r) for r in G["mp"].values()])]
            elif what == 5 and len(mp_h) > 3 and len(ml_h) > 3:
                hp, hl = pick(mp_h, 1)[0], pick(ml_h, 1)[0]
                mp_h.remove(hp)
                ml_h.remove(hl)
                del G["mp"][hp], G["ml"][hl]
                for r in G["kf"].values():
                    r["points"] = [-1 if x == hp else x for x in r["points"]]
                    r["lines"] = [-1 if x == hl else x for x in r["lines"]]
                ops += [("remove", POINT, hp), ("remove", LINE, hl), ("kfs", [snap(r) for r in G["kf"].values()])]
    return ops
