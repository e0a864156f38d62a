"""Hand-built graphs for KeyFrame::UpdateConnections, one per rule kept from the reference (src/KeyFrame.cc:200-234, 366-500), each
with the rows it must leave written out by hand, and seeded random scripts.  Nothing here imports the library.

A script is a list of operations that play() runs on lib.LocalMap or on conn_numpy.Store: those of lmap_scenarios and
    ("conn", rows)  ("connect", handles)
A scenario returns (script, expect, premise): expect has, per connect of the script, the hand-written counter, record, new_parent,
touched, weights, ordered, parent, first and flags (a key that is left out is not compared) and under "state" the rows of named
key frames afterwards; premise maps a called key frame to the KFcounter the scenario means it to have, which votes_of() recomputes
from the script's rows alone."""
import numpy as np

import lmap_scenarios as ls

KEYFRAME, POINT, LINE = ls.KEYFRAME, ls.POINT, ls.LINE
W, O, P = 1, 2, 4                  # flag bits: weights, ordered, parent


class Graph:
    """key frames by handle; see(a, [b, c], n) puts n new points into a's match row that b and c observe (so a votes n times for
    each); every point gets a handle of its own from 1000 up"""

    def __init__(self):
        self.kfs, self.pts, self.next = {}, [], 1000

    def kf(self, h, rank, **kw):
        self.kfs[h] = ls.kf(h, rank, **kw)
        return self

    def see(self, a, others, n, bad=0, own=False):
        for _ in range(n):
            self.pts.append(ls.mp(self.next, ([a] if own else []) + list(others), bad=bad))
            self.kfs[a]["points"].append(self.next)
            self.next += 1
        return self

    def ops(self):
        return [("kfs", [ls.snap(r) for r in self.kfs.values()]), ("points", [ls.snap(r) for r in self.pts])]


def conn(h, first=0, weights=(), ordered=()):
    return dict(handle=h, first=first, weights=list(weights), ordered=list(ordered))


def play(ops, store, mode="host"):
    """the results of the script's connects and updates, in order"""
    out = []
    for op in ops:
        if op[0] == "conn":
            store.set_connections(op[1])
        elif op[0] == "connect":
            out.append(store.connect(op[1], mode=mode))
        else:
            out += ls.play([op], store, mode=mode)
    return out


def votes_of(ops, h):
    """KFcounter of key frame h from the rows of the script: {handle: votes}"""
    kfs, pts = {}, {}
    for op in ops:
        if op[0] == "kfs":
            kfs.update({r["handle"]: r for r in op[1]})
        elif op[0] == "points":
            pts.update({r["handle"]: r for r in op[1]})
    votes = {}
    for p in kfs[h]["points"]:
        if p != -1 and not pts[p]["bad"]:
            for k in pts[p]["obs"]:
                if k != h:
                    votes[k] = votes.get(k, 0) + 1
    return votes


def pairs(a):
    return [(int(k), int(w)) for k, w in a]


def check(results, expect, store):
    """the hand-written expectations against what connect() returned and what the store holds afterwards"""
    assert len(results) == len(expect)
    for r, e in zip(results, expect):
        for k, want in e.items():
            if k == "state":
                continue
            if k in ("counter", "weights", "ordered"):
                got = [pairs(a) for a in r[k]]
            else:
                got = np.asarray(r[k]).tolist()
            assert got == want, (k, got, want)
    state = expect[-1].get("state", {})
    if state:
        hs = sorted(state)
        g = store.get_connections(hs)
        for i, h in enumerate(hs):
            for k, want in state[h].items():
                got = pairs(g[k][i]) if k in ("weights", "ordered") else np.asarray(g[k][i]).tolist()
                assert got == want, (h, k, got, want)


def threshold():
    """14, 15 and 16 votes beside each other: 15 is listed, 14 is not but stays in the weights.  Ranks run against the handles."""
    g = Graph().kf(1, 50).kf(2, 10).kf(3, 30).kf(4, 20).see(1, [2], 14).see(1, [3], 15).see(1, [4], 16)
    ops = g.ops() + [("conn", [conn(1, first=1)]), ("connect", [1])]
    expect = [dict(counter=[[(2, 14), (4, 16), (3, 15)]], record=[[3, 2, 16, 4]], new_parent=[4], touched=[4, 3, 1],
                   weights=[[(1, 16)], [(1, 15)], [(2, 14), (4, 16), (3, 15)]], ordered=[[(1, 16)], [(1, 15)], [(4, 16), (3, 15)]],
                   parent=[-1, -1, 4], first=[0, 0, 0], flags=[W | O, W | O, W | O | P],
                   state={2: dict(weights=[], ordered=[], children=[]), 4: dict(children=[1]), 1: dict(parent=4, first=0)})]
    return ops, expect, {1: {2: 14, 3: 15, 4: 16}}


def fallback_and_ties():
    """key frame 1: nothing reaches 15, 5 votes each for key frames 2 and 3: pKFmax is the one of lower rank (3) and it alone is
    listed.  Its stored weights hold two more entries of weight 5: the re-sorted list has equal weights, highest rank first.
    key frame 5: two key frames at 15: pKFmax is again the lower rank (6), but the list - and so the parent - starts with the
    higher one (7)."""
    g = (Graph().kf(1, 40).kf(2, 30).kf(3, 10).kf(4, 20).kf(5, 5).kf(6, 60).kf(7, 70)
         .see(1, [2, 3], 5).see(1, [4], 2).see(5, [6, 7], 15))
    ops = g.ops() + [("conn", [conn(3, weights=[(2, 5), (4, 5)], ordered=[(2, 5)]), conn(5, first=1)]), ("connect", [1, 5])]
    expect = [dict(counter=[[(3, 5), (4, 2), (2, 5)], [(6, 15), (7, 15)]], record=[[3, 1, 5, 3], [2, 2, 15, 6]], new_parent=[-1, 7],
                   touched=[5, 3, 1, 6, 7],
                   weights=[[(6, 15), (7, 15)], [(4, 5), (2, 5), (1, 5)], [(3, 5), (4, 2), (2, 5)], [(5, 15)], [(5, 15)]],
                   ordered=[[(7, 15), (6, 15)], [(1, 5), (2, 5), (4, 5)], [(3, 5)], [(5, 15)], [(5, 15)]],
                   parent=[7, -1, -1, -1, -1], first=[0, 0, 0, 0, 0], flags=[W | O | P, W | O, W | O, W | O, W | O],
                   state={7: dict(children=[5]), 6: dict(children=[])})]
    return ops, expect, {1: {2: 5, 3: 5, 4: 2}, 5: {6: 15, 7: 15}}


def self_double_null_bad():
    """the row holds one point twice (two votes), a null, a bad point (no vote) and the points name key frame 1 itself among
    their observations (skipped)"""
    g = Graph().kf(1, 10).kf(2, 20).kf(3, 30).see(1, [2], 1, own=True).see(1, [3], 1, bad=1, own=True)
    g.kfs[1]["points"] = [1000, -1, 1001, 1000]
    ops = g.ops() + [("connect", [1])]
    expect = [dict(counter=[[(2, 2)]], record=[[1, 1, 2, 2]], new_parent=[-1], touched=[1, 2], weights=[[(2, 2)], [(1, 2)]],
                   ordered=[[(2, 2)], [(1, 2)]], flags=[W | O, W | O], state={3: dict(weights=[], ordered=[])})]
    return ops, expect, {1: {2: 2}}


def bad_keyframe():
    """a bad key frame is counted, connected and becomes the parent"""
    g = Graph().kf(1, 10).kf(2, 5, bad=1).kf(3, 20).see(1, [2], 15).see(1, [3], 14)
    ops = g.ops() + [("conn", [conn(1, first=1)]), ("connect", [1])]
    expect = [dict(counter=[[(2, 15), (3, 14)]], record=[[2, 1, 15, 2]], new_parent=[2], touched=[2, 1], weights=[[(1, 15)], [(2, 15), (3, 14)]],
                   ordered=[[(1, 15)], [(2, 15)]], parent=[-1, 2], first=[0, 0], flags=[W | O, W | O | P],
                   state={2: dict(children=[1]), 3: dict(weights=[])})]
    return ops, expect, {1: {2: 15, 3: 14}}


def empty_counter_then_edge():
    """key frame 1's counter is empty (a null, a bad point, a point only it observes): its rows and first_connection stay.  Key
    frame 2, called after it, still lands its edge on 1, whose list grows to the full sort."""
    g = Graph().kf(1, 10).kf(2, 20).kf(3, 30).see(1, [3], 1, bad=1).see(1, [], 1, own=True).see(2, [1], 15)
    g.kfs[1]["points"].insert(0, -1)
    ops = g.ops() + [("conn", [conn(1, first=1, weights=[(3, 4)], ordered=[(3, 4)])]), ("connect", [1, 2])]
    expect = [dict(counter=[[], [(1, 15)]], record=[[0, 0, 0, -1], [1, 1, 15, 1]], new_parent=[-1, -1], touched=[1, 2],
                   weights=[[(2, 15), (3, 4)], [(1, 15)]], ordered=[[(2, 15), (3, 4)], [(1, 15)]], parent=[-1, -1], first=[1, 0],
                   flags=[W | O, W | O])]
    return ops, expect, {1: {}, 2: {1: 15}}


def same_weight_keeps_the_filtered_list():
    """key frame 5 holds the weight 15 for key frame 1 already: AddConnection returns, and 5 keeps the list its own last call left,
    although its weights hold a sub-threshold entry.  Key frame 6 holds 14: the entry changes and its list becomes the full sort."""
    g = Graph().kf(1, 10).kf(2, 20).kf(3, 30).kf(5, 50).kf(6, 60).see(1, [5], 15).see(1, [6], 16)
    ops = g.ops() + [("conn", [conn(5, weights=[(1, 15), (2, 3), (3, 20)], ordered=[(3, 20), (1, 15)]),
                               conn(6, weights=[(3, 20), (2, 3), (1, 14)], ordered=[(3, 20)])]), ("connect", [1])]
    expect = [dict(counter=[[(5, 15), (6, 16)]], record=[[2, 2, 16, 6]], touched=[1, 5, 6],
                   weights=[[(5, 15), (6, 16)], [(1, 15), (2, 3), (3, 20)], [(1, 16), (2, 3), (3, 20)]],
                   ordered=[[(6, 16), (5, 15)], [(3, 20), (1, 15)], [(3, 20), (1, 16), (2, 3)]], flags=[W | O, 0, W | O])]
    return ops, expect, {1: {5: 15, 6: 16}}


def asymmetric(order):
    """key frame 1 votes 16 times for 2, key frame 2 only 3 times for 1: whoever is called last writes both rows"""
    g = Graph().kf(1, 10).kf(2, 20).see(1, [2], 16).see(2, [1], 3)
    ops = g.ops() + [("connect", list(order))]
    w = 3 if tuple(order) == (1, 2) else 16
    per = {1: ([(2, 16)], [1, 1, 16, 2]), 2: ([(1, 3)], [1, 1, 3, 1])}
    expect = [dict(counter=[per[h][0] for h in order], record=[per[h][1] for h in order], touched=[1, 2], weights=[[(2, w)], [(1, w)]],
                   ordered=[[(2, w)], [(1, w)]], flags=[W | O, W | O])]
    return ops, expect, {1: {2: 16}, 2: {1: 3}}


def earlier_and_later_targets():
    """call (1, 2, 3).  1's edge onto 2 is made before 2's own call, which replaces it.  3's edge onto 2 is made after: it meets
    the 20 that 2's call wrote (not the stored row), changes it to 17, and 2's list becomes the full sort.  2's own list had the
    tie (3, 20), (1, 20): highest rank first, so its new parent is 3 although pKFmax is 1."""
    g = Graph().kf(1, 10).kf(2, 20).kf(3, 30).see(1, [2], 15).see(2, [1, 3], 20).see(3, [2], 17)
    ops = g.ops() + [("conn", [conn(2, first=1)]), ("connect", [1, 2, 3])]
    expect = [dict(counter=[[(2, 15)], [(1, 20), (3, 20)], [(2, 17)]], record=[[1, 1, 15, 2], [2, 2, 20, 1], [1, 1, 17, 2]],
                   new_parent=[-1, 3, -1], touched=[1, 2, 3], weights=[[(2, 20)], [(1, 20), (3, 17)], [(2, 17)]],
                   ordered=[[(2, 20)], [(1, 20), (3, 17)], [(2, 17)]], parent=[-1, 3, -1], first=[0, 0, 0], flags=[W | O, W | O | P, W | O],
                   state={3: dict(children=[2])})]
    return ops, expect, {1: {2: 15}, 2: {1: 20, 3: 20}, 3: {2: 17}}


def stale_reverse_entries():
    """key frame 2 still holds 30 for key frame 1, which now votes 5 for it: below the threshold nothing reaches 2, and its
    entry stays"""
    g = Graph().kf(1, 10).kf(2, 20).kf(3, 30).see(1, [2], 5).see(1, [3], 15)
    ops = g.ops() + [("conn", [conn(1, weights=[(2, 30)], ordered=[(2, 30)]), conn(2, weights=[(1, 30)], ordered=[(1, 30)])]),
                     ("connect", [1])]
    expect = [dict(counter=[[(2, 5), (3, 15)]], record=[[2, 1, 15, 3]], touched=[1, 3], weights=[[(2, 5), (3, 15)], [(1, 15)]],
                   ordered=[[(3, 15)], [(1, 15)]], flags=[W | O, W | O], state={2: dict(weights=[(1, 30)], ordered=[(1, 30)])})]
    return ops, expect, {1: {2: 5, 3: 15}}


def first_connection_set_and_cleared():
    """key frames 1 and 2 both list key frame 3; only 1 has the flag: it leaves its stored parent 7 for 3, and 7 keeps it as a
    child (nothing is erased); 2 keeps parent 7"""
    g = Graph().kf(1, 10, parent=7).kf(2, 20, parent=7).kf(3, 5).kf(7, 70, ch=[1, 2]).see(1, [3], 15).see(2, [3], 15)
    ops = g.ops() + [("conn", [conn(1, first=1), conn(2, first=0)]), ("connect", [1, 2])]
    expect = [dict(new_parent=[3, -1], touched=[3, 1, 2], weights=[[(1, 15), (2, 15)], [(3, 15)], [(3, 15)]],
                   ordered=[[(2, 15), (1, 15)], [(3, 15)], [(3, 15)]], parent=[-1, 3, 7], first=[0, 0, 0], flags=[W | O, W | O | P, W | O],
                   state={3: dict(children=[1]), 7: dict(children=[1, 2])})]
    return ops, expect, {1: {3: 15}, 2: {3: 15}}


HAND = {
    "threshold": threshold, "fallback_and_ties": fallback_and_ties, "self_double_null_bad": self_double_null_bad,
    "bad_keyframe": bad_keyframe, "empty_counter_then_edge": empty_counter_then_edge,
    "same_weight_keeps_the_filtered_list": same_weight_keeps_the_filtered_list, "asymmetric_1_then_2": lambda: asymmetric((1, 2)),
    "asymmetric_2_then_1": lambda: asymmetric((2, 1)), "earlier_and_later_targets": earlier_and_later_targets,
    "stale_reverse_entries": stale_reverse_entries, "first_connection_set_and_cleared": first_connection_set_and_cleared,
}


def clustered(rng, n_kf, row, window=4, mp_per_kf=None, bad=0.05):
    """a graph whose key frames share points with their neighbours in handle order, so that pairs pass, meet and miss the
    threshold: key-frame rows (ranks against the handle order) and point rows"""
    ranks = rng.permutation(n_kf) * 7 + 3
    kfs = {h: ls.kf(h, int(ranks[h])) for h in range(n_kf)}
    pts = []
    for h in range(n_kf):
        for _ in range(mp_per_kf if mp_per_kf is not None else row):
            near = [int(x) for x in rng.integers(max(0, h - window), min(n_kf, h + window + 1), int(rng.integers(0, 5)))]
            obs = list(dict.fromkeys([h] + near))
            p = ls.mp(len(pts), obs, bad=int(rng.random() < bad))
            pts.append(p)
            for k in obs:
                if len(kfs[k]["points"]) < row:
                    kfs[k]["points"].append(p["handle"] if rng.random() > 0.05 else -1)
    return kfs, pts


def random_script(seed, n_kf=36, row=70, calls=14, max_call=7, updates=True):
    """a seeded clustered graph and `calls` connects of 1 .. max_call key frames, with edits between them that keep every reference
    known - bad flags, replaced rows, a removed key frame with every mention of it purged from the rows and from the connection
    state - and UpdateLocalMap queries that read the committed graph.  The connection state that a purge must rewrite is taken
    from a conn_numpy.Store that the generator plays the script on as it writes it."""
    import conn_numpy as cn
    rng = np.random.default_rng(seed)
    kfs, pts = clustered(rng, n_kf, row)
    pts = {p["handle"]: p for p in pts}
    shadow = cn.Store()
    ops = []

    def emit(*new):
        for op in new:
            ops.append(op)
            play([op], shadow)

    emit(("kfs", [ls.snap(r) for r in kfs.values()]), ("points", [ls.snap(r) for r in pts.values()]),
         ("conn", [conn(h, first=int(rng.random() < 0.7)) for h in kfs if h != 0]))
    fid = 1
    for _ in range(calls):
        live = sorted(kfs)
        hs = [int(h) for h in rng.permutation(live)[:int(rng.integers(1, max_call + 1))]]
        emit(("connect", hs))
        if updates and rng.random() < 0.7:
            qs = []
            for _ in range(int(rng.integers(1, 4))):
                k = kfs[int(rng.choice(live))]
                qs.append(dict(frame_id=fid, points=[int(p) for p in k["points"]]))
                fid += 1
            emit(("update", qs))
        what = int(rng.integers(0, 5))
        if what == 0:
            hs = [int(h) for h in rng.choice(live, 3)]
            emit(("bad", KEYFRAME, hs, [int(rng.random() < 0.5) for _ in hs]))
        elif what == 1:
            hs = [int(h) for h in rng.choice(sorted(pts), 6)]
            fl = [int(rng.random() < 0.5) for _ in hs]
            for h, f in zip(hs, fl):
                pts[h]["bad"] = f
            emit(("bad", POINT, hs, fl))
        elif what == 2:
            k = kfs[int(rng.choice(live))]
            rng.shuffle(k["points"])
            k["points"] = k["points"][:int(rng.integers(0, len(k["points"]) + 1))]
            state = shadow.get_connections([k["handle"]])
            k["parent"], k["children"] = int(state["parent"][0]), [int(c) for c in state["children"][0]]
            k["neighbours"] = [int(x) for x in shadow.kf[k["handle"]].neighbours]
            emit(("kfs", [ls.snap(k)]))
        elif what == 3 and len(live) > 8:
            gone = int(rng.choice(live))
            del kfs[gone]
            for p in pts.values():
                p["obs"] = [x for x in p["obs"] if x != gone]
            rows, crows = [], []
            for h, k in kfs.items():
                sk = shadow.kf[h]
                k["parent"] = -1 if sk.parent == gone else sk.parent
                k["children"] = [c for c in sk.children if c != gone]
                k["neighbours"] = [x for x in sk.neighbours if x != gone]
                rows.append(ls.snap(k))
                st = shadow.conn.get(h, dict(first=False, weights={}, ordered=[]))
                crows.append(conn(h, first=int(st["first"]), weights=[(a, w) for a, w in st["weights"].items() if a != gone],
                                  ordered=[(a, w) for a, w in st["ordered"] if a != gone]))
            emit(("remove", KEYFRAME, gone), ("kfs", rows), ("points", [ls.snap(p) for p in pts.values()]), ("conn", crows))
    return ops
