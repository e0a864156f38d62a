"""Hand-built maps for what surrounds the solver of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2910-3131), each
with the vertices, the edge list or the moved points it must give written out by hand, builders for the shapes at the kernels'
seams, and seeded random scripts.  Nothing here imports the library.

A script is a list of operations that play() runs on lib.LocalMap or on essential_numpy.Store: those of gba_propagate_scenarios and
    ("loop_edges", rows)  ("essential_edges", loop_kf, cur_kf, sim3 rows, loop-connection rows)
    ("essential_commit", cur_kf, handles, Scw [n, 8], optimised [n, 8])
The hand cases use identity rotations, integer translations and scales that are powers of two, with points and centres on the z
axis, so every product, sum, quotient and square root in them is exact and the expected values are literals (compared by value: a
zero may carry either sign, except where a case says otherwise).  With key frame h at [I | (h, 0, 0)] and no table row, vScw[h] =
(I, (h, 0, 0), 1) and the edge i -> j measures (I, (j - i, 0, 0), 1).  A scenario returns (script, expect): expect has, per
essential call of the script, the hand-written outputs (a key that is left out is not compared)."""
import numpy as np

import gba_propagate_scenarios as gs
import loop_correct_scenarios as rs
import conn_scenarios as cs
import lmap_scenarios as ls

KEYFRAME, POINT = ls.KEYFRAME, ls.POINT
LC, TREE, LOOP, COVIS = 0, 1, 2, 3
NORMAL = 2
SCALES = [1.0, 2.0, 4.0]
pose, geo, conn = rs.pose, rs.geo, cs.conn


def play(ops, store, mode="host"):
    out = []
    for op in ops:
        if op[0] == "loop_edges":
            store.set_loop_edges(op[1])
        elif op[0] == "essential_edges":
            out.append(store.essential_edges(op[1], op[2], op[3], op[4], mode=mode))
        elif op[0] == "essential_commit":
            out.append(store.essential_commit(op[1], op[2], op[3], op[4], mode=mode))
        else:
            out += gs.play([op], store, mode=mode)
    return out


alive = gs.alive


def check(results, expect):
    calls = [r for r in results if "measurement" in r or "Swc" in r]
    assert len(calls) == len(expect)
    for r, e in zip(calls, expect):
        for k, want in e.items():
            if k == "positive_zero":
                t, c = want
                assert r["world"][t][c] == 0 and not np.signbit(r["world"][t][c]), r["world"][t]
                continue
            got = np.asarray(r[k])
            want = np.asarray(want, got.dtype).reshape((len(want),) + got.shape[1:])
            assert got.shape == want.shape and np.array_equal(got, want), (k, got, want)


def kf(h, parent=-1, ch=(), bad=0, rank=None, pts=()):
    return ls.kf(h, h if rank is None else rank, bad=bad, parent=parent, ch=ch, pts=pts)


def sim3(t=(0.0, 0.0, 0.0), s=1.0, q=rs.ID_Q):
    return [float(v) for v in q] + [float(v) for v in t] + [float(s)]


def meas(dx, s=1.0):
    return sim3((dx, 0, 0), s)


def on_x(handles):
    """key frame h at [I | (h, 0, 0)]"""
    return ("poses", list(handles), [pose(t=(h, 0, 0)) for h in handles])


# ---- the edge builder, by hand ---------------------------------------------------------------------------------------------------

def covisibility_prefixes():
    """No parents, no loop edges, so only GetCovisiblesByWeight(100) speaks.  6: weights 150, 100, 99: the prefix is two long and
    the entry at exactly 100 is kept.  5: 120, 50: one long.  4: 99, 50: none.  3: 200, 150: the prefix is the whole row,
    upper_bound returns end() and the list comes back EMPTY.  2 and 1 have empty rows."""
    hs = [1, 2, 3, 4, 5, 6]
    ops = [("kfs", [kf(h) for h in hs]), on_x(hs),
           ("conn", [conn(6, ordered=[(5, 150), (4, 100), (3, 99)]), conn(5, ordered=[(4, 120), (3, 50)]),
                     conn(4, ordered=[(3, 99), (2, 50)]), conn(3, ordered=[(2, 200), (1, 150)])]),
           ("essential_edges", 1, 6, [], [])]
    e = {"vertices": hs, "fixed": [1, 0, 0, 0, 0, 0], "Scw": [sim3((h, 0, 0)) for h in hs],
         "from": [5, 6, 6], "to": [4, 5, 4], "kind": [COVIS] * 3, "measurement": [meas(-1), meas(-1), meas(-2)]}
    return ops, [e], dict(prefixes_emptied=1, vertices=6, edges=3)


def covisibility_drop_reasons():
    """The ordered row of 10, every entry at 100 or more but the last: 9 is its parent, 8 its child, 7 its loop edge, 6 is bad, 11
    has the larger handle, the pair (5, 10) was inserted by the loop connection 10 -> 5 (weight 230), 4 is kept, 3 ends the prefix.
    Each dropped entry fails exactly one test.  7 holds the loop edge back to 10, which has the larger handle and gives no edge; 8
    has its parent edge.  Rank order: 3 4 5 7 8 9 10 11 (6 has no vertex)."""
    hs = [3, 4, 5, 6, 7, 8, 9, 10, 11]
    rows = [kf(h) for h in (3, 4, 5, 7, 11)] + [kf(6, bad=1), kf(8, parent=10), kf(9, ch=[10]), kf(10, parent=9, ch=[8])]
    ops = [("kfs", rows), on_x(hs),
           ("conn", [conn(10, weights=[(5, 230)],
                          ordered=[(9, 500), (8, 400), (7, 300), (6, 250), (11, 240), (5, 230), (4, 220), (3, 10)])]),
           ("loop_edges", [(10, [7]), (7, [10])]),
           ("essential_edges", 3, 10, [], [(10, [5])])]
    e = {"vertices": [3, 4, 5, 7, 8, 9, 10, 11], "fixed": [1, 0, 0, 0, 0, 0, 0, 0],
         "from": [10, 8, 10, 10, 10], "to": [5, 10, 9, 7, 4], "kind": [LC, TREE, TREE, LOOP, COVIS],
         "measurement": [meas(-5), meas(2), meas(-1), meas(-3), meas(-6)]}
    return ops, [e], dict(prefixes_emptied=0, vertices=8, edges=5)


def loop_connection_rules():
    """loop = 1, cur = 5.  Keys in rank order: 2 -> 5 has no entry in the weights row of 2, GetWeight gives 0 and the member is
    skipped; 3 -> 4 weighs exactly 100 and is kept, to the larger handle; 5 -> 1 weighs 30 and survives only as (cur, loop).  Then
    the key frames: 4 would add 4 -> 3 from its prefix but the pair is inserted; 5 adds 5 -> 2, the pair the skipped loop connection
    did not insert (1 ends its prefix).  The table names 5: corrected (I, (10, 0, 0), 2), non-corrected (I, (5, 0, 0), 1).  The
    loop connection 5 -> 1 uses the corrected one: its inverse is (I, (-5, 0, 0), 1/2), so S = (I, (1 - 5, 0, 0), 1/2).  The
    covisibility edge 5 -> 2 uses the non-corrected one: (I, (2 - 5, 0, 0), 1)."""
    hs = [1, 2, 3, 4, 5]
    ops = [("kfs", [kf(h) for h in hs]), on_x(hs),
           ("conn", [conn(3, weights=[(4, 100)]), conn(4, ordered=[(3, 100), (1, 5)]),
                     conn(5, weights=[(1, 30), (2, 150)], ordered=[(2, 150), (1, 30)])]),
           ("essential_edges", 1, 5, [(5, sim3((10, 0, 0), 2.0), sim3((5, 0, 0)))], [(5, [1]), (2, [5]), (3, [4])])]
    e = {"vertices": hs, "fixed": [1, 0, 0, 0, 0],
         "Scw": [sim3((1, 0, 0)), sim3((2, 0, 0)), sim3((3, 0, 0)), sim3((4, 0, 0)), sim3((10, 0, 0), 2.0)],
         "from": [3, 5, 5], "to": [4, 1, 2], "kind": [LC, LC, COVIS], "measurement": [meas(1), meas(-4, 0.5), meas(-3)]}
    return ops, [e], dict(prefixes_emptied=0, vertices=5, edges=3)


def rank_order_is_not_handle_order():
    """Handles 1, 2, 3 with ranks 30, 20, 10: the map is walked 3, 2, 1.  loop = 3, cur = 2.  The loop connections of 2 in rank
    order: 3 (kept as (cur, loop)), then 1 (weight 100).  Key frame 3: its loop edges 2 and 1, both smaller handles, in rank order.
    Key frame 2: its loop edge 3 has the larger handle; its prefix holds 1, whose pair is inserted.  Key frame 1: its parent 3."""
    ops = [("kfs", [kf(1, parent=3, rank=30), kf(2, rank=20), kf(3, ch=[1], rank=10)]), on_x([1, 2, 3]),
           ("conn", [conn(2, weights=[(1, 100)], ordered=[(1, 300), (3, 10)])]),
           ("loop_edges", [(3, [1, 2]), (2, [3]), (1, [3])]),
           ("essential_edges", 3, 2, [], [(2, [1, 3])])]
    e = {"vertices": [3, 2, 1], "fixed": [1, 0, 0], "from": [2, 2, 3, 3, 1], "to": [3, 1, 2, 1, 3],
         "kind": [LC, LC, LOOP, LOOP, TREE], "measurement": [meas(1), meas(-1), meas(-1), meas(-2), meas(2)]}
    return ops, [e], dict(prefixes_emptied=0, vertices=3, edges=5)


def no_refusal_without_an_edge():
    """What would be a null vertex gives no refusal where the reference adds no edge: the bad 4 is a loop-connection member of 5
    below 100 (skipped), a loop edge of 3 with the larger handle, and an entry of the prefix of 5 (dropped as bad).  3 also holds
    the loop edge 99, which no stored key frame answers to and which has the larger handle.  5 has no pose but the table names it."""
    ops = [("kfs", [kf(1), kf(3), kf(4, bad=1), kf(5)]), on_x([1, 3, 4]),
           ("conn", [conn(5, weights=[(4, 99)], ordered=[(4, 120), (3, 110), (1, 7)])]),
           ("loop_edges", [(3, [4, 99])]),
           ("essential_edges", 1, 5, [(5, sim3((5, 0, 0)), sim3((5, 0, 0)))], [(5, [4])])]
    e = {"vertices": [1, 3, 5], "fixed": [1, 0, 0], "from": [5], "to": [3], "kind": [COVIS], "measurement": [meas(-2)]}
    return ops, [e], dict(prefixes_emptied=0, vertices=3, edges=1)


# ---- the commit, by hand ---------------------------------------------------------------------------------------------------------

def commit_points():
    """cur = 2; the call names 2, then 1; 3 is bad, keeps its pose [I | (0, 0, -8)] and its centre (0, 0, 8).
    Key frame 1: Scw = identity, optimised (I, (0, 0, 1), 2): Swc = (I, (0, 0, -1/2), 1/2), pose [I | (0, 0, 1/2)], centre (0, 0, -1/2).
    Key frame 2: Scw (I, (0, 0, 1), 1), optimised (I, (0, 0, 2), 1): Swc = (I, (0, 0, -2), 1), pose [I | (0, 0, 2)], centre (0, 0, -2).
    100 (reference 1): (0, 0, 4) -> 4 / 2 - 1/2 = 3/2; seen from 1 at distance 2, level 1: max 4, min 1.
    101 was corrected by cur through 2 although its reference is 1: (0, 0, 3) -> + 1 -> - 2 = (0, 0, 2).  Its observers 2 (new centre,
      direction +z), 3 (not named: stored centre, -z) and 1 (new centre, +z): normal (0, 0, 1) / 3; distance to 1 is 5/2, level 0.
    102 has the bad 3 for reference: default-constructed Sim3s, the same arithmetic, which turns its -0.0 into 0.0; seen from 1 at
      (0, 0, 11/2), distance to 3 is 3, level 2: max 12, min 3.
    103 has no observations: it moves, (0, 0, 2) -> 1/2, status 0.  104 is bad and stays."""
    ops = [("kfs", [kf(1), kf(2), kf(3, bad=1)]),
           ("points", [ls.mp(100, [1]), ls.mp(101, [2, 3, 1]), ls.mp(102, [1]), ls.mp(103), ls.mp(104, [1], bad=1)]),
           ("scales", SCALES),
           ("poses", [1, 2, 3], [pose(), pose(t=(0, 0, 1)), pose(t=(0, 0, -8))]),
           ("geo", [geo(100, (0, 0, 4), 1, level=1), geo(101, (0, 0, 3), 1, by=2, byref=2), geo(102, (-0.0, 0, 5), 3, level=2),
                    geo(103, (0, 0, 2), 1), geo(104, (7, 7, 7), 1)]),
           ("essential_commit", 2, [2, 1], [sim3((0, 0, 1)), sim3()], [sim3((0, 0, 2)), sim3((0, 0, 1), 2.0)])]
    e = {"Tiw": [pose(t=(0, 0, 2)), pose(t=(0, 0, 0.5))], "Swc": [sim3((0, 0, -2)), sim3((0, 0, -0.5), 0.5)],
         "points": [100, 101, 102, 103], "ref": [1, 2, 3, 1],
         "world": [(0, 0, 1.5), (0, 0, 2), (0, 0, 5), (0, 0, 0.5)], "positive_zero": (2, 0),
         "normal": [(0, 0, 1), (0, 0, 1.0 / 3.0), (0, 0, 1), (0, 0, 0)],
         "max_distance": [4, 2.5, 12, 0], "min_distance": [1, 0.625, 3, 0], "status": [NORMAL, NORMAL, NORMAL, 0]}
    state = {"poses": {1: pose(t=(0, 0, 0.5)), 2: pose(t=(0, 0, 2)), 3: pose(t=(0, 0, -8))},
             "centres": {1: (0, 0, -0.5), 2: (0, 0, -2), 3: (0, 0, 8)},
             "points": {100: (0, 0, 1.5), 101: (0, 0, 2), 102: (0, 0, 5), 103: (0, 0, 0.5), 104: (7, 7, 7)},
             "stamps": {101: (2, 2), 100: (0, 0)}}
    return ops, [e], dict(points_moved=4, points_identity=1), state


def check_state(store, state):
    for h, T in state["poses"].items():
        assert np.array_equal(store.get_poses([h])["Tcw"][0], np.asarray(T, np.float32)), h
    for h, c in state["centres"].items():
        g = store.get_poses([h])
        assert np.array_equal(g["Ow"][0], np.asarray(c, np.float32)) and np.array_equal(g["Twc"][0][:3, 3], np.asarray(c, np.float32)), h
    for h, x in state["points"].items():
        assert np.array_equal(store.get_point_geometry([h])["world"][0], np.asarray(x, np.float32)), h
    for h, (by, byref) in state["stamps"].items():
        g = store.get_point_geometry([h])
        assert (int(g["corrected_by"][0]), int(g["corrected_ref"][0])) == (by, byref), h


HAND_EDGES = {f.__name__: f for f in (covisibility_prefixes, covisibility_drop_reasons, loop_connection_rules,
                                      rank_order_is_not_handle_order, no_refusal_without_an_edge)}


# ---- every refusal ---------------------------------------------------------------------------------------------------------------

def refusals():
    """(name, script, the refused call as an operation, code, the handle its message names or None)"""
    I = sim3()
    base = [("kfs", [kf(1), kf(2, parent=1), kf(3), kf(4, bad=1)]), on_x([1, 2, 3, 4]), ("scales", SCALES),
            ("points", [ls.mp(100, [1, 2])]), ("geo", [geo(100, (0, 0, 4), 1)]),
            ("conn", [conn(3, weights=[(4, 150), (2, 120)], ordered=[(2, 120), (1, 4)]), conn(4, weights=[(3, 150)])])]
    edges = lambda *a, **k: ("essential_edges",) + a
    out = [
        ("table_names_a_handle_twice", base, edges(1, 3, [(2, I, I), (2, I, I)], []), "INVALID", 2),
        ("loop_connections_name_a_key_twice", base, edges(1, 3, [], [(3, [1]), (3, [2])]), "INVALID", 3),
        ("loop_connection_row_names_a_member_twice", base, edges(1, 3, [], [(3, [2, 2])]), "INVALID", 2),
        ("loop_kf_unknown", base, edges(9, 3, [], []), "STATE", 9),
        ("cur_kf_unknown", base, edges(1, 9, [], []), "STATE", 9),
        ("loop_connection_key_unknown", base, edges(1, 3, [], [(9, [1])]), "STATE", 9),
        ("loop_connection_member_unknown", base, edges(1, 3, [], [(3, [9])]), "STATE", 9),
        ("kept_loop_connection_member_is_bad", base, edges(1, 3, [], [(3, [4])]), "STATE", 4),
        ("kept_member_of_a_bad_key", base, edges(1, 3, [], [(4, [3])]), "STATE", 4),
        ("key_frame_without_pose_outside_the_table", base + [("kfs", [kf(5)])], edges(1, 3, [(2, I, I)], []), "STATE", 5),
        ("parent_is_bad", base + [("kfs", [kf(5, parent=4)]), on_x([5])], edges(1, 3, [], []), "STATE", 4),
        ("loop_edge_of_a_smaller_handle_is_bad", base + [("kfs", [kf(5)]), on_x([5]), ("loop_edges", [(5, [4])])], edges(1, 3, [], []), "STATE", 4),
        ("loop_edge_of_a_smaller_handle_is_unknown", base + [("loop_edges", [(3, [0])])], edges(1, 3, [], []), "STATE", 0),
        ("vertices_capacity_short", base, edges(1, 3, [], []) + ((2, 16),), "CAPACITY", None),
        ("edges_capacity_short", base, edges(1, 3, [], [(3, [2])]) + ((3, 1),), "CAPACITY", None),
    ]
    commit = lambda hs, cur=3: ("essential_commit", cur, hs, [I] * len(hs), [I] * len(hs))
    out += [
        ("commit_names_an_unknown_key_frame", base, commit([1, 2, 3, 9]), "INVALID", 9),
        ("commit_names_a_key_frame_twice", base, commit([1, 2, 3, 3]), "INVALID", 3),
        ("commit_names_a_bad_key_frame", base, commit([1, 2, 3, 4]), "STATE", 4),
        ("commit_misses_a_key_frame", base, commit([1, 3]), "STATE", 2),
        ("point_without_geometry", base + [("points", [ls.mp(101, [1])])], commit([1, 2, 3]), "STATE", 101),
        ("reference_key_frame_unknown", base + [("geo", [geo(100, (0, 0, 4), 9)])], commit([1, 2, 3]), "STATE", 100),
        ("nIDr_is_not_a_stored_key_frame", base + [("geo", [geo(100, (0, 0, 4), 1, by=3, byref=9)])], commit([1, 2, 3]), "STATE", 100),
        ("ref_level_out_of_range", base + [("geo", [geo(100, (0, 0, 4), 1, level=3)])], commit([1, 2, 3]), "STATE", 100),
        ("observer_not_named_and_without_a_pose", base + [("kfs", [kf(5, bad=1)]), ("points", [ls.mp(100, [1, 5])])], commit([1, 2, 3]), "STATE", 100),
        ("reference_not_named_and_without_a_pose", base + [("kfs", [kf(5, bad=1)]), ("geo", [geo(100, (0, 0, 4), 5)])], commit([1, 2, 3]), "STATE", 100),
        ("points_capacity_short", base, commit([1, 2, 3]) + (0,), "CAPACITY", None),
    ]
    no_scales = [op for op in base if op[0] != "scales"]
    out.append(("no_scale_factors", no_scales, commit([1, 2, 3]), "STATE", None))
    return out


def call(store, op, mode="host"):
    """the refused operation, with its capacity when the case gives one"""
    if op[0] == "essential_edges":
        return store.essential_edges(op[1], op[2], op[3], op[4], mode=mode, capacity=op[5] if len(op) > 5 else None)
    return store.essential_commit(op[1], op[2], op[3], op[4], mode=mode, capacity=op[5] if len(op) > 5 else None)


# ---- seeded maps and the shapes at the seams -------------------------------------------------------------------------------------

def rand_pose(rng):
    a = rng.normal(size=(3, 3))
    q, _ = np.linalg.qr(a)
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return pose(q.astype(np.float32), rng.uniform(-4, 4, 3).astype(np.float32))


def rand_sim3(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return list(q) + list(rng.uniform(-4, 4, 3)) + [float(rng.uniform(0.5, 2.0))]


def build(n_kf, n_pt, seed, prefix=None, n_bad=0, row=12):
    """A map of n_kf key frames whose handles are a permutation against their ranks, a spanning tree, loop edges, ordered rows with
    weights around 100 (prefix: every row is `prefix` entries at 100 or more, then one below; alternate entries are made children
    or loop edges so that they drop), n_bad bad key frames that only rows, observations and references name, and n_pt points.
    Returns (ops, edges operation, handles of the map in rank order, point handles)."""
    rng = np.random.default_rng(seed)
    total = n_kf + n_bad
    handles = [int(h) for h in rng.permutation(total) + 1]
    good, bad = handles[:n_kf], handles[n_kf:]
    rows = {h: kf(h, rank=10 * (i + 1)) for i, h in enumerate(good)}
    rows.update({h: kf(h, bad=1, rank=10 * (n_kf + i + 1)) for i, h in enumerate(bad)})
    for i, h in enumerate(good[1:], 1):
        p = good[int(rng.integers(0, i))]
        rows[h]["parent"] = p
        rows[p]["children"].append(h)
    loops = {h: set() for h in handles}
    for _ in range(max(1, n_kf // 3)):
        a, b = (int(x) for x in rng.choice(good, 2, replace=len(good) < 2))
        if a != b:
            loops[a].add(b)
            loops[b].add(a)
    conns = []
    for h in good:
        others = [o for o in handles if o != h]
        rng.shuffle(others)
        if prefix is None:
            others = others[:int(rng.integers(0, min(row, len(others)) + 1))]
            ws = sorted((int(w) for w in rng.integers(60, 160, len(others))), reverse=True)
        else:
            assert len(others) > prefix, "the map is too small for the prefix"
            others = others[:prefix + 1]
            ws = [100 + prefix - k for k in range(prefix)] + [50]
            for k in range(0, prefix, 2):                      # alternate entries drop: a loop edge of h, or bad
                if others[k] in good:
                    loops[h].add(others[k])
        pairs = list(zip(others, ws))
        conns.append(conn(h, weights=[(o, w) for o, w in pairs if rng.random() < 0.8], ordered=pairs))
    ops = [("kfs", list(rows.values())), ("scales", SCALES), ("poses", handles, [rand_pose(rng) for _ in handles]), ("conn", conns),
           ("loop_edges", [(h, sorted(s)) for h, s in loops.items() if s])]
    pts = list(range(1000, 1000 + n_pt))
    prow, grow = [], []
    cur = good[-1]
    for k, p in enumerate(pts):
        obs = [int(o) for o in rng.choice(handles, int(rng.integers(0, min(4, total) + 1)), replace=False)]
        is_bad = int(k % 7 == 3)
        prow.append(ls.mp(p, obs, bad=is_bad))
        by = cur if k % 3 == 0 else 0
        grow.append(geo(p, rng.uniform(-5, 5, 3).astype(np.float32), int(rng.choice(handles)), level=int(rng.integers(0, 3)), by=by,
                        byref=int(rng.choice(handles))))
    if pts:
        ops += [("points", prow), ("geo", grow)]
    table = [(h, rand_sim3(rng), rand_sim3(rng)) for h in good if rng.random() < 0.5]
    lcs = {}
    for _ in range(max(1, n_kf // 2)):
        a, b = (int(x) for x in rng.choice(good, 2, replace=len(good) < 2))
        if a != b:
            lcs.setdefault(a, set()).add(b)
    loop = good[0]
    lcs.setdefault(cur, set())
    if cur != loop:
        lcs[cur].add(loop)
    edges = ("essential_edges", loop, cur, table, [(k, sorted(v)) for k, v in lcs.items()])
    return ops, edges, good, pts


def script(n_kf, n_pt, seed, **kw):
    """the map, an edges call, a commit of perturbed estimates, a second edges call on the moved map"""
    ops, edges, good, pts = build(n_kf, n_pt, seed, **kw)
    rng = np.random.default_rng(seed + 1000)
    order = [int(h) for h in rng.permutation(good)]
    commit = ("essential_commit", edges[2], order, [rand_sim3(rng) for _ in order], [rand_sim3(rng) for _ in order])
    return ops + [edges, commit, edges]


def seeded(seed):
    return script(9 + seed, 40 + 5 * seed, seed, n_bad=2)
