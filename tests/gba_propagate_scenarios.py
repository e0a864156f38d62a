"""Hand-built maps for the map update that ends LoopClosing::RunGlobalBundleAdjustment (reference src/LoopClosing.cc:722-783), each
with the values it must leave written out by hand, builders for the shapes at the kernels' seams, and seeded random scripts.
Nothing here imports the library.

A script is a list of operations that play() runs on lib.LocalMap or on gba_propagate_numpy.Store: those of loop_correct_scenarios
and
    ("gba_kfs", handles, TcwGBA [n, 4, 4], stamps)  ("gba_pts", handles, PosGBA [n, 3], stamps)  ("gba", loop, origins)
The hand cases use poses that are integer translations and quarter turns about z, so every float product in them is exact and the
expected values are literals (compared by value: a zero may carry either sign).  A scenario returns (script, expect): expect has,
per gba of the script, the hand-written outputs."""
import itertools

import numpy as np

import gba_propagate_numpy as gn
import loop_correct_scenarios as rs
import lmap_scenarios as ls

KEYFRAME, POINT = ls.KEYFRAME, ls.POINT
RZ = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]            # a quarter turn about z: (x, y, z) -> (-y, x, z)
pose, geo = rs.pose, rs.geo


def play(ops, store, mode="host"):
    out = []
    for op in ops:
        if op[0] == "gba_kfs":
            store.set_gba_keyframes(op[1], op[2], op[3])
        elif op[0] == "gba_pts":
            store.set_gba_points(op[1], op[2], op[3])
        elif op[0] == "gba":
            out.append(store.gba(op[1], op[2], mode=mode))
        else:
            out += rs.play([op], store, mode=mode)
    return out


def alive(ops):
    kfs, pts = set(), set()
    for op in ops:
        if op[0] == "kfs":
            kfs |= {r["handle"] for r in op[1]}
        elif op[0] == "points":
            pts |= {r["handle"] for r in op[1]}
        elif op[0] == "remove":
            (kfs if op[1] == KEYFRAME else pts).discard(op[2])
    return sorted(kfs), sorted(pts)


def check(results, expect):
    calls = [r for r in results if "composed" in r]
    assert len(calls) == len(expect)
    for r, e in zip(calls, expect):
        for k, want in e.items():
            got = np.asarray(r[k])
            want = np.asarray(want, got.dtype).reshape((len(want),) + got.shape[1:])
            assert got.shape == want.shape and np.array_equal(got, want), (k, got, want)


def kf(h, children=(), parent=-1, bad=0, rank=None):
    return dict(handle=h, rank=h if rank is None else rank, children=list(children), parent=parent, bad=bad)


def pt(h, bad=0):
    return dict(handle=h, bad=bad)


def three_levels():
    """1 is the origin with children 2 and 4; 3 is the child of 2 and was made while the adjustment ran (no state).  5 stands apart.
    The FIFO is 1, 2, 4, 3.  Key frame 3: Tchildc = [Rz | (0, 1, 0)] * [I | (-3, 0, 0)] = [Rz | (0, -2, 0)], then times
    [I | (5, 0, 0)] = [Rz | (0, 3, 0)].  Point 10 holds the stamp; 11 goes through the stamped 2: (1, 2, 3) + (3, 0, 0), then
    - (5, 0, 0); 12 through the composed 3: Rz (1, 0, 0) + (0, 1, 0) = (0, 2, 0), then Rz^T (0, 2, 0) - Rz^T (0, 3, 0) = (2, 0, 0) -
    (3, 0, 0); 13 is bad; 14 has the unstamped, unreached 5 for reference."""
    ops = [("kfs", [kf(1, [2, 4]), kf(2, [3], 1), kf(3, [], 2), kf(4, [], 1), kf(5)]),
           ("points", [pt(10), pt(11), pt(12), pt(13, 1), pt(14)]),
           ("scales", [1.0]),
           ("poses", [1, 2, 3, 4, 5], [pose(t=(1, 0, 0)), pose(t=(3, 0, 0)), pose(RZ, (0, 1, 0)), pose(t=(0, 0, 1)), pose()]),
           ("geo", [geo(10, (1, 1, 1), 1), geo(11, (1, 2, 3), 2), geo(12, (1, 0, 0), 3), geo(13, (4, 4, 4), 1), geo(14, (5, 5, 5), 5)]),
           ("gba_kfs", [1, 2, 4], [pose(t=(2, 0, 0)), pose(t=(5, 0, 0)), pose(t=(0, 0, 4))], [7, 7, 7]),
           ("gba_pts", [10, 13], [(9, 9, 9), (8, 8, 8)], [7, 7]),
           ("gba", 7, [1])]
    expect = [dict(keyframes=[1, 2, 4, 3], composed=[0, 0, 0, 1],
                   Tcw=[pose(t=(2, 0, 0)), pose(t=(5, 0, 0)), pose(t=(0, 0, 4)), pose(RZ, (0, 3, 0))],
                   TcwBef=[pose(t=(1, 0, 0)), pose(t=(3, 0, 0)), pose(t=(0, 0, 1)), pose(RZ, (0, 1, 0))],
                   points=[10, 11, 12], kind=[1, 2, 2], world=[(9, 9, 9), (-1, 2, 3), (-1, 0, 0)])]
    return ops, expect


def chain_of_two():
    """1 -> 2 -> 3 with only 1 adjusted.  2: [I | (3, 0, 0)] * [I | (-1, 0, 0)] = [I | (2, 0, 0)], times [I | (2, 0, 0)] =
    [I | (4, 0, 0)].  3: [Rz | (0, 1, 0)] * [I | (-3, 0, 0)] (the old pose of 2) = [Rz | (0, -2, 0)], times the composed
    [I | (4, 0, 0)] = [Rz | (0, 2, 0)].  Had the inverse of 1 been taken after its SetPose, 2 would end at [I | (3, 0, 0)]."""
    ops = [("kfs", [kf(1, [2]), kf(2, [3], 1), kf(3, [], 2)]),
           ("scales", [1.0]),
           ("poses", [1, 2, 3], [pose(t=(1, 0, 0)), pose(t=(3, 0, 0)), pose(RZ, (0, 1, 0))]),
           ("gba_kfs", [1], [pose(t=(2, 0, 0))], [3]),
           ("gba", 3, [1])]
    expect = [dict(keyframes=[1, 2, 3], composed=[0, 1, 1],
                   Tcw=[pose(t=(2, 0, 0)), pose(t=(4, 0, 0)), pose(RZ, (0, 2, 0))],
                   TcwBef=[pose(t=(1, 0, 0)), pose(t=(3, 0, 0)), pose(RZ, (0, 1, 0))], points=[], kind=[])]
    return ops, expect


def the_two_readings_differ():
    """on the restatement: the inverse before SetPose against the inverse after it"""
    ops, _ = chain_of_two()
    a, b = gn.Store(), gn.Store()
    play(ops[:-1], a)
    play(ops[:-1], b)
    ra, rb = a.gba(3, [1]), b.gba(3, [1], inverse_after_set_pose=True)
    assert not np.array_equal(ra["Tcw"][1], rb["Tcw"][1])
    assert np.array_equal(rb["Tcw"][1], pose(t=(3, 0, 0)))
    return True


def stamps_after_the_walk():
    """2 is unstamped but reached, so 20 moves through it (kind 2, with the composed pose [I | (4, 0, 0)] and the old [I | (3, 0, 0)]:
    (1, 1, 1) + 3 - 4); 5 is unstamped and not reached, so 21 stays."""
    ops = [("kfs", [kf(1, [2]), kf(2, [], 1), kf(5)]), ("points", [pt(20), pt(21)]), ("scales", [1.0]),
           ("poses", [1, 2, 5], [pose(t=(1, 0, 0)), pose(t=(3, 0, 0)), pose()]),
           ("geo", [geo(20, (1, 1, 1), 2), geo(21, (2, 2, 2), 5)]),
           ("gba_kfs", [1], [pose(t=(2, 0, 0))], [3]), ("gba", 3, [1])]
    expect = [dict(keyframes=[1, 2], composed=[0, 1], points=[20], kind=[2], world=[(0, 1, 1)])]
    return ops, expect


def loop_zero():
    """nLoopKF == 0 with untouched stamps: 2 has mTcwGBA and stamp 0, so it is not composed; the points take mPosGBA"""
    ops = [("kfs", [kf(1, [2]), kf(2, [], 1)]), ("points", [pt(20)]), ("scales", [1.0]),
           ("poses", [1, 2], [pose(t=(1, 0, 0)), pose(t=(3, 0, 0))]), ("geo", [geo(20, (1, 1, 1), 2)]),
           ("gba_kfs", [1, 2], [pose(t=(2, 0, 0)), pose(t=(7, 0, 0))], [0, 0]), ("gba_pts", [20], [(6, 6, 6)], [0]), ("gba", 0, [1])]
    expect = [dict(keyframes=[1, 2], composed=[0, 0], Tcw=[pose(t=(2, 0, 0)), pose(t=(7, 0, 0))], points=[20], kind=[1],
                   world=[(6, 6, 6)])]
    return ops, expect


def bad_keyframes_count():
    """the bad 2 is still in the children row of 1 and is walked; it is the reference of 20 and is used"""
    ops, _ = stamps_after_the_walk()
    ops[0] = ("kfs", [kf(1, [2]), kf(2, [], 1, bad=1), kf(5)])
    expect = [dict(keyframes=[1, 2], composed=[0, 1], points=[20], kind=[2], world=[(0, 1, 1)])]
    return ops, expect


def sibling_orders():
    """the children 2, 3, 4 of 1 (ranks 30, 10, 20) given in every order of the setter: the visited list follows rank"""
    out = []
    for perm in itertools.permutations([2, 3, 4]):
        ops = [("kfs", [dict(handle=1, rank=1, children=list(perm))] + [dict(handle=h, rank=r, parent=1) for h, r in ((2, 30), (3, 10), (4, 20))]),
               ("scales", [1.0]), ("poses", [1, 2, 3, 4], [pose(t=(h, 0, 0)) for h in (1, 2, 3, 4)]),
               ("gba_kfs", [1, 2, 3, 4], [pose(t=(0, h, 0)) for h in (1, 2, 3, 4)], [5, 5, 5, 5]), ("gba", 5, [1])]
        out.append((ops, [dict(keyframes=[1, 3, 4, 2], composed=[0, 0, 0, 0])]))
    return out


def origins(n):
    """n origins with a child each; the FIFO takes the origins in the caller's order, then their children"""
    roots = [10 * (i + 1) for i in range(n)]
    ops = [("kfs", [kf(r, [r + 1]) for r in roots] + [kf(r + 1, [], r) for r in roots]), ("scales", [1.0]),
           ("poses", roots + [r + 1 for r in roots], [pose(t=(r, 0, 0)) for r in roots] + [pose(t=(r + 1, 0, 0)) for r in roots]),
           ("gba_kfs", roots, [pose(t=(0, r, 0)) for r in roots], [4] * n), ("gba", 4, roots[::-1])]
    want = roots[::-1] + [r + 1 for r in roots[::-1]]
    # child: [I | (r + 1)] * [I | (-r)] = [I | (1, 0, 0)], times [I | (0, r, 0)] = [I | (1, r, 0)]
    expect = [dict(keyframes=want, composed=[0] * n + [1] * n, Tcw=[pose(t=(0, r, 0)) for r in roots[::-1]] + [pose(t=(1, r, 0)) for r in roots[::-1]])]
    return ops, expect


def second_call():
    """a second adjustment on the store the first left: 2 reads the pose the first call composed, and the point 21 of the unreached,
    stamped 5 goes through the mTcwBefGBA the first call of 5 left, stale as it is.  First call (loop 3, origins 1 and 5): 5 goes
    from [I | 0] to [I | (0, 0, 2)].  Second call (loop 9, origin 1 only; 5 is given the stamp 9 by hand but not walked): 21 at
    (2, 2, 2) -> Xc with the stale [I | 0] = (2, 2, 2), then - (0, 0, 2)."""
    ops, _ = stamps_after_the_walk()
    ops = ops[:-2] + [("gba_kfs", [1, 5], [pose(t=(2, 0, 0)), pose(t=(0, 0, 2))], [3, 3]), ("gba", 3, [1, 5]),
                      ("gba_kfs", [1, 5], [pose(t=(0, 0, 0)), pose(t=(0, 0, 2))], [9, 9]), ("gba", 9, [1])]
    # after the first: 2 at [I | (4, 0, 0)], 20 at (0, 1, 1), 21 (ref 5, reached) at (2, 2, 2) + 0 - (0, 0, 2) = (2, 2, 0).
    # second: 2 = [I | (4, 0, 0)] * [I | (-2, 0, 0)] * [I | 0] = [I | (2, 0, 0)]; 20: (0, 1, 1) + 4 - 2 = (2, 1, 1); 21: (2, 2, 0) - (0, 0, 2)
    expect = [dict(keyframes=[1, 5, 2], composed=[0, 0, 1], points=[20, 21], kind=[2, 2], world=[(0, 1, 1), (2, 2, 0)]),
              dict(keyframes=[1, 2], composed=[0, 1], Tcw=[pose(), pose(t=(2, 0, 0))], TcwBef=[pose(t=(2, 0, 0)), pose(t=(4, 0, 0))],
                   points=[20, 21], kind=[2, 2], world=[(2, 1, 1), (2, 2, -2)])]
    return ops, expect


HAND = {"three_levels": three_levels, "chain_of_two": chain_of_two, "stamps_after_the_walk": stamps_after_the_walk,
        "loop_zero": loop_zero, "bad_keyframes_count": bad_keyframes_count, "two_origins": lambda: origins(2),
        "three_origins": lambda: origins(3), "second_call": second_call}


# ---- refusals: (name, script up to the call, (loop, origins), status name, the handle the message names) -------------------------

def refusals():
    base, _ = three_levels()
    base = base[:-1]
    out = []

    def case(name, extra, call, rc, handle, drop=None):
        ops = [op for op in base if op[0] != drop] if drop else list(base)
        out.append((name, ops + extra, call, rc, handle))

    case("unknown_origin", [], (7, [99]), "state", 99)
    case("origin_without_pose", [("kfs", [kf(6)]), ("gba_kfs", [6], [pose()], [7])], (7, [1, 6]), "state", 6)
    case("reached_without_pose", [("kfs", [kf(4, [6], 1), kf(6, [], 4)])], (7, [1]), "state", 6)
    case("stamped_without_TcwGBA", [("kfs", [kf(4, [6], 1), kf(6, [], 4)]), ("poses", [6], [pose()]), ("gba", 7, [1]),
                                    ("kfs", [kf(6, [8], 4), kf(8, [], 6)]), ("poses", [8], [pose()])], (0, [1]), "state", 8)
    case("origin_without_TcwGBA", [], (7, [5]), "state", 5)
    case("two_children_rows", [("kfs", [kf(4, [3], 1)])], (7, [1]), "state", 3)
    case("origin_as_child", [], (7, [1, 2]), "state", 2)
    case("cycle", [("kfs", [kf(3, [1], 2)])], (7, [1]), "state", 1)
    zero = [op for op in loop_zero()[0][:-1] if op[0] != "gba_pts"]      # the stamp 0 of a point without state is nLoopKF
    out.append(("kind1_without_PosGBA", zero, (0, [1]), "state", 20))
    case("point_without_geometry", [("points", [pt(15)])], (7, [1]), "state", 15)
    case("unknown_reference", [("points", [pt(15)]), ("geo", [geo(15, (1, 1, 1), 77)])], (7, [1]), "state", 15)
    case("reference_without_pose", [("kfs", [kf(6)]), ("gba_kfs", [6], [pose()], [7]), ("points", [pt(15)]),
                                    ("geo", [geo(15, (1, 1, 1), 6)])], (7, [1]), "state", 15)
    case("unreached_without_TcwBefGBA", [("gba_kfs", [5], [pose()], [7])], (7, [1]), "state", 14)
    case("no_origins", [], (7, []), "invalid", None)
    case("duplicate_origin", [], (7, [1, 1]), "invalid", None)
    return out


# ---- shapes at the kernels' seams -------------------------------------------------------------------------------------------------

def rot(rng):
    """a general rotation (float32 of a QR factor) with a translation"""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return pose(q.astype(np.float32), rng.uniform(-3, 3, 3))


def points_shape(n_points, moving, seed=0):
    """two key frames, 1 adjusted with the child 2 composed, and n_points points that alternate between mPosGBA and the way
    through 2.  moving: "none" (every point has the unstamped, unreached 3 for reference), "all", or "alternate" (the odd ones
    stay)."""
    rng = np.random.default_rng(seed)
    hs = list(range(100, 100 + n_points))
    stays = lambda i: moving == "none" or (moving == "alternate" and i % 2 == 1)
    ops = [("kfs", [kf(1, [2]), kf(2, [], 1), kf(3)]), ("points", [pt(h) for h in hs]), ("scales", [1.0]),
           ("poses", [1, 2, 3], [rot(rng), rot(rng), rot(rng)]),
           ("geo", [geo(h, rng.uniform(-5, 5, 3), 3 if stays(i) else 2) for i, h in enumerate(hs)]),
           ("gba_kfs", [1], [rot(rng)], [4])]
    stamped = [h for i, h in enumerate(hs) if not stays(i) and i % 4 < 2]
    if stamped:
        ops.append(("gba_pts", stamped, rng.uniform(-5, 5, (len(stamped), 3)), [4] * len(stamped)))
    ops.append(("gba", 4, [1]))
    return ops


def many_points(n_points, seed=0):
    """points_shape(n_points, "all") for a large n_points: drawn at once"""
    rng = np.random.default_rng(seed)
    hs = np.arange(100, 100 + n_points)
    X = rng.uniform(-5, 5, (n_points, 3))
    stamped = hs[np.arange(n_points) % 4 < 2]
    return [("kfs", [kf(1, [2]), kf(2, [], 1), kf(3)]), ("points", [pt(int(h)) for h in hs]), ("scales", [1.0]),
            ("poses", [1, 2, 3], [rot(rng), rot(rng), rot(rng)]),
            ("geo", [dict(handle=int(h), world=x, ref_kf=2) for h, x in zip(hs, X)]),
            ("gba_kfs", [1], [rot(rng)], [4]), ("gba_pts", stamped, rng.uniform(-5, 5, (len(stamped), 3)), [4] * len(stamped)),
            ("gba", 4, [1])]


def chain_shape(depths, seed=0, siblings=0):
    """an adjusted origin 1 with one chain of unstamped key frames per entry of depths under it, and `siblings` more unstamped
    children of 1; a point on every key frame"""
    rng = np.random.default_rng(seed)
    rows, h, kids = {1: kf(1)}, 2, []
    for d in depths:
        parent = 1
        for _ in range(d):
            rows[h] = kf(h, [], parent)
            rows[parent]["children"].append(h)
            parent, h = h, h + 1
    for _ in range(siblings):
        rows[h] = kf(h, [], 1)
        rows[1]["children"].append(h)
        h += 1
    hs = sorted(rows)
    ops = [("kfs", [rows[k] for k in hs]), ("points", [pt(1000 + k) for k in hs]), ("scales", [1.0]),
           ("poses", hs, [rot(rng) for _ in hs]), ("geo", [geo(1000 + k, rng.uniform(-5, 5, 3), k) for k in hs]),
           ("gba_kfs", [1], [rot(rng)], [6]), ("gba", 6, [1])]
    return ops


def seeded(seed, n_kf=40, n_pt=600):
    """a random tree, random stamps, general rotations; three adjustments interleaved with a CorrectLoop call and pose edits"""
    rng = np.random.default_rng(seed)
    hs = list(range(1, n_kf + 1))
    rows = {h: kf(h, rank=int(rng.integers(1, 10 ** 6)) * 64 + h) for h in hs}
    for h in hs[1:]:
        p = int(rng.integers(1, h))
        rows[h]["parent"] = p
        rows[p]["children"].append(h)
    ph = list(range(1000, 1000 + n_pt))
    obs = {p: sorted(set(int(v) for v in rng.integers(1, n_kf + 1, 3))) for p in ph}
    for h in hs:
        rows[h]["points"] = [p for p in ph if h in obs[p]][:40]
    ops = [("kfs", [rows[h] for h in hs]),
           ("points", [dict(handle=p, bad=int(rng.random() < 0.05), obs=[h for h in obs[p] if p in rows[h]["points"]]) for p in ph]),
           ("scales", [1.0, 1.2, 1.44]), ("poses", hs, [rot(rng) for _ in hs]),
           ("geo", [geo(p, rng.uniform(-5, 5, 3), obs[p][0], level=int(rng.integers(0, 3))) for p in ph])]
    for loop in (11, 12, 13):
        adj = [h for h in hs if h == 1 or rng.random() < 0.8]
        ops.append(("gba_kfs", adj, [rot(rng) for _ in adj], [loop] * len(adj)))
        pa = [p for p in ph if rng.random() < 0.7]
        ops.append(("gba_pts", pa, rng.uniform(-5, 5, (len(pa), 3)), [loop] * len(pa)))
        ops.append(("gba", loop, [1]))
        if loop == 11:
            q = rng.standard_normal(4)
            called = sorted(set([5] + [int(v) for v in rng.integers(1, n_kf + 1, 6)]))
            ops.append(("correct", 5, rs.scw(q / np.linalg.norm(q), rng.uniform(-1, 1, 3), 1.25), called))
        else:
            ed = [int(v) for v in rng.integers(1, n_kf + 1, 4)]
            ops.append(("poses", ed, [rot(rng) for _ in ed]))
            ops.append(("kfs", [rows[ed[0]]]))
    return ops
