"""Hand-built maps for the Sim3 propagation of LoopClosing::CorrectLoop (reference src/LoopClosing.cc:480-562), each with the
values it must leave written out by hand, and seeded random scripts.  Nothing here imports the library.

A script is a list of operations that play() runs on lib.LocalMap or on loop_correct_numpy.Store: those of conn_scenarios and
    ("scales", factors)  ("poses", handles, Tcw [n, 4, 4])  ("geo", rows)  ("correct", cur, Scw, handles)
The hand cases use rotations by half turns, translations and scales that are small integers and powers of two, and points on the
z axis, so every product, sum, quotient and square root in them is exact and the expected values are literals.  A scenario
returns (script, expect): expect has, per correct of the script, the hand-written outputs (a key that is left out is not compared)
and under "state_poses" / "state_centres" / "state_points" what the store holds afterwards."""
import numpy as np

import conn_scenarios as cs
import lmap_scenarios as ls

KEYFRAME, POINT, LINE = ls.KEYFRAME, ls.POINT, ls.LINE
NORMAL = 2
SCALES = [1.0, 2.0, 4.0]
ID_Q = (0.0, 0.0, 0.0, 1.0)


def pose(R=None, t=(0.0, 0.0, 0.0)):
    T = np.eye(4, dtype=np.float32)
    if R is not None:
        T[:3, :3] = np.asarray(R, np.float32)
    T[:3, 3] = np.asarray(t, np.float32)
    return T


def geo(h, world, ref, level=0, by=0, byref=0):
    return dict(handle=h, world=[float(v) for v in world], ref_kf=ref, ref_level=level, corrected_by=by, corrected_ref=byref)


def scw(q=ID_Q, t=(0.0, 0.0, 0.0), s=1.0):
    return np.array(list(q) + list(t) + [s], np.float64)


def play(ops, store, mode="host"):
    """the results of the script's corrects, connects and updates, in order"""
    out = []
    for op in ops:
        if op[0] == "scales":
            store.set_scales(op[1])
        elif op[0] == "poses":
            store.set_poses(op[1], op[2])
        elif op[0] == "geo":
            store.set_point_geometry(op[1])
        elif op[0] == "correct":
            out.append(store.correct(op[1], op[2], op[3], mode=mode))
        else:
            out += cs.play([op], store, mode=mode)
    return out


def check(results, expect, store):
    corrects = [r for r in results if "claimed_by" in r]
    assert len(corrects) == len(expect)
    for r, e in zip(corrects, expect):
        for k, want in e.items():
            if k.startswith("state_"):
                continue
            got = np.asarray(r[k])
            want = np.asarray(want, got.dtype).reshape((len(want),) + got.shape[1:])
            assert got.shape == want.shape and np.array_equal(got, want), (k, got, want)
    last = expect[-1]
    for h, T in last.get("state_poses", {}).items():
        assert np.array_equal(store.get_poses([h])["Tcw"][0], np.asarray(T, np.float32)), h
    for h, c in last.get("state_centres", {}).items():
        g = store.get_poses([h])
        assert np.array_equal(g["Ow"][0], np.asarray(c, np.float32)), h
        assert np.array_equal(g["Twc"][0][:3, 3], np.asarray(c, np.float32)), h
    for h, (world, by, byref) in last.get("state_points", {}).items():
        g = store.get_point_geometry([h])
        assert np.array_equal(g["world"][0], np.asarray(world, np.float32)), h
        assert (int(g["corrected_by"][0]), int(g["corrected_ref"][0])) == (by, byref), h


def z(v):
    return (0.0, 0.0, float(v))


# ---- the hand cases ------------------------------------------------------------------------------------------------------------

def identity_scale_two():
    """all poses identity, Scw = (identity, (1, 2, 3), 2): x -> x / 2 - (0.5, 1, 1.5).  The point (1, 1, 1) seen by cur moves to
    (0, -0.5, -1); (1, 2, 11) lands on (0, 0, 4); cur's new pose has t = (0.5, 1, 1.5) and centre (-0.5, -1, -1.5)."""
    ops = [("kfs", [ls.kf(5, 10, pts=[100, -1, 101])]), ("points", [ls.mp(100, [5]), ls.mp(101, [5])]), ("scales", SCALES),
           ("poses", [5], [pose()]), ("geo", [geo(100, (1, 1, 1), 5), geo(101, (1, 2, 11), 5, level=1)]),
           ("correct", 5, scw(t=(1, 2, 3), s=2), [5])]
    T = pose(t=(0.5, 1, 1.5))
    expect = [dict(walk_pos=[0], corrected=[[0, 0, 0, 1, 1, 2, 3, 2]], non_corrected=[[0, 0, 0, 1, 0, 0, 0, 1]], Tiw=[T],
                   points=[100, 101], claimed_by=[5, 5], world=[[0, -0.5, -1], [0, 0, 4]], status=[NORMAL, NORMAL],
                   state_poses={5: T}, state_centres={5: (-0.5, -1, -1.5)},
                   state_points={100: ((0, -0.5, -1), 5, 5), 101: ((0, 0, 4), 5, 5)})]
    return ops, expect


def shared_points(order=(1, 2, 3)):
    """1 (rank 1, t = (1, 0, 0)), 2 (rank 2) and cur 3 (rank 3): point 100 is in the rows of 2 and 3, point 101 in all three; the
    lowest rank claims, whatever the call order.  Corrected_1 = (identity, (2, 2, 3), 2), its new pose t = (1, 1, 1.5)."""
    ops = [("kfs", [ls.kf(1, 1, pts=[101]), ls.kf(2, 2, pts=[100, 101]), ls.kf(3, 3, pts=[101, 100])]),
           ("points", [ls.mp(100, [2, 3]), ls.mp(101, [1, 2, 3])]), ("scales", SCALES),
           ("poses", [1, 2, 3], [pose(t=(1, 0, 0)), pose(), pose()]),
           ("geo", [geo(100, (1, 2, 11), 3), geo(101, (1, 2, 11), 3)]), ("correct", 3, scw(t=(1, 2, 3), s=2), list(order))]
    by = {1: 0, 2: 1, 3: 2}
    expect = [dict(walk_pos=[by[h] for h in order], points=[101, 100], claimed_by=[1, 2], world=[[0, 0, 4], [0, 0, 4]],
                   state_poses={1: pose(t=(1, 1, 1.5)), 2: pose(t=(0.5, 1, 1.5)), 3: pose(t=(0.5, 1, 1.5))},
                   state_centres={1: (-1, -1, -1.5), 2: (-0.5, -1, -1.5)},
                   state_points={100: ((0, 0, 4), 3, 2), 101: ((0, 0, 4), 3, 1)})]
    return ops, expect


def observers_and_references():
    """Scw = (identity, 0, 2) halves every position and centre.  Called: 1 (rank 1), cur 2 (rank 2), 3 (rank 3); 9 is not called.
    1 and 3 sit at (0, 0, 6) and move to (0, 0, 3); 2 sits at the origin; 9 at (0, 0, -4).  Every point is at (0, 0, 8), in the
    row of 2 only, and moves to (0, 0, 4).  Point 100 is observed by 1, 2, 3 and 9: 1 is before the claimant (new centre, below
    the point: +1), 2 is the claimant (stored: +1), 3 comes after (stored, above: -1), 9 is not called (+1): normal (0, 0, 2/4);
    all stored centres would give 0 and all new ones 1.  Its reference 9 is 8 away.  Points 101, 102, 103: references 9 (not an
    observer), 1 (called, earlier: new centre, 1 away) and 3 (called, later: stored centre, 2 away)."""
    ops = [("kfs", [ls.kf(1, 1), ls.kf(2, 2, pts=[100, 101, 102, 103]), ls.kf(3, 3), ls.kf(9, 9)]),
           ("points", [ls.mp(100, [1, 2, 3, 9]), ls.mp(101, [2]), ls.mp(102, [2]), ls.mp(103, [2])]), ("scales", SCALES),
           ("poses", [1, 2, 3, 9], [pose(t=z(-6)), pose(), pose(t=z(-6)), pose(t=z(4))]),
           ("geo", [geo(100, z(8), 9, level=1), geo(101, z(8), 9, level=0), geo(102, z(8), 1, level=1), geo(103, z(8), 3, level=2)]),
           ("correct", 2, scw(s=2), [3, 2, 1])]
    expect = [dict(walk_pos=[2, 1, 0], points=[100, 101, 102, 103], claimed_by=[2, 2, 2, 2], world=[z(4)] * 4,
                   normal=[z(0.5), z(1), z(1), z(1)], max_distance=[16, 8, 2, 8], min_distance=[4, 2, 0.5, 2], status=[NORMAL] * 4,
                   state_centres={1: z(3), 2: z(0), 3: z(3), 9: z(-4)}, state_points={100: (z(4), 2, 2), 103: (z(4), 2, 2)})]
    return ops, expect


def skipped_entries():
    """null, bad and already stamped entries are skipped, a second mention too; a point without observations moves but gets no
    normal"""
    ops = [("kfs", [ls.kf(7, 1, pts=[-1, 100, 101, 102, 103, 102])]),
           ("points", [ls.mp(100, [7], bad=1), ls.mp(101, [7]), ls.mp(102, [7]), ls.mp(103, [])]), ("scales", SCALES), ("poses", [7], [pose()]),
           ("geo", [geo(100, z(8), 7), geo(101, z(8), 7, by=7, byref=3), geo(102, z(8), 7, by=3, byref=7), geo(103, z(8), 7)]),
           ("correct", 7, scw(s=2), [7])]
    expect = [dict(points=[102, 103], claimed_by=[7, 7], world=[z(4), z(4)], normal=[z(1), z(0)], max_distance=[4, 0],
                   min_distance=[1, 0], status=[NORMAL, 0],
                   state_points={100: (z(8), 0, 0), 101: (z(8), 7, 3), 102: (z(4), 7, 7), 103: (z(4), 7, 7)})]
    return ops, expect


def current_zero():
    """mpCurrentKF->mnId == 0 meets the constructors' mnCorrectedByKF = 0: no point moves, the poses still do"""
    ops = [("kfs", [ls.kf(0, 5, pts=[100]), ls.kf(1, 6, pts=[100, 101])]), ("points", [ls.mp(100, [0, 1]), ls.mp(101, [1])]),
           ("scales", SCALES), ("poses", [0, 1], [pose(), pose()]), ("geo", [geo(100, z(8), 0), geo(101, z(8), 1)]),
           ("correct", 0, scw(t=(1, 2, 3), s=2), [1, 0])]
    T = pose(t=(0.5, 1, 1.5))
    expect = [dict(walk_pos=[1, 0], points=[], claimed_by=[], Tiw=[T, T], state_poses={0: T, 1: T},
                   state_centres={0: (-0.5, -1, -1.5)}, state_points={100: (z(8), 0, 0), 101: (z(8), 0, 0)})]
    return ops, expect


def half_turn(axis=2):
    """key frame 1 is turned by half a turn about an axis: Quaterniond(R) takes the branch of that axis (trace -1) and every
    coefficient is exact.  About z: q = (0, 0, 1, 0), Corrected_1 = (q, (-1, -2, 3), 2), new pose [R | (-0.5, -1, 1.5)]; its point
    (1, 2, 11) lands on (0, 0, 4) like everyone's."""
    d = [-1.0, -1.0, -1.0]
    d[axis] = 1.0
    R = np.diag(d)
    q = [0.0, 0.0, 0.0, 0.0]
    q[axis] = 1.0
    t = R @ np.array([1.0, 2.0, 3.0])
    ops = [("kfs", [ls.kf(1, 1, pts=[100]), ls.kf(2, 2)]), ("points", [ls.mp(100, [1])]), ("scales", SCALES),
           ("poses", [1, 2], [pose(R), pose()]), ("geo", [geo(100, (1, 2, 11), 2)]), ("correct", 2, scw(t=(1, 2, 3), s=2), [2, 1])]
    expect = [dict(walk_pos=[1, 0], corrected=[[0, 0, 0, 1, 1, 2, 3, 2], q + list(t) + [2.0]],
                   non_corrected=[[0, 0, 0, 1, 0, 0, 0, 1], q + [0, 0, 0, 1.0]], points=[100], claimed_by=[1], world=[z(4)],
                   state_poses={1: pose(R, t / 2), 2: pose(t=(0.5, 1, 1.5))})]
    return ops, expect


def scale_one_and_half():
    """4 sits at (0, 0, 1).  With cur = 4 and Scw = (identity, (0, 0, -1), 1), its own pose, nothing moves but the stamps.  Then
    cur = 8 (identity pose) and Scw = (identity, 0, 1/2) double everything: 4 claims the point, (0, 0, 2.5) -> (0, 0, 5), four
    above 4's stored centre; 4 moves to (0, 0, 2)."""
    ops = [("kfs", [ls.kf(4, 4, pts=[100]), ls.kf(8, 8, pts=[100])]), ("points", [ls.mp(100, [4])]), ("scales", SCALES),
           ("poses", [4, 8], [pose(t=z(-1)), pose()]), ("geo", [geo(100, z(2.5), 4)]),
           ("correct", 4, scw(t=z(-1), s=1), [4]), ("correct", 8, scw(s=0.5), [8, 4])]
    expect = [dict(points=[100], claimed_by=[4], world=[z(2.5)], Tiw=[pose(t=z(-1))]),
              dict(walk_pos=[1, 0], points=[100], claimed_by=[4], world=[z(5)], normal=[z(1)], max_distance=[4], min_distance=[1],
                   Tiw=[pose(), pose(t=z(-2))], state_centres={4: z(2), 8: z(0)}, state_points={100: (z(5), 8, 4)})]
    return ops, expect


HAND = {
    "identity_scale_two": identity_scale_two, "shared_points": shared_points, "observers_and_references": observers_and_references,
    "skipped_entries": skipped_entries, "current_zero": current_zero, "half_turn_x": lambda: half_turn(0),
    "half_turn_y": lambda: half_turn(1), "half_turn_z": lambda: half_turn(2), "scale_one_and_half": scale_one_and_half,
}


# ---- seeded maps and scripts ---------------------------------------------------------------------------------------------------

def random_rotation(rng):
    q = rng.normal(size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_pose(rng):
    return pose(random_rotation(rng), rng.uniform(-3, 3, 3))


def random_scw(rng, s=None):
    q = rng.normal(size=4)
    return scw(q / np.linalg.norm(q), rng.uniform(-2, 2, 3), float(rng.uniform(0.6, 1.7)) if s is None else s)


def scale_factors(n=8):
    f = [np.float32(1.0)]
    for _ in range(n - 1):
        f.append(f[-1] * np.float32(1.2))
    return np.array(f, np.float32)


def random_map(rng, n_kf=24, n_mp=160, row=40, obs=5, bad=0.05, levels=8):
    """operations that set a whole map with geometry; ranks are a permutation, so handle order is not rank order"""
    ranks = rng.permutation(n_kf) + 1
    kfs = [ls.kf(h, int(ranks[h]), pts=[int(p) if rng.random() > 0.15 else -1 for p in rng.integers(0, n_mp, int(rng.integers(1, row)))])
           for h in range(n_kf)]
    pts = [ls.mp(p, [int(k) for k in rng.permutation(n_kf)[:int(rng.integers(0, obs + 1))]], bad=int(rng.random() < bad)) for p in range(n_mp)]
    g = [geo(p, rng.uniform(-5, 5, 3), int(rng.integers(0, n_kf)), int(rng.integers(0, levels))) for p in range(n_mp)]
    return [("kfs", kfs), ("points", pts), ("scales", scale_factors(levels)), ("poses", list(range(n_kf)), [random_pose(rng) for _ in range(n_kf)]),
            ("geo", g)]


def random_script(seed, n_kf=24, n_mp=160, calls=6):
    """corrects interleaved with setters, removes and connects; every correct is followed by the connect of its key frames in rank
    order, as CorrectLoop's loop interleaves them"""
    rng = np.random.default_rng(seed)
    ops = random_map(rng, n_kf, n_mp)
    kfs = {r["handle"]: r for r in ops[0][1]}
    pts = {r["handle"]: r for r in ops[1][1]}
    gs = {r["handle"]: r for r in ops[4][1]}
    # a key frame leaves before the graph has any connection: out of every observation and reference first
    k = int(rng.integers(0, n_kf))
    seen = [r for r in pts.values() if k in r["obs"]]
    for r in seen:
        r["obs"] = [x for x in r["obs"] if x != k]
    refs = [g for g in gs.values() if g["ref_kf"] == k]
    for g in refs:
        g["ref_kf"] = (k + 1) % n_kf
    ops += [("points", [ls.snap(r) for r in seen]), ("geo", [dict(g) for g in refs]), ("remove", KEYFRAME, k)]
    del kfs[k]
    for c in range(calls):
        alive = sorted(kfs)
        called = [int(h) for h in rng.permutation(alive)[:int(rng.integers(1, 9))]]
        cur = called[int(rng.integers(0, len(called)))]
        ops.append(("correct", cur, random_scw(rng, s=(1.0, 2.0, None)[c % 3]), called))
        ops.append(("connect", sorted(called, key=lambda h: kfs[h]["rank"])))
        what = c % 4
        if what == 0:        # new poses and positions for some
            hs = [int(h) for h in rng.permutation(alive)[:3]]
            ops.append(("poses", hs, [random_pose(rng) for _ in hs]))
            ps = [int(p) for p in rng.permutation(sorted(pts))[:5]]
            for p in ps:
                gs[p] = geo(p, rng.uniform(-5, 5, 3), int(rng.choice(alive)), int(rng.integers(0, 8)))
            ops.append(("geo", [dict(gs[p]) for p in ps]))
        elif what == 1:      # a point leaves: out of every row first
            p = int(rng.choice(sorted(pts)))
            rows = [r for r in kfs.values() if p in r["points"]]
            for r in rows:
                r["points"] = [-1 if x == p else x for x in r["points"]]
            if rows:
                ops.append(("kfs", [ls.snap(r) for r in rows]))
            ops.append(("remove", POINT, p))
            del pts[p], gs[p]
        elif what == 2:      # a key frame gets a new match row
            k = int(rng.choice(alive))
            kfs[k]["points"] = [int(p) if rng.random() > 0.2 else -1 for p in rng.choice(sorted(pts), int(rng.integers(1, 40)))]
            ops.append(("kfs", [ls.snap(kfs[k])]))
        else:                # bad flags
            ps = [int(p) for p in rng.permutation(sorted(pts))[:6]]
            ops.append(("bad", POINT, ps, [int(rng.random() < 0.5) for _ in ps]))
            for p, f in zip(ps, ops[-1][3]):
                pts[p]["bad"] = f
    return ops
