"""CPU tests of the Sim3 propagation of LoopClosing::CorrectLoop on the map store (drfe_lmap_correct_host):
the host entry against tests/loop_correct_numpy.py, byte for byte, and against the hand-written values of
tests/loop_correct_scenarios.py; the store afterwards through the getters; a following connect and update; every refusal leaving
the store unchanged; the committed crossover; the native caller on the host entries."""
import itertools
import json

import numpy as np
import pytest

import loop_correct_numpy as rn
import loop_correct_scenarios as rs
import conn_numpy as cn
import lmap_numpy as ln
import lmap_scenarios as ls
from dr_slam_amd import lib

LIM = lib.LocalMap.correct_limits()            # without the feature the module fails here, at the first symbol
T = LIM["claim_tile"]


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        (rn.same_correct if "claimed_by" in x else cn.same_connect if "touched" in x else ln.same)(x, y)


def alive(ops):
    kfs, pts = set(), set()
    for op in ops:
        if op[0] == "kfs":
            kfs |= {r["handle"] for r in op[1]}
        elif op[0] == "points":
            pts |= {r["handle"] for r in op[1]}
        elif op[0] == "remove":
            (kfs if op[1] == ls.KEYFRAME else pts).discard(op[2])
    return sorted(kfs), sorted(pts)


def both(ops, mode="host"):
    """a script on the host entry and in the restatement: equal results, equal stores, equal counters"""
    db, ref = lib.LocalMap(), rn.Store()
    r, r_ref = rs.play(ops, db, mode=mode), rs.play(ops, ref)
    same_results(r, r_ref)
    kfs, pts = alive(ops)
    rn.same_geometry(db, ref, kfs, pts)
    st = db.correct_stats()
    assert all(st[k] == v for k, v in ref.rcounts.items()), (st, ref.rcounts)
    assert st["device_calls"] == 0 and st["device_chunks"] == 0
    return r, r_ref, db


def test_limits_and_symbols():
    assert T >= 64 and LIM["threads"] % 64 == 0 and LIM["entry_bytes"] >= 41
    assert all(hasattr(lib.load(), s) for s in lib.SYMBOLS if "correct" in s or "geometry" in s or "poses" in s or "scales" in s)


def test_device_from_is_the_measured_crossover():
    """profiles/loop_correct_timing.jsonl (tools/loop_correct_timing.py): its last line is the constant, and the rows give it"""
    rows = [json.loads(x) for x in open(lib.os.path.join(lib._HERE, "..", "profiles", "loop_correct_timing.jsonl"))]
    measured = rows[-1]["device_from"]
    assert LIM["device_from"] == (measured if measured is not None else 2 ** 31 - 1)
    shapes = rows[:-1]
    assert {r["keyframes"] for r in shapes} == {100, 1000, 4000} and {r["called"] for r in shapes} == {1, 4, 16, 64, 256}
    assert all(r["equal"] and r["device_reps"] >= 5 and r["host_reps"] >= 5 for r in shapes)
    for r in shapes:
        assert r["device_wins"] == (r["host_ms"] - r["device_ms"] > max(r["host_iqr_ms"], r["device_iqr_ms"]))      # medians
    sizes = sorted({r["called"] for r in shapes})
    wins = {n: all(r["device_wins"] for r in shapes if r["called"] == n) for n in sizes}
    want = None
    for n in reversed(sizes):                       # the smallest size from which the device wins at every store size
        if not wins[n]:
            break
        want = n
    assert measured == want


def test_native_caller_on_the_host_entries():
    """tests/native/loop_correct_caller.cpp: the adaptor's CorrectLoop on stand-in types next to a pointer walk of :480-562"""
    import subprocess
    import native_build
    exe = native_build.caller("loop_correct_caller")
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "loop_correct_caller ok (host, 8 calls, 1 call of 30, 1518 points moved, device calls 0)" in p.stdout, (p.returncode, p.stdout, p.stderr)


@pytest.mark.parametrize("name", sorted(rs.HAND))
def test_hand_built(name):
    ops, expect = rs.HAND[name]()
    r, r_ref, db = both(ops)
    rs.check(r, expect, db)
    ref = rn.Store()
    rs.check(rs.play(ops, ref), expect, ref)


@pytest.mark.parametrize("order", list(itertools.permutations((1, 2, 3))))
def test_lowest_rank_claims_under_every_call_order(order):
    ops, expect = rs.shared_points(order)
    r, _, db = both(ops)
    rs.check(r, expect, db)


def test_centre_selection_shows_in_the_normal():
    """the observers before, at and after the claimant and the one not called: (0, 0, 0.5), where stored centres alone give 0 and
    corrected centres alone 1"""
    ops, _ = rs.observers_and_references()
    r, _, _ = both(ops)
    nz = float(r[0]["normal"][0][2])
    assert nz == 0.5 and nz != 0.0 and nz != 1.0
    # the two variants, from the same restatement on maps in which no observer or every observer has moved already
    old = rs.play(ops[:-1] + [("correct", 2, rs.scw(s=2), [2])], rn.Store())[0]            # nobody else is called: all stored
    assert float(old["normal"][0][2]) == 0.0
    moved = [("poses", [1, 3], [rs.pose(t=rs.z(-3)), rs.pose(t=rs.z(-3))]), ("correct", 2, rs.scw(s=2), [2])]
    new = rs.play(ops[:-1] + moved, rn.Store())[0]                                         # 1 and 3 already at their new place
    assert float(new["normal"][0][2]) == 1.0


@pytest.mark.parametrize("seed", [1, 7, 23, 51])
def test_seeded_scripts(seed):
    r, _, _ = both(rs.random_script(seed))
    assert sum(len(x["points"]) for x in r if "claimed_by" in x) > 50


@pytest.mark.parametrize("s", [1.0, 2.0, 0.5, 3.0, 0.7])
def test_scales(s):
    rng = np.random.default_rng(int(s * 10))
    ops = rs.random_map(rng) + [("correct", 3, rs.random_scw(rng, s=s), [0, 3, 5, 9, 11])]
    r, _, _ = both(ops)
    assert len(r[0]["points"]) > 20


def test_rotations_reach_every_branch_of_the_quaternion():
    """trace > 0 and each of the three other branches of Quaterniond(Matrix3d), on rotations that are not exact"""
    rng = np.random.default_rng(5)
    base = rs.random_map(rng, n_kf=6, n_mp=60, row=30)
    c, s = np.cos(2.9), np.sin(2.9)
    Rs = [np.eye(3), np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
          np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])]
    assert [int(np.trace(R) > 0) for R in Rs] == [1, 0, 0, 0] and [int(np.argmax(np.diag(R))) for R in Rs[1:]] == [0, 1, 2]
    ops = base + [("poses", [0, 1, 2, 3], [rs.pose(R, rng.uniform(-1, 1, 3)) for R in Rs]), ("correct", 4, rs.random_scw(rng), [0, 1, 2, 3, 4])]
    both(ops)


def rows_map(sizes, n_mp=300, seed=3):
    rng = np.random.default_rng(seed)
    n_kf = len(sizes)
    kfs = [ls.kf(h, 100 - h, pts=[int(p) for p in rng.integers(-1, n_mp, s)]) for h, s in enumerate(sizes)]
    pts = [ls.mp(p, [int(k) for k in rng.permutation(n_kf)[:int(rng.integers(0, 4))]], bad=int(rng.random() < 0.05)) for p in range(n_mp)]
    g = [rs.geo(p, rng.uniform(-5, 5, 3), int(rng.integers(0, n_kf)), int(rng.integers(0, 8))) for p in range(n_mp)]
    return [("kfs", kfs), ("points", pts), ("scales", rs.scale_factors()), ("poses", list(range(n_kf)), [rs.random_pose(rng) for _ in range(n_kf)]),
            ("geo", g)]


def test_rows_around_the_claim_tile():
    sizes = (T - 1, T, T + 1, 1, 2 * T + 3, 0)
    r, _, _ = both(rows_map(sizes) + [("correct", 2, rs.random_scw(np.random.default_rng(1)), [5, 3, 0, 4, 1, 2])])
    assert len(r[0]["points"]) > T


def test_observation_counts():
    """points with no observation, one, and 70"""
    rng = np.random.default_rng(9)
    kfs = [ls.kf(h, 1000 - h) for h in range(70)] + [ls.kf(100, 5, pts=[0, 1, 2]), ls.kf(101, 2000, pts=[2, 1])]
    pts = [ls.mp(0), ls.mp(1, [33]), ls.mp(2, [int(k) for k in rng.permutation(70)])]
    hs = list(range(70)) + [100, 101]
    ops = [("kfs", kfs), ("points", pts), ("scales", rs.scale_factors()), ("poses", hs, [rs.random_pose(rng) for _ in hs]),
           ("geo", [rs.geo(p, rng.uniform(-5, 5, 3), 33, 3) for p in range(3)]),
           ("correct", 100, rs.random_scw(rng), [100, 101] + list(range(0, 70, 2)))]
    r, _, _ = both(ops)
    assert r[0]["points"].tolist() == [0, 1, 2] and r[0]["status"].tolist() == [0, 2, 2]


@pytest.mark.parametrize("n", [1, 2, 200])
def test_call_sizes(n):
    rng = np.random.default_rng(n)
    ops = rs.random_map(rng, n_kf=max(n, 4) + 3, n_mp=400, row=12)
    called = [int(h) for h in rng.permutation(max(n, 4) + 3)[:n]]
    r, _, _ = both(ops + [("correct", called[-1], rs.random_scw(rng), called)])
    assert sorted(r[0]["walk_pos"].tolist()) == list(range(n))


def test_batch_without_a_context_runs_on_the_host():
    ops = rs.random_map(np.random.default_rng(2), n_kf=40) + [("correct", 0, rs.random_scw(np.random.default_rng(3)), list(range(40)))]
    both(ops, mode="batch")


def test_geometry_setters_and_getters():
    db = lib.LocalMap()
    db.set_scales([1.0, 1.5])
    assert db.get_scales().tolist() == [1.0, 1.5]
    T0 = rs.pose(np.diag([1.0, -1.0, -1.0]), (1, 2, 3))
    db.set_poses([7, 8], [T0, rs.pose()])                       # not stored yet: allowed
    g = db.get_poses([7])
    assert np.array_equal(g["Tcw"][0], T0) and g["Ow"][0].tolist() == [-1, 2, 3] and np.array_equal(g["Twc"][0][:3, :3], T0[:3, :3].T)
    db.set_poses([7], [rs.pose()])                              # a row replaces the stored one
    assert db.get_poses([7])["Ow"][0].tolist() == [0, 0, 0]
    db.set_point_geometry([dict(handle=3, world=(1, 2, 3), ref_kf=7)])
    g = db.get_point_geometry([3])
    assert g["world"].tolist() == [[1, 2, 3]] and (g["ref_kf"][0], g["ref_level"][0], g["corrected_by"][0], g["corrected_ref"][0]) == (7, 0, 0, 0)
    with pytest.raises(lib.DrfeError) as e:
        db.get_point_geometry([4])
    assert e.value.rc == lib.ERR_INVALID
    db.set_keyframes([ls.kf(7, 1, pts=[3])])
    db.set_points([ls.mp(3, [7])])
    db.remove(ls.POINT, 3)                                      # the geometry goes with the item
    with pytest.raises(lib.DrfeError):
        db.get_point_geometry([3])
    db.set_keyframes([ls.kf(7, 1)])
    db.remove(ls.KEYFRAME, 7)
    with pytest.raises(lib.DrfeError):
        db.get_poses([7])
    assert db.get_poses([8])["Ow"].tolist() == [[0, 0, 0]]


def snapshot(db, kfs, pts):
    p = db.get_poses(kfs)
    g = db.get_point_geometry(pts)
    return (b"".join(np.ascontiguousarray(v).tobytes() for v in list(p.values()) + list(g.values())), db.get_scales().tobytes(),
            db.correct_stats(), db.connect_stats(), db.stats())


def refusal_map():
    ops, _ = rs.observers_and_references()
    db = lib.LocalMap()
    rs.play(ops[:-1], db)
    return db, [1, 2, 3, 9], [100, 101, 102, 103]


REFUSALS = {
    "duplicate": (lambda db: None, dict(handles=[1, 2, 1]), lib.ERR_INVALID, "twice"),
    "without_cur": (lambda db: None, dict(handles=[1, 3]), lib.ERR_INVALID, "current key frame"),
    "unknown_handle": (lambda db: None, dict(handles=[1, 2, 55]), lib.ERR_INVALID, "unknown"),
    "empty": (lambda db: None, dict(handles=[]), lib.ERR_INVALID, "invalid"),
    "capacity": (lambda db: None, dict(capacity=3), lib.ERR_CAPACITY, "points_capacity"),
    "keyframe_without_pose": (lambda db: (db.set_keyframes([ls.kf(4, 4)]),), dict(handles=[1, 2, 4]), lib.ERR_STATE, "key frame 4"),
    "point_without_geometry": (lambda db: (db.set_points([ls.mp(104, [2])]), db.set_keyframes([ls.kf(2, 2, pts=[100, 104])])), {},
                               lib.ERR_STATE, "map point 104"),
    "observer_without_pose": (lambda db: (db.set_keyframes([ls.kf(4, 4)]), db.set_points([ls.mp(101, [2, 4])])), {}, lib.ERR_STATE,
                              "key frame 4"),
    "reference_unknown": (lambda db: (db.set_point_geometry([rs.geo(102, rs.z(8), 77)]),), {}, lib.ERR_STATE, "reference key frame 77"),
    "reference_without_pose": (lambda db: (db.set_keyframes([ls.kf(4, 4)]), db.set_point_geometry([rs.geo(102, rs.z(8), 4)])), {},
                               lib.ERR_STATE, "reference key frame 4"),
    "level_out_of_range": (lambda db: (db.set_point_geometry([rs.geo(103, rs.z(8), 3, level=3)]),), {}, lib.ERR_STATE, "ref_level of map point 103"),
    "level_negative": (lambda db: (db.set_point_geometry([rs.geo(103, rs.z(8), 3, level=-1)]),), {}, lib.ERR_STATE, "ref_level of map point 103"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_a_refused_call_changes_nothing(name):
    edit, kw, rc, word = REFUSALS[name]
    db, kfs, pts = refusal_map()
    edit(db)
    before = snapshot(db, kfs, pts)
    with pytest.raises(lib.DrfeError) as e:
        db.correct(2, rs.scw(s=2), kw.get("handles", [3, 2, 1]), mode="host", capacity=kw.get("capacity"))
    assert e.value.rc == rc and word in str(e.value), str(e.value)
    assert snapshot(db, kfs, pts) == before


def test_a_store_without_scales_refuses():
    ops, _ = rs.observers_and_references()
    db = lib.LocalMap()
    rs.play([op for op in ops[:-1] if op[0] != "scales"], db)
    with pytest.raises(lib.DrfeError) as e:
        db.correct(2, rs.scw(s=2), [1, 2, 3], mode="host")
    assert e.value.rc == lib.ERR_STATE and "scale" in str(e.value)


def test_missing_geometry_of_untouched_items_does_not_matter():
    """a key frame that is neither called nor observing, and a point the walk does not move, may lack geometry"""
    ops, expect = rs.observers_and_references()
    db = lib.LocalMap()
    rs.play(ops[:-1], db)
    db.set_keyframes([ls.kf(4, 4, pts=[105]), ls.kf(2, 2, pts=[100, 101, 102, 103, 106])])
    db.set_points([ls.mp(105, [4]), ls.mp(106, [4], bad=1)])          # 105 is in no called row, 106 is bad
    r = db.correct(2, rs.scw(s=2), [3, 2, 1], mode="host")
    rs.check([r], expect, db)


def test_connect_after_correct_reads_the_same_graph():
    """the integer graph is untouched: connect of the called key frames in rank order gives what it gives without the correct"""
    ops = rs.random_map(np.random.default_rng(4))
    a, b = lib.LocalMap(), lib.LocalMap()
    rs.play(ops, a)
    rs.play(ops, b)
    called = [2, 9, 4, 17, 11]
    r = a.correct(9, rs.random_scw(np.random.default_rng(8)), called, mode="host")
    in_rank = [h for _, h in sorted(zip(r["walk_pos"].tolist(), called))]
    cn.same_connect(a.connect(in_rank, mode="host"), b.connect(in_rank, mode="host"))
