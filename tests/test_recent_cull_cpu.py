"""LocalMapping::MapPointCulling and MapLineCulling on the host (drfe_lmap_recent_cull_host, dr_slam_amd/csrc/lmap_recent.cpp with
recent_core.h) against tests/recent_cull_numpy.py and against values worked out by hand (tests/recent_cull_scenarios.py).  Equal
bytes everywhere; no GPU.

Parity with a build of the reference's LocalMapping.cc is not pinned: it includes OpenCV, Eigen and PCL headers that are not
installed where this was written."""
import re

import numpy as np
import pytest

import conn_numpy as cn
import cull_numpy as un
import lmap_numpy as ln
import recent_cull_numpy as rn
import recent_cull_scenarios as rs
from dr_slam_amd import lib

SEEDS = tuple(range(71, 77))
POINT, LINE = rs.POINT, rs.LINE


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        (rn.same_recent if "lines" in x and "points" in x else un.same_cull if "culled" in x else cn.same_connect if "touched" in x else ln.same)(x, y)


def rows_of(ops):
    """the key-frame rows a script sets, by handle"""
    rows = {}
    for op in ops:
        if op[0] == "kfs":
            rows.update({r["handle"]: r for r in op[1]})
        elif op[0] == "remove" and op[1] == rs.KEYFRAME:
            rows.pop(op[2], None)
    return rows


def same_store(db, ref, mode="host"):
    """every getter; then an UpdateLocalMap over every point and line, in which culled items are not listed, and an
    UpdateConnections of every key frame that is left, in which nulled entries do not vote"""
    kfs = sorted(ref.kf)
    cn.same_state(db, ref, kfs)
    un.same_attributes(db, ref, sorted(h for h in ref.cull_kf if h in ref.kf), sorted(h for h in ref.cull_mp if h in ref.mp))
    rn.same_attributes(db, ref, sorted(h for h in ref.rec_mp if h in ref.mp), sorted(h for h in ref.rec_ml if h in ref.ml))
    assert db.size() == ref.size()
    q = [dict(frame_id=10 ** 9, points=sorted(ref.mp), lines=sorted(ref.ml))]
    q += [dict(frame_id=10 ** 9 + 1 + i, points=ref.kf[h].mvpMapPoints, lines=ref.kf[h].mvpMapLines) for i, h in enumerate(kfs[:8])]
    ln.same(db.update(q, mode=mode), ref.update(q))
    alive = [h for h in kfs if not ref.kf[h].bad]
    cn.same_connect(db.connect(alive, mode=mode), ref.connect(alive))
    cn.same_state(db, ref, kfs)


def same_counters(db, ref):
    st = db.recent_cull_stats()
    for k, v in ref.rcounts.items():
        assert st[k] == v, (k, st[k], v)
    return st


def both(ops):
    ref = rn.Store()
    r_np = rs.play(ops, ref)
    db = lib.LocalMap()
    r_lib = rs.play(ops, db)
    same_results(r_lib, r_np)
    assert same_counters(db, ref)["device_calls"] == 0
    return r_lib, ref, db


def test_symbols_and_constants():
    L = lib.load()
    for s in lib.SYMBOLS:
        if "recent" in s:
            assert hasattr(L, s), s
    text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    lim = lib.LocalMap.recent_cull_limits()
    most = int(re.search(r"DRFE_LMAP_RECENT_MAX_ENTRIES = 1 << (\d+)", text).group(1))
    assert lim["max_entries"] == 1 << most
    assert re.search(r"DRFE_LMAP_RECENT_DEVICE_FROM = 2 \* DRFE_LMAP_RECENT_MAX_ENTRIES \+ 1 ", text) and lim["device_from"] == 2 * lim["max_entries"] + 1
    assert lim["entry_tile"] % 64 == 0 and lim["erase_tile"] % 64 == 0 and lim["wavefront"] == 64 and lim["entry_bytes"] == 8
    assert (lib.RECENT_KEPT, lib.RECENT_WAS_BAD, lib.RECENT_RATIO, lib.RECENT_OBSERVATIONS, lib.RECENT_AGED) == (
        rn.KEPT, rn.WAS_BAD, rn.RATIO, rn.OBSERVATIONS, rn.AGED)
    assert set(lib.LMAP_RECENT_STATS) == set(rn.Store().rcounts) | {"device_calls"}


def test_device_from_is_the_measured_crossover():
    """profiles/recent_cull_timing.jsonl (tools/recent_cull_timing.py): its last line is the constant, and the rows give it"""
    import json
    rows = [json.loads(x) for x in open(lib.os.path.join(lib._HERE, "..", "profiles", "recent_cull_timing.jsonl"))]
    measured = rows[-1]["device_from"]
    lim = lib.LocalMap.recent_cull_limits()
    assert lim["device_from"] == (measured if measured is not None else 2 * lim["max_entries"] + 1)
    shapes = rows[:-1]
    assert {r["keyframes"] for r in shapes} == {100, 400, 1600} and {r["entries"] for r in shapes} == {64, 512, 4096, 32768}
    assert {r["culled_tenth"] for r in shapes} == {0, 1} and len(shapes) == 24
    assert all(r["equal"] and r["device_reps"] >= 5 and r["host_reps"] >= 5 for r in shapes)
    assert all((r["culled"] > 0) == bool(r["culled_tenth"]) for r in shapes)
    for r in shapes:
        assert r["device_wins"] == (r["host_ms"] - r["device_ms"] > max(r["host_iqr_ms"], r["device_iqr_ms"]))      # medians
    sizes = sorted({r["entries"] for r in shapes})
    wins = {n: all(r["device_wins"] for r in shapes if r["entries"] == n) for n in sizes}
    want = None
    for n in reversed(sizes):                       # the smallest length from which the device wins at every store size
        if not wins[n]:
            break
        want = n
    assert measured == want


def test_premises():
    """what the hand-built stores rest on, in numpy alone"""
    f32 = np.float32
    found, visible = 16777219, 67108877
    assert f32(found) / f32(visible) == f32(0.25) and 4 * found < visible                 # the float quotient is kept, the integers cull
    assert f32(1) / f32(4) == f32(0.25) and f32(1) / f32(5) < f32(0.25)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.isnan(f32(0) / f32(0)) and not f32(0) / f32(0) < f32(0.25)
        assert np.isinf(f32(3) / f32(0)) and not f32(3) / f32(0) < f32(0.25) and f32(-3) / f32(0) < f32(0.25)
    assert rn.c_div(2, 3) == 0 and rn.c_div(99, 100) == 0 and rn.c_div(6, 2) == 3 and rn.c_div(-7, 2) == -3
    assert rn.c_int((1 << 32) + 5) == 5 and rn.c_int(-1) == -1 and rn.c_int(1 << 31) == -(1 << 31)
    assert rn.c_int(1) - rn.c_int(-1) == 2 and rn.c_int(5) - rn.c_int((1 << 32) + 2) == 3
    # the stale index of stale_index_nulls_a_live_item lands on the kept item, and the store shows it afterwards
    ops, expect, _ = rs.stale_index_nulls_a_live_item()
    ref = rn.Store()
    rs.play(ops, ref)
    (bp, ep), (bl, el) = ops[-1][2], ops[-1][3]
    assert ref.mp[bp].bad and not ref.mp[ep].bad and 2 in ref.mp[ep].observations and ep not in ref.kf[2].mvpMapPoints
    assert ref.ml[bl].bad and not ref.ml[el].bad and 2 in ref.rec_ml[el]["observations"] and el not in ref.kf[2].mvpMapLines
    ops, _, _ = rs.two_culled_items_name_one_entry()
    ref = rn.Store()
    rs.play(ops, ref)
    assert ref.rcounts["nulled"] == 6 and ref.paths()["nulled_already_null"] == 2          # 8 erased observations, 6 entries


@pytest.mark.parametrize("name", sorted(rs.HAND))
def test_hand_built(name):
    ops, expect, paths = rs.HAND[name]()
    r, ref, db = both(ops)
    reached = ref.paths()
    for p in paths:
        assert reached[p] > 0, p                               # the premise: the store takes the branch it was built for
    rs.check(r, expect)
    same_store(db, ref)


def test_the_hand_built_stores_reach_every_path_together():
    reached = dict.fromkeys(rn.PATHS, 0)
    for f in rs.HAND.values():
        ref = rn.Store()
        rs.play(f()[0], ref)
        for k, v in ref.paths().items():
            reached[k] += v
    missing = [k for k, v in reached.items() if v == 0]
    assert missing == [], missing


@pytest.fixture(scope="module")
def random_runs():
    runs = []
    for seed in SEEDS:
        ops = rs.random_script(seed)
        ref = rn.Store()
        runs.append((ops, rs.play(ops, ref), ref))
    return runs


def test_random_scripts_take_every_branch(random_runs):
    kinds = {op[0] for ops, _, _ in random_runs for op in ops}
    assert kinds >= {"kfs", "points", "lines", "attr", "recent", "rcull", "inc", "cull", "connect", "update", "bad"}
    calls = [r for _, rsl, _ in random_runs for r in rsl if "lines" in r and "points" in r]
    for name in ("points", "lines"):
        actions = np.concatenate([r[name]["action"] for r in calls])
        assert set(actions.tolist()) == {0, 1, 2, 3, 4}, name
        assert sum(len(e) for r in calls for e in r[name]["erased"]) > 0
    total = dict.fromkeys(rn.PATHS, 0)
    for _, _, ref in random_runs:
        for k, v in ref.paths().items():
            total[k] += v
    for k in ("second_of_culled", "second_of_kept", "nulled_own", "nulled_already_null", "nulled_other", "bad_observer", "no_observations",
              "point_ratio_nan", "was_bad"):
        assert total[k] > 0, k


@pytest.mark.parametrize("i", range(len(SEEDS)))
def test_random_scripts_match_the_restatement(random_runs, i):
    ops, r_np, ref = random_runs[i]
    db = lib.LocalMap()
    same_results(rs.play(ops, db), r_np)
    same_counters(db, ref)
    assert all(db.cull_stats()[k] == v for k, v in ref.ucounts.items())
    assert all(db.stats()[k] == v for k, v in ref.counts.items())
    same_store(db, ref)


def _refused(fn, rc=lib.ERR_INVALID):
    with pytest.raises(lib.DrfeError) as e:
        fn()
    assert e.value.rc == rc
    return str(e.value)


def _base():
    ops, expect, _ = rs.each_action()
    db = lib.LocalMap()
    rs.play(ops[:-1], db)
    return db, ops, expect


def _answers_as_untouched(db, ops, expect):
    """the refused call changed nothing: the store answers the scenario's call as a fresh store does, and ends up the same"""
    assert db.recent_cull_stats()["calls"] == 0
    r = rs.play(ops[-1:], db)
    rs.check(r, expect)
    ref = rn.Store()
    rs.play(ops, ref)
    same_store(db, ref)


def test_unknown_handles_are_refused():
    db, ops, expect = _base()
    pts, lns = ops[-1][2], ops[-1][3]
    _refused(lambda: db.recent_cull(rs.CUR, pts + [77777], lns, mode="host"))
    _refused(lambda: db.recent_cull(rs.CUR, pts, [lns[0], pts[0]], mode="host"))          # a point's handle in the line list
    _refused(lambda: db.recent_increase(POINT, [77777], [1], [1]))
    _refused(lambda: db.recent_increase(7, [pts[0]], [1], [1]))
    _refused(lambda: db.get_recent_attributes([77777], []))
    _answers_as_untouched(db, ops, expect)


def test_missing_attributes_and_bad_indices_are_named():
    db, ops, expect = _base()
    pts, lns = ops[-1][2], ops[-1][3]
    kfs = rows_of(ops)
    rec = [op for op in ops if op[0] == "recent"][0]
    # a point and a line that are stored without recent-list attributes
    db.set_points([dict(handle=5000, obs=[])])
    db.set_cull_attributes([], [dict(handle=5000, n_obs=0, obs_index=[])])
    db.set_lines([5001])
    assert "map point 5000" in _refused(lambda: db.recent_cull(rs.CUR, pts + [5000], lns, mode="host"), lib.ERR_STATE)
    assert "map line 5001" in _refused(lambda: db.recent_cull(rs.CUR, pts, lns + [5001], mode="host"), lib.ERR_STATE)
    # a listed item that is bad is dropped whatever it lacks
    db.set_bad(POINT, [5000], [1])
    db.set_bad(LINE, [5001], [1])
    assert db.recent_cull(rs.CUR, [5000], [5001], mode="host")["points"]["action"].tolist() == [1]
    db.remove(POINT, 5000)
    db.remove(LINE, 5001)
    # recent-list attributes without culling attributes that fit
    db.set_points([dict(handle=5002, obs=[1])])
    db.set_recent_attributes([dict(handle=5002, found=1, visible=1, first_kf=rs.CUR)], [])
    assert "map point 5002" in _refused(lambda: db.recent_cull(rs.CUR, [5002], [], mode="host"), lib.ERR_STATE)
    # an obs_index outside the observer's row, of a point and of a line
    db.set_cull_attributes([], [dict(handle=5002, n_obs=1, obs_index=[len(kfs[1]["points"])])])
    assert "obs_index" in _refused(lambda: db.recent_cull(rs.CUR, [5002], [], mode="host"), lib.ERR_STATE)
    db.remove(POINT, 5002)
    line = dict(rec[2][1])
    db.set_recent_attributes([], [dict(line, obs=[1], obs_index=[-1])])
    assert "obs_index -1" in _refused(lambda: db.recent_cull(rs.CUR, pts, lns, mode="host"), lib.ERR_STATE)
    # an observation of a line that names an unknown key frame refuses every call, as one of a point does
    db.set_recent_attributes([], [dict(line, obs=[4242], obs_index=[0])])
    assert "map line %d names unknown handle 4242" % line["handle"] in _refused(lambda: db.recent_cull(rs.CUR, pts, lns, mode="host"), lib.ERR_STATE)
    assert "4242" in _refused(lambda: db.update([dict(frame_id=5, points=pts)], mode="host"), lib.ERR_STATE)
    db.set_recent_attributes([], [line])
    st = db.recent_cull_stats()
    assert st["calls"] == 1 and st["dropped_bad"] == 2
    r = rs.play(ops[-1:], db)
    rs.check(r, expect)


@pytest.mark.parametrize("found,visible", [(0, 0), (5, 0), (-(1 << 31), -1)])
def test_an_undefined_line_division_is_refused(found, visible):
    db, ops, expect = _base()
    pts, lns = ops[-1][2], ops[-1][3]
    line = dict([op for op in ops if op[0] == "recent"][0][2][-1])
    db.set_recent_attributes([], [dict(line, found=found, visible=visible)])
    why = _refused(lambda: db.recent_cull(rs.CUR, pts, lns, mode="host"), lib.ERR_STATE)
    assert "map line %d" % line["handle"] in why and "not defined" in why
    db.set_recent_attributes([], [line])
    _answers_as_untouched(db, ops, expect)


@pytest.mark.parametrize("which", [0, 1])
def test_too_small_output_array_changes_nothing(which):
    db, ops, expect = _base()
    pts, lns = ops[-1][2], ops[-1][3]
    need = [sum(len(e) for e in expect[0][k]["erased"]) for k in ("points", "lines")]
    assert min(need) > 0
    cap = list(need)
    cap[which] -= 1
    assert "erased_capacity" in _refused(lambda: db.recent_cull(rs.CUR, pts, lns, mode="host", capacity=cap), lib.ERR_CAPACITY)
    ref = rn.Store()
    rs.play(ops[:-1], ref)
    with pytest.raises(rn.Refused) as e:
        ref.recent_cull(rs.CUR, pts, lns, capacity=cap)
    assert e.value.rc == lib.ERR_CAPACITY
    assert db.recent_cull_stats()["calls"] == 0
    rn.same_recent(db.recent_cull(rs.CUR, pts, lns, mode="host", capacity=need), ref.recent_cull(rs.CUR, pts, lns, capacity=need))
    same_store(db, ref)


def test_device_entry_without_a_context_is_a_state_error():
    db, ops, expect = _base()
    _refused(lambda: db.recent_cull(rs.CUR, ops[-1][2], ops[-1][3], mode="device"), lib.ERR_STATE)
    r = db.recent_cull(rs.CUR, ops[-1][2], ops[-1][3], mode="batch")                      # _batch runs on the host
    rs.check([r], expect)


def test_a_store_without_the_attributes_behaves_as_before():
    ops, _, _ = rs.each_action()
    plain = [op for op in ops if op[0] not in ("recent", "rcull")]
    ref = rn.Store()
    rs.play(plain, ref)
    db = lib.LocalMap()
    rs.play(plain, db)
    cn.same_state(db, ref, sorted(ref.kf))
    q = [dict(frame_id=9, points=sorted(ref.mp), lines=sorted(ref.ml))]
    ln.same(db.update(q, mode="host"), ref.update(q))
    assert db.recent_cull_stats()["calls"] == 0


def test_an_empty_call_and_empty_lists():
    db, ops, expect = _base()
    r = db.recent_cull(rs.CUR, [], [], mode="host")
    for k in ("points", "lines"):
        assert len(r[k]["action"]) == 0 and len(r[k]["kept"]) == 0 and len(r[k]["culled"]) == 0 and r[k]["erased"] == []
    assert db.recent_cull_stats()["calls"] == 0
    pts, lns = ops[-1][2], ops[-1][3]
    ref = rn.Store()
    rs.play(ops[:-1], ref)
    rn.same_recent(db.recent_cull(rs.CUR, pts, [], mode="host"), ref.recent_cull(rs.CUR, pts, []))
    rn.same_recent(db.recent_cull(rs.CUR, [], lns, mode="host"), ref.recent_cull(rs.CUR, [], lns))
    same_store(db, ref)


def test_setter_getter_increase_and_remove():
    db, ops, _ = _base()
    ref = rn.Store()
    rs.play(ops[:-1], ref)
    pts, lns = sorted(ref.rec_mp), sorted(ref.rec_ml)
    rn.same_attributes(db, ref, pts, lns)
    big = (1 << 31) - 1
    for s in (db, ref):
        s.recent_increase(POINT, [pts[0], pts[1], pts[0]], [1, 2, big], [3, 0, 0])         # a handle twice, and wrap-around
        s.recent_increase(LINE, [lns[0]], [-2], [5])
        s.set_recent_attributes([dict(handle=pts[2], found=7, visible=9, first_kf=-1)],
                                [dict(handle=lns[1], found=7, visible=9, first_kf=1 << 40, n_obs=5, obs=[3, 1], obs_index=[0, 0])])
    rn.same_attributes(db, ref, pts, lns)
    assert db.get_recent_attributes([pts[0]], [])["points"][0]["found"] == rn.wrap32(ref.rec_mp[pts[0]]["found"])
    _refused(lambda: db.set_recent_attributes([], [dict(handle=lns[1], found=1, visible=1, first_kf=0, n_obs=2, obs=[3, 3], obs_index=[0, 1])]))
    for s in (db, ref):
        s.remove(POINT, pts[0])
        s.remove(LINE, lns[0])
    _refused(lambda: db.get_recent_attributes([pts[0]], []))
    _refused(lambda: db.get_recent_attributes([], [lns[0]]))
    rn.same_attributes(db, ref, pts[1:], lns[1:])


def test_native_caller_on_the_host_entry():
    """tests/native/recent_cull_caller.cpp: the adaptor's SyncRecent / MapPointCulling / MapLineCulling on stand-in types whose
    SetBadFlag restates the reference's, next to the reference's rules on a twin; the store against the objects after every call"""
    import subprocess
    import native_build
    exe = native_build.caller("recent_cull_caller")
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "recent_cull_caller ok (host, 8 calls, 390 culled" in p.stdout, (p.returncode, p.stdout, p.stderr)
