"""LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag on the host (drfe_lmap_cull_host, dr_slam_amd/csrc/lmap_cull.cpp with
cull_core.h) against tests/cull_numpy.py and against values worked out by hand (tests/cull_scenarios.py).  Equal bytes everywhere;
no GPU.

Parity with a build of the reference's LocalMapping.cc and KeyFrame.cc is not pinned: they include OpenCV, Eigen and PCL headers
that are not installed where this was written."""
import json
import re

import numpy as np
import pytest

import conn_numpy as cn
import cull_numpy as un
import cull_scenarios as us
import lmap_numpy as ln
import lmap_scenarios as ls
from dr_slam_amd import lib

SEEDS = tuple(range(61, 69))


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        (un.same_cull if "culled" in x else cn.same_connect if "touched" in x else ln.same)(x, y)


def same_store(db, ref):
    """every getter, then an UpdateLocalMap over every point and an UpdateConnections of every key frame that is left"""
    kfs = sorted(ref.kf)
    cn.same_state(db, ref, kfs)
    un.same_attributes(db, ref, sorted(h for h in ref.cull_kf if h in ref.kf), sorted(h for h in ref.cull_mp if h in ref.mp))
    geo = sorted(h for h in ref.geo if h in ref.mp)
    if geo:
        a, b = db.get_point_geometry(geo), ref.get_point_geometry(geo)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    assert db.size() == ref.size()
    q = [dict(frame_id=10 ** 9, points=sorted(ref.mp))]
    ln.same(db.update(q, mode="host"), ref.update(q))
    alive = [h for h in kfs if not ref.kf[h].bad]
    cn.same_connect(db.connect(alive, mode="host"), ref.connect(alive))
    cn.same_state(db, ref, kfs)


def both(ops):
    ref = un.Store()
    r_np = us.play(ops, ref)
    db = lib.LocalMap()
    r_lib = us.play(ops, db)
    same_results(r_lib, r_np)
    st = db.cull_stats()
    for k, v in ref.ucounts.items():
        assert st[k] == v, (k, st[k], v)
    assert st["device_calls"] == 0
    return r_lib, ref, db


def test_symbols_and_constants():
    L = lib.load()
    for s in lib.SYMBOLS:
        if "cull" in s:
            assert hasattr(L, s), s
    text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    lim = lib.LocalMap.cull_limits()
    assert int(re.search(r"DRFE_LMAP_CULL_DEVICE_FROM = (\d+)", text).group(1)) == lim["device_from"]
    assert lim["record_tile"] % 64 == 0 and lim["walk_threads"] % 64 == 0 and lim["entry_bytes"] == 8
    assert (lib.CULL_NOT_ERASE, lib.CULL_ORIGIN, lib.CULL_TO_BE_ERASED) == (un.NOT_ERASE, un.ORIGIN, un.TO_BE_ERASED)
    assert (lib.CULL_KEPT, lib.CULL_CULLED, lib.CULL_DEFERRED, lib.CULL_SKIPPED_ORIGIN) == (un.KEPT, un.CULLED, un.DEFERRED, un.SKIPPED_ORIGIN)
    assert (lib.CONN_WEIGHTS, lib.CONN_ORDERED, lib.CONN_PARENT, lib.CULL_CHILDREN, lib.CULL_NULLED, lib.CULL_WENT_BAD) == (
        us.W, us.O, us.P, us.CH, us.NU, us.BAD)
    assert set(lib.LMAP_CULL_STATS) == set(un.Store().ucounts) | {"device_calls"}


def test_device_from_is_the_measured_crossover():
    """profiles/cull_timing.jsonl (tools/cull_timing.py): its last line is the constant, and the rows give it"""
    rows = [json.loads(x) for x in open(lib.os.path.join(lib._HERE, "..", "profiles", "cull_timing.jsonl"))]
    measured = rows[-1]["device_from"]
    above = int(re.search(r"DRFE_LMAP_MAX_QUERIES = (\d+)", open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()).group(1)) + 1
    assert lib.LocalMap.cull_limits()["device_from"] == (measured if measured is not None else above)
    shapes = rows[:-1]
    assert {r["keyframes"] for r in shapes} == {100, 400, 1600} and {r["called"] for r in shapes} == {1, 4, 16, 64, 256}
    assert {r["culled_tenth"] for r in shapes} == {0, 1}
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


@pytest.mark.parametrize("name", sorted(us.HAND))
def test_hand_built(name):
    ops, expect, paths = us.HAND[name]()[:3]
    r, ref, db = both(ops)
    reached = ref.paths()
    for p in paths:
        assert reached[p] > 0, p                               # the premise: the graph takes the branch it was built for
    us.check(r, expect, db)
    us.check(r, expect, ref)
    same_store(db, ref)


def test_premises_of_the_hand_built_graphs():
    ops, expect, _, alone, shared = us.earlier_cull_dooms_a_later_one()
    ref = un.Store()
    r = us.play(alone, ref)[0]
    assert r["record"].tolist() == [[11, 9, 0, 0]] and 0.9 * 11 > 9 > 0.9 * 9          # alone it is kept
    ref = un.Store()
    us.play(ops, ref)
    assert all(ref.mp[p].bad and not ref.mp[p].observations for p in shared)
    assert ref.kf[6].mvpMapPoints[9:11] == [-1, -1]
    ops, _, _, (a, b, c, red6) = us.observation_and_row_disagree()
    ref = un.Store()
    us.play(ops, ref)
    assert ref.mp[a].bad and 6 in ref.mp[b].observations and ref.kf[6].mvpMapPoints[0] == -1 and ref.kf[6].mvpMapPoints[1] == c
    assert all(6 not in ref.mp[p].observations for p in red6)
    from fractions import Fraction
    assert Fraction(0.9 * 10) == 9 and Fraction(0.9 * 11) != Fraction(99, 10) and 9 < 0.9 * 11 < 10     # the exact and the inexact product
    ops, _, _ = us.reference_key_frame()
    ref = un.Store()
    us.play(ops, ref)
    assert ref.ucounts["empty_begin"] == 1 and ref.geo[1001].ref_kf == 5 and ref.geo[1000].ref_kf == 2


def test_the_hand_built_graphs_reach_every_path_together():
    reached = dict.fromkeys(un.PATHS, 0)
    for f in us.HAND.values():
        ref = un.Store()
        us.play(f()[0], ref)
        for k, v in ref.paths().items():
            reached[k] += v
    missing = [k for k, v in reached.items() if v == 0]
    assert missing == [], missing


@pytest.fixture(scope="module")
def random_runs():
    runs = []
    for seed in SEEDS:
        ops = us.random_script(seed)
        ref = un.Store()
        runs.append((ops, us.play(ops, ref), ref))
    return runs


def test_random_scripts_take_every_branch(random_runs):
    kinds = {op[0] for ops, _, _ in random_runs for op in ops}
    assert kinds >= {"kfs", "points", "conn", "attr", "cull", "connect", "update", "bad", "remove"}
    culls = [r for _, rs, _ in random_runs for r in rs if "culled" in r]
    actions = np.concatenate([r["record"][:, 3] for r in culls])
    assert set(actions.tolist()) == {un.KEPT, un.CULLED, un.DEFERRED, un.SKIPPED_ORIGIN}
    assert max(len(r["culled"]) for r in culls) >= 3
    assert sum(int(r["point_bad"].sum()) for r in culls) > 0 and sum(sum(len(x) for x in r["nulled"]) for r in culls) > 0
    flags = np.concatenate([r["flags"] for r in culls])
    for bit in (us.W, us.O, us.P, us.CH, us.NU, us.BAD):
        assert (flags & bit).any(), bit
    total = dict.fromkeys(un.PATHS, 0)
    for _, _, ref in random_runs:
        for k, v in ref.paths().items():
            total[k] += v
    for k in ("decision_saw_null_from_this_call", "decision_saw_lowered_count", "tree_winner", "erase_stereo", "erase_mono", "depth_far", "monocular_entry", "stopped_at_3", "list_ended_short"):
        assert total[k] > 0, k


@pytest.mark.parametrize("i", range(len(SEEDS)))
def test_random_scripts_match_the_restatement(random_runs, i):
    ops, r_np, ref = random_runs[i]
    db = lib.LocalMap()
    same_results(us.play(ops, db), r_np)
    st = db.cull_stats()
    assert all(st[k] == v for k, v in ref.ucounts.items())
    assert all(db.connect_stats()[k] == v for k, v in ref.ccounts.items())
    assert all(db.stats()[k] == v for k, v in ref.counts.items())
    same_store(db, ref)


def _refused(fn, rc=lib.ERR_INVALID):
    with pytest.raises(lib.DrfeError) as e:
        fn()
    assert e.value.rc == rc
    return str(e.value)


def _base(name="earlier_cull_dooms_a_later_one"):
    ops, expect = us.HAND[name]()[:2]
    db = lib.LocalMap()
    us.play(ops[:-1], db)
    return db, ops, expect


def _answers_as_untouched(db, ops, expect):
    """the refused calls left nothing behind: the scenario's own call still gives the hand-written answer, and the store then
    equals the restatement's"""
    assert db.cull_stats()["calls"] == 0
    ref = un.Store()
    r_np = us.play(ops, ref)
    r = us.play(ops[-1:], db)
    same_results(r, r_np)
    us.check(r, expect, db)
    same_store(db, ref)


def test_duplicate_unknown_and_bad_handles_are_refused():
    db, ops, expect = _base()
    _refused(lambda: db.cull([5, 6, 5], mode="host"))
    _refused(lambda: db.cull([5, 99], mode="host"))
    _refused(lambda: db.cull([-1], mode="host"))
    db.set_bad(ls.KEYFRAME, [6], [1])
    msg = _refused(lambda: db.cull([5, 6], mode="host"))
    assert "already bad" in msg
    db.set_bad(ls.KEYFRAME, [6], [0])
    _answers_as_untouched(db, ops, expect)


def test_missing_attributes_are_named():
    db, ops, expect = _base()
    attr = ops[-2]
    assert attr[0] == "attr"
    kf5 = [r for r in attr[1] if r["handle"] == 5][0]
    kf2 = [r for r in attr[1] if r["handle"] == 2][0]
    p = [r for r in attr[2] if r["handle"] == 1000][0]
    db.remove(ls.KEYFRAME, 5)                                  # drops the attributes with the key frame
    db.set_keyframes([r for r in ops[0][1] if r["handle"] == 5])
    _refused(lambda: db.get_cull_attributes([5], []))
    msg = _refused(lambda: db.cull([5, 6], mode="host"), lib.ERR_STATE)
    assert "key frame 5" in msg
    db.set_cull_attributes([dict(kf5, octave=kf5["octave"][:-1], depth=kf5["depth"][:-1], stereo=kf5["stereo"][:-1])], [])
    assert "key frame 5" in _refused(lambda: db.cull([5, 6], mode="host"), lib.ERR_STATE)          # arrays that do not fit the row
    db.set_cull_attributes([kf5], [])
    db.remove(ls.POINT, 1000)
    db.set_points([r for r in ops[1][1] if r["handle"] == 1000])
    assert "map point 1000" in _refused(lambda: db.cull([6], mode="host"), lib.ERR_STATE)
    db.set_cull_attributes([], [dict(p, obs_index=[0, 0, 0, 400])])
    msg = _refused(lambda: db.cull([6], mode="host"), lib.ERR_STATE)
    assert "obs_index 400" in msg and "map point 1000" in msg
    db.set_cull_attributes([], [p])
    db.remove(ls.KEYFRAME, 2)
    db.set_keyframes([r for r in ops[0][1] if r["handle"] == 2])
    msg = _refused(lambda: db.cull([6], mode="host"), lib.ERR_STATE)
    assert "observing key frame 2" in msg and "map point" in msg
    db.set_cull_attributes([kf2], [])
    _answers_as_untouched(db, ops, expect)


def test_a_culled_key_frame_without_a_parent_undoes_the_call():
    """5 is culled, its points die and null 6's row; then 6 would be culled and has no parent: everything 5 did is taken back"""
    db, ops, expect = _base()
    kf6 = [r for r in ops[0][1] if r["handle"] == 6][0]
    db.set_keyframes([dict(kf6, parent=-1)])
    msg = _refused(lambda: db.cull([5, 6], mode="host"), lib.ERR_STATE)
    assert "key frame 6" in msg and "no parent" in msg
    g = db.get_cull_attributes([], [1009, 1010])
    assert [p["n_obs"] for p in g["points"]] == [2, 2]
    db.set_keyframes([kf6])
    _answers_as_untouched(db, ops, expect)


@pytest.mark.parametrize("which", range(7))
def test_too_small_output_array_changes_nothing(which):
    db, ops, expect = _base("stereo_and_mono_cross_the_line")
    e = expect[0]
    need = [len(e["touched"]), 0, 0, 3, 2, len(e["points"]), sum(len(o) for o in e["obs"])]
    if need[which] == 0:
        cap = list(need)
        db.cull(ops[-1][1], mode="host", capacity=cap)         # nothing of that kind is returned: 0 suffices
        return
    cap = list(need)
    cap[which] -= 1
    _refused(lambda: db.cull(ops[-1][1], mode="host", capacity=cap), lib.ERR_CAPACITY)
    ref = un.Store()
    r_np = us.play(ops, ref)
    r = [db.cull(ops[-1][1], mode="host", capacity=need)]      # the exact sizes suffice
    same_results(r, r_np)
    us.check(r, expect, db)
    assert db.cull_stats()["calls"] == 1
    same_store(db, ref)


def test_device_entry_without_a_context_is_a_state_error():
    db, ops, expect = _base()
    _refused(lambda: db.cull(ops[-1][1], mode="device"), lib.ERR_STATE)
    r = [db.cull(ops[-1][1], mode="batch")]                    # _batch of a host-only store runs on the host
    us.check(r, expect, db)
    assert db.cull_stats()["device_calls"] == 0


def test_a_store_without_attributes_behaves_as_before():
    ops = us.earlier_cull_dooms_a_later_one()[0]
    plain = [op for op in ops if op[0] in ("kfs", "points")]
    db, ref = lib.LocalMap(), un.Store()
    us.play(plain, db)
    us.play(plain, ref)
    q = [dict(frame_id=5, points=sorted(ref.mp))]
    ln.same(db.update(q, mode="host"), ref.update(q))
    cn.same_connect(db.connect([5, 6], mode="host"), ref.connect([5, 6]))
    assert "key frame 5" in _refused(lambda: db.cull([5], mode="host"), lib.ERR_STATE)


def test_an_empty_call():
    db, ops, expect = _base()
    r = db.cull([], mode="host")
    assert len(r["touched"]) == 0 and r["record"].shape == (0, 4) and len(r["culled"]) == 0
    _answers_as_untouched(db, ops, expect)


def test_native_caller_on_the_host_entries():
    """tests/native/cull_caller.cpp: the adaptor's SyncCulling / KeyFrameCulling on stand-in types whose SetBadFlag and
    EraseObservation restate the reference's; every store row against the objects' accessors after every call"""
    import subprocess
    import native_build
    exe = native_build.caller("cull_caller")
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "cull_caller ok (host, 6 calls, 7 culled" in p.stdout, (p.returncode, p.stdout, p.stderr)
