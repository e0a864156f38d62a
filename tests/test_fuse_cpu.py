"""The fuse commit on the host (drfe_lmap_fuse_host, dr_slam_amd/csrc/lmap_fuse.cpp with fuse_core.h) against tests/fuse_numpy.py
and against values worked out by hand (tests/fuse_scenarios.py).  Equal bytes everywhere; no GPU.

Parity with a build of the reference's ORBmatcher.cc, LSDmatcher.cpp, MapPoint.cc, MapLine.cpp and LoopClosing.cc is not pinned:
they include OpenCV, Eigen and PCL headers that are not installed where this was written."""
import itertools
import re

import numpy as np
import pytest

import fuse_numpy as fn
import fuse_scenarios as fs
from dr_slam_amd import lib

POINT, LINE = fs.POINT, fs.LINE
SEEDS = tuple(range(311, 319))
FRAME_IDS = itertools.count(10 ** 6)                                   # frame ids rise on a store


def _refused(call, rc):
    with pytest.raises(lib.DrfeError) as e:
        call()
    assert e.value.rc == rc, str(e.value)
    return str(e.value)


def store_of(w, ctx=None):
    db = lib.LocalMap(ctx)
    fs.load(db, w)
    return db


def same_following(a, b, w, mode_a="host", mode_b="host", connect=True):
    """an UpdateLocalMap over every point and line and over the rows, and an UpdateConnections of every key frame that is not
    bad, on two stores that should hold the same"""
    q = [dict(frame_id=next(FRAME_IDS), points=sorted(w.items[POINT]), lines=sorted(w.items[LINE]))]
    q += [dict(frame_id=next(FRAME_IDS), points=k["rows"][POINT], lines=k["rows"][LINE]) for k in w.kfs.values()]
    ua, ub = a.update(q, mode=mode_a), b.update(q, mode=mode_b)
    for key in ua:
        for x, y in zip(ua[key], ub[key]):
            assert np.array_equal(x, y), key
    if not connect:                                                     # a connect changes the graph the next update expands over
        return
    alive = [h for h, k in w.kfs.items() if not k["bad"]]
    ca, cb = a.connect(alive, mode=mode_a), b.connect(alive, mode=mode_b)
    # the votes are over exactly the rows a fusion rewrites; what a connect leaves of parents and change flags depends on the
    # connects before it, which only one of the two stores has seen
    assert len(ca["counter"]) == len(cb["counter"]) and all(np.array_equal(x, y) for x, y in zip(ca["counter"], cb["counter"]))
    assert np.array_equal(ca["record"], cb["record"])


def test_symbols_and_constants():
    L = lib.load()
    for s in lib.SYMBOLS:
        if "fuse" in s or s in ("drfe_lmap_get_replaced", "drfe_lmap_get_match_row", "drfe_lmap_get_observers"):
            assert hasattr(L, s), s
    text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    lim = lib.LocalMap.fuse_limits()
    most = int(re.search(r"DRFE_LMAP_FUSE_MAX_CANDIDATES = 1 << (\d+)", text).group(1))
    assert lim["max_candidates"] == 1 << most
    assert lim["tile"] % 64 == 0 and lim["wavefront"] == 64 and lim["tile_bytes"] == 4 * lim["tile"] + 4
    assert lim["log_entries"] > 0 and lim["record_entries"] >= lim["log_entries"] and lim["max_kfs"] % 32 == 0
    forms = re.search(r"DRFE_LMAP_FUSE_NEIGHBOURS = (\d), DRFE_LMAP_FUSE_LOOP = (\d), DRFE_LMAP_FUSE_MATCHED = (\d)", text).groups()
    assert tuple(int(v) for v in forms) == (lib.FUSE_NEIGHBOURS, lib.FUSE_LOOP, lib.FUSE_MATCHED) == (fn.NEIGHBOURS, fn.LOOP, fn.MATCHED)
    for name, value in (("NONE", fn.NONE), ("SKIPPED", fn.SKIPPED), ("ADDED", fn.ADDED), ("ROW_ONLY", fn.ROW_ONLY),
                        ("OCCUPANT_BAD", fn.OCCUPANT_BAD), ("CANDIDATE_REPLACED", fn.CANDIDATE_REPLACED),
                        ("OCCUPANT_REPLACED", fn.OCCUPANT_REPLACED), ("SELF", fn.SELF), ("RECORDED", fn.RECORDED)):
        assert int(re.search(r"DRFE_LMAP_FUSE_%s = (\d)" % name, text).group(1)) == value == getattr(lib, "FUSE_" + name)
    assert (lib.LMAP_POINT, lib.LMAP_LINE) == (POINT, LINE)


def test_device_from_is_the_measured_crossover():
    """profiles/fuse_timing.jsonl (tools/fuse_timing.py): its last line is the constant, and the rows give it by the rule of DESIGN.md
    section 32 - the smallest number of candidates per call from which the device entry wins at every measured store size in both
    answered shares, else above the longest call"""
    import json
    rows = [json.loads(x) for x in open(lib.os.path.join(lib._HERE, "..", "profiles", "fuse_timing.jsonl"))]
    measured = rows[-1]["device_from"]
    lim = lib.LocalMap.fuse_limits()
    assert lim["device_from"] == (measured if measured is not None else lim["max_candidates"] + 1)
    shapes = rows[:-1]
    assert {r["keyframes"] for r in shapes} == {100, 400, 1600} and {r["shape"] for r in shapes} == {"neighbours", "loop"}
    assert {r["answered_share"] for r in shapes} == {0.05, 0.2} and len(shapes) == 12 and all(r["equal"] for r in shapes)
    assert all({"device_ms", "host_ms", "baseline_ms"} <= set(r) for r in shapes)
    sizes = sorted({r["candidates"] for r in shapes}, reverse=True)
    want = None
    for n in sizes:
        if not all(r["device_wins"] for r in shapes if r["candidates"] == n):
            break
        want = n
    assert measured == want
    for r in shapes:
        assert r["device_wins"] == (r["host_ms"] - r["device_ms"] > max(r["device_iqr_ms"], r["host_iqr_ms"]))
    assert max(sizes) < lim["max_candidates"]
    if measured is None:
        text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
        assert re.search(r"DRFE_LMAP_FUSE_DEVICE_FROM = DRFE_LMAP_FUSE_MAX_CANDIDATES \+ 1 ", text)


@pytest.mark.parametrize("scenario", fs.SCENARIOS, ids=lambda f: getattr(f, "__name__", "snapshot_neighbours"))
def test_scenarios_by_hand(scenario):
    """the restatement and the host entry against the hand-written results, and against each other in everything"""
    w, steps, expect = scenario()
    db = store_of(w)
    fs.same_state(fs.state_of_store(db, w), fs.state_of_world(w))      # the bridge itself
    want = w.fuse(steps)
    fs.check_expect(want, fs.state_of_world(w), expect)
    got = db.fuse(steps, mode="host")
    fs.check_expect(got, fs.state_of_store(db, w), expect)
    fs.same_result(got, want)
    fs.same_state(fs.state_of_store(db, w), fs.state_of_world(w))
    same_following(db, store_of(w), w)
    st = db.fuse_stats()
    assert st["calls"] == 1 and st["device_calls"] == 0 and st["candidates"] == sum(len(s["candidates"]) for s in steps)
    assert st["replaced"] == len(want["replaced"]) and st["moved"] + st["erased"] == sum(len(r[3]) for r in want["replaced"])


def test_the_scenarios_take_every_branch():
    total = {}
    for scenario in fs.SCENARIOS:
        w, steps, _ = scenario()
        w.fuse(steps)
        for k, v in w.paths().items():
            total[k] = total.get(k, 0) + v
    for k in ("none", "skipped_bad", "skipped_in_kf", "tie", "replace_self", "replace_emptied", "replace_bad_winner", "replace_moved",
              "replace_erased", "add_observation_noop", "insert_front", "insert_middle", "insert_end", "loop_candidate_bad_in_pass2",
              "form_0", "form_1", "form_2") + tuple("action_%d" % a for a in range(9)):
        assert total.get(k, 0) > 0, k


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_scripts(seed):
    """calls interleaved with set_bad, counter edits, recent_cull, update and connect: the store follows the restatement, and a
    store loaded afresh from the restatement gives the same following calls"""
    rng = np.random.default_rng(seed)
    w = fs.random_world(rng)
    db = store_of(w)
    for round_ in range(4):
        steps = fs.random_steps(rng, w)
        fs.same_result(db.fuse(steps, mode="host"), w.fuse(steps))
        fs.same_state(fs.state_of_store(db, w), fs.state_of_world(w))
        same_following(db, store_of(w), w, connect=round_ == 3)
        pts = [int(p) for p in rng.choice(sorted(w.items[POINT]), 6, replace=False)]
        flags = [int(v) for v in rng.integers(0, 2, 6)]
        db.set_bad(POINT, pts, flags)
        db.recent_increase(POINT, pts, [3] * 6, [5] * 6)
        for p, f in zip(pts, flags):
            w.items[POINT][p]["bad"] = f
            w.items[POINT][p]["found"] += 3
            w.items[POINT][p]["visible"] += 5
        if round_ == 1:
            # MapPointCulling between two fusions: the store's own walk; the restatement is told what it did
            listed = [int(p) for p in rng.choice(sorted(w.items[POINT]), 20, replace=False)]
            r = db.recent_cull(6, listed, [], mode="host")["points"]
            for h, erased in zip(r["culled"], r["erased"]):
                w.items[POINT][int(h)].update(bad=1, obs=[])
                for kf, idx in erased:
                    w.kfs[int(kf)]["rows"][POINT][int(idx)] = -1
            fs.same_state(fs.state_of_store(db, w), fs.state_of_world(w))
    assert w.paths().get("replace_moved", 0) > 0 and w.paths().get("replace_erased", 0) > 0


def test_fuse_after_a_keyframe_cull():
    """a KeyFrameCulling between two fusions: observations of the culled key frames are gone, nObs shrank, the culled key frames'
    rows still name the points; the fusion after it runs on that, also on a culled key frame"""
    w = fs.redundant_world()
    db = store_of(w)
    before, after = fs.steps_around_a_cull()
    fs.same_result(db.fuse(before, mode="host"), w.fuse(before))
    n_obs = w.items[POINT][101]["n_obs"]
    r = db.cull([30, 40], mode="host")
    assert [int(h) for h in r["culled"]] == [30, 40]
    fs.apply_cull(w, r)
    assert w.items[POINT][101]["n_obs"] == n_obs - 2 and not w._in_kf(POINT, 100, 30) and w.kfs[30]["rows"][POINT][0] == 100
    fs.same_state(fs.state_of_store(db, w), fs.state_of_world(w))
    fs.same_result(db.fuse(after, mode="host"), w.fuse(after))
    fs.same_state(fs.state_of_store(db, w), fs.state_of_world(w))
    assert w.paths()["replace_moved"] > 0 and w.paths()["replace_erased"] > 0 and w.kfs[30]["rows"][POINT][14] == 100


def test_capacity_refuses_and_changes_nothing():
    w, steps, _ = fs.tie_occupant_loses()
    db = store_of(w)
    before = fs.state_of_store(db, w)
    for cap in ((0, 8, 8), (8, 1, 8), (8, 8, 0)):
        assert "returns more than" in _refused(lambda: db.fuse(steps, mode="host", capacity=cap), lib.ERR_CAPACITY)
        fs.same_state(fs.state_of_store(db, w), before)
    fs.same_result(db.fuse(steps, mode="host", capacity=(1, 2, 1)), w.fuse(steps))
    assert db.fuse_stats()["calls"] == 1


def test_refusals_change_nothing():
    w = fs.base()
    w.add_item(POINT, 100, [(20, 0)])
    w.add_item(POINT, 101, [(10, 2)])
    w.add_item(LINE, 500, [(10, 0)])
    db = store_of(w)
    before = fs.state_of_store(db, w)
    S = fs.step
    cases = [
        ([S(99, [100], [1])], lib.ERR_INVALID, "unknown key frame 99"),
        ([S(10, [4242], [1])], lib.ERR_INVALID, "unknown map point 4242"),
        ([S(10, [4242], [1], kind=LINE)], lib.ERR_INVALID, "unknown map line 4242"),
        ([S(10, [100], [1], form=7)], lib.ERR_INVALID, "unknown form"),
        ([S(10, [100], [1], kind=0)], lib.ERR_INVALID, "unknown kind"),
        ([S(10, [500], [1], kind=LINE, form=fs.LOOP)], lib.ERR_STATE, "for map points"),
        ([S(10, [-1] * 4, kind=LINE, form=fs.MATCHED)], lib.ERR_STATE, "for map points"),
        ([S(10, [100, -1], [1, 1], form=fs.LOOP)], lib.ERR_STATE, "null candidate at 1"),
        ([S(10, [100] * 7, form=fs.MATCHED)], lib.ERR_STATE, "MATCHED list of 7"),
        ([S(10, [100], [8])], lib.ERR_STATE, "best_idx 8"),
        ([S(10, [500], [4], kind=LINE)], lib.ERR_STATE, "best_idx 4"),
        # a good first step does not save the call: nothing of it is applied
        ([S(10, [100], [2]), S(10, [100], [9])], lib.ERR_STATE, "best_idx 9"),
    ]
    for steps, rc, text in cases:
        assert text in _refused(lambda: db.fuse(steps, mode="host"), rc), text
        fs.same_state(fs.state_of_store(db, w), before)
    assert db.fuse_stats()["calls"] == 0
    assert "without a context" in _refused(lambda: db.fuse([S(10, [100], [1])], mode="device"), lib.ERR_STATE)


def test_refusals_for_missing_state():
    """an item that can take part without its attributes, an obs_index outside its observer's row, a key frame without stereo
    flags; an item that cannot take part may lack them"""
    S = fs.step
    w = fs.base()
    w.add_item(POINT, 100, [(20, 0)])
    w.add_item(POINT, 101, [(10, 2)])
    w.add_item(POINT, 102, [(30, 0)])
    w.add_item(LINE, 500, [(10, 0)])
    w.add_item(LINE, 501, [(20, 0)])

    def fresh(points=True, lines=True, cull=True, cull_kf=True, skip=()):
        db = lib.LocalMap()
        fs.load(db, w)
        db2 = lib.LocalMap()
        db2.set_keyframes([dict(handle=h, rank=k["rank"], points=k["rows"][POINT], lines=k["rows"][LINE]) for h, k in w.kfs.items()])
        db2.set_points([dict(handle=h, bad=p["bad"], obs=[k for k, _ in p["obs"]]) for h, p in w.items[POINT].items()])
        db2.set_lines(sorted(w.items[LINE]))
        db2.set_cull_attributes(
            kfs=[dict(handle=h, th_depth=40.0, octave=[0] * 8, depth=[1.0] * 8, stereo=k["stereo"]) for h, k in w.kfs.items()
                 if cull_kf or h != 10],
            points=[dict(handle=h, n_obs=p["n_obs"], obs_index=[i for _, i in p["obs"]]) for h, p in w.items[POINT].items()
                    if cull and h not in skip])
        db2.set_recent_attributes(
            points=[dict(handle=h, found=1, visible=1, first_kf=0) for h in w.items[POINT] if points and h not in skip],
            lines=[dict(handle=h, found=1, visible=1, first_kf=0, n_obs=1, obs=[k for k, _ in l["obs"]], obs_index=[i for _, i in l["obs"]])
                   for h, l in w.items[LINE].items() if lines and h not in skip])
        return db2

    assert "map point 100 has no recent-list counters" in _refused(lambda: fresh(skip=(100,)).fuse([S(10, [100], [4])], mode="host"), lib.ERR_STATE)
    # the occupant takes part as well
    assert "map point 101 has no recent-list counters" in _refused(lambda: fresh(skip=(101,)).fuse([S(10, [100], [2])], mode="host"), lib.ERR_STATE)
    assert "map line 500 has no recent-list state" in _refused(lambda: fresh(skip=(500,)).fuse([S(10, [501], [0], kind=LINE)], mode="host"), lib.ERR_STATE)
    assert "key frame 10 has no culling attributes" in _refused(lambda: fresh(cull_kf=False).fuse([S(10, [100], [4])], mode="host"), lib.ERR_STATE)
    # 102 lacks everything and is not named: the call runs
    db = fresh(skip=(102,))
    assert [int(a) for a in db.fuse([S(10, [100], [4])], mode="host")["steps"][0]["action"]] == [fs.ADDED]
    # an obs_index outside the observer's row
    db = fresh()
    db.set_cull_attributes(points=[dict(handle=100, n_obs=1, obs_index=[8])])
    assert "map point 100: obs_index 8 lies outside the row of key frame 20" in _refused(lambda: db.fuse([S(10, [100], [4])], mode="host"), lib.ERR_STATE)


def test_replaced_field():
    w, steps, _ = fs.tie_occupant_loses()
    db = store_of(w)
    assert list(db.get_replaced(POINT, [100, 101])) == [-1, -1]
    db.fuse(steps, mode="host")
    assert list(db.get_replaced(POINT, [100, 101])) == [-1, 100]
    assert _refused(lambda: db.get_replaced(POINT, [4242]), lib.ERR_INVALID)
    db.set_points([dict(handle=101, obs=[])])                           # a new object under the handle
    assert list(db.get_replaced(POINT, [101])) == [-1]
    w2, steps2, _ = fs.lines_and_bad_keyframe()
    db2 = store_of(w2)
    db2.fuse(steps2, mode="host")
    assert list(db2.get_replaced(LINE, [500, 501, 502])) == [-1, 500, -1]
    db2.remove(LINE, 501)
    assert _refused(lambda: db2.get_replaced(LINE, [501]), lib.ERR_INVALID)
    db2.set_lines([501])
    assert list(db2.get_replaced(LINE, [501])) == [-1]


def test_batch_is_the_host_below_the_crossover():
    w, steps, _ = fs.second_meets_first()
    a, b = store_of(w), store_of(w)
    fs.same_results(a.fuse(steps, mode="batch"), b.fuse(steps, mode="host"))
    fs.same_state(fs.state_of_store(a, w), fs.state_of_store(b, w))
    assert a.fuse_stats() == b.fuse_stats()


def test_native_caller_on_the_host_entry():
    """tests/native/fuse_caller.cpp: the adaptor's Fuse (points and lines), FuseLoop and FuseMatched on stand-in types whose Replace
    and AddObservation restate the reference's, next to the reference's loops on a twin; the store against the objects through the
    getters after every round"""
    import subprocess
    import native_build
    exe = native_build.caller("fuse_caller")
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "fuse_caller ok (host, 68 calls, 142 added, 340 replaced" in p.stdout, (p.returncode, p.stdout, p.stderr)
