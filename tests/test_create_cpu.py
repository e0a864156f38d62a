"""CPU tests of map-point and map-line creation on the local-map store (drfe_lmap_create_host): the host
entry against tests/create_numpy.py - displaced handles and records bit for bit, the store afterwards through every getter, the
counters - on every hand-built store of tests/create_scenarios.py, whose hand-written expectations are first proved on the
restatement; the store against one built from scratch through the setters from the final state, through the getters and through a
following call of every other operation; the append that leaves no image stale; every refusal with the store unchanged; the
capacities; and seeded scripts that interleave the call with the other operations of the store."""
import itertools
import re

import numpy as np
import pytest

import create_numpy as cn
import create_scenarios as sc
import insert_scenarios as ins
from dr_slam_amd import lib

POINT, LINE = sc.POINT, sc.LINE
FRAME_IDS = itertools.count(4 * 10 ** 6)


def refused(call, rc):
    with pytest.raises(lib.DrfeError) as e:
        call()
    assert e.value.rc == rc, str(e.value)
    return str(e.value)


def store_of(w, ctx=None, geometry=True):
    db = lib.LocalMap(ctx)
    sc.load(db, w, geometry)
    return db


def same_any(x, y, where=""):
    """two results of one operation on two stores, byte for byte, whatever their shape"""
    if isinstance(x, dict):
        assert set(x) == set(y), where
        for k in x:
            same_any(x[k], y[k], "%s.%s" % (where, k))
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), where
        for i, (p, q) in enumerate(zip(x, y)):
            same_any(p, q, "%s[%d]" % (where, i))
    elif isinstance(x, np.ndarray):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), where
    else:
        assert x == y, where


def follow(a, b, w, mode_a="host", mode_b="host", seed=0):
    """one call of every other operation of the store on two stores that should hold the same, in an order in which the ones that
    take something away come last; every result byte for byte"""
    rng = np.random.default_rng(seed)
    kfs = sorted(w.kfs)
    pts, lns = sorted(w.items[POINT]), sorted(w.items[LINE])
    root = min(w.kfs, key=lambda h: w.kfs[h]["rank"])

    def both(name, call):
        same_any(call(a, mode_a), call(b, mode_b), name)

    def update():
        q = [dict(frame_id=next(FRAME_IDS), points=pts, lines=lns)]
        q += [dict(frame_id=next(FRAME_IDS), points=k["rows"][POINT], lines=k["rows"][LINE]) for k in w.kfs.values()]
        ids = [f["frame_id"] for f in q]
        both("update", lambda lm, m: lm.update([dict(f, frame_id=i) for f, i in zip(q, ids)], mode=m))
    update()
    both("insert", lambda lm, m: lm.insert(kfs[:3], mode=m, normals=True))
    if len(pts) >= 6:
        cands = [int(c) for c in rng.choice(pts, 6, replace=False)]
        best = [int(v) for v in rng.integers(-1, len(w.kfs[kfs[0]]["rows"][POINT]), 6)]
        both("fuse", lambda lm, m: lm.fuse([dict(keyframe=kfs[-1], kind=POINT, form=0, candidates=cands, best_idx=best)], mode=m))
    if pts:
        Scw = [0.0, 0.0, 0.0, 1.0, 0.0625, -0.125, 0.03125, 1.0]
        both("correct", lambda lm, m: lm.correct(kfs[0], Scw, kfs[:3], mode=m))
        T = np.stack([w.poses[h] for h in kfs]).copy()
        T[:, 0, 3] += np.float32(0.25)
        X = np.zeros((len(pts), 3), np.float32) + np.float32(0.125)
        for lm in (a, b):
            lm.set_gba_keyframes(kfs, T, [root] * len(kfs))
            lm.set_gba_points(pts, X, [root] * len(pts))
        both("gba", lambda lm, m: lm.gba(root, [root], mode=m))
    alive = [h for h in kfs if not w.kfs[h]["bad"]]
    both("connect", lambda lm, m: lm.connect(alive, mode=m))
    update()
    both("recent_cull", lambda lm, m: lm.recent_cull(7, [h for h in pts if not w.items[POINT][h].get("no_cull")][:40], lns[:10], mode=m))
    both("cull", lambda lm, m: lm.cull(alive[:6], mode=m))
    update()


def expected_stats(want, stale=0, device=0, chunks=0):
    disp = sum(int(v) >= 0 for name in ("point_displaced", "line_displaced") for r in want[name] for v in r)
    return dict(calls=1, device_calls=device, points_created=len(want["point_displaced"]), lines_created=len(want["line_displaced"]),
                displaced=disp, stale_calls=stale, device_chunks=chunks)


def stats_less_relayouts(db):
    st = db.create_stats()
    st.pop("relayouts")
    return st


def test_symbols_and_constants():
    L = lib.load()
    mine = [s for s in lib.SYMBOLS if s.startswith("drfe_lmap_create_")]
    assert len(mine) == 6 and all(hasattr(L, s) for s in mine)
    text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    for s in mine:
        assert re.search(r"\bint %s\(" % s, text), s
    assert (cn.ERR_INVALID, cn.ERR_CAPACITY, cn.ERR_STATE) == (lib.ERR_INVALID, lib.ERR_CAPACITY, lib.ERR_STATE)
    lim = lib.LocalMap.create_limits()
    assert lim["tile"] % 64 == 0 and lim["wavefront"] == 64 and lim["claim_bytes"] == 4 and lim["item_bytes"] == 4
    assert lim["device_from"] == int(re.search(r"DRFE_LMAP_CREATE_DEVICE_FROM = (\w+)", text).group(1), 0)
    assert lib.C.sizeof(lib.LmapCreateCall) == 8 + 8 * len(lib.LMAP_CREATE_IN_FIELDS) + 16 + 8 * len(lib.LMAP_CREATE_OUT_FIELDS)


@pytest.mark.parametrize("scenario", sc.SCENARIOS, ids=lambda f: f.__name__)
def test_scenarios_on_the_host(scenario):
    w, points, lines, expect = scenario()
    db = store_of(w)
    want = cn.create(w, points, lines)
    sc.check_expect(dict(want, normal=np.array(want["normal"])), sc.state_of_world(w), expect)     # the premise, on the restatement
    got = db.create(points, lines, mode="host")
    sc.same_result(got, want)
    sc.check_expect(got, sc.state_of_store(db, w), expect)
    sc.same_state(sc.state_of_store(db, w), sc.state_of_world(w))
    assert stats_less_relayouts(db) == expected_stats(want, stale=expect["stale"])
    follow(db, store_of(w), w)
    # the batch entry runs on the host below the crossover: the same bytes
    v, p2, l2, _ = scenario()
    sc.same_results(store_of(v).create(p2, l2, mode="batch"), got)


@pytest.mark.parametrize("scenario", (sc.descending_rank, sc.two_on_one_entry, sc.lines_alone), ids=lambda f: f.__name__)
def test_without_normals_the_level_is_still_stored(scenario):
    w, points, lines, _ = scenario()
    db = store_of(w, geometry=False)
    if points:
        refused(lambda: db.create(points, lines, mode="host", normals=True), lib.ERR_STATE)
    got = db.create(points, lines, mode="host", normals=False)
    want = cn.create(w, points, lines, normals=False)
    sc.same_result(got, want, normals=False)
    sc.same_state(sc.state_of_store(db, w), sc.state_of_world(w))


@pytest.mark.parametrize("case", sc.refusals(), ids=lambda c: c[0])
def test_refusals_change_nothing(case):
    _, w, points, lines, normals, rc, word = case
    db = store_of(w)
    before = sc.state_of_store(db, w)
    with pytest.raises(cn.Refused) as e:
        cn.create(w.clone(), points, lines, normals=normals)
    assert e.value.rc == rc
    assert word in refused(lambda: db.create(points, lines, mode="host", normals=normals), rc)
    refused(lambda: db.create(points, lines, mode="batch", normals=normals), rc)
    assert sc.state_of_store(db, w) == before
    assert db.size() == (len(w.kfs), len(w.items[POINT]), len(w.items[LINE]))
    assert db.create_stats()["calls"] == 0
    if rc == lib.ERR_INVALID:                                           # the stores of the other cases lack what the operations read
        follow(db, store_of(w), w)


def test_capacities():
    """an output array that is too small refuses the call and changes nothing"""
    w, points, lines, _ = sc.both_kinds()
    db = store_of(w)
    before = sc.state_of_store(db, w)
    assert "displaced_capacity[0]" in refused(lambda: db.create(points, lines, mode="host", capacity=(3, 2)), lib.ERR_CAPACITY)
    assert "record_capacity" in refused(lambda: db.create(points, lines, mode="host", capacity=(4, 1)), lib.ERR_CAPACITY)
    assert "displaced_capacity[1]" in refused(lambda: db.create([], lines, mode="host", capacity=(1, 0)), lib.ERR_CAPACITY)
    assert sc.state_of_store(db, w) == before and db.create_stats()["calls"] == 0
    sc.same_result(db.create(points, lines, mode="host", capacity=(4, 2)), cn.create(w, points, lines))


@pytest.mark.parametrize("seed", (3401, 3402))
def test_same_store_as_the_setters(seed):
    """after create calls, the store against one built from scratch through the setters from the final state: every getter, and a
    following call of every other operation.  Also against a store that received the same items through the five setters."""
    rng = np.random.default_rng(seed)
    w = sc.random_world(rng)
    db, old_way = store_of(w), store_of(w)
    for _ in range(3):
        points, lines = sc.random_creations(rng, w, 9, 4)
        sc.same_result(db.create(points, lines, mode="host"), cn.create(w, points, lines))
        sc.by_setters(old_way, w, [c["handle"] for c in points], [c["handle"] for c in lines])
    assert db.create_stats()["stale_calls"] == 0 and db.create_stats()["displaced"] > 0
    fresh = store_of(w)
    want = sc.state_of_world(w)
    for lm in (db, fresh, old_way):
        sc.same_state(sc.state_of_store(lm, w), want)
    assert db.size() == fresh.size()
    follow(db, fresh, w, seed=seed)
    follow(store_of(w), old_way, w, seed=seed)


def test_a_qualifying_call_leaves_no_image_stale():
    """create, an operation, create again: the appended slots are what the next host call walks, without a rebuild in between
    (stale_calls stays 0); one call below the stored handles is counted and the call after it is served by the rebuilt image"""
    rng = np.random.default_rng(3410)
    w = sc.random_world(rng)
    db = store_of(w)
    for r in range(3):
        points, lines = sc.random_creations(rng, w, 5, 3)
        sc.same_result(db.create(points, lines, mode="host"), cn.create(w, points, lines))
        st = db.create_stats()
        assert st["stale_calls"] == 0 and st["calls"] == r + 1
        # the room doubles: the first call lays the rows, attribute, recent-list and geometry blocks out anew, the next ones fit
        assert st["relayouts"] == 4
        q = [dict(frame_id=next(FRAME_IDS), points=sorted(w.items[POINT]), lines=sorted(w.items[LINE]))]
        same_any(db.update(q, mode="host"), store_of(w).update(q, mode="host"))
    points, lines = sc.random_creations(rng, w, 2, 0, first_point=3)
    sc.same_result(db.create(points, lines, mode="host"), cn.create(w, points, lines))
    assert db.create_stats()["stale_calls"] == 1
    points, lines = sc.random_creations(rng, w, 4, 2)
    sc.same_result(db.create(points, lines, mode="host"), cn.create(w, points, lines))
    assert db.create_stats()["stale_calls"] == 1
    sc.same_state(sc.state_of_store(db, w), sc.state_of_world(w))
    follow(db, store_of(w), w)


def sync_world(w, lm, culled=()):
    """the restatement's world brought to what an operation without a restatement here left in the store, through the getters"""
    st = ins.state_of_store(lm, w)
    for (h, kind), row in st["rows"].items():
        w.kfs[h]["rows"][kind] = list(row)
    for (kind, h), it in st["items"].items():
        w.items[kind][h].update(it)
    for h in culled:
        w.kfs[int(h)]["bad"] = 1
    kfs, pts = sorted(w.kfs), sorted(w.items[POINT])
    T = lm.get_poses(kfs)["Tcw"]
    for i, h in enumerate(kfs):
        w.poses[h] = T[i].copy()
    g = lm.get_point_geometry(pts)
    for i, h in enumerate(pts):
        w.geo[h] = dict(world=g["world"][i].copy(), ref_kf=int(g["ref_kf"][i]), ref_level=int(g["ref_level"][i]),
                        by=int(g["corrected_by"][i]), by_ref=int(g["corrected_ref"][i]))


OPS = ("update", "connect", "insert", "fuse", "recent_cull", "cull", "correct", "gba")


def run_script(seed, ctx=None, mode="host"):
    """Rounds of a create call and one of the other operations of the store, so that every later create appends behind what the
    operation left - on the device in the resident blocks.  After every create the result is held to the restatement and the
    store to its world.  A twin store runs the same script on the host entries: with a context through the host create entry,
    without one with every created item pushed through the five setters instead; every result of an operation is compared with
    the twin's, and at the end every other operation runs on both."""
    rng = np.random.default_rng(seed)
    w = sc.random_world(rng)
    db = store_of(w, ctx)
    twin = store_of(w)
    kfs = sorted(w.kfs)
    root = min(w.kfs, key=lambda h: w.kfs[h]["rank"])
    stores = [db, twin]

    def both(call):
        r = call(db, mode)
        same_any(r, call(twin, "host"))
        return r

    for r in range(len(OPS) + 1):
        points, lines = sc.random_creations(rng, w, int(rng.integers(1, 12)), int(rng.integers(0, 5)))
        normals = r % 3 != 2
        if ctx is not None:
            got = both(lambda lm, m: lm.create(points, lines, mode=m, normals=normals))
        else:
            got = db.create(points, lines, mode=mode, normals=normals)
        sc.same_result(got, cn.create(w, points, lines, normals=normals), normals=normals)
        if ctx is None:
            sc.by_setters(twin, w, [c["handle"] for c in points], [c["handle"] for c in lines])
        for lm in stores:
            sc.same_state(sc.state_of_store(lm, w), sc.state_of_world(w))
        if r == len(OPS):
            break
        op = OPS[r]
        pts, lns = sorted(w.items[POINT]), sorted(w.items[LINE])
        culled = ()
        if op == "update":
            q = [dict(frame_id=next(FRAME_IDS), points=pts, lines=lns)]
            q += [dict(frame_id=next(FRAME_IDS), points=w.kfs[h]["rows"][POINT], lines=w.kfs[h]["rows"][LINE]) for h in kfs[:4]]
            both(lambda lm, m: lm.update(q, mode=m))
        elif op == "connect":
            alive = [h for h in kfs if not w.kfs[h]["bad"]]
            both(lambda lm, m: lm.connect(alive, mode=m))
        elif op == "insert":
            called = [int(k) for k in rng.choice(kfs, 3, replace=False)]
            ins.random_puts(rng, w, called, share=0.4)
            for lm in stores:
                sc.push_rows(lm, w, called)
            a = both(lambda lm, m: lm.insert(called, mode=m, normals=True))
            assert len(a["added_points"]) > 0
        elif op == "fuse":
            cands = [int(c) for c in rng.choice(pts, 8, replace=False)]
            best = [int(b) for b in rng.integers(-1, len(w.kfs[kfs[0]]["rows"][POINT]), 8)]
            step = dict(keyframe=int(rng.choice(kfs)), kind=POINT, form=0, candidates=cands, best_idx=best)
            both(lambda lm, m: lm.fuse([step], mode=m))
        elif op == "recent_cull":
            a = both(lambda lm, m: lm.recent_cull(5, pts[::2], lns[::2], mode=m))
            assert len(a["points"]["culled"]) + len(a["lines"]["culled"]) > 0
        elif op == "cull":
            alive = [h for h in kfs if not w.kfs[h]["bad"]]
            culled = both(lambda lm, m: lm.cull(alive, mode=m))["culled"]
        elif op == "correct":
            Scw = [0.0, 0.0, 0.0, 1.0, 0.0625, -0.125, 0.03125, 1.0]
            a = both(lambda lm, m: lm.correct(kfs[1], Scw, kfs[:5], mode=m))
            assert len(a["points"]) > 0
        else:
            T = np.stack([w.poses[h] for h in kfs]).copy()
            T[:, 0, 3] += np.float32(0.25)
            X = np.stack([w.geo[p]["world"] for p in pts]) + np.float32(0.125)
            for lm in stores:
                lm.set_gba_keyframes(kfs, T, [root] * len(kfs))
                lm.set_gba_points(pts, X, [root] * len(pts))
            a = both(lambda lm, m: lm.gba(root, [root], mode=m))
            assert len(a["points"]) > 0
        sync_world(w, db, culled=culled)
        sc.same_state(sc.state_of_store(db, w), sc.state_of_world(w))
    return db, twin, w


@pytest.mark.parametrize("seed", (3421, 3422, 3423))
def test_seeded_scripts(seed):
    db, twin, w = run_script(seed)
    st = db.create_stats()
    assert st["calls"] == len(OPS) + 1 and st["device_calls"] == 0 and st["points_created"] > 0 and st["lines_created"] > 0
    assert st["stale_calls"] == 0 and twin.create_stats()["calls"] == 0
    follow(db, twin, w, seed=seed)


def test_native_caller_on_the_host_entry():
    """tests/native/create_caller.cpp: the adaptor's LocalMapTracker::CreateMapPoints and CreateMapLines, the two-observer and the
    single-observer form, on stand-in types whose AddObservation and AddMapPoint restate the reference's, next to the tail of
    CreateNewMapPoints with UpdateNormalAndDepth on a twin; the records bit for bit and the store against the objects after
    every call"""
    import subprocess
    import native_build
    exe = native_build.caller("create_caller")
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "create_caller host: ok, 265 points created" in p.stdout, (p.returncode, p.stdout, p.stderr)
