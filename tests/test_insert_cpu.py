"""CPU tests of the item loops of ProcessNewKeyFrame on the local-map store (drfe_lmap_insert_host): the host
entry against tests/insert_numpy.py - actions, lists, records bit for bit, the store afterwards through its getters, the counters
- on every hand-built store of tests/insert_scenarios.py, whose hand-written expectations are first proved on the restatement;
every refusal with the store unchanged; the capacities; and seeded scripts that interleave the call with the other operations of
the store and with setter edits, held to a store loaded afresh from the restatement's world."""
import itertools
import re

import numpy as np
import pytest

import insert_numpy as inp
import insert_scenarios as sc
from dr_slam_amd import lib

POINT, LINE = sc.POINT, sc.LINE
FRAME_IDS = itertools.count(3 * 10 ** 6)


def refused(call, rc):
    with pytest.raises(lib.DrfeError) as e:
        call()
    assert e.value.rc == rc, str(e.value)
    return str(e.value)


def store_of(w, ctx=None, geometry=True):
    db = lib.LocalMap(ctx)
    sc.load(db, w, geometry)
    return db


def same_following(a, b, w, mode_a="host", mode_b="host", connect=True):
    """an UpdateLocalMap over every item and over the rows and an UpdateConnections of every live key frame, on two stores that
    should hold the same"""
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
    assert len(ca["counter"]) == len(cb["counter"]) and all(np.array_equal(x, y) for x, y in zip(ca["counter"], cb["counter"]))
    assert np.array_equal(ca["record"], cb["record"])


def same_culls(a, b, w, mode_a="host", mode_b="host"):
    """the two operations that take something away: run last, on stores that are not compared with the world afterwards"""
    kfs = [h for h, k in w.kfs.items() if not k["bad"]][:6]
    x, y = a.cull(kfs, mode=mode_a), b.cull(kfs, mode=mode_b)
    assert np.array_equal(x["record"], y["record"]) and np.array_equal(x["culled"], y["culled"])
    pts = [h for h, p in w.items[POINT].items() if not p.get("no_cull")][:40]
    lns = [h for h, l in w.items[LINE].items() if not l.get("no_state")][:10]
    x, y = a.recent_cull(7, pts, lns, mode=mode_a), b.recent_cull(7, pts, lns, mode=mode_b)
    for name in ("points", "lines"):
        assert np.array_equal(x[name]["action"], y[name]["action"]) and np.array_equal(x[name]["culled"], y[name]["culled"])
        assert all(np.array_equal(p, q) for p, q in zip(x[name]["erased"], y[name]["erased"]))


def expected_stats(want, n_kfs, device=0, chunks=0):
    return dict(calls=1, keyframes=n_kfs, device_calls=device, points_added=len(want["added_points"]), lines_added=len(want["added_lines"]),
                recent_points=len(want["recent_points"]), recent_lines=len(want["recent_lines"]), device_chunks=chunks)


def test_symbols_and_constants():
    L = lib.load()
    for s in lib.SYMBOLS:
        if "lmap_insert" in s:
            assert hasattr(L, s), s
    assert sum("lmap_insert" in s for s in lib.SYMBOLS) == 6
    text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    for s in lib.SYMBOLS:
        if "lmap_insert" in s:
            assert re.search(r"\bint %s\(" % s, text), s
    names = re.search(r"DRFE_LMAP_INSERT_NULL = (\d), DRFE_LMAP_INSERT_BAD = (\d), DRFE_LMAP_INSERT_RECENT = (\d), DRFE_LMAP_INSERT_ADDED = (\d)", text)
    assert tuple(int(v) for v in names.groups()) == (lib.INSERT_NULL, lib.INSERT_BAD, lib.INSERT_RECENT, lib.INSERT_ADDED) == (
        inp.NULL, inp.BAD, inp.RECENT, inp.ADDED)
    assert (inp.ERR_INVALID, inp.ERR_CAPACITY, inp.ERR_STATE) == (lib.ERR_INVALID, lib.ERR_CAPACITY, lib.ERR_STATE)
    lim = lib.LocalMap.insert_limits()
    assert lim["tile"] % 64 == 0 and lim["wavefront"] == 64 and lim["claim_bytes"] == 4
    assert lim["max_keyframes"] == int(re.search(r"DRFE_LMAP_MAX_QUERIES = (\d+)", text).group(1))
    assert lim["device_from"] == int(re.search(r"DRFE_LMAP_INSERT_DEVICE_FROM = (\w+)", text).group(1), 0)
    assert C_sizeof_call() == 8 + 8 + 24 + 8 * len(lib.LMAP_INSERT_CALL_FIELDS)


def C_sizeof_call():
    return lib.C.sizeof(lib.LmapInsertCall)


@pytest.mark.parametrize("scenario", sc.SCENARIOS, ids=lambda f: f.__name__)
def test_scenarios_on_the_host(scenario):
    w, handles, expect = scenario()
    db = store_of(w)
    want = w.insert(handles)
    sc.check_expect({k: (np.array(v) if k in ("normal", "max_distance", "min_distance") else v) for k, v in want.items()},
                    sc.state_of_world(w), expect)                        # the premise, on the restatement
    got = db.insert(handles, mode="host")
    sc.same_result(got, want)
    sc.check_expect(got, sc.state_of_store(db, w), expect)
    sc.same_state(sc.state_of_store(db, w), sc.state_of_world(w))
    assert db.insert_stats() == expected_stats(want, len(handles))
    same_following(db, store_of(w), w)
    # the batch entry runs on the host below the crossover: the same bytes
    v, h2, _ = scenario()
    sc.same_results(store_of(v).insert(h2, mode="batch"), got)


@pytest.mark.parametrize("case", sc.refusals(), ids=lambda c: c[0])
def test_refusals_change_nothing(case):
    _, w, handles, normals, rc = case
    db = store_of(w)
    before = sc.state_of_store(db, w)
    with pytest.raises(inp.Refused) as e:
        w.clone().insert(handles, normals=normals)
    assert e.value.rc == rc
    refused(lambda: db.insert(handles, mode="host", normals=normals), rc)
    refused(lambda: db.insert(handles, mode="batch", normals=normals), rc)
    assert sc.state_of_store(db, w) == before
    assert db.insert_stats()["calls"] == 0
    same_following(db, store_of(w), w)


def test_refusal_names_the_item():
    by = {c[0]: c for c in sc.refusals()}
    for name, word in (("point_without_attributes", "map point 100"), ("line_without_state", "map line 500"),
                       ("keyframe_attributes_do_not_fit", "key frame 20"), ("no_position", "map point 100"),
                       ("observer_without_pose", "observer 10"), ("unknown_keyframe", "77")):
        _, w, handles, normals, rc = by[name]
        assert word in refused(lambda: store_of(w).insert(handles, mode="host", normals=normals), rc), name


def test_without_normals_no_geometry_is_read():
    """normals=False on a store that holds no geometry at all: integer-only, and the same integers as with normals"""
    w, handles, _ = sc.two_and_three_callers()
    db = store_of(w, geometry=False)
    refused(lambda: db.insert(handles, mode="host", normals=True), lib.ERR_STATE)
    got = db.insert(handles, mode="host", normals=False)
    assert "normal" not in got
    want = w.insert(handles, normals=False)
    sc.same_result(got, want, normals=False)
    sc.same_state(sc.state_of_store(db, w), sc.state_of_world(w))


def test_capacities():
    """the total length of the called rows always suffices; an array that is too small refuses the call and changes nothing"""
    w, handles, _ = sc.two_and_three_callers()
    db = store_of(w)
    before = sc.state_of_store(db, w)
    assert "action_capacity[0]" in refused(lambda: db.insert(handles, mode="host", capacity=(23, 24, 24)), lib.ERR_CAPACITY)
    assert "added_capacity[0]" in refused(lambda: db.insert(handles, mode="host", capacity=(24, 4, 24)), lib.ERR_CAPACITY)
    v, h2, _ = sc.lines_mirror()
    dl = store_of(v)
    assert "recent_capacity[1]" in refused(lambda: dl.insert(h2, mode="host", capacity=(16, 16, 2)), lib.ERR_CAPACITY)
    assert "added_capacity[1]" in refused(lambda: dl.insert(h2, mode="host", capacity=(16, 1, 16)), lib.ERR_CAPACITY)
    assert sc.state_of_store(db, w) == before and db.insert_stats()["calls"] == 0
    sc.same_result(db.insert(handles, mode="host", capacity=(24, 5, 0)), w.insert(handles))


def test_a_second_call_meets_the_first():
    """the same key frame again: every entry that was ADDED is RECENT now, and nothing changes"""
    w, handles, _ = sc.insertion_places()
    db = store_of(w)
    sc.same_result(db.insert(handles, mode="host"), w.insert(handles))
    state = sc.state_of_store(db, w)
    got = db.insert(handles, mode="host")
    sc.same_result(got, w.insert(handles))
    assert [int(a) for a in got["point_action"][0]] == [0, 0, 0, 0, 2, 2, 2, 2] and len(got["added_points"]) == 0
    assert sc.state_of_store(db, w) == state


def sync_world(w, lm, culled=()):
    """the restatement's world brought to what an operation without a restatement here left in the store: rows, flags,
    observations, counters, poses and positions, through the getters"""
    st = sc.state_of_store(lm, w)
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
        w.geo[h] = dict(world=g["world"][i].copy(), ref_kf=int(g["ref_kf"][i]), ref_level=int(g["ref_level"][i]))


def same_arrays(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        if isinstance(x, list):
            assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)), k
        else:
            assert x.tobytes() == y.tobytes(), k


OPS = ("fuse", "edit", "recent_cull", "correct", "gba", "cull", "connect")


def run_script(seed, ctx=None, mode="host"):
    """Rounds of: new row entries pushed through the setters, an insert, then one of the other operations of the store - a fuse
    step, setter edits, a recent cull, a Sim3 correction, the map update after a global adjustment, a key-frame cull, a connect
    - so that every later insert meets the flags, nulled rows, nObs, poses and positions the operation left, on the device in
    the resident blocks.  After every step the store is held to the restatement's world; with a context a twin store runs the
    same script on the host entries and every result is compared with its."""
    rng = np.random.default_rng(seed)
    w = sc.random_world(rng)
    db = store_of(w, ctx)
    twin = store_of(w) if ctx is not None else None
    kfs = sorted(w.kfs)
    root = min(w.kfs, key=lambda h: w.kfs[h]["rank"])
    graph_changed = False

    def both(call):
        """the operation on the store and, on the host entry, on the twin"""
        r = call(db, mode)
        return r, (call(twin, "host") if twin is not None else None)

    for r in range(len(OPS) + 1):
        called = [int(k) for k in rng.choice(kfs, int(rng.integers(1, 5)), replace=False)]
        sc.random_puts(rng, w, called, share=0.4)
        normals = r % 2 == 0
        for lm in (db, twin):
            if lm is not None:
                sc.push_rows(lm, w, called)
        got, ref = both(lambda lm, m: lm.insert(called, mode=m, normals=normals))
        if ref is not None:
            sc.same_results(got, ref)
        sc.same_result(got, w.insert(called, normals=normals), normals=normals)
        sc.same_state(sc.state_of_store(db, w), sc.state_of_world(w))
        if twin is not None:
            same_following(db, twin, w, mode_a=mode, connect=False)
        elif not graph_changed:
            same_following(db, store_of(w), w, mode_a=mode, connect=False)
        if r == len(OPS):
            break
        op = OPS[r]
        if op == "fuse":
            # the restatement's World.fuse runs beside the store
            kf = int(rng.choice(kfs))
            cands = [int(c) for c in rng.choice(sorted(w.items[POINT]), 6, replace=False)]
            best = [int(b) for b in rng.integers(-1, len(w.kfs[kf]["rows"][POINT]), 6)]
            steps = [dict(keyframe=kf, kind=POINT, form=0, candidates=cands, best_idx=best)]
            fr, _ = both(lambda lm, m: lm.fuse(steps, mode=m))
            assert [int(a) for a in fr["steps"][0]["action"]] == w.fuse(steps)["steps"][0]["action"]
        elif op == "edit":
            pts = [int(p) for p in rng.choice(sorted(w.items[POINT]), 5, replace=False)]
            flags = [int(v) for v in rng.integers(0, 2, 5)]
            for lm in (db, twin):
                if lm is not None:
                    lm.set_bad(POINT, pts, flags)
                    lm.recent_increase(POINT, pts, [2] * 5, [3] * 5)
            for p, f in zip(pts, flags):
                w.items[POINT][p]["bad"] = f
                w.items[POINT][p]["found"] += 2
                w.items[POINT][p]["visible"] += 3
        elif op == "recent_cull":
            pts = [int(p) for p in rng.choice(sorted(w.items[POINT]), 25, replace=False)]
            lns = [int(l) for l in rng.choice(sorted(w.items[LINE]), 8, replace=False)]
            a, b = both(lambda lm, m: lm.recent_cull(5, pts, lns, mode=m))
            for name in ("points", "lines"):
                if b is not None:
                    same_arrays(a[name], b[name], ("action", "kept", "culled", "erased"))
            assert len(a["points"]["culled"]) + len(a["lines"]["culled"]) > 0
            sync_world(w, db if twin is None else twin)
        elif op == "correct":
            cur = int(rng.choice(kfs))
            hs = sorted(set([cur] + [int(k) for k in rng.choice(kfs, 4, replace=False)]))
            Scw = [0.0, 0.0, 0.0, 1.0, 0.0625, -0.125, 0.03125, 1.0]
            a, b = both(lambda lm, m: lm.correct(cur, Scw, hs, mode=m))
            if b is not None:
                same_arrays(a, b, ("Tiw", "points", "world", "normal", "max_distance", "min_distance", "status"))
            assert len(a["points"]) > 0
            sync_world(w, db if twin is None else twin)
        elif op == "gba":
            pts = sorted(w.items[POINT])
            T = np.stack([w.poses[h] for h in kfs]).copy()
            T[:, 0, 3] += np.float32(0.25)
            X = np.stack([w.geo[p]["world"] for p in pts]) + np.float32(0.125)
            for lm in (db, twin):
                if lm is not None:
                    lm.set_gba_keyframes(kfs, T, [root] * len(kfs))
                    lm.set_gba_points(pts, X, [root] * len(pts))
            a, b = both(lambda lm, m: lm.gba(root, [root], mode=m))
            if b is not None:
                same_arrays(a, b, ("keyframes", "Tcw", "points", "world", "kind"))
            assert len(a["keyframes"]) > 0 and len(a["points"]) > 0
            sync_world(w, db if twin is None else twin)
        elif op == "cull":
            alive = [h for h in kfs if not w.kfs[h]["bad"]]
            a, b = both(lambda lm, m: lm.cull(alive, mode=m))
            if b is not None:
                same_arrays(a, b, ("record", "culled", "points", "point_n_obs", "point_bad"))
            sync_world(w, db if twin is None else twin, culled=a["culled"])
            graph_changed = True
        else:
            alive = [h for h in kfs if not w.kfs[h]["bad"]]
            a, b = both(lambda lm, m: lm.connect(alive, mode=m))
            if b is not None:
                assert np.array_equal(a["record"], b["record"]) and all(np.array_equal(x, y) for x, y in zip(a["counter"], b["counter"]))
            graph_changed = True
        sc.same_state(sc.state_of_store(db, w), sc.state_of_world(w))
    if twin is not None:
        same_following(db, twin, w, mode_a=mode)
        same_culls(db, twin, w, mode_a=mode)
    return db


@pytest.mark.parametrize("seed", (3301, 3302, 3303))
def test_seeded_scripts(seed):
    db = run_script(seed)
    st = db.insert_stats()
    assert st["calls"] == len(OPS) + 1 and st["device_calls"] == 0 and st["points_added"] > 0 and st["lines_added"] > 0
    assert st["recent_points"] > 0


def test_native_caller_on_the_host_entry():
    """tests/native/insert_caller.cpp: the adaptor's LocalMapTracker::ProcessNewKeyFrame, one key frame at a time and as a queue,
    on stand-in types whose AddObservation restates the reference's, next to the reference's loop with UpdateNormalAndDepth on a
    twin; the records bit for bit and the store against the objects after every call"""
    import subprocess
    import native_build
    exe = native_build.caller("insert_caller")
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "insert_caller host: ok, 218 points added" in p.stdout, (p.returncode, p.stdout, p.stderr)
