"""CPU tests of what surrounds the solver of Optimizer::OptimizeEssentialGraph on the map store (drfe_lmap_essential_edges_host,
drfe_lmap_essential_commit_host, the loop edges as store state): the host entries against
tests/essential_numpy.py, byte for byte and in the order of every list, and against the hand-written values of
tests/essential_scenarios.py; the store afterwards through every getter; every refusal leaving the store unchanged; seeded
scripts; the counters; a loop closure chained through correct, connect, the edges, a stand-in for the solver, the commit and gba;
the dispatch constants against the recorded measurement; the native caller and the sanitizer build on the host entries."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import essential_numpy as en
import essential_scenarios as es
import lmap_numpy as ln
from dr_slam_amd import lib

LIM = lib.LocalMap.essential_limits()          # without the feature the module fails here, at the first symbol
RC = {"STATE": lib.ERR_STATE, "INVALID": lib.ERR_INVALID, "CAPACITY": lib.ERR_CAPACITY}
NATIVE = os.path.join(lib._HERE, "..", "tests", "native")


def counters(db, ref):
    st = db.essential_stats()
    assert all(st[k] == v for k, v in ref.ecounts.items()), (st, ref.ecounts)
    return st


def both(ops, mode="host", ctx=None):
    """a script on the entry and in the restatement: equal results, equal stores through every getter, equal counters"""
    db, ref = lib.LocalMap(ctx), en.Store()
    r, r_ref = es.play(ops, db, mode=mode), es.play(ops, ref)
    assert len(r) == len(r_ref)
    for x, y in zip(r, r_ref):
        en.same_result(x, y)
    kfs, pts = es.alive(ops)
    en.same_store(db, ref, kfs, pts)
    counters(db, ref)
    return r, db


def test_limits_symbols_and_argtypes():
    assert LIM["threads"] % LIM["wavefront"] == 0 and LIM["wavefront"] == 64
    assert LIM["point_bytes"] >= 41 and LIM["kf_bytes"] >= 128 and LIM["edge_bytes"] >= 78 and LIM["vertex_bytes"] >= 256
    L = lib.load()
    mine = [s for s in lib.SYMBOLS if "essential" in s or "loop_edges" in s]
    assert len(mine) == 12 and all(hasattr(L, s) for s in mine)
    for s in mine:
        assert not any(w in s for w in ("gba", "correct", "cull", "insert", "connect")) and not s.startswith("drfe_lmap_create_")
    nargs = {"drfe_lmap_set_loop_edges": 5, "drfe_lmap_get_loop_edges": 6, "drfe_lmap_essential_upload_bytes": 2,
             "drfe_lmap_essential_edges_host": 2, "drfe_lmap_essential_edges_device": 3, "drfe_lmap_essential_edges_batch": 3,
             "drfe_lmap_essential_commit_host": 2, "drfe_lmap_essential_commit_device": 3, "drfe_lmap_essential_commit_batch": 3,
             "drfe_lmap_essential_limits": 1, "drfe_lmap_essential_scratch": 3, "drfe_lmap_essential_stats": 2}
    assert sorted(nargs) == sorted(mine)
    for s, n in nargs.items():
        assert len(getattr(L, s).argtypes) == n
    assert lib.ESSENTIAL_MIN_FEAT == es_min_feat_of_the_header() == en.MIN_FEAT == 100


def es_min_feat_of_the_header():
    txt = open(os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    return int(re.search(r"DRFE_LMAP_ESSENTIAL_MIN_FEAT\s*=\s*(\d+)", txt).group(1))


def test_the_call_structures_are_the_header_s():
    """field order of the two ctypes structures against the typedefs"""
    txt = open(os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    for name, cls in (("drfe_lmap_essential_edges_call", lib.LmapEssentialEdgesCall), ("drfe_lmap_essential_commit_call", lib.LmapEssentialCommitCall)):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert fields == [f[0] for f in cls._fields_], (fields, [f[0] for f in cls._fields_])


@pytest.mark.parametrize("name", sorted(es.HAND_EDGES))
def test_hand_built_edges(name):
    ops, expect, counts = es.HAND_EDGES[name]()
    r, db = both(ops)
    es.check(r, expect)
    st = db.essential_stats()
    assert all(st[k] == v for k, v in counts.items()) and st["edges_calls"] == 1 and st["device_calls"] == 0


def test_hand_built_commit():
    ops, expect, counts, state = es.commit_points()
    r, db = both(ops)
    es.check(r, expect)
    es.check_state(db, state)
    st = db.essential_stats()
    assert all(st[k] == v for k, v in counts.items()) and st["commit_calls"] == 1


def test_an_edges_call_does_not_change_the_store():
    ops, _, _ = es.covisibility_drop_reasons()
    db = lib.LocalMap()
    es.play(ops[:-1], db)
    kfs, pts = es.alive(ops)
    before = en.snapshot(db, kfs, pts)
    es.play(ops[-1:], db)
    en.gn.same_snapshot(before, en.snapshot(db, kfs, pts))


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_seeded_scripts(seed):
    r, db = both(es.seeded(seed))
    assert len(r) == 3 and db.essential_stats()["edges_calls"] == 2


@pytest.mark.parametrize("prefix", [0, 1, 5])
def test_seeded_prefix_shapes(prefix):
    r, _ = both(es.script(12, 10, 50 + prefix, prefix=prefix, n_bad=1))
    kinds = r[0]["kind"]
    assert list(kinds) == sorted(kinds[kinds == 0].tolist()) + kinds[kinds != 0].tolist()      # the loop connections lead


@pytest.mark.parametrize("case", es.refusals(), ids=lambda c: c[0])
def test_refusals_leave_the_store_untouched(case):
    name, ops, op, rc, handle = case
    db, ref = lib.LocalMap(), en.Store()
    es.play(ops, db)
    es.play(ops, ref)
    kfs, pts = es.alive(ops)
    before, st = en.snapshot(db, kfs, pts), db.essential_stats()
    with pytest.raises(lib.DrfeError) as e:
        es.call(db, op)
    with pytest.raises(en.Refused) as f:
        es.call(ref, op)
    assert e.value.rc == RC[rc] == RC[f.value.rc], (str(e.value), str(f.value))
    if handle is not None:
        assert re.search(rf"\b{handle}\b", str(e.value).split(":", 1)[1]), str(e.value)
    if "edge" in name and rc == "STATE" and "unknown" not in name:
        assert "->" in str(e.value), "the message names the edge"
    en.gn.same_snapshot(before, en.snapshot(db, kfs, pts))
    assert db.essential_stats() == st
    en.same_store(db, ref, kfs, pts)


def test_loop_edges_as_store_state():
    db, ref = lib.LocalMap(), en.Store()
    rows = [es.kf(1, rank=30), es.kf(2, rank=20), es.kf(3, rank=10), es.kf(4, rank=40)]
    for s in (db, ref):
        s.set_keyframes(rows)
        assert [list(r) for r in s.get_loop_edges([1, 2, 3, 4])] == [[], [], [], []]         # never given: empty rows
        s.set_loop_edges([(1, [2, 3, 4]), (2, [1]), (1, [4, 3, 9])])                          # the last row of a handle wins
        assert [list(r) for r in s.get_loop_edges([1, 2])] == [[3, 4, 9], [1]]                # ascending rank, the unknown 9 last
        s.set_loop_edges([(2, [])])                                                           # a row replaces the stored one
        assert [list(r) for r in s.get_loop_edges([2])] == [[]]
        s.remove(ln.KEYFRAME, 1)                                                              # and goes with its key frame
        s.set_keyframes([es.kf(1, rank=30)])
        assert [list(r) for r in s.get_loop_edges([1])] == [[]]
    for bad in ([(1, [2, 2])], [(1, [-1])], [(-1, [2])]):
        with pytest.raises(lib.DrfeError) as e:
            db.set_loop_edges([(3, [4])] + bad)
        assert e.value.rc == lib.ERR_INVALID
    assert [list(r) for r in db.get_loop_edges([3])] == [[]]                                  # a refused edit changes nothing
    with pytest.raises(lib.DrfeError) as e:
        db.get_loop_edges([7])
    assert e.value.rc == lib.ERR_INVALID


def test_a_store_without_loop_edges_behaves_as_before():
    """the state is optional: the scripts of the sibling operations give the same results with and without an unrelated row"""
    import gba_propagate_scenarios as gs
    ops, expect = gs.three_levels()
    a, b = lib.LocalMap(), lib.LocalMap()
    b.set_loop_edges([(1, [2]), (77, [78])])
    ra, rb = gs.play(ops, a), gs.play(ops, b)
    gs.check(ra, expect)
    gs.check(rb, expect)
    assert a.gba_stats() == b.gba_stats()


def derive_loop_connections(store, connected, mode="host"):
    """LoopClosing.cc:594-610 on either store: per connected key frame its neighbours before, UpdateConnections, then the connected
    key frames after it less the earlier neighbours and less the connected set"""
    out, results = [], []
    for h in connected:
        previous = [int(k) for k, _ in store.get_connections([h])["ordered"][0]]
        results.append(store.connect([h], mode=mode))
        now = [int(k) for k, _ in store.get_connections([h])["weights"][0]]
        out.append((h, [k for k in now if k not in previous and k not in connected]))
    return out, results


def perturb(Scw):
    """a fixed stand-in for the solver: every estimate nudged by the same small Sim3 from the left, in plain numpy"""
    out = np.array(Scw, np.float64)
    out[:, 4:7] = out[:, 4:7] * 1.03125 + np.array([0.125, -0.0625, 0.03125])
    out[:, 7] = out[:, 7] * 1.03125
    return out


def chain(store, mode="host"):
    """correct, connect with the derived loop connections, the edges, the stand-in solver, the commit, gba"""
    g = es.cs.Graph()
    for h in (1, 2, 3, 4, 5, 6):
        g.kf(h, 10 * h, parent=h - 1 if h > 1 else -1, ch=[h + 1] if h < 6 else [])
    g.see(6, [1, 2], 120, own=True).see(5, [1], 105, own=True).see(6, [5, 4], 110, own=True).see(4, [3], 30, own=True)
    rng = np.random.default_rng(7)
    ops = g.ops() + [("scales", es.SCALES), ("poses", [1, 2, 3, 4, 5, 6], [es.rand_pose(rng) for _ in range(6)])]
    pts = [r["handle"] for r in ops[1][1]]
    ops.append(("geo", [es.geo(p, rng.uniform(-3, 3, 3).astype(np.float32), int(rng.integers(1, 7)), level=int(rng.integers(0, 3))) for p in pts]))
    ops.append(("conn", [es.conn(4, weights=[(3, 30)], ordered=[(3, 30)])]))
    es.play(ops, store, mode=mode)
    cur, loop, connected = 6, 1, [6, 5, 4]
    out = [store.correct(cur, es.rand_sim3(np.random.default_rng(8)), connected, mode=mode)]
    table = [(h, out[0]["corrected"][i], out[0]["non_corrected"][i]) for i, h in enumerate(connected)]
    lcs, conns = derive_loop_connections(store, connected, mode)
    out += conns
    edges = store.essential_edges(loop, cur, table, lcs, mode=mode)
    out.append(edges)
    out.append(store.essential_commit(cur, edges["vertices"], edges["Scw"], perturb(edges["Scw"]), mode=mode))
    store.set_loop_edges([(loop, [cur]), (cur, [loop])])                                      # :618-619
    store.set_gba_keyframes([1], store.get_poses([1])["Tcw"], [cur])
    out.append(store.gba(cur, [1], mode=mode))
    out.append(store.essential_edges(loop, cur, [], [], mode=mode))                           # the new loop edge gives its edge
    return out, lcs, [1, 2, 3, 4, 5, 6], pts


def test_a_loop_closure_chained_through_the_store():
    db, ref = lib.LocalMap(), en.Store()
    r, lcs, kfs, pts = chain(db)
    r_ref, lcs_ref, _, _ = chain(ref)
    assert lcs == lcs_ref and any(ms for _, ms in lcs), lcs
    assert len(r) == len(r_ref)
    for x, y in zip(r, r_ref):
        en.same_result(x, y)
    en.same_store(db, ref, kfs, pts)
    counters(db, ref)
    assert (r[-1]["kind"] == es.LOOP).sum() == 1 and (r[4]["kind"] == es.LC).sum() >= 1


def test_device_from_constants_are_the_measured_crossovers():
    """profiles/essential_timing.jsonl (tools/essential_timing.py): its last line holds the two constants, and the rows give them"""
    rows = [json.loads(x) for x in open(os.path.join(lib._HERE, "..", "profiles", "essential_timing.jsonl"))]
    last, rows = rows[-1], rows[:-1]
    assert all(r["equal"] for r in rows)
    for call, size, key in (("edges", "keyframes", "edges_device_from"), ("commit", "points", "commit_device_from")):
        mine = [r for r in rows if r["call"] == call]
        assert {r["keyframes"] for r in mine} == {100, 1000, 4000}
        if call == "commit":
            assert {r["points"] for r in mine} == {12500, 125000, 500000}
        assert all(r["device_wins"] == (r["host_ms"] - r["device_ms"] > max(r["device_iqr_ms"], r["host_iqr_ms"])) for r in mine)
        wins = {}
        for r in mine:
            wins.setdefault(r[size], []).append(r["device_wins"])
        want = None
        for n in sorted(wins, reverse=True):
            if not all(wins[n]):
                break
            want = n
        assert last[key] == want
        assert LIM[key] == (want if want is not None else 2 ** 31 - 1)


def test_device_entries_need_a_context():
    db = lib.LocalMap()
    es.play(es.covisibility_prefixes()[0][:-1], db)
    with pytest.raises(lib.DrfeError) as e:
        db.essential_edges(1, 6, mode="device")
    assert e.value.rc == lib.ERR_STATE
    with pytest.raises(lib.DrfeError) as e:
        db.essential_commit(6, [1], [es.sim3()], [es.sim3()], mode="device")
    assert e.value.rc == lib.ERR_STATE
    assert db.essential_stats()["edges_calls"] == 0


def test_native_caller_on_the_host_entries():
    """tests/native/essential_caller.cpp through the adaptor header, host mode"""
    exe = os.path.join(NATIVE, "essential_caller")
    assert os.path.exists(exe), "build() makes it"
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout


def test_sanitizer_build_of_the_host_sources():
    """tests/native/essential_asan.mk: the store's host sources under ASan and UBSan in a stand-alone program, host mode"""
    subprocess.run(["make", "-C", NATIVE, "-f", "essential_asan.mk"], check=True, capture_output=True, timeout=900)
    p = subprocess.run([os.path.join(NATIVE, "essential_asan"), "host"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
