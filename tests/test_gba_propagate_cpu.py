"""CPU tests of the map update that ends LoopClosing::RunGlobalBundleAdjustment on the map store (drfe_lmap_gba_host, DESIGN.md
section 29): the host entry against tests/gba_propagate_numpy.py, byte for byte and in the order of both lists, and against the
hand-written values of tests/gba_propagate_scenarios.py; the store afterwards through every getter; every refusal leaving the
store unchanged; capacities; seeded scripts interleaved with CorrectLoop calls and edits; non-finite values; the counters; the
native caller on the host entry."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gba_propagate_numpy as gn
import gba_propagate_scenarios as gs
import loop_correct_numpy as rn
from dr_slam_amd import lib

LIM = lib.LocalMap.gba_limits()                # without the feature the module fails here, at the first symbol
RC = {"state": lib.ERR_STATE, "invalid": lib.ERR_INVALID, "capacity": lib.ERR_CAPACITY}


def both(ops, mode="host", ctx=None):
    """a script on the entry and in the restatement: equal results, equal stores through every getter, equal counters"""
    db, ref = lib.LocalMap(ctx), gn.Store()
    r, r_ref = gs.play(ops, db, mode=mode), gs.play(ops, ref)
    assert len(r) == len(r_ref)
    for x, y in zip(r, r_ref):
        (gn.same_gba if "composed" in x else rn.same_correct)(x, y)
    kfs, pts = gs.alive(ops)
    gn.same_store(db, ref, kfs, pts)
    st = db.gba_stats()
    assert all(st[k] == v for k, v in ref.gcounts.items()), (st, ref.gcounts)
    return r, db


def test_limits_and_symbols():
    assert LIM["threads"] % LIM["wavefront"] == 0 and LIM["point_bytes"] >= 18 and LIM["depth_limit"] >= 0
    assert all(hasattr(lib.load(), s) for s in lib.SYMBOLS if "gba" in s)


def test_device_from_is_the_measured_crossover():
    """profiles/gba_propagate_timing.jsonl (tools/gba_propagate_timing.py): its last line is the constant, and the rows give it"""
    rows = [json.loads(x) for x in open(os.path.join(lib._HERE, "..", "profiles", "gba_propagate_timing.jsonl"))]
    measured, rows = rows[-1]["device_from"], rows[:-1]
    assert all(r["equal"] for r in rows) and {r["keyframes"] for r in rows} == {100, 1000, 4000} and len({r["mix"] for r in rows}) == 3
    assert all(r["device_wins"] == (r["host_ms"] - r["device_ms"] > max(r["device_iqr_ms"], r["host_iqr_ms"])) for r in rows)
    wins = {}
    for r in rows:
        wins.setdefault(r["points"], []).append(r["device_wins"])
    want = None
    for n in sorted(wins, reverse=True):
        if not all(wins[n]):
            break
        want = n
    assert measured == want
    assert LIM["device_from"] == (measured if measured is not None else 2 ** 31 - 1)


@pytest.mark.parametrize("name", sorted(gs.HAND))
def test_hand_written_values(name):
    ops, expect = gs.HAND[name]()
    r, _ = both(ops)
    gs.check(r, expect)
    ref = gn.Store()
    gs.check(gs.play(ops, ref), expect)


def test_parent_inverse_is_taken_before_its_set_pose():
    assert gs.the_two_readings_differ()
    ops, expect = gs.chain_of_two()
    r, _ = both(ops)
    assert np.array_equal(r[0]["Tcw"][1], gs.pose(t=(4, 0, 0)))


def test_children_are_walked_in_rank_order():
    for ops, expect in gs.sibling_orders():
        r, _ = both(ops)
        gs.check(r, expect)


@pytest.mark.parametrize("case", gs.refusals(), ids=lambda c: c[0])
def test_refusals_change_nothing(case):
    name, ops, (loop, origins), rc, handle = case
    db = lib.LocalMap()
    gs.play(ops, db)
    kfs, pts = gs.alive(ops)
    before, st = gn.snapshot(db, kfs, pts), db.gba_stats()
    with pytest.raises(lib.DrfeError) as e:
        db.gba(loop, origins, mode="host")
    assert e.value.rc == RC[rc], e.value
    if handle is not None:
        assert re.search(rf"\b{handle}\b", str(e.value)), e.value
        ref = gn.Store()
        gs.play(ops, ref)
        with pytest.raises(gn.Refused) as f:
            ref.gba(loop, origins)
        assert f.value.handle == handle
    gn.same_snapshot(before, gn.snapshot(db, kfs, pts))
    assert db.gba_stats() == st


def test_capacities():
    ops, expect = gs.three_levels()
    for cap, ok in (((4, 3), True), ((3, 3), False), ((4, 2), False)):
        db = lib.LocalMap()
        gs.play(ops[:-1], db)
        kfs, pts = gs.alive(ops)
        before = gn.snapshot(db, kfs, pts)
        if ok:
            gs.check([db.gba(7, [1], mode="host", capacity=cap)], expect)
        else:
            with pytest.raises(lib.DrfeError) as e:
                db.gba(7, [1], mode="host", capacity=cap)
            assert e.value.rc == lib.ERR_CAPACITY
            gn.same_snapshot(before, gn.snapshot(db, kfs, pts))


def test_setters_last_row_wins_unknown_handles_and_remove():
    db = lib.LocalMap()
    db.set_gba_keyframes([7, 7], [gs.pose(t=(1, 0, 0)), gs.pose(t=(2, 0, 0))], [3, 4])       # not stored yet, twice
    db.set_gba_points([9, 9], [(1, 1, 1), (2, 2, 2)], [3, 4])
    g = db.get_gba_keyframes([7])
    assert np.array_equal(g["TcwGBA"][0], gs.pose(t=(2, 0, 0))) and g["stamp"][0] == 4
    assert g["has_TcwGBA"][0] == 1 and g["has_TcwBefGBA"][0] == 0 and not g["TcwBefGBA"].any()
    p = db.get_gba_points([9])
    assert np.array_equal(p["PosGBA"][0], (2, 2, 2)) and p["stamp"][0] == 4 and p["has_PosGBA"][0] == 1
    db.set_keyframes([gs.kf(7)])
    db.set_points([gs.pt(9)])
    db.remove(gs.KEYFRAME, 7)
    db.remove(gs.POINT, 9)
    for get in (db.get_gba_keyframes, db.get_gba_points):
        with pytest.raises(lib.DrfeError) as e:
            get([7 if get == db.get_gba_keyframes else 9])
        assert e.value.rc == lib.ERR_INVALID


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_scripts(seed):
    ops = gs.seeded(seed)
    db, ref = lib.LocalMap(), gn.Store()
    kfs, pts = gs.alive(ops)
    for op in ops:                                                       # the getters after each step
        r, r_ref = gs.play([op], db), gs.play([op], ref)
        for x, y in zip(r, r_ref):
            (gn.same_gba if "composed" in x else rn.same_correct)(x, y)
        if op[0] in ("gba", "correct", "poses"):
            gn.same_store(db, ref, kfs, pts)
    st = db.gba_stats()
    assert st["calls"] == 3 and st["composed"] > 0 and st["kind_ref"] > 0 and st["kind_pos"] > 0
    assert all(st[k] == v for k, v in ref.gcounts.items()), (st, ref.gcounts)


def test_non_finite_values_pass_through():
    ops, _ = gs.three_levels()
    ops = list(ops)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    bad2 = gs.pose(t=(inf, 0, 0))
    ops[3] = ("poses", [1, 2, 3, 4, 5], [gs.pose(t=(1, 0, 0)), bad2, gs.pose(gs.RZ, (0, nan, 0)), gs.pose(t=(0, 0, 1)), gs.pose()])
    ops[4] = ("geo", [gs.geo(10, (1, 1, 1), 1), gs.geo(11, (-inf, 2, nan), 2), gs.geo(12, (1, inf, 0), 3), gs.geo(13, (4, 4, 4), 1),
                      gs.geo(14, (5, 5, 5), 5)])
    ops[6] = ("gba_pts", [10, 13], [(nan, -inf, 9), (8, 8, 8)], [7, 7])
    with np.errstate(all="ignore"):
        r, _ = both(ops)
    assert np.isnan(r[0]["world"]).any() and np.isinf(r[0]["world"]).any()


def test_counters_and_upload_bytes_on_a_host_store():
    ops, _ = gs.three_levels()
    _, db = both(ops)
    st = db.gba_stats()
    assert st == dict(calls=1, device_calls=0, visited=4, composed=1, deepest_chain=1, kind_pos=1, kind_ref=2, skipped_ref=1)
    up = db.upload_bytes()
    assert list(up) == ["rows", "graph", "geometry", "attributes", "gba"] and up["gba"] == 0 and sum(up.values()) == 0
    _, db2 = both(gs.chain_of_two()[0])
    assert db2.gba_stats()["deepest_chain"] == 2


def test_native_caller_on_the_host_entry():
    """tests/native/gba_propagate_caller.cpp: the adaptor's SyncGlobalBA / PropagateGlobalBA next to :722-783 on stand-in objects"""
    import native_build
    exe = native_build.caller("gba_propagate_caller")     # built here if the tests directory holds no build products
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout
