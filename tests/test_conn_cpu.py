"""KeyFrame::UpdateConnections on the host (drfe_lmap_connect_host, dr_slam_amd/csrc/lmap_conn.cpp with conn_core.h) against
tests/conn_numpy.py and against rows worked out by hand (tests/conn_scenarios.py).  Equal bytes everywhere; no GPU.

Parity with a build of the reference's KeyFrame.cc is not pinned: it includes OpenCV, Eigen and DBoW2 headers that are not
installed where this was written."""
import copy
import json
import re

import numpy as np
import pytest

import conn_numpy as cn
import conn_scenarios as cs
import lmap_numpy as ln
import lmap_scenarios as ls
from dr_slam_amd import lib

SEEDS = tuple(range(41, 49))


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        (cn.same_connect if "touched" in x else ln.same)(x, y)


def both(ops):
    ref = cn.Store()
    r_np = cs.play(ops, ref)
    db = lib.LocalMap()
    r_lib = cs.play(ops, db)
    same_results(r_lib, r_np)
    st = db.connect_stats()
    for k, v in ref.ccounts.items():
        assert st[k] == v, k
    assert st["device_calls"] == 0
    cn.same_state(db, ref, sorted(ref.kf))
    return r_lib, ref, db


def test_symbols_and_constants():
    L = lib.load()
    for s in lib.SYMBOLS:
        if "lmap" in s:
            assert hasattr(L, s), s
    text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    lim = lib.LocalMap.connect_limits()
    assert int(re.search(r"DRFE_LMAP_CONNECT_TH = (\d+)", text).group(1)) == lim["threshold"] == lib.LMAP_CONNECT_TH == cn.TH == 15
    assert int(re.search(r"DRFE_LMAP_CONNECT_DEVICE_FROM = (\d+)", text).group(1)) == lim["device_from"]
    assert lim["sort_tile"] % 64 == 0 and lim["row_groups"] > 0
    assert (lib.CONN_WEIGHTS, lib.CONN_ORDERED, lib.CONN_PARENT) == (cs.W, cs.O, cs.P)


def test_device_from_is_the_measured_crossover():
    """profiles/conn_timing.jsonl (tools/conn_timing.py): its last line is the constant, and the rows give it"""
    rows = [json.loads(x) for x in open(lib.os.path.join(lib._HERE, "..", "profiles", "conn_timing.jsonl"))]
    measured = rows[-1]["device_from"]
    assert lib.LocalMap.connect_limits()["device_from"] == (measured if measured is not None else 2 ** 31 - 1)
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
    """tests/native/conn_caller.cpp: the adaptor's UpdateConnections on stand-in types next to a restatement of the three functions"""
    import subprocess
    import native_build
    exe = native_build.caller("conn_caller")
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "conn_caller ok (host, 40 single calls, 1 call of 30, device calls 0)" in p.stdout, (p.returncode, p.stdout, p.stderr)


@pytest.mark.parametrize("name", sorted(cs.HAND))
def test_hand_built(name):
    ops, expect, premise = cs.HAND[name]()
    for h, votes in premise.items():
        assert cs.votes_of(ops, h) == votes                    # the premise: the tie is a tie, the counter is empty, ...
    r, _, db = both(ops)
    cs.check(r, expect, db)


def test_premises_of_the_hand_built_graphs():
    ops, _, v = cs.fallback_and_ties()
    ranks = {r["handle"]: r["rank"] for r in ops[0][1]}
    assert v[1][2] == v[1][3] < cn.TH and ranks[3] < ranks[2]                       # a vote tie below the threshold
    assert v[5][6] == v[5][7] == cn.TH and ranks[6] < ranks[7]                      # and one at it
    assert sorted(cs.threshold()[2][1].values()) == [cn.TH - 1, cn.TH, cn.TH + 1]
    ops, _, v = cs.bad_keyframe()
    assert {r["handle"]: r["bad"] for r in ops[0][1]}[2] == 1 and v[1][2] >= cn.TH
    ops, _, v = cs.same_weight_keeps_the_filtered_list()
    stored = {r["handle"]: r for r in ops[2][1]}
    assert dict(stored[5]["weights"])[1] == v[1][5] and dict(stored[6]["weights"])[1] != v[1][6]
    assert min(w for _, w in stored[5]["weights"]) < cn.TH and len(stored[5]["ordered"]) < len(stored[5]["weights"])
    a, b = cs.asymmetric((1, 2)), cs.asymmetric((2, 1))
    assert a[2] == b[2] and a[1][0]["weights"] != b[1][0]["weights"]
    ops, _, v = cs.stale_reverse_entries()
    assert 0 < v[1][2] < cn.TH and dict({r["handle"]: r for r in ops[2][1]}[2]["weights"])[1] == 30


@pytest.fixture(scope="module")
def random_runs():
    runs = []
    for seed in SEEDS:
        ops = cs.random_script(seed)
        ref = cn.Store()
        runs.append((ops, cs.play(ops, ref), ref))
    return runs


def test_random_scripts_take_every_branch(random_runs):
    kinds = {op[0] for ops, _, _ in random_runs for op in ops}
    assert kinds == {"kfs", "points", "conn", "connect", "update", "bad", "remove"}
    conns = [r for _, rs, _ in random_runs for r in rs if "touched" in r]
    rec = np.concatenate([r["record"] for r in conns])
    assert (rec[:, 1] > 1).any() and ((rec[:, 1] == 1) & (rec[:, 2] < cn.TH) & (rec[:, 0] > 0)).any()     # listed, and the fallback
    assert (rec[:, 0] > rec[:, 1]).any()                                                                   # sub-threshold entries
    flags = np.concatenate([r["flags"] for r in conns])
    assert set(flags.tolist()) >= {0, cs.W | cs.O, cs.W | cs.O | cs.P} and sum((r["new_parent"] >= 0).sum() for r in conns) > 0
    grown = sum(1 for r in conns for w, o in zip(r["weights"], r["ordered"]) if len(o) == len(w) and len(w) and w[:, 1].min() < cn.TH)
    kept = sum(1 for r in conns for w, o in zip(r["weights"], r["ordered"]) if len(o) < len(w))
    assert grown > 0 and kept > 0
    ups = [r for _, rs, _ in random_runs for r in rs if "touched" not in r]
    assert sum(int((r["record"][:, 2] > 0).sum()) for r in ups) > 0        # UpdateLocalMap expanded through the committed graph


@pytest.mark.parametrize("i", range(len(SEEDS)))
def test_random_scripts_match_the_restatement(random_runs, i):
    ops, r_np, ref = random_runs[i]
    db = lib.LocalMap()
    same_results(cs.play(ops, db), r_np)
    st = db.connect_stats()
    assert all(st[k] == v for k, v in ref.ccounts.items())
    assert all(db.stats()[k] == v for k, v in ref.counts.items())
    cn.same_state(db, ref, sorted(ref.kf))


def _refused(fn, rc=lib.ERR_INVALID):
    with pytest.raises(lib.DrfeError) as e:
        fn()
    assert e.value.rc == rc
    return str(e.value)


def _base():
    ops, expect, _ = cs.earlier_and_later_targets()
    db = lib.LocalMap()
    cs.play(ops[:-1], db)
    return db, ops[-1][1], expect


def _answers_as_untouched(db, call, expect):
    assert db.connect_stats()["calls"] == 0
    cs.check([db.connect(call, mode="host")], expect, db)


def test_duplicate_and_unknown_handles_are_refused():
    db, call, expect = _base()
    _refused(lambda: db.connect([1, 2, 1], mode="host"))
    _refused(lambda: db.connect([1, 99], mode="host"))
    _refused(lambda: db.connect([-1], mode="host"))
    _refused(lambda: db.get_connections([99]))
    _answers_as_untouched(db, call, expect)


def test_connection_rows_are_checked():
    db, call, expect = _base()
    _refused(lambda: db.set_connections([cs.conn(1, weights=[(2, 0)])]))
    _refused(lambda: db.set_connections([cs.conn(1, ordered=[(2, -3)])]))
    _refused(lambda: db.set_connections([cs.conn(3), cs.conn(1, weights=[(2, 4), (2, 5)])]))
    _refused(lambda: db.set_connections([cs.conn(1, ordered=[(2, 4), (3, 4), (2, 4)])]))
    _refused(lambda: db.set_connections([cs.conn(-1)]))
    _refused(lambda: db.set_connections([cs.conn(1, weights=[(-1, 4)])]))
    _answers_as_untouched(db, call, expect)


def test_an_entry_that_names_a_removed_key_frame_fails_the_query():
    db, call, expect = _base()
    db.set_keyframes([ls.kf(9, 90)])
    db.set_connections([cs.conn(1, weights=[(9, 7)]), cs.conn(3, ordered=[(9, 7)])])
    db.remove(ls.KEYFRAME, 9)
    msg = _refused(lambda: db.connect(call, mode="host"), lib.ERR_STATE)
    assert "connection weight" in msg and "key frame 1" in msg and "9" in msg
    _refused(lambda: db.update([dict(frame_id=1, points=[])], mode="host"), lib.ERR_STATE)
    db.set_connections([cs.conn(1)])
    msg = _refused(lambda: db.connect(call, mode="host"), lib.ERR_STATE)
    assert "ordered connection" in msg and "key frame 3" in msg
    db.set_connections([cs.conn(3)])
    _answers_as_untouched(db, call, expect)


@pytest.mark.parametrize("which", range(4))
def test_too_small_output_array_changes_nothing(which):
    db, call, expect = _base()
    e = expect[0]
    need = [sum(len(c) for c in e["counter"]), len(e["touched"]), sum(len(w) for w in e["weights"]), sum(len(o) for o in e["ordered"])]
    before = db.get_connections([1, 2, 3])
    cap = list(need)
    cap[which] -= 1
    _refused(lambda: db.connect(call, mode="host", capacity=cap), lib.ERR_CAPACITY)
    after = db.get_connections([1, 2, 3])
    assert all(np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes() for k in ("parent", "first"))
    assert all(len(x) == 0 for k in ("weights", "children") for x in after[k])
    assert db.connect_stats()["calls"] == 0
    cs.check([db.connect(call, mode="host", capacity=need)], expect, db)       # the exact sizes suffice


def test_device_entry_without_a_context_is_a_state_error():
    db, call, expect = _base()
    _refused(lambda: db.connect(call, mode="device"), lib.ERR_STATE)
    assert db.connect_stats()["calls"] == 0
    cs.check([db.connect(call, mode="batch")], expect, db)                     # _batch of a host-only store runs on the host
    assert db.connect_stats()["device_calls"] == 0


def test_set_keyframes_keeps_and_remove_drops_the_connection_state():
    db, call, _ = _base()
    db.connect(call, mode="host")
    was = db.get_connections([2])
    db.set_keyframes([ls.kf(2, 20, parent=3, ch=[], pts=[])])
    now = db.get_connections([2])
    assert cs.pairs(now["weights"][0]) == cs.pairs(was["weights"][0]) == [(1, 20), (3, 17)] and cs.pairs(now["ordered"][0]) == [(1, 20), (3, 17)]
    db.remove(ls.KEYFRAME, 2)
    db.set_keyframes([ls.kf(2, 20)])
    g = db.get_connections([2])
    assert len(g["weights"][0]) == 0 and len(g["ordered"][0]) == 0 and g["first"][0] == 0


def test_connect_commits_what_update_local_map_reads():
    """after the call the neighbours are the first 10 of the list, the parent and the child are set: a frame that sees only key
    frame 2's points gets 2's new parent 3 and its best covisible through the expansion"""
    db, call, _ = _base()
    ref = cn.Store()
    ops = cs.earlier_and_later_targets()[0]
    cs.play(ops, ref)
    db.connect(call, mode="host")
    q = [dict(frame_id=1, points=[p for p in ops[0][1][1]["points"]][:3])]
    r = db.update(q, mode="host")
    ln.same(r, ref.update(q))
    assert r["record"][0].tolist()[2] > 0


def test_an_empty_call():
    db, call, expect = _base()
    r = db.connect([], mode="host")
    assert len(r["touched"]) == 0 and r["record"].shape == (0, 4) and db.connect_stats()["calls"] == 0
    _answers_as_untouched(db, call, expect)
    assert copy.deepcopy(db.connect_stats())["keyframes"] == 3
