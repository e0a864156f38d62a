"""Tracking::UpdateLocalMap on the host (drfe_lmap_update_host, dr_slam_amd/csrc/lmap.cpp) against tests/lmap_numpy.py and against
lists worked out by hand (tests/lmap_scenarios.py).  Equal bytes everywhere; no GPU.

Parity with a build of the reference's Tracking.cc is not pinned: it includes OpenCV, Eigen, PCL and Pangolin headers that are
not installed where this was written, so the reference's own three functions could not be compiled."""
import re

import numpy as np
import pytest

import lmap_numpy as ln
import lmap_scenarios as ls
from dr_slam_amd import lib

SEEDS = tuple(range(31, 39))        # 8 scripts x 32 calls x 8 frames: 2048 queries


def both(ops):
    ref = ln.Store()
    r_np = ls.play(ops, ref)
    db = lib.LocalMap()
    r_lib = ls.play(ops, db)
    assert len(r_np) == len(r_lib)
    for a, b in zip(r_lib, r_np):
        ln.same(a, b)
    st = db.stats()
    for k, v in ref.counts.items():
        assert st[k] == v, k
    assert st["device_calls"] == 0 and st["uploads"] == 0
    return r_lib, ref, db


def test_symbols_and_constants():
    L = lib.load()
    for s in lib.SYMBOLS:
        if "lmap" in s:
            assert hasattr(L, s), s
    text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    lim = lib.LocalMap.limits()
    assert int(re.search(r"DRFE_LMAP_DEVICE_FROM = (\d+)", text).group(1)) == lim["device_from"]
    assert int(re.search(r"DRFE_LMAP_NEIGHBOURS = (\d+)", text).group(1)) == lib.LMAP_NEIGHBOURS
    assert re.search(r"DRFE_LMAP_KEYFRAME = 0, DRFE_LMAP_POINT = 1, DRFE_LMAP_LINE = 2", text)
    assert (lib.LMAP_KEYFRAME, lib.LMAP_POINT, lib.LMAP_LINE) == (ls.KEYFRAME, ls.POINT, ls.LINE) == (ln.KEYFRAME, ln.POINT, ln.LINE)
    assert lim["vote_threads"] % 64 == 0 and lim["gather_entries"] > 0 and lim["lds_keyframes"] > 0


def test_device_from_is_the_measured_crossover():
    """profiles/lmap_timing.jsonl (tools/lmap_timing.py): its last line is the constant, and the rows give it"""
    import json
    rows = [json.loads(x) for x in open(lib.os.path.join(lib._HERE, "..", "profiles", "lmap_timing.jsonl"))]
    measured = rows[-1]["device_from"]
    assert lib.LocalMap.limits()["device_from"] == (measured if measured is not None else 2 ** 31 - 1)
    shapes = rows[:-1]
    assert {r["keyframes"] for r in shapes} == {100, 1000, 4000} and {r["queries"] for r in shapes} == {1, 4, 16, 64, 256}
    assert all(r["equal"] and r["device_reps"] >= 5 and r["host_reps"] >= 5 for r in shapes)
    if measured is not None:
        assert all(r["device_wins"] for r in shapes if r["queries"] >= measured)
        below = [r for r in shapes if r["queries"] < measured]
        assert not below or not all(r["device_wins"] for r in below if r["queries"] == max(b["queries"] for b in below))


def test_native_caller_on_the_host_entries():
    """tests/native/lmap_caller.cpp: the adaptor's LocalMapTracker on stand-in types next to a literal copy of the three loops"""
    import subprocess
    import native_build
    exe = native_build.caller("lmap_caller")
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "lmap_caller ok (host, 50 frames, device calls 0)" in p.stdout, (p.returncode, p.stdout, p.stderr)


@pytest.mark.parametrize("name", sorted(ls.HAND))
def test_hand_built(name):
    ops, expect, votes = ls.HAND[name]()
    assert ls.votes_of(ops) == votes                       # the premise: the tie is a tie, the counter is empty, ...
    r, _, _ = both(ops)
    ls.check(r, expect)


def test_premises_of_the_hand_built_graphs():
    v = ls.vote_tie()[2]
    assert v[1] == v[2] > v[3]
    ops = ls.vote_tie()[0]
    ranks = {r["handle"]: r["rank"] for r in ops[0][1]}
    order = sorted(ranks, key=ranks.get)
    assert order != sorted(ranks) and order != [r["handle"] for r in ops[0][1]]      # neither handle nor insertion order
    v = ls.best_bad()[2]
    assert max(v, key=v.get) == 1 and ls.best_bad()[0][0][1][0]["bad"] == 1
    assert all(r["bad"] for r in ls.all_bad()[0][0][1] if r["handle"] in ls.all_bad()[2])
    assert ls.empty_counter()[2] == {} and len(ls.empty_counter()[0][-1][1][0]["points"]) == 3
    assert len(ls.limit_80(80)[2]) == 80 and len(ls.limit_80(81)[2]) == 81 and len(ls.limit_80(78)[2]) == 78
    kfs = {r["handle"]: r for r in ls.children_by_rank()[0][0][1]}
    assert sorted(kfs[1]["children"], key=lambda h: kfs[h]["rank"]) == [6, 7, 5] != kfs[1]["children"]
    assert {r["handle"]: r["bad"] for r in ls.bad_parent()[0][0][1]}[9] == 1


@pytest.fixture(scope="module")
def random_runs():
    runs = []
    for seed in SEEDS:
        ops = ls.random_script(seed, calls=32)
        ref = ln.Store()
        runs.append((ops, ls.play(ops, ref), ref.counts))
    return runs


def test_random_scripts_take_every_branch(random_runs):
    n_queries = sum(c["queries"] for _, _, c in random_runs)
    assert n_queries >= 2000
    rec = np.concatenate([r["record"] for _, rs, _ in random_runs for r in rs])
    refs = np.concatenate([r["ref_kf"] for _, rs, _ in random_runs for r in rs])
    assert (rec[:, 0] == 0).any() and (rec[:, 2] > 0).any() and (rec[:, 0] > rec[:, 1]).any() and (refs == -1).any()
    kinds = {op[0] for ops, _, _ in random_runs for op in ops}
    assert kinds == {"kfs", "points", "lines", "bad", "remove", "update"}
    assert sum(c["nulled"] for _, _, c in random_runs) > 0
    ins = np.concatenate([x for _, rs, _ in random_runs for r in rs for x in r["mp_in_frame"] + r["ml_in_frame"]])
    assert ins.any() and not ins.all()


@pytest.mark.parametrize("i", range(len(SEEDS)))
def test_random_scripts_match_the_restatement(random_runs, i):
    ops, r_np, counts = random_runs[i]
    db = lib.LocalMap()
    r_lib = ls.play(ops, db)
    for a, b in zip(r_lib, r_np):
        ln.same(a, b)
    st = db.stats()
    assert all(st[k] == v for k, v in counts.items())


def test_random_script_past_80_key_frames():
    ops = ls.random_script(7, n_kf=150, n_mp=600, obs=4, calls=3, per_call=6, frame_points=200)
    r, _, _ = both(ops)
    listed = np.concatenate([x["record"][:, 1] for x in r])
    assert listed.max() > 80 and listed.min() < 80


def _small():
    db = lib.LocalMap()
    db.set_keyframes([ls.kf(1, 10, pts=[100, 101], lns=[300]), ls.kf(2, 20, nb=[1], pts=[101])])
    db.set_points([ls.mp(100, [1]), ls.mp(101, [1, 2], bad=1)])
    db.set_lines([300])
    return db


Q = dict(points=[100, 101], lines=[300])
WANT = dict(kfs=[[1]], ref_kf=[1], record=[[1, 1, 0, 1]], mps=[[100]], mp_in_frame=[[1]], mls=[[300]], ml_in_frame=[[1]], nulled=[[1]])


def _refused(fn, rc=lib.ERR_INVALID):
    with pytest.raises(lib.DrfeError) as e:
        fn()
    assert e.value.rc == rc
    return str(e.value)


def _unchanged(db, frame_id, stats):
    """the store answers as a fresh one does, and the refused calls counted nothing"""
    assert db.stats() == stats
    ls.check([db.update([dict(Q, frame_id=frame_id)], mode="host")], [WANT])


def test_frame_ids_must_increase_and_never_be_zero():
    db = _small()
    _refused(lambda: db.update([dict(Q, frame_id=0)], mode="host"))
    db.update([dict(Q, frame_id=5)], mode="host")
    st = db.stats()
    _refused(lambda: db.update([dict(Q, frame_id=5)], mode="host"))
    _refused(lambda: db.update([dict(Q, frame_id=4)], mode="host"))
    _refused(lambda: db.update([dict(Q, frame_id=6), dict(Q, frame_id=6)], mode="host"))
    _refused(lambda: db.update([dict(Q, frame_id=7), dict(Q, frame_id=0)], mode="host"))
    _unchanged(db, 6, st)                                         # the refused calls used no id


def test_duplicate_observation_is_refused():
    db = _small()
    st = db.stats()
    _refused(lambda: db.set_points([ls.mp(100, [2]), ls.mp(102, [1, 2, 1])]))
    assert db.size() == (2, 2, 1)                                 # neither row of the refused call was stored
    _unchanged(db, 1, st)


def test_duplicate_rank_is_refused():
    db = _small()
    st = db.stats()
    _refused(lambda: db.set_keyframes([ls.kf(3, 10)]))            # key frame 1 has rank 10
    _refused(lambda: db.set_keyframes([ls.kf(3, 30), ls.kf(4, 30)]))
    assert db.size() == (2, 2, 1)
    db.set_keyframes([ls.kf(1, 20, pts=[100, 101], lns=[300]), ls.kf(2, 10, nb=[1], pts=[101])])   # a swap within one call
    db.set_keyframes([ls.kf(3, 10), ls.kf(3, 30)])                # the last row of a handle wins
    db.remove(ls.KEYFRAME, 3)
    _unchanged(db, 1, st)


def test_dangling_handles_fail_the_query_and_name_the_reference():
    for rows, what, handle in (([ls.kf(3, 30, parent=9)], "parent", 9), ([ls.kf(3, 30, nb=[8])], "neighbour", 8),
                               ([ls.kf(3, 30, ch=[7])], "child", 7), ([ls.kf(3, 30, pts=[555])], "map-point match", 555),
                               ([ls.kf(3, 30, lns=[444])], "map-line match", 444)):
        db = _small()
        st = db.stats()
        db.set_keyframes(rows)                                    # a set_* may name handles that are not stored yet
        msg = _refused(lambda: db.update([dict(Q, frame_id=1)], mode="host"), lib.ERR_STATE)
        assert what in msg and str(handle) in msg and "key frame 3" in msg
        db.remove(ls.KEYFRAME, 3)
        _unchanged(db, 1, st)
    db = _small()
    st = db.stats()
    db.set_points([ls.mp(102, [6])])
    msg = _refused(lambda: db.update([dict(Q, frame_id=1)], mode="host"), lib.ERR_STATE)
    assert "observation" in msg and "map point 102" in msg and "6" in msg
    db.set_keyframes([ls.kf(6, 60)])                              # storing the named key frame mends it
    _unchanged(db, 1, st)
    db.remove(ls.KEYFRAME, 1)                                     # now point 100's observation dangles
    _refused(lambda: db.update([dict(Q, frame_id=2)], mode="host"), lib.ERR_STATE)


def test_unknown_handles_in_a_query_and_in_the_edits_are_refused():
    db = _small()
    st = db.stats()
    _refused(lambda: db.update([dict(Q, frame_id=1, points=[999])], mode="host"))
    _refused(lambda: db.update([dict(Q, frame_id=1, lines=[999])], mode="host"))
    _refused(lambda: db.update([dict(Q, frame_id=1, prev_kfs=[999])], mode="host"))
    _refused(lambda: db.update([dict(Q, frame_id=1, prev_kfs=[-1])], mode="host"))
    for kind in (ls.KEYFRAME, ls.POINT, ls.LINE):
        _refused(lambda: db.set_bad(kind, [999], [1]))
        _refused(lambda: db.remove(kind, 999))
    _refused(lambda: db.set_bad(3, [1], [1]))
    _refused(lambda: db.set_bad(ls.POINT, [100, 999], [1, 1]))    # the first flag of the refused call is not set either
    _refused(lambda: db.set_keyframes([ls.kf(-2, 5)]))
    _refused(lambda: db.set_keyframes([ls.kf(5, 5, ch=[1, 1])]))
    _refused(lambda: db.configure(0))
    _unchanged(db, 1, st)


@pytest.mark.parametrize("which", range(4))
def test_too_small_output_array_changes_nothing(which):
    db = _small()
    st = db.stats()
    cap = [1, 1, 1, 1]
    cap[which] = 0
    _refused(lambda: db.update([dict(Q, frame_id=3)], mode="host", capacity=cap), lib.ERR_CAPACITY)
    _unchanged(db, 3, st)                                         # the id was not used, nothing was counted
    nk, npt, nl = db.size()
    ls.check([db.update([dict(Q, frame_id=4)], mode="host", capacity=(nk, npt, nl, 2))], [WANT])   # drfe_lmap_size's bounds suffice


def test_device_entry_without_a_context_is_a_state_error():
    db = _small()
    st = db.stats()
    _refused(lambda: db.update([dict(Q, frame_id=1)], mode="device"), lib.ERR_STATE)
    _unchanged(db, 1, st)
    ls.check([db.update([dict(Q, frame_id=2)] * 1, mode="batch")], [WANT])         # _batch of a host-only store runs on the host
    many = [dict(Q, frame_id=10 + k) for k in range(lib.LocalMap.limits()["device_from"] if lib.LocalMap.limits()["device_from"] < 64 else 8)]
    r = db.update(many, mode="batch")
    assert r["ref_kf"].tolist() == [1] * len(many) and db.stats()["device_calls"] == 0


def test_set_bad_is_followed_by_the_next_query():
    db = _small()
    db.set_bad(ls.POINT, [101], [0])
    r = db.update([dict(Q, frame_id=1)], mode="host")
    assert [x.tolist() for x in r["kfs"]] == [[1, 2]] and r["nulled"][0].tolist() == [] and r["record"].tolist() == [[2, 2, 0, 2]]
    db.set_bad(ls.KEYFRAME, [1], [1])
    r = db.update([dict(Q, frame_id=2)], mode="host")
    assert [x.tolist() for x in r["kfs"]] == [[2]] and r["ref_kf"].tolist() == [2] and r["mps"][0].tolist() == [101]
    db.set_bad(ls.LINE, [300], [1])
    db.set_bad(ls.KEYFRAME, [1], [0])
    r = db.update([dict(Q, frame_id=3)], mode="host")
    assert r["mls"][0].tolist() == [] and r["ref_kf"].tolist() == [1]


def test_an_empty_call_and_an_empty_store():
    db = lib.LocalMap()
    r = db.update([], mode="host")
    assert r["record"].shape == (0, 4) and db.stats()["calls"] == 0
    r = db.update([dict(frame_id=1, points=[-1, -1])], mode="host")
    assert r["kfs"][0].tolist() == [] and r["nulled"][0].tolist() == [] and r["ref_kf"].tolist() == [-1]
