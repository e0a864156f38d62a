"""KeyFrameDatabase on the host (drfe_kfdb_*_host, dr_slam_amd/csrc/kfdb.cpp) against tests/kfdb_numpy.py and against candidate
lists worked out by hand (tests/kfdb_scenarios.py).  Equal bytes everywhere; no GPU.

Parity with a DBoW2 build is not pinned: ScoringObject.cpp includes TemplatedVocabulary.h, which needs OpenCV headers that are
not installed where this was written, so the reference's own L1Scoring::score could not be compiled."""
import re

import numpy as np
import pytest

import kfdb_numpy as kn
import kfdb_scenarios as ks
from dr_slam_amd import lib

SEEDS = (3, 11, 29)


def both(ops):
    ref = kn.Database()
    r_np = ks.play(ops, ref)
    db = lib.KeyFrameDatabase()
    r_lib = ks.play(ops, db)
    assert len(r_np) == len(r_lib)
    for a, b in zip(r_lib, r_np):
        kn.same(a, b)
    return r_lib, ref, db


def cands(results):
    return [[list(map(int, c)) for c in r["candidates"]] for r in results]


def test_symbols_and_constants():
    L = lib.load()
    for s in lib.SYMBOLS:
        if "kfdb" in s:
            assert hasattr(L, s), s
    text = open(lib.os.path.join(lib._HERE, "..", "include", "drfe.h")).read()
    assert int(re.search(r"DRFE_KFDB_DEVICE_FROM = (\d+)", text).group(1)) == lib.KFDB_DEVICE_FROM
    assert int(re.search(r"DRFE_KFDB_NEIGHBOURS = (\d+)", text).group(1)) == lib.KFDB_NEIGHBOURS
    for k, name in enumerate(("L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA", "DOT_PRODUCT")):
        assert getattr(lib, "KFDB_" + name) == k and re.search(r"DRFE_KFDB_L1_NORM = 0, DRFE_KFDB_L2_NORM, DRFE_KFDB_CHI_SQUARE", text)


def test_native_caller_on_the_host_entries():
    """tests/native/kfdb_caller.cpp: the adaptor's KeyFrameDatabase through add, a loop query, erase, a relocalisation query and
    the two batch forms on stand-in types, against lists worked out by hand in its source"""
    import subprocess
    import native_build
    exe = native_build.caller("kfdb_caller")              # built here if the tests directory holds no build products
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "kfdb_caller ok (host, 4 loop + 4 relocalisation queries, device calls 0)" in p.stdout, (
        p.returncode, p.stdout, p.stderr)


def test_same_first_word_follows_latest_add():
    ops, expect = ks.same_first_word()
    r, _, _ = both(ops)
    assert cands(r) == expect


@pytest.mark.parametrize("M", [5, 6, 10])
def test_min_common_words_truncates(M):
    ops, expect, scored = ks.truncation(M)
    r, _, _ = both(ops)
    assert cands(r) == expect
    assert r[0]["record"][0].tolist()[1] == scored and r[0]["record"][0].tolist()[3] == M


def test_score_equal_to_min_score_is_kept():
    r, _, _ = both(ks.score_equals_min_score(1.0))
    assert cands(r) == [[[10]]] and r[0]["record"][0].tolist() == [2, 1, 1, 2]
    r, ref, _ = both(ks.score_equals_min_score(float(np.nextafter(np.float32(1.0), np.float32(2.0)))))
    assert cands(r) == [[[]]] and r[0]["record"][0].tolist() == [2, 1, 0, 2]
    assert ref.counters["below_min_score"] == 1


def test_acc_equal_to_retain_threshold_is_dropped():
    ops, expect = ks.acc_equals_retain()
    r, _, _ = both(ops)
    assert cands(r) == expect and r[0]["record"][0].tolist() == [3, 3, 3, 4]


def test_two_kept_elect_the_same_neighbour():
    ops, expect = ks.same_best_neighbour()
    r, ref, _ = both(ops)
    assert cands(r) == expect
    assert ref.counters["duplicate_dropped"] == 1 and ref.counters["best_replaced"] == 2


@pytest.mark.parametrize("connected", [True, False])
def test_connected_key_frame_with_the_best_score(connected):
    ops, expect = ks.connected_best(connected)
    r, ref, _ = both(ops)
    assert cands(r) == expect
    assert (ref.counters["connected_met"] > 0) == connected


@pytest.mark.parametrize("how", ["none", "same_call", "earlier_call"])
def test_reloc_neighbour_adds_a_stale_score(how):
    ops, expect, uninit = ks.reloc_stale(how)
    r, ref, db = both(ops)
    assert cands(r) == expect
    assert [x["uninit_reads"].tolist() for x in r] == uninit
    assert ref.counters["stale_read"] == 1
    assert db.stats()["uninit_reads"] == sum(map(sum, uninit))


def test_query_that_shares_no_word():
    ops, expect = ks.no_shared_word()
    r, ref, _ = both(ops)
    assert cands(r) == expect
    assert ref.counters["empty_loop_no_shared"] == 1 and ref.counters["empty_reloc_no_shared"] == 1
    assert not r[0]["record"].any() and not r[1]["record"].any()


def test_nothing_reaches_min_score():
    ops, expect = ks.below_min_score()
    r, ref, _ = both(ops)
    assert cands(r) == expect and ref.counters["empty_loop_none_kept"] == 1
    assert r[0]["record"][0].tolist() == [1, 1, 0, 4]


def test_add_after_across_three_queued_key_frames():
    ops, expect = ks.add_after_queue()
    r, _, db = both(ops)
    assert cands(r) == expect
    assert db.size() == (4, 4)


def test_min_score_from_covisible_with_a_waiting_key_frame():
    ops, expect, ms = ks.covisible_min_score()
    r, _, _ = both(ops)
    assert cands(r) == expect
    assert r[0]["min_score"][0] == ms


def test_batch_form_without_a_context_runs_on_the_host():
    ops, expect = ks.same_best_neighbour()
    db = lib.KeyFrameDatabase()
    assert cands(ks.play(ops, db, mode="batch")) == expect
    assert db.stats()["device_calls"] == 0
    with pytest.raises(lib.DrfeError) as e:
        db.loop_queries([dict(handle=1, id=6, min_score=0.0)], mode="device")
    assert e.value.rc == lib.ERR_STATE


@pytest.fixture(scope="module")
def random_runs():
    runs = []
    for seed in SEEDS:
        ops = ks.random_script(seed)
        ref = kn.Database()
        runs.append((ops, ks.play(ops, ref), ref.counters))
    return runs


def test_random_scripts_take_every_branch(random_runs):
    total = dict.fromkeys(kn.COUNTERS, 0)
    n_queries = n_two = 0
    for _, results, counters in random_runs:
        for k in kn.COUNTERS:
            total[k] += counters[k]
        for r in results:
            for c in r["candidates"]:
                n_queries += 1
                n_two += len(c) >= 2
    print(total, n_queries, n_two)
    assert all(total[k] > 0 for k in kn.COUNTERS), total
    assert 2 * n_two >= n_queries, (n_two, n_queries)


@pytest.mark.parametrize("i", range(len(SEEDS)))
def test_random_scripts_match_the_restatement(random_runs, i):
    ops, r_np, _ = random_runs[i]
    db = lib.KeyFrameDatabase()
    r_lib = ks.play(ops, db)
    for a, b in zip(r_lib, r_np):
        kn.same(a, b)
    st = db.stats()
    assert st["candidates"] == sum(len(c) for r in r_np for c in r["candidates"])


def test_l1_score_matches_the_restatement():
    rng = np.random.RandomState(5)
    for _ in range(200):
        ia = np.sort(rng.choice(60, rng.randint(0, 30), replace=False))
        ib = np.sort(rng.choice(60, rng.randint(0, 30), replace=False))
        va, vb = rng.randn(len(ia)), rng.randn(len(ib))         # signs too: fabs is part of the formula
        got = lib.kfdb_score(ia, va, ib, vb)
        want = kn.l1_score(dict(zip(ia.tolist(), va)), dict(zip(ib.tolist(), vb)))
        assert np.float32(got).tobytes() == np.float32(want).tobytes()
    assert lib.kfdb_score([], [], [1], [1.0]).tobytes() == np.float32(-0.0).tobytes()


def _small():
    db = lib.KeyFrameDatabase()
    db.put(1, [1, 2], [0.5, 0.5])
    db.put(2, [1, 2], [0.5, 0.5])
    db.add(2)
    return db


def _refused(fn, rc=lib.ERR_INVALID):
    with pytest.raises(lib.DrfeError) as e:
        fn()
    assert e.value.rc == rc


def test_query_ids_must_increase():
    db = _small()
    q = dict(handle=1, min_score=0.0)
    _refused(lambda: db.loop_queries([dict(q, id=0)]))
    db.loop_queries([dict(q, id=5)])
    _refused(lambda: db.loop_queries([dict(q, id=5)]))
    _refused(lambda: db.loop_queries([dict(q, id=6), dict(q, id=6)]))
    db.loop_queries([dict(q, id=6)])                             # the refused call used no id
    _refused(lambda: db.reloc_queries([(0, [1], [1.0])]))
    db.reloc_queries([(5, [1], [1.0])])                          # relocalisation ids are counted apart
    _refused(lambda: db.reloc_queries([(4, [1], [1.0])]))


def test_unknown_handles_are_refused():
    db = _small()
    q = dict(handle=1, id=1, min_score=0.0)
    _refused(lambda: db.loop_queries([dict(q, handle=9)]))
    _refused(lambda: db.loop_queries([dict(q, connected=[9])]))
    _refused(lambda: db.loop_queries([dict(handle=1, id=1, covisible=[9])]))
    for fn in (db.add, db.erase, db.remove):
        _refused(lambda: fn(9))
    _refused(lambda: db.set_neighbours([9], [[1]]))
    _refused(lambda: db.set_neighbours([1], [[9]]))
    _refused(lambda: db.add(2))                                  # visible already
    _refused(lambda: db.erase(1))                                # not visible
    _refused(lambda: db.put(1, [3], [1.0]))                      # stored already
    _refused(lambda: db.loop_queries([dict(q, handle=2, add_after=True)]))
    assert db.size() == (2, 1)
    db.remove(2)
    assert db.size() == (1, 0)
    db.put(2, [7], [1.0])


def test_unsorted_word_ids_are_refused():
    db = _small()
    _refused(lambda: db.put(3, [2, 1], [0.5, 0.5]))
    _refused(lambda: db.put(3, [1, 1], [0.5, 0.5]))
    _refused(lambda: db.reloc_queries([(1, [2, 1], [0.5, 0.5])]))
    assert db.size() == (2, 1)


@pytest.mark.parametrize("scoring", [lib.KFDB_L2_NORM, lib.KFDB_CHI_SQUARE, lib.KFDB_KL, lib.KFDB_BHATTACHARYYA, lib.KFDB_DOT_PRODUCT])
def test_other_scoring_types_are_refused(scoring):
    _refused(lambda: lib.KeyFrameDatabase(scoring=scoring))


def test_too_small_candidate_array_changes_nothing():
    ops, _, _ = ks.reloc_stale("same_call")
    db = lib.KeyFrameDatabase()
    ks.play(ops[:-1], db)
    _refused(lambda: db.reloc_queries(ops[-1][1], capacity=1), lib.ERR_CAPACITY)
    # neither the ids nor mRelocScore were committed: the same call again, then the uninitialised read is still there
    fresh = lib.KeyFrameDatabase()
    ks.play(ops[:-1], fresh)
    _refused(lambda: fresh.reloc_queries([ks.RELOC_S], capacity=0), lib.ERR_CAPACITY)
    r = fresh.reloc_queries([ks.RELOC_A])
    assert r["uninit_reads"].tolist() == [1] and cands([r]) == [[[10]]]


def test_clear_empties_the_inverted_file_only():
    ops, _ = ks.same_best_neighbour()
    db = lib.KeyFrameDatabase()
    ks.play(ops[:-1], db)
    db.clear()
    assert db.size() == (4, 0)
    assert cands([db.loop_queries([dict(handle=1, id=9, min_score=0.0)])]) == [[[]]]
    db.add(12)
    assert cands([db.loop_queries([dict(handle=1, id=10, min_score=0.0)])]) == [[[12]]]
