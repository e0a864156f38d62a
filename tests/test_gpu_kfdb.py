"""GPU tests of KeyFrameDatabase's device entries (drfe_kfdb_*_queries_device, dr_slam_amd/csrc/kfdb_kernels.hip, DESIGN.md
section 23): the same bytes and the same state as the host entries and as tests/kfdb_numpy.py, on the hand-built databases of
tests/test_kfdb_cpu.py, the seeded random scripts, and shapes chosen for the kernels: 1, 63, 64, 65 and 257 visible key frames
(the workgroup has 256 lanes), 1, 2 and 70 queries a call, vectors of 3000 words, a key frame of one word, holes left by erase and
remove, calls in a row on one database, host and device calls mixed."""
import numpy as np
import pytest

import kfdb_numpy as kn
import kfdb_scenarios as ks
from dr_slam_amd import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def cands(results):
    return [[list(map(int, c)) for c in r["candidates"]] for r in results]


def three_ways(ctx, ops):
    """a script on the device, on the host and in the restatement: all equal; returns the device's results and database"""
    ref = kn.Database()
    r_np = ks.play(ops, ref)
    host = lib.KeyFrameDatabase()
    r_host = ks.play(ops, host)
    dev = lib.KeyFrameDatabase(ctx)
    r_dev = ks.play(ops, dev, mode="device")
    assert len(r_dev) == len(r_np) == len(r_host)
    for d, h, n in zip(r_dev, r_host, r_np):
        kn.same(d, n)
        for k in ("cand_offsets", "record", "min_score", "uninit_reads"):
            assert d[k].tobytes() == h[k].tobytes(), k
    n_calls = sum(1 for r in r_np if len(r["candidates"]))
    assert dev.stats()["device_calls"] == n_calls and host.stats()["device_calls"] == 0
    assert dev.size() == host.size()
    return r_dev, dev


HAND = {
    "same_first_word": lambda: ks.same_first_word()[:2],
    "truncation_5": lambda: ks.truncation(5)[:2],
    "truncation_6": lambda: ks.truncation(6)[:2],
    "truncation_10": lambda: ks.truncation(10)[:2],
    "score_equals_min_score": lambda: (ks.score_equals_min_score(1.0), [[[10]]]),
    "score_below_min_score": lambda: (ks.score_equals_min_score(float(np.nextafter(np.float32(1.0), np.float32(2.0)))), [[[]]]),
    "acc_equals_retain": ks.acc_equals_retain,
    "same_best_neighbour": ks.same_best_neighbour,
    "connected_best": lambda: ks.connected_best(True),
    "not_connected_best": lambda: ks.connected_best(False),
    "reloc_uninit": lambda: ks.reloc_stale("none")[:2],
    "reloc_stale_same_call": lambda: ks.reloc_stale("same_call")[:2],
    "reloc_stale_earlier_call": lambda: ks.reloc_stale("earlier_call")[:2],
    "no_shared_word": ks.no_shared_word,
    "below_min_score": ks.below_min_score,
    "add_after_queue": ks.add_after_queue,
    "covisible_min_score": lambda: ks.covisible_min_score()[:2],
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_databases(ctx, name):
    ops, expect = HAND[name]()
    r, _ = three_ways(ctx, ops)
    assert cands(r) == expect


def test_uninitialised_reads_are_counted(ctx):
    ops, _, uninit = ks.reloc_stale("none")
    r, dev = three_ways(ctx, ops)
    assert [x["uninit_reads"].tolist() for x in r] == uninit and dev.stats()["uninit_reads"] == 1


@pytest.mark.parametrize("seed", (3, 11, 29))
def test_random_scripts(ctx, seed):
    three_ways(ctx, ks.random_script(seed))


@pytest.mark.parametrize("n_queries", (1, 2, 70))
@pytest.mark.parametrize("n_visible", (1, 63, 64, 65, 257))
def test_database_sizes_and_queries_per_call(ctx, n_visible, n_queries):
    r, dev = three_ways(ctx, ks.sized_script(n_visible, n_queries, seed=n_visible + n_queries))
    assert len(r) == 3 and all(len(x["candidates"]) == n_queries for x in r)
    if n_visible >= 63:
        assert sum(len(c) for x in r for c in x["candidates"]) > 0


def test_long_vectors_and_a_single_word(ctx):
    ops = ks.sized_script(65, 2, seed=4, long_vectors=True)
    assert max(len(o[2]) for o in ops if o[0] == "put") == 3000 and min(len(o[2]) for o in ops if o[0] == "put") == 1
    r, _ = three_ways(ctx, ops)
    assert r[0]["record"][0, 3] > 500               # the long query meets the long key frame


def test_holes_left_by_erase_and_remove(ctx):
    ops = ks.sized_script(130, 2, seed=8)
    tail = [o for o in ops if o[0] in ("loop", "reloc")]
    head = [o for o in ops if o[0] not in ("loop", "reloc")]
    holes = [("erase", 1000 + i) for i in range(0, 130, 3)] + [("remove", 1000 + i) for i in range(0, 130, 6)]
    refill = [("put", 7000, [1, 2, 3], [0.5, 0.25, 0.25]), ("add", 7000), ("add", 1003)]
    # a call, then the holes and a slot used again, then the same queries under new ids
    again = [("reloc", [(q[0] + 1000, q[1], q[2]) for q in tail[1][1]])]
    connected_gone = {1000 + i for i in range(0, 130, 6)}
    loop = [dict(q, connected=[h for h in q["connected"] if h not in connected_gone],
                 covisible=[h for h in q["covisible"] if h not in connected_gone]) for q in tail[0][1]]
    three_ways(ctx, head + [tail[1]] + holes + refill + [("loop", loop)] + again)


def test_calls_in_a_row_and_host_calls_between(ctx):
    ops = ks.sized_script(100, 5, seed=21)
    setup = [o for o in ops if o[0] not in ("loop", "reloc")]
    calls = [o for o in ops if o[0] in ("loop", "reloc")]
    ref = kn.Database()
    ks.play(setup, ref)
    db = lib.KeyFrameDatabase(ctx)
    ks.play(setup, db)
    want = ks.play(calls, ref)
    # relocalisation on the device, the loop call on the host, relocalisation on the device again: mRelocScore and the
    # sequence numbers have to follow the database wherever the call ran
    got = [db.loop_queries(calls[0][1], mode="host"), db.reloc_queries(calls[1][1], mode="device")]
    extra = [("reloc", [(q[0] + 500, q[1], q[2]) for q in calls[1][1]]), ("reloc", [(q[0] + 900, q[1], q[2]) for q in calls[2][1]])]
    want += ks.play(extra, ref)
    got.append(db.reloc_queries(calls[2][1], mode="host"))
    got.append(db.reloc_queries(extra[0][1], mode="device"))
    got.append(db.reloc_queries(extra[1][1], mode="device"))
    for g, w in zip(got, want):
        kn.same(g, w)
    assert db.stats()["device_calls"] == 3


def test_too_small_candidate_array_changes_nothing_on_the_device(ctx):
    ops, _, _ = ks.reloc_stale("same_call")
    db = lib.KeyFrameDatabase(ctx)
    ks.play(ops[:-1], db)
    with pytest.raises(lib.DrfeError) as e:
        db.reloc_queries([ks.RELOC_S], mode="device", capacity=0)
    assert e.value.rc == lib.ERR_CAPACITY
    r = db.reloc_queries([ks.RELOC_A], mode="device")
    assert r["uninit_reads"].tolist() == [1] and cands([r]) == [[[10]]]


def test_batch_form_follows_the_crossover(ctx):
    for n, calls in ((lib.KFDB_DEVICE_FROM - 1, 0), (lib.KFDB_DEVICE_FROM, 3)):
        ops = ks.sized_script(64, n, seed=2)
        ref = kn.Database()
        db = lib.KeyFrameDatabase(ctx)
        for g, w in zip(ks.play(ops, db, mode="batch"), ks.play(ops, ref)):
            kn.same(g, w)
        assert db.stats()["device_calls"] == calls


def test_native_caller_on_the_device_entries():
    """tests/native/kfdb_caller.cpp with every query call forced to the device entries"""
    import subprocess
    import native_build
    exe = native_build.caller("kfdb_caller")
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "kfdb_caller ok (device, 4 loop + 4 relocalisation queries, device calls 6)" in p.stdout, (
        p.returncode, p.stdout, p.stderr)
