"""GPU tests of Tracking::UpdateLocalMap's device entry (drfe_lmap_update_device, dr_slam_amd/csrc/lmap_kernels.hip, DESIGN.md
section 25): the same bytes and the same counters as the host entry and as tests/lmap_numpy.py, on every hand-built graph of
tests/lmap_scenarios.py, on seeded scripts with edits, and on shapes placed from drfe_lmap_limits(): frames of the vote
workgroup's size - 1, + 0, + 1 and of one point; points with 0, 1 and more than 64 observations; stores at the LDS histogram's
limit and one key frame above it; match rows of the gather's pass size - 1, + 0, + 1; a call of an empty, a one-point and a large
frame, whole and in chunks of one and two queries; an edit between two device calls; host and device calls in turn."""
import numpy as np
import pytest

import lmap_numpy as ln
import lmap_scenarios as ls
from dr_slam_amd import lib

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.limits()
SAME_STATS = ("calls", "queries", "local_kfs", "local_points", "local_lines", "nulled")


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def three_ways(ctx, ops, configure=None):
    """a script on the device, on the host and in the restatement: all equal; returns the device's results and store"""
    ref = ln.Store()
    r_np = ls.play(ops, ref)
    host = lib.LocalMap()
    r_host = ls.play(ops, host)
    dev = lib.LocalMap(ctx)
    if configure:
        dev.configure(configure)
    r_dev = ls.play(ops, dev, mode="device")
    assert len(r_dev) == len(r_np) == len(r_host)
    for d, h, n in zip(r_dev, r_host, r_np):
        ln.same(d, n)
        ln.same(d, h)
    sd, sh = dev.stats(), host.stats()
    for k in SAME_STATS:
        assert sd[k] == sh[k] == ref.counts[k], k
    n_calls = sum(1 for op in ops if op[0] == "update" and len(op[1]))
    assert sd["device_calls"] == n_calls and sh["device_calls"] == 0 and sh["uploads"] == 0
    assert dev.size() == host.size()
    return r_dev, dev


@pytest.mark.parametrize("name", sorted(ls.HAND))
def test_hand_built(ctx, name):
    ops, expect, _ = ls.HAND[name]()
    r, _ = three_ways(ctx, ops)
    ls.check(r, expect)


@pytest.mark.parametrize("seed", [2, 13, 101])
def test_seeded_scripts(ctx, seed):
    three_ways(ctx, ls.random_script(seed))


def test_seeded_script_past_80_key_frames(ctx):
    """150 key frames and frames of 200 points: the vote lists more than 80, about 80 and fewer"""
    ops = ls.random_script(7, n_kf=150, n_mp=600, obs=4, calls=3, per_call=6, frame_points=200)
    r, _ = three_ways(ctx, ops)
    listed = np.concatenate([x["record"][:, 1] for x in r])
    assert listed.max() > 80 and listed.min() < 80


def small_store(rng, n_kf, n_mp, row, obs):
    kfs = [ls.kf(h, int(rng.integers(1, 2 ** 40)) * 4096 + h, pts=[int(p) for p in rng.integers(-1, n_mp, row)]) for h in range(n_kf)]
    pts = [ls.mp(h, obs=[int(k) for k in rng.permutation(n_kf)[:int(rng.integers(0, obs + 1))]], bad=int(rng.random() < 0.2))
           for h in range(n_mp)]
    return [("kfs", kfs), ("points", pts)]


def test_frame_sizes_around_the_vote_workgroup(ctx):
    T = LIM["vote_threads"]
    rng = np.random.default_rng(5)
    ops = small_store(rng, 20, 2 * T, 40, 5)
    frames = [dict(frame_id=i + 1, points=[int(p) for p in rng.integers(-1, 2 * T, n)]) for i, n in enumerate((T - 1, T, T + 1, 1, 2 * T + 3))]
    r, _ = three_ways(ctx, ops + [("update", frames)])
    assert sum(len(x) for x in r[0]["nulled"]) > 0


def test_observation_counts(ctx):
    """points with no observation, one, and 70 (more than a wavefront)"""
    kfs = [ls.kf(h, 1000 - h, pts=[0, 1, 2]) for h in range(70)]
    pts = [ls.mp(0), ls.mp(1, [33]), ls.mp(2, list(range(70)))]
    qs = [dict(frame_id=1, points=[0]), dict(frame_id=2, points=[1]), dict(frame_id=3, points=[2]), dict(frame_id=4, points=[2, 1, 0, 2])]
    r, _ = three_ways(ctx, [("kfs", kfs), ("points", pts), ("update", qs)])
    assert r[0]["record"].tolist() == [[0, 0, 0, 0], [1, 1, 0, 1], [70, 70, 0, 1], [70, 70, 0, 3]]
    assert r[0]["ref_kf"].tolist() == [-1, 33, 69, 33]


@pytest.mark.parametrize("extra", [0, 1])
def test_histogram_at_the_lds_limit(ctx, extra):
    """the limit's count of stored key frames (histogram in LDS) and one more (a row of global scratch), tiny rows; the votes
    reach the first and the last slot"""
    n = LIM["lds_keyframes"] + extra
    kfs = [ls.kf(h, h + 1, pts=[h % 7], nb=[(h + 1) % n]) for h in range(n)]
    pts = [ls.mp(p, obs=[0, n - 1, n // 2 + p] if p < 5 else []) for p in range(7)]
    qs = [dict(frame_id=1, points=[0, 1, 6]), dict(frame_id=2, points=[6]), dict(frame_id=3, points=[4, 4, 3])]
    r, _ = three_ways(ctx, [("kfs", kfs), ("points", pts), ("update", qs)])
    assert r[0]["kfs"][0].tolist()[:2] == [0, n // 2] and n - 1 in r[0]["kfs"][0].tolist()


def test_match_rows_around_the_gather_pass(ctx):
    G = LIM["gather_entries"]
    rng = np.random.default_rng(9)
    n_mp = 3 * G
    sizes = (G - 1, G, G + 1, 2 * G + 1, 0, 1)
    kfs = [ls.kf(h, 50 - h, pts=[int(p) for p in rng.integers(-1, n_mp, s)], lns=[int(p) for p in rng.integers(-1, 40, s // 2)])
           for h, s in enumerate(sizes)]
    pts = [ls.mp(p, obs=[int(rng.integers(0, len(sizes)))], bad=int(rng.random() < 0.1)) for p in range(n_mp)]
    qs = [dict(frame_id=k + 1, points=[int(p) for p in rng.integers(0, n_mp, 30 if k != 2 else 0)], lines=[int(p) for p in rng.integers(-1, 40, 9)],
               prev_kfs=[5, 3, 2]) for k in range(4)]
    three_ways(ctx, [("kfs", kfs), ("points", pts), ("lines", list(range(40)), [int(p % 9 == 0) for p in range(40)]), ("update", qs)])


def mixed_call(rng):
    ops = small_store(rng, 60, 900, 120, 6)
    big = [int(p) for p in rng.integers(-1, 900, 700)]
    return ops + [("update", [dict(frame_id=1, points=[]), dict(frame_id=2, points=[17]), dict(frame_id=3, points=big),
                              dict(frame_id=4, points=[]), dict(frame_id=5, points=big[:100], prev_kfs=[3, 4])])]


def test_mixed_call(ctx):
    three_ways(ctx, mixed_call(np.random.default_rng(21)))


def test_mixed_call_in_chunks(ctx):
    """the smallest scratch budget the call runs with fits exactly one query, so it ran in chunks of one; twice that is chunks
    of two; one byte less and _device refuses while _batch runs the call on the host"""
    ops = mixed_call(np.random.default_rng(21))
    whole, _ = three_ways(ctx, ops)
    dev = lib.LocalMap(ctx)
    ls.play(ops[:-1], dev)
    lo, hi = 1, 1 << 30                     # lo refuses, hi runs
    dev.configure(hi)
    ln.same(dev.update(ops[-1][1], mode="device"), whole[0])
    base = 5
    while hi - lo > 1:
        mid = (lo + hi) // 2
        dev.configure(mid)
        try:
            dev.update([dict(q, frame_id=q["frame_id"] + base) for q in ops[-1][1]], mode="device")
            base += 5
            hi = mid
        except lib.DrfeError as e:
            assert e.rc == lib.ERR_CAPACITY
            lo = mid
    for budget in (hi, 2 * hi, 2 * hi + 1):
        three_ways(ctx, ops, configure=budget)
    dev.configure(lo)
    before = dev.stats()
    with pytest.raises(lib.DrfeError) as e:
        dev.update([dict(q, frame_id=q["frame_id"] + base) for q in ops[-1][1]], mode="device")
    assert e.value.rc == lib.ERR_CAPACITY and dev.stats() == before
    ln.same(dev.update([dict(q, frame_id=q["frame_id"] + base) for q in ops[-1][1]], mode="batch"), whole[0])
    assert dev.stats()["device_calls"] == before["device_calls"]


def test_edit_between_device_calls(ctx):
    """what the setters change is uploaded before the next device call and counted; a call without an edit uploads nothing"""
    rng = np.random.default_rng(4)
    ops = small_store(rng, 30, 200, 40, 5)
    frame = [int(p) for p in rng.integers(0, 200, 80)]
    dev, ref = lib.LocalMap(ctx), ln.Store()
    ls.play(ops, dev), ls.play(ops, ref)
    fid = [0]

    def step(uploads):
        fid[0] += 1
        q = [dict(frame_id=fid[0], points=frame)]
        d = dev.update(q, mode="device")
        ln.same(d, ref.update(q))
        assert dev.stats()["uploads"] == uploads
        return d

    a = step(1)
    step(1)
    voted = int(a["ref_kf"][0])
    for s in (dev, ref):
        s.set_bad(ls.KEYFRAME, [voted], [1])
    b = step(2)
    assert voted in a["kfs"][0].tolist() and int(b["ref_kf"][0]) != voted
    for s in (dev, ref):
        s.set_points([ls.mp(frame[0], obs=[], bad=1)])
    c = step(3)
    assert 0 in c["nulled"][0].tolist()
    for s in (dev, ref):
        s.set_keyframes([ls.kf(999, 7, pts=[frame[1]], nb=[voted])])
        s.set_points([ls.mp(frame[1], obs=[999])])
    d = step(4)
    assert 999 in d["kfs"][0].tolist()


def test_host_and_device_calls_in_turn(ctx):
    ops = ls.random_script(17, calls=6)
    ref, dev = ln.Store(), lib.LocalMap(ctx)
    k = 0
    for op in ops:
        r = ls.play([op], ref)
        d = ls.play([op], dev, mode=("device", "host", "batch")[k % 3])
        if op[0] == "update":
            k += 1
            ln.same(d[0], r[0])
    st = dev.stats()
    assert st["device_calls"] == 2 + (2 if LIM["device_from"] <= 8 else 0) and st["calls"] == 6


def test_batch_entry_follows_the_crossover(ctx):
    """_batch runs on the host below DRFE_LMAP_DEVICE_FROM queries and on the device from it, with the same bytes"""
    n = LIM["device_from"]
    if n > lib.LocalMap.limits()["vote_threads"] * 16:          # "never": every _batch call stays on the host
        n = 8
    rng = np.random.default_rng(8)
    ops = small_store(rng, 25, 150, 30, 4)
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    ls.play(ops, dev), ls.play(ops, host)
    frames = [[int(p) for p in rng.integers(-1, 150, 40)] for _ in range(n)]
    few = [dict(frame_id=1 + k, points=f) for k, f in enumerate(frames[:n - 1])]
    many = [dict(frame_id=100 + k, points=f) for k, f in enumerate(frames)]
    if few:
        ln.same(dev.update(few, mode="batch"), host.update(few, mode="host"))
    assert dev.stats()["device_calls"] == 0
    ln.same(dev.update(many, mode="batch"), host.update(many, mode="host"))
    assert dev.stats()["device_calls"] == (1 if LIM["device_from"] == n else 0)


def test_dangling_reference_refused_before_anything_runs(ctx):
    dev = lib.LocalMap(ctx)
    dev.set_keyframes([ls.kf(1, 1, pts=[5])])
    with pytest.raises(lib.DrfeError) as e:
        dev.update([dict(frame_id=1, points=[])], mode="device")
    assert e.value.rc == lib.ERR_STATE and "5" in str(e.value) and dev.stats()["uploads"] == 0


def test_native_caller_on_the_device_entry():
    """tests/native/lmap_caller.cpp with every call forced to the device entry: 40 single frames and one batch on the seeded
    graph, one frame on each hand-built one"""
    import subprocess
    import native_build
    exe = native_build.caller("lmap_caller")
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "lmap_caller ok (device, 50 frames, device calls 43)" in p.stdout, (p.returncode, p.stdout, p.stderr)
