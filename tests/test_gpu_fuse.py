"""GPU tests of the device entry of the fuse commit (drfe_lmap_fuse_device, dr_slam_amd/csrc/fuse_kernels.hip, DESIGN.md section
32): the same bytes, the same store afterwards (through the getters and a following update, connect, cull and recent_cull on the
device, which read the resident blocks the walk stored into) and the same counters as the host entry and as tests/fuse_numpy.py,
on every hand-built store of tests/fuse_scenarios.py, on seeded scripts with edits, and on shapes placed from
drfe_lmap_fuse_limits(): steps of 0, 1, 63, 64, 65 and the tile's size - 1, + 0, + 1 candidates with all, none and every other
one live; losers with 0, 1, 63, 64, 65 and 300 observers; a coupled pair across a wavefront seam and across a workgroup seam of
the pre-pass; the append log one short of full, full and one over (the hand-back to the host), and the seam inside later steps;
the scratch budget of a call, and one byte less; and the bytes that travel after a call.  No test provokes a fault: every refused
input is refused on the host before a launch."""
import itertools

import numpy as np
import pytest

import fuse_numpy as fn
import fuse_scenarios as fs
from dr_slam_amd import lib
from test_fuse_cpu import _refused, same_following, store_of

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.fuse_limits()
T, WAVE, LOG = LIM["tile"], LIM["wavefront"], LIM["log_entries"]
POINT, LINE = fs.POINT, fs.LINE
FRAME_IDS = itertools.count(2 * 10 ** 6)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def same_stats(dev, host, handed_back=None):
    sd, sh = dev.fuse_stats(), host.fuse_stats()
    skip = ("device_calls", "handed_back")
    assert {k: v for k, v in sd.items() if k not in skip} == {k: v for k, v in sh.items() if k not in skip}
    assert sh["device_calls"] == 0 and sh["handed_back"] == 0
    if handed_back is not None:
        assert sd["handed_back"] == handed_back
    return sd


def read_back_on_device(dev, host, w, cull=True):
    """what the kernels of the other operations find in the resident blocks the walk stored into"""
    same_following(dev, host, w, mode_a="device", mode_b="host")
    if cull:
        kfs = [h for h, k in w.kfs.items() if not k["bad"]][:6]
        a, b = dev.cull(kfs, mode="device"), host.cull(kfs, mode="host")
        assert np.array_equal(a["record"], b["record"]) and np.array_equal(a["culled"], b["culled"])
    pts, lns = sorted(w.items[POINT])[:40], sorted(w.items[LINE])[:10]
    a, b = dev.recent_cull(7, pts, lns, mode="device"), host.recent_cull(7, pts, lns, mode="host")
    for name in ("points", "lines"):
        assert np.array_equal(a[name]["action"], b[name]["action"]) and np.array_equal(a[name]["culled"], b[name]["culled"])
        assert all(np.array_equal(x, y) for x, y in zip(a[name]["erased"], b[name]["erased"]))
    fs.same_state(fs.state_of_store(dev, w), fs.state_of_store(host, w))


def three_ways(ctx, w, steps, handed_back=0, read_back=True, capacity=None):
    """a call on the device, on the host and in the restatement (which changes w)"""
    dev, host = store_of(w, ctx), store_of(w)
    r_dev, r_host = dev.fuse(steps, mode="device", capacity=capacity), host.fuse(steps, mode="host", capacity=capacity)
    fs.same_results(r_dev, r_host)
    fs.same_result(r_dev, w.fuse(steps))
    fs.same_state(fs.state_of_store(dev, w), fs.state_of_world(w))
    fs.same_state(fs.state_of_store(host, w), fs.state_of_world(w))
    sd = same_stats(dev, host, handed_back)
    assert sd["device_calls"] == (1 if sum(len(s["candidates"]) for s in steps) else 0)
    if read_back:
        read_back_on_device(dev, host, w, cull=False)
    return r_dev, dev, host


@pytest.mark.parametrize("scenario", fs.SCENARIOS, ids=lambda f: getattr(f, "__name__", "snapshot_neighbours"))
def test_scenarios_on_the_device(ctx, scenario):
    w, steps, expect = scenario()
    r, dev, _ = three_ways(ctx, w, steps)
    fs.check_expect(r, fs.state_of_world(w), expect)


@pytest.mark.parametrize("seed", (411, 412, 413, 414))
def test_seeded_scripts_on_the_device(ctx, seed):
    rng = np.random.default_rng(seed)
    w = fs.random_world(rng)
    dev, host = store_of(w, ctx), store_of(w)
    for round_ in range(3):
        steps = fs.random_steps(rng, w)
        r = dev.fuse(steps, mode="device")
        fs.same_results(r, host.fuse(steps, mode="host"))
        fs.same_result(r, w.fuse(steps))
        fs.same_state(fs.state_of_store(dev, w), fs.state_of_world(w))
        same_following(dev, host, w, mode_a="device", mode_b="host", connect=False)
        pts = [int(p) for p in rng.choice(sorted(w.items[POINT]), 6, replace=False)]
        flags = [int(v) for v in rng.integers(0, 2, 6)]
        for s in (dev, host):
            s.set_bad(POINT, pts, flags)
            s.recent_increase(POINT, pts, [3] * 6, [5] * 6)
        for p, f in zip(pts, flags):
            w.items[POINT][p]["bad"] = f
            w.items[POINT][p]["found"] += 3
            w.items[POINT][p]["visible"] += 5
    same_stats(dev, host, 0)
    read_back_on_device(dev, host, w)


def wide_world(n_items, row, extra_kfs=2):
    """key frame 10 with a row of `row` empty entries, a few more key frames, and n_items points without observations"""
    w = fn.World()
    w.add_kf(10, 1, row, 4, stereo=[i % 3 == 0 for i in range(row)])
    for k in range(extra_kfs):
        w.add_kf(20 + 10 * k, 2 + k, 8, 4)
    for i in range(n_items):
        w.add_item(POINT, 1000 + i, [], found=i % 7, visible=1 + i % 5)
    return w


@pytest.mark.parametrize("n", (0, 1, WAVE - 1, WAVE, WAVE + 1, T - 1, T, T + 1))
@pytest.mark.parametrize("live", ("all", "none", "other"))
def test_step_lengths(ctx, n, live):
    """the pre-pass packs the live candidates of a tile in order; the dead ones get action 0 from it"""
    w = wide_world(T + 2, T + 2)
    cands = [1000 + i for i in range(n)]
    best = [i if live == "all" or (live == "other" and i % 2 == 0) else -1 for i in range(n)]
    if live == "other":
        cands = [c if i % 4 != 1 else -1 for i, c in enumerate(cands)]
    # a second step on the same key frame meets what the first left: every occupant that was added loses the tie to its rival
    rivals = [1000 + (i + 1) % max(n, 1) for i in range(n)]
    steps = [fs.step(10, cands, best), fs.step(10, rivals, list(range(n)), form=fs.LOOP), fs.step(10, [], [])]
    r, _, _ = three_ways(ctx, w, steps, read_back=False)
    assert r["steps"][0]["n_fused"] == sum(1 for c, b in zip(cands, best) if c >= 0 and b >= 0)


def loser_world(n_obs, n_kfs=304):
    """a loser with n_obs observers at index 1 of each; the candidate observes every third of them (the erase branch) at index
    2, and two key frames the loser does not"""
    w = fn.World()
    for k in range(n_kfs):
        w.add_kf(k + 1, n_kfs - k, 4, 2, stereo=[0, k % 2, 0, 0])      # ranks fall as handles rise
    w.add_item(POINT, 100, [(k + 1, 1) for k in range(n_obs)], n_obs=1)
    w.add_item(POINT, 101, [(k + 1, 2) for k in range(0, n_obs, 3)] + [(n_kfs - 1, 2), (n_kfs, 2)], n_obs=5)
    w.kfs[n_kfs]["rows"][POINT][0] = 100                                # the entry the candidate is sent to; stale when n_obs is 0
    return w


@pytest.mark.parametrize("n_obs", (0, 1, WAVE - 1, WAVE, WAVE + 1, 300))
def test_loser_sizes(ctx, n_obs):
    """a Replace spreads the loser's observations over the lanes: less than a wave, a wave, more, more than the workgroup"""
    w = loser_world(n_obs)
    steps = [fs.step(304, [-1] * 4, form=fs.MATCHED)]
    steps[0]["candidates"][0] = 101
    r, dev, host = three_ways(ctx, w, steps, read_back=False)
    (kind, loser, winner, rec), = r["replaced"]
    assert (loser, winner, len(rec)) == (100, 101, n_obs) and int(rec[:, 2].sum()) == n_obs - len(range(0, n_obs, 3))
    # and the other way round in a second call on the same store: the emptied 100 wins everything back from 101
    steps = [fs.step(304, [-1, -1, 100, -1], form=fs.MATCHED)]
    fs.same_results(dev.fuse(steps, mode="device"), host.fuse(steps, mode="host"))
    fs.same_state(fs.state_of_store(dev, w), fs.state_of_store(host, w))


@pytest.mark.parametrize("seam", (WAVE, T))
def test_coupled_pair_across_a_seam(ctx, seam):
    """candidates seam - 1 and seam share a best_idx: the second meets the first, whichever lane or workgroup packed them"""
    n = seam + 3
    w = wide_world(n, n)
    w.items[POINT][1000 + seam]["n_obs"] = 3                            # the later one wins
    best = list(range(n))
    best[seam] = seam - 1
    r, _, _ = three_ways(ctx, w, [fs.step(10, [1000 + i for i in range(n)], best)], read_back=False)
    a = r["steps"][0]["action"]
    assert a[seam - 1] == fs.ADDED and a[seam] == fs.OCCUPANT_REPLACED and w.kfs[10]["rows"][POINT][seam - 1] == 1000 + seam
    assert w.kfs[10]["rows"][POINT][seam] == -1


@pytest.mark.parametrize("n", (LOG - 1, LOG, LOG + 1))
def test_append_log_at_its_end(ctx, n):
    """n additions fill the log: one short of full and full stay on the device, one over hands the last candidate to the host"""
    w = wide_world(n, n, extra_kfs=0)
    r, dev, host = three_ways(ctx, w, [fs.step(10, [1000 + i for i in range(n)], list(range(n)))], handed_back=1 if n > LOG else 0,
                              read_back=False)
    assert r["steps"][0]["n_fused"] == n
    same_following(dev, host, w, mode_a="device", mode_b="host", connect=False)


@pytest.mark.parametrize("room", (0, 1, 3, 10, 40))
def test_hand_back_seam_inside_later_steps(ctx, room):
    """the log has `room` entries left when seeded steps of every form begin: the walk stops where an addition, or the
    observations of a loser, no longer fit - in a pass 1, in a pass 2, in front of a Replace - and the host goes on from the
    downloaded state: the same bytes and the same store as the host alone"""
    rng = np.random.default_rng(500 + room)
    w = fs.random_world(rng)
    n = LOG - room
    w.add_kf(5, 0, n, 2)
    for i in range(n):
        w.add_item(POINT, 100000 + i, [])
    steps = [fs.step(5, [100000 + i for i in range(n)], list(range(n)))] + fs.random_steps(rng, w, n_steps=6, answered=0.7)
    ref = w.clone()
    ref.fuse(steps)
    appended = sum(ref.paths().get(k, 0) for k in ("insert_front", "insert_middle", "insert_end"))   # every gained observation
    assert appended > LOG, "the steps do not reach the end of the log"
    _, dev, host = three_ways(ctx, w, steps, handed_back=1, read_back=False)
    read_back_on_device(dev, host, w)


def test_fuse_after_a_keyframe_cull_on_the_device(ctx):
    """a device KeyFrameCulling between two device fusions: the walk reads the observations, nObs and flags the cull left in the
    resident blocks"""
    w = fs.redundant_world()
    dev, host = store_of(w, ctx), store_of(w)
    before, after = fs.steps_around_a_cull()
    fs.same_results(dev.fuse(before, mode="device"), host.fuse(before, mode="host"))
    w.fuse(before)
    r, rh = dev.cull([30, 40], mode="device"), host.cull([30, 40], mode="host")
    assert [int(h) for h in r["culled"]] == [30, 40] == [int(h) for h in rh["culled"]]
    fs.apply_cull(w, r)
    fs.same_state(fs.state_of_store(dev, w), fs.state_of_world(w))
    rd = dev.fuse(after, mode="device")
    fs.same_results(rd, host.fuse(after, mode="host"))
    fs.same_result(rd, w.fuse(after))
    fs.same_state(fs.state_of_store(dev, w), fs.state_of_world(w))
    fs.same_state(fs.state_of_store(host, w), fs.state_of_world(w))
    assert dev.fuse_stats()["device_calls"] == 2 and dev.fuse_stats()["handed_back"] == 0


def record_room_world(n_losers, n_kfs):
    """n_losers points that each observe all n_kfs key frames and stand in a row of key frame 1, and one point that observes all
    of them too: every Replace by it erases n_kfs entries and appends nothing to the log"""
    w = fn.World()
    for k in range(n_kfs):
        w.add_kf(k + 1, k + 1, n_losers + 1, 1)
    for i in range(n_losers):
        w.add_item(POINT, 1000 + i, [(k + 1, i) for k in range(n_kfs)], n_obs=1)
    w.add_item(POINT, 500, [(k + 1, n_losers) for k in range(n_kfs)], n_obs=2)
    return w


def test_record_room_at_its_end(ctx):
    """the walk's second reason to stop: the records of the Replace at hand no longer fit its record room.  Every Replace here
    erases 256 entries and appends nothing, so the log stays empty and the record room fills: the host finishes the call"""
    n_kfs = 256
    n = LIM["record_entries"] // n_kfs + 3
    w = record_room_world(n, n_kfs)
    dev, host = store_of(w, ctx), store_of(w)
    steps = [fs.step(1, [500] * n + [-1], form=fs.MATCHED)]
    r = dev.fuse(steps, mode="device")
    fs.same_results(r, host.fuse(steps, mode="host"))
    assert len(r["replaced"]) == n and all(len(rec) == n_kfs and not rec[:, 2].any() for _, _, _, rec in r["replaced"])
    assert dev.fuse_stats()["handed_back"] == 1 and dev.fuse_stats()["moved"] == 0 and dev.fuse_stats()["erased"] == n * n_kfs
    for kf in (1, 2, n_kfs):
        assert np.array_equal(dev.get_match_row(POINT, kf), host.get_match_row(POINT, kf))
    assert list(dev.get_replaced(POINT, [1000, 1000 + n - 1])) == [500, 500]
    same_following(dev, host, w, mode_a="device", mode_b="host", connect=False)


def test_scratch_budget(ctx):
    """a call needs its scratch whole: the walk is one launch.  With one byte less the device entry refuses on the host, before
    any launch, and nothing changes; _batch is the host entry below the crossover."""
    w, steps, _ = fs.second_meets_first()
    dev = store_of(w, ctx)
    whole, least, fixed = dev.fuse_scratch(2, 1)
    assert whole == least and fixed == 12 * LOG + 9 * LIM["record_entries"] + 1024 and whole - fixed >= LIM["tile_bytes"]
    before = fs.state_of_store(dev, w)
    dev.configure(whole - 1)
    assert "does not fit the configured device scratch" in _refused(lambda: dev.fuse(steps, mode="device"), lib.ERR_CAPACITY)
    fs.same_state(fs.state_of_store(dev, w), before)
    assert dev.fuse_stats()["calls"] == 0
    dev.configure(whole)
    fs.same_result(dev.fuse(steps, mode="device"), w.fuse(steps))
    assert dev.fuse_stats()["device_calls"] == 1


def test_capacity_is_settled_before_the_launch(ctx):
    """the device commits as it goes: capacities below the bounds are settled by a walk of the host first"""
    w, steps, _ = fs.tie_occupant_loses()
    dev = store_of(w, ctx)
    before = fs.state_of_store(dev, w)
    for cap in ((0, 8, 8), (8, 1, 8), (8, 8, 0)):
        assert "returns more than" in _refused(lambda: dev.fuse(steps, mode="device", capacity=cap), lib.ERR_CAPACITY)
        fs.same_state(fs.state_of_store(dev, w), before)
    fs.same_result(dev.fuse(steps, mode="device", capacity=(1, 2, 1)), w.fuse(steps))
    assert dev.fuse_stats()["device_calls"] == 1


def test_what_travels_after_a_call(ctx):
    """The walk stores the match rows, the bad flags, nObs and the counters into the resident blocks itself: the call and the
    device call after it send no match rows and no graph block, only the observations with their offsets and indices."""
    rng = np.random.default_rng(77)
    pad = 4000
    w = fs.random_world(rng, n_kf=8, row=pad, n_pts=60, n_lns=2, max_obs=4)
    dev, host = store_of(w, ctx), store_of(w)
    steps = fs.random_steps(rng, w, n_steps=3, n_cand=30, answered=0.8)
    steps = [s for s in steps if s["kind"] == POINT and s["form"] != fs.MATCHED] or [fs.step(10, [1000, 1001], [0, 1])]
    pts = sorted(w.items[POINT])
    q, q2, q3 = ([dict(frame_id=next(FRAME_IDS), points=pts)] for _ in range(3))
    dev.update(q, mode="device")                                        # the rows and the graph are resident now
    host.update(q, mode="host")
    b0 = dev.upload_bytes()
    match_rows = 4 * 8 * pad
    assert b0["rows"] > match_rows and b0["graph"] > 0
    r = dev.fuse(steps, mode="device")
    fs.same_results(r, host.fuse(steps, mode="host"))
    assert len(r["replaced"]) > 0 and len(r["touched_points"]) > 0
    b1 = dev.upload_bytes()
    assert b1["graph"] == b0["graph"] and b1["geometry"] == b0["geometry"]
    assert b1["rows"] == b0["rows"]                                     # the rows were current: the call itself sent nothing
    a, b = dev.update(q2, mode="device"), host.update(q2, mode="host")   # reads the flags and entries the walk stored
    assert all(np.array_equal(x, y) for key in a for x, y in zip(a[key], b[key]))
    b2 = dev.upload_bytes()
    total_obs = sum(len(p["obs"]) for p in w.items[POINT].values()) + 2 * 90
    tail = 4 * (len(pts) + 1) + 4 * total_obs + 2 * 16                  # the offsets and the observations
    assert 0 < b2["rows"] - b1["rows"] <= tail < match_rows and b2["graph"] == b1["graph"]
    dev.update(q3, mode="device")
    assert dev.upload_bytes() == b2
    assert dev.fuse_stats()["device_calls"] == 1 and dev.fuse_stats()["handed_back"] == 0


def test_native_caller_on_the_device_entry():
    """tests/native/fuse_caller.cpp with every call forced onto the device entry: the same two worlds, and the store read back
    through the getters and a device UpdateLocalMap"""
    import subprocess
    import native_build
    exe = native_build.caller("fuse_caller")
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "fuse_caller ok (device, 68 calls, 142 added, 340 replaced" in p.stdout, (p.returncode, p.stdout, p.stderr)
