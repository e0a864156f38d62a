"""GPU tests of the device entry of the item loops of ProcessNewKeyFrame (drfe_lmap_insert_device,
dr_slam_amd/csrc/insert_kernels.hip): the same bytes, the same store afterwards (through the getters and a
following update, connect, cull, recent_cull and fuse on the device, which read the resident blocks the call added into) and the
same counters as the host entry and as tests/insert_numpy.py, on every hand-built store of tests/insert_scenarios.py, on seeded
scripts with edits, and on shapes placed from drfe_lmap_insert_limits(): rows of 0, 1, 63, 64, 65 and the tile's size - 1, + 0,
+ 1 entries with all, none and every other entry added; a handle twice across a wavefront seam and across a tile seam; items with
0, 1, 64, 65 and 300 stored observers; 1, 2 and 65 called key frames that add one shared point; the scratch budget of one chunk,
of two, of one key frame a chunk, and one byte less; _batch below the crossover; and the bytes that travel after a call.  No test
provokes a fault: every refused input is refused on the host before a launch."""
import numpy as np
import pytest

import insert_scenarios as sc
from dr_slam_amd import lib
from insert_numpy import ADDED, RECENT, Store
from test_insert_cpu import FRAME_IDS, OPS, expected_stats, refused, run_script, same_culls, same_following, store_of

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.insert_limits()
T, WAVE = LIM["tile"], LIM["wavefront"]
POINT, LINE = sc.POINT, sc.LINE


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def read_back_on_device(dev, host, w, culls=True):
    """what the kernels of the other operations find in the resident blocks the call added into"""
    same_following(dev, host, w, mode_a="device", mode_b="host")
    kf = sorted(w.kfs)[0]
    cands = sorted(w.items[POINT])[:4]
    steps = [dict(keyframe=kf, kind=POINT, form=0, candidates=cands, best_idx=list(range(len(cands))))]
    a, b = dev.fuse(steps, mode="device"), host.fuse(steps, mode="host")
    assert np.array_equal(a["steps"][0]["action"], b["steps"][0]["action"]) and len(a["replaced"]) == len(b["replaced"])
    if culls:
        same_culls(dev, host, w, mode_a="device", mode_b="host")
    sc.same_state(sc.state_of_store(dev, w), sc.state_of_store(host, w))


def three_ways(ctx, w, handles, normals=True, read_back=True, chunks=1, configure=None):
    """a call on the device, on the host and in the restatement (which changes w)"""
    dev, host = store_of(w, ctx), store_of(w)
    if configure is not None:
        dev.configure(configure)
    r_dev, r_host = dev.insert(handles, mode="device", normals=normals), host.insert(handles, mode="host", normals=normals)
    sc.same_results(r_dev, r_host)
    want = w.insert(handles, normals=normals)
    sc.same_result(r_dev, want, normals=normals)
    sc.same_state(sc.state_of_store(dev, w), sc.state_of_world(w))
    sc.same_state(sc.state_of_store(host, w), sc.state_of_world(w))
    entries = sum(len(w.kfs[h]["rows"][k]) for h in handles for k in (POINT, LINE))
    assert dev.insert_stats() == expected_stats(want, len(handles), device=1 if entries else 0, chunks=chunks if entries else 0)
    assert host.insert_stats() == expected_stats(want, len(handles))
    if read_back:
        read_back_on_device(dev, host, w)
    return r_dev, dev, host


@pytest.mark.parametrize("scenario", sc.SCENARIOS, ids=lambda f: f.__name__)
def test_scenarios_on_the_device(ctx, scenario):
    w, handles, expect = scenario()
    r, dev, _ = three_ways(ctx, w, handles)
    sc.check_expect(r, sc.state_of_world(w), expect)


@pytest.mark.parametrize("case", sc.refusals(), ids=lambda c: c[0])
def test_refusals_on_the_device_entry(ctx, case):
    """refused on the host, before any launch"""
    _, w, handles, normals, rc = case
    dev = store_of(w, ctx)
    before = sc.state_of_store(dev, w)
    refused(lambda: dev.insert(handles, mode="device", normals=normals), rc)
    assert sc.state_of_store(dev, w) == before
    st = dev.insert_stats()
    assert st["calls"] == 0 and st["device_calls"] == 0 and st["device_chunks"] == 0
    same_following(dev, store_of(w), w, mode_a="device")


@pytest.mark.parametrize("seed", (3311, 3312, 3313))
def test_seeded_scripts_on_the_device(ctx, seed):
    dev = run_script(seed, ctx, mode="device")
    st = dev.insert_stats()
    assert st["calls"] == len(OPS) + 1 and st["device_calls"] == len(OPS) + 1 and st["points_added"] > 0 and st["lines_added"] > 0


def test_without_normals_on_the_device(ctx):
    """integer-only on a store without geometry: no geometry block is built or sent"""
    w, handles, _ = sc.two_and_three_callers()
    dev = store_of(w, ctx, geometry=False)
    got = dev.insert(handles, mode="device", normals=False)
    sc.same_result(got, w.insert(handles, normals=False), normals=False)
    sc.same_state(sc.state_of_store(dev, w), sc.state_of_world(w))
    assert dev.upload_bytes()["geometry"] == 0 and dev.insert_stats()["device_calls"] == 1


def wide_world(row, line_row=4, n_kfs=3):
    """key frames 10, 20, .. with point rows of `row` entries and as many points 1000.. that nothing observes yet"""
    w = Store()
    w.scales = [1.0, 1.2, 1.44]
    for k in range(n_kfs):
        h = 10 * (k + 1)
        w.add_kf(h, k + 1, row, line_row, stereo=[int(i % 3 == 0) for i in range(row)])
        w.set_pose(h, (0.5 * k, 0.25, 0.0))
    for i in range(row):
        sc.point(w, 1000 + i, [], world=(0.5 + i % 7, 1.0 + i % 5, 3.0), ref=20, level=i % 3, found=i % 7)
    return w


@pytest.mark.parametrize("n", (0, 1, WAVE - 1, WAVE, WAVE + 1, T - 1, T, T + 1))
@pytest.mark.parametrize("share", ("all", "none", "other"))
def test_row_lengths(ctx, n, share):
    """the lists are packed in walk order across wavefronts and workgroups: all, none and every other entry ADDED (the rest
    RECENT: key frame 10 already observes them)"""
    w = wide_world(n)
    for i in range(n):
        sc.put(w, POINT, 10, i, 1000 + i)
        if share == "none" or (share == "other" and i % 2):
            w.items[POINT][1000 + i]["obs"] = [(10, i)]
            w.items[POINT][1000 + i]["n_obs"] = 1
    r, _, _ = three_ways(ctx, w, [10], read_back=False)
    want = [RECENT if share == "none" or (share == "other" and i % 2) else ADDED for i in range(n)]
    assert [int(a) for a in r["point_action"][0]] == want


@pytest.mark.parametrize("first, second", ((WAVE - 1, WAVE), (T - 1, T), (0, T + WAVE)))
def test_twice_across_a_seam(ctx, first, second):
    """the first occurrence of a handle is found by the claim word, whatever wavefront or workgroup holds the second"""
    w = wide_world(T + WAVE + 1)
    for i in range(T + WAVE + 1):
        sc.put(w, POINT, 10, i, 1000 + i)
    sc.put(w, POINT, 10, second, 1000 + first)
    r, _, _ = three_ways(ctx, w, [10], read_back=False)
    a = [int(v) for v in r["point_action"][0]]
    assert a[first] == ADDED and a[second] == RECENT and a.count(RECENT) == 1
    assert [int(v) for v in r["recent_points"]] == [1000 + first]


@pytest.mark.parametrize("n_obs", (0, 1, WAVE, WAVE + 1, 300))
def test_stored_observers(ctx, n_obs):
    """a point with n_obs stored observers, in falling rank order, gains a key frame of the middle rank and one that it already
    holds; the normal runs over n_obs + 1 centres in one lane"""
    w = Store()
    w.scales = [1.0, 1.2]
    n_kfs = 304
    for k in range(n_kfs):
        w.add_kf(k + 1, n_kfs - k, 4, 2, stereo=[0, k % 2, 0, 0])      # ranks fall as handles rise
        w.set_pose(k + 1, ((k % 9) / 4.0, (k % 5) / 2.0, -(k % 3) / 8.0))
    sc.point(w, 100, [(k + 1, 1) for k in range(n_obs)], world=(0.125, 0.5, 4.0), ref=302, level=1)
    sc.put(w, POINT, 303, 1, 100)
    sc.put(w, POINT, 150 if n_obs < 150 else 303, 2, 100)
    if n_obs:
        sc.put(w, POINT, 1, 3, 100)                                     # observes it already, at index 1
    handles = [303, 1] if n_obs >= 150 else [303, 150, 1]
    r, _, _ = three_ways(ctx, w, handles, read_back=n_obs in (0, 300))
    assert len(r["added_points"]) == (1 if n_obs >= 150 else 2)
    assert len(w.items[POINT][100]["obs"]) == n_obs + len(r["added_points"])


@pytest.mark.parametrize("n_called", (1, 2, 65))
def test_called_key_frames_share_a_point(ctx, n_called):
    """every called key frame adds the same point: report t covers t + 2 observers, whatever the call order is against the ranks"""
    w = Store()
    w.scales = [1.0, 1.2]
    rng = np.random.default_rng(n_called)
    ranks = rng.permutation(n_called + 1) + 1
    for k in range(n_called + 1):
        w.add_kf(k + 1, int(ranks[k]), 3, 1, stereo=[k % 2, 0, 0])
        w.set_pose(k + 1, ((k % 7) / 4.0, (k % 4) / 2.0, 0.0))
    sc.point(w, 100, [(1, 0)], world=(0.25, 0.75, 5.0), ref=1)
    handles = [k + 1 for k in range(1, n_called + 1)]
    for h in handles:
        sc.put(w, POINT, h, 0, 100)
    r, _, _ = three_ways(ctx, w, handles, read_back=n_called == 65)
    assert len(r["added_points"]) == n_called and len(w.items[POINT][100]["obs"]) == n_called + 1


def test_scratch_budget(ctx):
    """the claim words go chunk after chunk under the configured scratch: one chunk, two, one key frame a chunk - the same bytes
    - and with one byte less the device entry refuses on the host, before any launch"""
    handles = [40, 20, 30]

    def world():
        v, _, _ = sc.two_and_three_callers()
        for i in range(9):                                              # claim words enough to tell the chunk sizes apart
            sc.point(v, 200 + i, [], ref=10)
        return v
    w = world()
    whole, least, fixed = store_of(w, ctx).insert_scratch(handles)
    n_items = len(w.items[POINT]) + len(w.items[LINE])
    assert fixed < least < whole and whole - fixed <= 3 * (LIM["claim_bytes"] * n_items + 32)
    for budget, chunks in ((whole, 1), (whole - 1, 2), (least, 3)):
        three_ways(ctx, world(), handles, chunks=chunks, configure=budget, read_back=False)
    dev = store_of(w, ctx)
    before = sc.state_of_store(dev, w)
    dev.configure(least - 1)
    assert "does not fit the configured device scratch" in refused(lambda: dev.insert(handles, mode="device"), lib.ERR_CAPACITY)
    assert sc.state_of_store(dev, w) == before and dev.insert_stats()["calls"] == 0
    sc.same_result(dev.insert(handles, mode="batch"), w.insert(handles))  # _batch is the host entry below the crossover
    assert dev.insert_stats()["device_calls"] == 0


def test_capacity_is_settled_before_the_launch(ctx):
    """the device commits as it goes: capacities below the bounds are settled by a walk of the host first"""
    w, handles, _ = sc.two_and_three_callers()
    dev = store_of(w, ctx)
    before = sc.state_of_store(dev, w)
    for cap in ((23, 24, 24), (24, 4, 24)):
        assert "returns more than" in refused(lambda: dev.insert(handles, mode="device", capacity=cap), lib.ERR_CAPACITY)
        assert sc.state_of_store(dev, w) == before
    sc.same_result(dev.insert(handles, mode="device", capacity=(24, 5, 0)), w.insert(handles))
    assert dev.insert_stats()["device_calls"] == 1


def test_batch_below_the_crossover(ctx):
    """DRFE_LMAP_INSERT_DEVICE_FROM stands above the longest call: _batch of a store with a context runs on the host"""
    assert LIM["device_from"] > LIM["max_keyframes"] * 4096
    w, handles, _ = sc.lines_mirror()
    dev = store_of(w, ctx)
    sc.same_result(dev.insert(handles, mode="batch"), w.insert(handles))
    assert dev.insert_stats()["device_calls"] == 0 and dev.insert_stats()["calls"] == 1


def test_what_travels_after_a_call(ctx):
    """The call adds to nObs in the resident blocks itself: the call sends no match rows and no graph, and the device calls
    after it only the observations with their offsets and indices - no match rows, no graph, no geometry, no counters."""
    rng = np.random.default_rng(78)
    pad = 4000
    w = sc.random_world(rng, n_kfs=8, n_points=60, n_lines=6, row=pad, line_row=8)
    called = sorted(w.kfs)[:3]
    sc.random_puts(rng, w, called, share=0.02)
    dev, host = store_of(w, ctx), store_of(w)
    pts, lns = sorted(w.items[POINT]), sorted(w.items[LINE])
    q, q2, q3 = ([dict(frame_id=next(FRAME_IDS), points=pts)] for _ in range(3))
    dev.update(q, mode="device")                                        # the rows and the graph are resident now
    host.update(q, mode="host")
    b0 = dev.upload_bytes()
    match_rows = 4 * 8 * pad
    assert b0["rows"] > match_rows and b0["graph"] > 0
    r = dev.insert(called, mode="device")
    sc.same_results(r, host.insert(called, mode="host"))
    assert len(r["added_points"]) > 20 and len(r["added_lines"]) > 0
    b1, c1 = dev.upload_bytes(), dev.recent_upload_bytes()
    assert b1["graph"] == b0["graph"] and b1["rows"] == b0["rows"]      # the rows were current: the call itself sent none
    a, b = dev.update(q2, mode="device"), host.update(q2, mode="host")
    assert all(np.array_equal(x, y) for key in a for x, y in zip(a[key], b[key]))
    b2 = dev.upload_bytes()
    total_obs = sum(len(p["obs"]) for p in w.items[POINT].values()) + len(r["added_points"])
    tail = 4 * (len(pts) + 1) + 4 * total_obs + 2 * 16                  # the offsets and the observations
    assert 0 < b2["rows"] - b1["rows"] <= tail < match_rows and b2["graph"] == b1["graph"] and b2["geometry"] == b1["geometry"]
    dev.update(q3, mode="device")
    assert dev.upload_bytes() == b2
    # a recent cull reads nObs of both kinds, which the call stored, and gets the spliced indices and line observations
    x, y = dev.recent_cull(7, pts[:10], lns, mode="device"), host.recent_cull(7, pts[:10], lns, mode="host")
    assert np.array_equal(x["points"]["action"], y["points"]["action"]) and np.array_equal(x["lines"]["action"], y["lines"]["action"])
    b3, c3 = dev.upload_bytes(), dev.recent_upload_bytes()
    assert 0 < b3["attributes"] - b1["attributes"] <= 4 * total_obs + 16   # the observation indices: no nObs, no stereo flags
    line_obs = sum(len(l["obs"]) for l in w.items[LINE].values()) + len(r["added_lines"])
    assert 0 < c3 - c1 <= 4 * (len(lns) + 1) + 8 * line_obs + 3 * 16    # the lines' offsets, observers and indices: no counters
    assert b3["graph"] == b1["graph"] and b3["geometry"] == b1["geometry"]


def test_native_caller_on_the_device_entry():
    """tests/native/insert_caller.cpp with every call forced onto the device entry: the same two worlds, the same records"""
    import subprocess
    import native_build
    exe = native_build.caller("insert_caller")
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "insert_caller device: ok, 218 points added" in p.stdout, (p.returncode, p.stdout, p.stderr)
