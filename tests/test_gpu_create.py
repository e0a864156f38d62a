"""GPU tests of the device entry of map-point and map-line creation (drfe_lmap_create_device, dr_slam_amd/csrc/create_kernels.hip,
DESIGN.md section 34): the same bytes, the same store afterwards and the same counters as the host entry and as
tests/create_numpy.py, on every hand-built store of tests/create_scenarios.py, on seeded scripts, and on shapes placed from
drfe_lmap_create_limits(): 0, 1, 63, 64, 65 and the tile's size - 1, + 0, + 1 creations with 1, 2 and alternating observer counts;
one row entry named by two creations across a wavefront seam and across a tile seam; a call that fills the granted room exactly
and one that needs a slot more; two calls in a row with nothing of the rows, the graph or the geometry travelling between them;
the scratch budget of one chunk, of two, and one byte less than the least; _batch below the crossover; and every other operation
on the device afterwards, which reads what the kernels wrote in place.  No test provokes a fault: every refused input is refused
on the host before a launch."""
import numpy as np
import pytest

import create_numpy as cn
import create_scenarios as sc
from dr_slam_amd import lib
from insert_numpy import Store
from test_create_cpu import FRAME_IDS, OPS, expected_stats, follow, refused, run_script, stats_less_relayouts, store_of

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.create_limits()
T, WAVE = LIM["tile"], LIM["wavefront"]
POINT, LINE = sc.POINT, sc.LINE


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def three_ways(ctx, w, points, lines, normals=True, read_back=True, chunks=None, configure=None):
    """a call on the device, on the host and in the restatement (which changes w)"""
    dev, host = store_of(w, ctx), store_of(w)
    if configure is not None:
        dev.configure(configure)
    r_dev = dev.create(points, lines, mode="device", normals=normals)
    r_host = host.create(points, lines, mode="host", normals=normals)
    sc.same_results(r_dev, r_host)
    want = cn.create(w, points, lines, normals=normals)
    sc.same_result(r_dev, want, normals=normals)
    for lm in (dev, host):
        sc.same_state(sc.state_of_store(lm, w), sc.state_of_world(w))
    if chunks is None:
        chunks = (1 if points else 0) + (1 if lines else 0)
    assert stats_less_relayouts(dev) == expected_stats(want, device=1 if chunks else 0, chunks=chunks)
    assert stats_less_relayouts(host) == expected_stats(want)
    assert dev.create_stats()["relayouts"] == host.create_stats()["relayouts"]
    if read_back:
        follow(dev, host, w, mode_a="device", mode_b="host")
        sc.same_state(sc.state_of_store(dev, w), sc.state_of_store(host, w))
    return r_dev, dev, host


@pytest.mark.parametrize("scenario", sc.SCENARIOS, ids=lambda f: f.__name__)
def test_scenarios_on_the_device(ctx, scenario):
    w, points, lines, expect = scenario()
    if expect["stale"]:
        # handles that do not qualify: no slot at the end for a kernel to write, so the device entry commits on the host
        dev = store_of(w, ctx)
        got = dev.create(points, lines, mode="device")
        sc.same_result(got, cn.create(w, points, lines))
        sc.same_state(sc.state_of_store(dev, w), sc.state_of_world(w))
        st = dev.create_stats()
        assert st["stale_calls"] == 1 and st["device_calls"] == 0
        follow(dev, store_of(w), w, mode_a="device")
        return
    r, _, _ = three_ways(ctx, w, points, lines)
    sc.check_expect(r, sc.state_of_world(w), expect)


@pytest.mark.parametrize("case", sc.refusals(), ids=lambda c: c[0])
def test_refusals_on_the_device_entry(ctx, case):
    """refused on the host, before any launch"""
    _, w, points, lines, normals, rc, word = case
    dev = store_of(w, ctx)
    before = sc.state_of_store(dev, w)
    assert word in refused(lambda: dev.create(points, lines, mode="device", normals=normals), rc)
    assert sc.state_of_store(dev, w) == before
    st = dev.create_stats()
    assert st["calls"] == 0 and st["device_calls"] == 0 and st["device_chunks"] == 0


@pytest.mark.parametrize("seed", (3431, 3432))
def test_seeded_scripts_on_the_device(ctx, seed):
    dev, twin, w = run_script(seed, ctx, mode="device")
    st = dev.create_stats()
    assert st["calls"] == len(OPS) + 1 and st["device_calls"] == len(OPS) + 1 and st["stale_calls"] == 0
    assert st["points_created"] > 0 and st["lines_created"] > 0 and st["displaced"] == twin.create_stats()["displaced"]
    follow(dev, twin, w, mode_a="device", seed=seed)


def wide_world(row, n_kfs=3, line_row=None):
    """key frames 10, 20, .. with point rows of `row` entries (every third a stereo keypoint, the octave of entry i is i % 3) and
    line rows of as many, and one stored point and line"""
    w = Store()
    w.scales = [1.0, 1.2, 1.44]
    for k in range(n_kfs):
        h = 10 * (k + 1)
        w.add_kf(h, n_kfs - k, row, row if line_row is None else line_row, stereo=[int(i % 3 == 0) for i in range(row)])
        w.kfs[h]["octave"] = [i % 3 for i in range(row)]
        w.set_pose(h, (0.5 * k, 0.25, 0.0))
    sc.ins.point(w, 100, [(10, 0)], world=(1.0, 2.0, 3.0), ref=10)
    w.add_item(LINE, 500, [(10, 0)])
    return w


def creations(n, observers, row, first=1000, shift=1):
    """n creations on distinct entries of key frames 10, 20 (and 30); observers: 1, 2 or "alt" (1, 2, 1, ..)"""
    pts, lns = [], []
    for t in range(n):
        m = observers if observers != "alt" else 1 + t % 2
        obs = [(20, (t + shift) % row), (10, (t + shift) % row)][:m] if t % 3 else [(30, (t + shift) % row), (20, (t + shift) % row)][:m]
        pts.append(sc.pt(first + t, obs, ref=obs[-1][0], world=(0.5 + t % 7, 1.0 + t % 5, 3.0), first_kf=t))
        lns.append(sc.ln(first + t, obs, ref=obs[0][0], first_kf=t))
    return pts, lns


@pytest.mark.parametrize("n", (0, 1, WAVE - 1, WAVE, WAVE + 1, T - 1, T, T + 1))
@pytest.mark.parametrize("observers", (1, 2, "alt"))
def test_call_sizes(ctx, n, observers):
    """the scanned observation offsets differ from the creation index as soon as one creation has two observers; the offsets of
    the new slots cross wavefronts and workgroups"""
    w = wide_world(T + 2)
    pts, lns = creations(n, observers, T + 2)
    r, dev, _ = three_ways(ctx, w, pts, lns, read_back=False)
    for h in (c["handle"] for c in pts[-2:]):
        want = 1 if observers == 1 or (observers == "alt" and (h - 1000) % 2 == 0) else 2
        assert len(dev.get_observers(POINT, h)[1]) == want


@pytest.mark.parametrize("first, second", ((WAVE - 1, WAVE), (T - 1, T), (0, T // 2 + WAVE)))
def test_one_entry_across_a_seam(ctx, first, second):
    """creations `first` and `second` name the same row entry, as the observation entries (two per creation) of different
    wavefronts and workgroups: the later holds the row and reports the earlier"""
    n = T + WAVE + 1
    w = wide_world(n + 1)
    pts, lns = creations(n, 2, n + 1)
    for cs in (pts, lns):
        cs[second]["obs"][0] = cs[first]["obs"][0]
        cs[second]["ref_kf"] = cs[second]["obs"][1][0]
    r, dev, _ = three_ways(ctx, w, pts, lns, read_back=False)
    k, i = pts[first]["obs"][0]
    assert int(r["point_displaced"][second][0]) == 1000 + first and int(r["line_displaced"][second][0]) == 1000 + first
    assert int(dev.get_match_row(POINT, k)[i]) == 1000 + second and int(dev.get_match_row(LINE, k)[i]) == 1000 + second


def test_filling_the_room_and_one_more(ctx):
    """the first call of n creations leaves room for 2 (stored + n) slots: a second call that fills it exactly lays nothing out
    anew, and the next creation does, once"""
    w = wide_world(T)
    dev, host = store_of(w, ctx), store_of(w)

    def call(n, first, shift):
        pts, lns = creations(n, 1, T, first=first, shift=shift)
        a, b = dev.create(pts, lns, mode="device"), host.create(pts, lns, mode="host")
        sc.same_results(a, b)
        sc.same_result(a, cn.create(w, pts, lns))
        return dev.create_stats()["relayouts"]
    n = 20
    assert call(n, 1000, 1) == 4                                        # rows, attributes, recent list, geometry
    room = 2 * (1 + n) - (1 + n)                                        # slots left behind the stored ones
    before = dev.upload_bytes()
    assert call(room, 2000, 1 + n) == 4
    after = dev.upload_bytes()
    assert {k: after[k] - before[k] for k in ("rows", "graph", "geometry", "attributes")} == dict(rows=0, graph=0, geometry=0, attributes=0)
    assert call(1, 3000, 1 + n + room) == 8
    assert host.create_stats()["relayouts"] == 8
    sc.same_state(sc.state_of_store(dev, w), sc.state_of_world(w))
    follow(dev, host, w, mode_a="device")


def test_two_calls_in_a_row_upload_nothing(ctx):
    """the second call appends behind the first in the resident blocks: no rows, graph or geometry traffic between them, nor with
    the update that follows on the device"""
    w = wide_world(T)
    dev = store_of(w, ctx)
    pts, lns = creations(40, "alt", T)
    dev.create(pts, lns, mode="device")
    cn.create(w, pts, lns)
    before, rec = dev.upload_bytes(), dev.recent_upload_bytes()
    pts, lns = creations(30, "alt", T, first=2000, shift=50)
    sc.same_result(dev.create(pts, lns, mode="device"), cn.create(w, pts, lns))
    q = [dict(frame_id=next(FRAME_IDS), points=sorted(w.items[POINT]), lines=sorted(w.items[LINE]))]
    got = dev.update(q, mode="device")
    after = dev.upload_bytes()
    assert after == before and dev.recent_upload_bytes() == rec
    want = store_of(w).update(q, mode="host")
    for key in got:
        assert all(np.array_equal(x, y) for x, y in zip(got[key], want[key])), key
    assert dev.create_stats()["device_calls"] == 2


def test_host_entry_then_device_call_uploads_the_tails(ctx):
    """after a host create the next device call sends the appended tails and the touched row entries, not the blocks"""
    w = wide_world(T)
    dev = store_of(w, ctx)
    pts, lns = creations(10, 2, T)
    dev.create(pts, lns, mode="host")
    cn.create(w, pts, lns)
    dev.update([dict(frame_id=next(FRAME_IDS), points=sorted(w.items[POINT]), lines=sorted(w.items[LINE]))], mode="device")
    before = dev.upload_bytes()
    pts, lns = creations(10, 2, T, first=2000, shift=20)
    dev.create(pts, lns, mode="host")
    cn.create(w, pts, lns)
    q = [dict(frame_id=next(FRAME_IDS), points=sorted(w.items[POINT]), lines=sorted(w.items[LINE]))]
    got = dev.update(q, mode="device")
    sent = dev.upload_bytes()["rows"] - before["rows"]
    # 10 bad flags of each kind, 10 offsets, 20 observations, 40 row entries
    assert sent == 10 + 10 + 4 * 10 + 4 * 20 + 4 * 40 and dev.upload_bytes()["graph"] == before["graph"]
    want = store_of(w).update(q, mode="host")
    for key in got:
        assert all(np.array_equal(x, y) for x, y in zip(got[key], want[key])), key


def test_scratch_budgets(ctx):
    """one chunk a kind, two, one tile a chunk, and one byte less than that"""
    n = 2 * T + 5
    w = wide_world(n + 1)
    whole, least, shared = store_of(w, ctx).create_scratch(n, n)
    assert whole > least > shared and least == store_of(w, ctx).create_scratch(T, T)[0]
    pts, lns = creations(n, "alt", n + 1)
    three_ways(ctx, wide_world(n + 1), pts, lns, read_back=False, chunks=2, configure=whole)
    two = store_of(w, ctx).create_scratch(2 * T, 2 * T)[0]
    three_ways(ctx, wide_world(n + 1), pts, lns, read_back=False, chunks=4, configure=two)
    w3 = wide_world(n + 1)
    _, dev, host = three_ways(ctx, w3, pts, lns, read_back=False, chunks=6, configure=least)
    dev.configure(1 << 30)                                              # the other operations need their own scratch
    follow(dev, host, w3, mode_a="device")
    dev = store_of(w, ctx)
    dev.configure(least - 1)
    before = sc.state_of_store(dev, w)
    assert "scratch" in refused(lambda: dev.create(pts, lns, mode="device"), lib.ERR_CAPACITY)
    assert sc.state_of_store(dev, w) == before and dev.create_stats()["calls"] == 0


def test_batch_below_the_crossover_runs_on_the_host(ctx):
    w = wide_world(T)
    dev = store_of(w, ctx)
    pts, lns = creations(12, 2, T)
    sc.same_result(dev.create(pts, lns, mode="batch"), cn.create(w, pts, lns))
    st = dev.create_stats()
    assert st["calls"] == 1 and st["device_calls"] == 0 and LIM["device_from"] > 12


def test_native_caller_on_the_device_entry():
    """tests/native/create_caller.cpp with every call forced onto the device entry: the same two worlds, the same records"""
    import subprocess
    import native_build
    exe = native_build.caller("create_caller")
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "create_caller device: ok, 265 points created" in p.stdout, (p.returncode, p.stdout, p.stderr)
