"""GPU tests of the device entry of the map update that ends LoopClosing::RunGlobalBundleAdjustment (drfe_lmap_gba_device,
dr_slam_amd/csrc/gba_kernels.hip): the same bytes, the same store afterwards through every getter and the
same counters as the host entry and as tests/gba_propagate_numpy.py, on every hand-built map of tests/gba_propagate_scenarios.py,
on seeded scripts, and on shapes placed from drfe_lmap_gba_limits(): point counts around a wavefront and a workgroup with none, all
and alternate points moving; unstamped chains of depth 0, 1, 2 and 300, a round wider than a workgroup and two chains of different
depth under one parent; the scratch budget of one chunk, of two, and one byte less; the commit in place; every refusal."""
import os
import re
import subprocess

import numpy as np
import pytest

import gba_propagate_numpy as gn
import gba_propagate_scenarios as gs
import lmap_numpy as ln
import loop_correct_numpy as rn
from dr_slam_amd import lib
from test_gba_propagate_cpu import RC

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.gba_limits()
WG, WAVE = LIM["threads"], LIM["wavefront"]


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        (gn.same_gba if "composed" in x else rn.same_correct)(x, y)


def three_ways(ctx, ops, configure=None, restate=True, mode="device"):
    """a script on the device, on the host and in the restatement: equal results, equal stores through every getter, equal
    counters; returns the device's results and store"""
    host = lib.LocalMap()
    r_host = gs.play(ops, host)
    dev = lib.LocalMap(ctx)
    if configure:
        dev.configure(configure)
    r_dev = gs.play(ops, dev, mode=mode)
    same_results(r_dev, r_host)
    sd, sh = dev.gba_stats(), host.gba_stats()
    assert {k: v for k, v in sd.items() if k != "device_calls"} == {k: v for k, v in sh.items() if k != "device_calls"}
    if mode == "device":
        assert sd["device_calls"] == sum(1 for op in ops if op[0] == "gba") and sh["device_calls"] == 0
    kfs, pts = gs.alive(ops)
    gn.same_store(dev, host, kfs, pts)
    if restate:
        ref = gn.Store()
        same_results(r_dev, gs.play(ops, ref))
        assert all(sd[k] == v for k, v in ref.gcounts.items())
        gn.same_store(dev, ref, kfs, pts)
    return r_dev, dev


@pytest.mark.parametrize("name", sorted(gs.HAND))
def test_hand_built(ctx, name):
    ops, expect = gs.HAND[name]()
    r, _ = three_ways(ctx, ops)
    gs.check(r, expect)


def test_children_are_walked_in_rank_order(ctx):
    for ops, expect in gs.sibling_orders():
        r, _ = three_ways(ctx, ops)
        gs.check(r, expect)


POINT_COUNTS = sorted({1, WAVE - 1, WAVE, WAVE + 1, WG - 1, WG, WG + 1, 2 * WG + 1})


@pytest.mark.parametrize("moving", ["none", "all", "alternate"])
@pytest.mark.parametrize("n", POINT_COUNTS)
def test_point_counts_at_the_seams(ctx, n, moving):
    r, _ = three_ways(ctx, gs.points_shape(n, moving, seed=n))
    want = 0 if moving == "none" else n if moving == "all" else (n + 1) // 2
    assert len(r[0]["points"]) == want and list(r[0]["points"]) == sorted(r[0]["points"])


def depths():
    d = [0, 1, 2, 300]
    if LIM["depth_limit"] > 0:
        d += [LIM["depth_limit"] - 1, LIM["depth_limit"], LIM["depth_limit"] + 1]
    return sorted(set(d))


@pytest.mark.parametrize("depth", depths())
def test_unstamped_chain_depth(ctx, depth):
    r, dev = three_ways(ctx, gs.chain_shape([depth] if depth else [], seed=depth))
    assert dev.gba_stats()["deepest_chain"] == depth and int(r[0]["composed"].sum()) == depth


def test_a_round_wider_than_a_workgroup(ctx):
    r, dev = three_ways(ctx, gs.chain_shape([], seed=5, siblings=WG + 1))
    assert int(r[0]["composed"].sum()) == WG + 1 and dev.gba_stats()["deepest_chain"] == 1


def test_two_chains_of_different_depth_under_one_parent(ctx):
    r, dev = three_ways(ctx, gs.chain_shape([2, 5], seed=6, siblings=3))
    assert int(r[0]["composed"].sum()) == 10 and dev.gba_stats()["deepest_chain"] == 5


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_scripts(ctx, seed):
    r, dev = three_ways(ctx, gs.seeded(seed))
    assert dev.gba_stats()["device_calls"] == 3


def test_scratch_budget_one_chunk_two_chunks_and_one_byte_less(ctx):
    n = 2 * WG + 1
    ops = gs.points_shape(n, "alternate", seed=9)
    probe = lib.LocalMap()
    gs.play(ops[:-1], probe)
    whole, least, fixed = probe.gba_scratch()
    assert whole == fixed + LIM["point_bytes"] * n and least == fixed + LIM["point_bytes"] and fixed == LIM["fixed_bytes"]
    three_ways(ctx, ops, configure=whole)
    three_ways(ctx, ops, configure=fixed + LIM["point_bytes"] * ((n + 1) // 2))
    three_ways(ctx, ops, configure=fixed + LIM["point_bytes"] * (WG + 3))          # chunks that end inside a workgroup
    dev = lib.LocalMap(ctx)
    dev.configure(least - 1)
    gs.play(ops[:-1], dev)
    kfs, pts = gs.alive(ops)
    before = gn.snapshot(dev, kfs, pts)
    with pytest.raises(lib.DrfeError) as e:
        dev.gba(4, [1], mode="device")
    assert e.value.rc == lib.ERR_CAPACITY
    gn.same_snapshot(before, gn.snapshot(dev, kfs, pts))
    assert dev.gba_stats()["calls"] == 0


def test_commit_in_place_is_what_later_device_calls_read(ctx):
    ops = gs.seeded(4)
    first = next(i for i, op in enumerate(ops) if op[0] == "gba")
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    gs.play(ops[:first - 2], dev)
    gs.play(ops[:first - 2], host)
    rows = {r["handle"]: r for r in ops[0][1]}
    q = [dict(frame_id=77, points=rows[3]["points"])]
    ln.same(dev.update(q, mode="device"), host.update(q, mode="host"))              # the image becomes resident
    S = np.array([0, 0, 0, 1, 0.5, 0, 0, 1.0])
    rn.same_correct(dev.correct(2, S, [1, 2, 3], mode="device"), host.correct(2, S, [1, 2, 3], mode="host"))   # and the geometry
    gs.play(ops[first - 2:first], dev)
    gs.play(ops[first - 2:first], host)
    up0 = dev.upload_bytes()
    gn.same_gba(dev.gba(11, [1], mode="device"), host.gba(11, [1], mode="host"))
    up1 = dev.upload_bytes()
    assert all(up1[k] == up0[k] for k in ("rows", "graph", "geometry", "attributes")) and up1["gba"] > up0["gba"]
    called = [1, 2, 3, 5, 8, 13]
    rn.same_correct(dev.correct(5, S, called, mode="device"), host.correct(5, S, called, mode="host"))
    q[0]["frame_id"] = 78
    ln.same(dev.update(q, mode="device"), host.update(q, mode="host"))
    assert dev.upload_bytes() == up1                                                # nothing the call wrote went up again
    dev.set_gba_points([1000], [(1, 2, 3)], [12])                                   # an edit of the state sends its block alone
    dev.set_gba_keyframes([1], [gs.pose()], [12])
    host.set_gba_points([1000], [(1, 2, 3)], [12])
    host.set_gba_keyframes([1], [gs.pose()], [12])
    gn.same_gba(dev.gba(12, [1], mode="device"), host.gba(12, [1], mode="host"))
    up2 = dev.upload_bytes()
    assert all(up2[k] == up1[k] for k in ("rows", "graph", "geometry", "attributes")) and up2["gba"] > up1["gba"]
    kfs, pts = gs.alive(ops)
    gn.same_store(dev, host, kfs, pts)


def test_host_and_device_calls_interleaved(ctx):
    ops = gs.seeded(5)
    dev, ref = lib.LocalMap(ctx), gn.Store()
    modes = iter(["device", "host", "device"])
    kfs, pts = gs.alive(ops)
    for op in ops:
        mode = next(modes) if op[0] == "gba" else "device"
        same_results(gs.play([op], dev, mode=mode), gs.play([op], ref))
        if op[0] == "gba":
            gn.same_store(dev, ref, kfs, pts)
    assert dev.gba_stats()["device_calls"] == 2


def test_batch_uses_the_device_from_the_crossover(ctx):
    if LIM["device_from"] >= 2 ** 31 - 1:
        pytest.skip("DRFE_LMAP_GBA_DEVICE_FROM is beyond any store: the device entry did not win at every stamp mix, _batch stays on the host")
    n = LIM["device_from"]
    for count, want in ((n - 1, 0), (n, 1)):
        ops = gs.many_points(count, seed=3)
        dev, host = lib.LocalMap(ctx), lib.LocalMap()
        gn.same_gba(gs.play(ops, dev, mode="batch")[0], gs.play(ops, host)[0])
        assert dev.gba_stats()["device_calls"] == want
        gn.same_store(dev, host, [1, 2, 3], [100, 101, 100 + count // 2, 99 + count])


def test_batch_stays_on_the_host_below_the_crossover(ctx):
    _, dev = three_ways(ctx, gs.points_shape(WG + 1, "all", seed=3), mode="batch", restate=False)
    assert dev.gba_stats()["device_calls"] == (1 if LIM["device_from"] <= WG + 1 else 0)


@pytest.mark.parametrize("case", gs.refusals(), ids=lambda c: c[0])
def test_refusals_on_the_device_entry(ctx, case):
    name, ops, (loop, origins), rc, handle = case
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    gs.play(ops, dev, mode="device")
    gs.play(ops, host)
    kfs, pts = gs.alive(ops)
    before, st, up = gn.snapshot(dev, kfs, pts), dev.gba_stats(), dev.upload_bytes()
    with pytest.raises(lib.DrfeError) as e:
        dev.gba(loop, origins, mode="device")
    with pytest.raises(lib.DrfeError) as f:
        host.gba(loop, origins, mode="host")
    assert e.value.rc == f.value.rc == RC[rc] and str(e.value).split(":", 1)[1] == str(f.value).split(":", 1)[1]
    if handle is not None:
        assert re.search(rf"\b{handle}\b", str(e.value))
    gn.same_snapshot(before, gn.snapshot(dev, kfs, pts))
    assert dev.gba_stats() == st and dev.upload_bytes() == up


def test_native_caller_on_the_device_entry():
    """tests/native/gba_propagate_caller.cpp with the adaptor forced onto the device entry"""
    exe = os.path.join(lib._HERE, "..", "tests", "native", "gba_propagate_caller")
    assert os.path.exists(exe), "build() makes it"
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout
