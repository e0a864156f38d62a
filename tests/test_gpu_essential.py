"""GPU tests of the device entries of what surrounds the solver of Optimizer::OptimizeEssentialGraph
(drfe_lmap_essential_edges_device, drfe_lmap_essential_commit_device, dr_slam_amd/csrc/essential_kernels.hip, DESIGN.md section
35): the same bytes, the same store afterwards through every getter and the same counters as the host entries and as
tests/essential_numpy.py, on every hand-built map of tests/essential_scenarios.py, on seeded scripts, and on shapes placed from
drfe_lmap_essential_limits(): key-frame counts around a wavefront and above a workgroup, ordered-row prefixes around a wavefront
with alternate entries dropped, point counts around a wavefront and a workgroup, the scratch budget of one chunk, of two, and one
byte less; the commit in place; every refusal; the native caller."""
import os
import re
import subprocess

import numpy as np
import pytest

import essential_numpy as en
import essential_scenarios as es
import lmap_numpy as ln
from dr_slam_amd import lib
from test_essential_cpu import RC, chain

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.essential_limits()
WG, WAVE = LIM["threads"], LIM["wavefront"]
ESSENTIAL = ("essential_edges", "essential_commit")


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        en.same_result(x, y)


def three_ways(ctx, ops, configure=None, restate=True, mode="device"):
    """a script on the device, on the host and in the restatement: equal results, equal stores through every getter, equal
    counters; returns the device's results and store"""
    host = lib.LocalMap()
    r_host = es.play(ops, host)
    dev = lib.LocalMap(ctx)
    if configure:
        dev.configure(configure)
    r_dev = es.play(ops, dev, mode=mode)
    same_results(r_dev, r_host)
    sd, sh = dev.essential_stats(), host.essential_stats()
    assert {k: v for k, v in sd.items() if k != "device_calls"} == {k: v for k, v in sh.items() if k != "device_calls"}
    if mode == "device":
        assert sd["device_calls"] == sum(1 for op in ops if op[0] in ESSENTIAL) and sh["device_calls"] == 0
    kfs, pts = es.alive(ops)
    en.same_store(dev, host, kfs, pts)
    if restate:
        ref = en.Store()
        same_results(r_dev, es.play(ops, ref))
        assert all(sd[k] == v for k, v in ref.ecounts.items())
        en.same_store(dev, ref, kfs, pts)
    return r_dev, dev


@pytest.mark.parametrize("name", sorted(es.HAND_EDGES))
def test_hand_built_edges(ctx, name):
    ops, expect, counts = es.HAND_EDGES[name]()
    r, dev = three_ways(ctx, ops)
    es.check(r, expect)
    assert all(dev.essential_stats()[k] == v for k, v in counts.items())


def test_hand_built_commit(ctx):
    ops, expect, counts, state = es.commit_points()
    r, dev = three_ways(ctx, ops)
    es.check(r, expect)
    es.check_state(dev, state)
    assert all(dev.essential_stats()[k] == v for k, v in counts.items())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_scripts(ctx, seed):
    r, dev = three_ways(ctx, es.seeded(seed))
    assert dev.essential_stats()["device_calls"] == 3


@pytest.mark.parametrize("n", sorted({1, 2, WAVE - 1, WAVE, WAVE + 1, WG + 1}))
def test_key_frame_counts_at_the_seams(ctx, n):
    r, _ = three_ways(ctx, es.script(n, 8, seed=n, n_bad=1))
    assert len(r[0]["vertices"]) == n and len(r[1]["Tiw"]) == n


@pytest.mark.parametrize("prefix", sorted({0, 1, WAVE - 1, WAVE, WAVE + 1}))
def test_ordered_row_prefixes_at_the_seams(ctx, prefix):
    """every row is `prefix` entries at 100 or more and one below; alternate entries drop, so ballot ranks cross words"""
    r, _ = three_ways(ctx, es.script(WAVE + 6, 4, seed=100 + prefix, prefix=prefix, n_bad=2))
    covis = int((r[0]["kind"] == es.COVIS).sum())
    assert covis <= (WAVE + 6) * ((prefix + 1) // 2 + 1) and (prefix < 2 or covis > 0)


@pytest.mark.parametrize("n", sorted({1, WAVE - 1, WAVE + 1, WG - 1, WG + 1, 2 * WG + 1}))
def test_point_counts_at_the_seams(ctx, n):
    r, _ = three_ways(ctx, es.script(5, n, seed=200 + n, n_bad=1))
    pts = r[1]["points"]
    assert len(pts) == n - sum(1 for k in range(n) if k % 7 == 3) and list(pts) == sorted(pts)


def commit_script(n_kf, n_pt, seed):
    s = es.script(n_kf, n_pt, seed, n_bad=1)
    return s[:-3] + [s[-2]]


def test_commit_scratch_one_chunk_two_chunks_and_one_byte_less(ctx):
    n = 2 * WG + 1
    ops = commit_script(6, n, seed=9)
    probe = lib.LocalMap()
    es.play(ops[:-1], probe)
    s = probe.essential_scratch()
    whole, least, fixed = s["commit_whole"], s["commit_least"], s["commit_fixed"]
    assert whole == fixed + LIM["point_bytes"] * n and least == fixed + LIM["point_bytes"] and fixed > LIM["kf_bytes"] * 7
    three_ways(ctx, ops, configure=whole)
    three_ways(ctx, ops, configure=fixed + LIM["point_bytes"] * ((n + 1) // 2))
    three_ways(ctx, ops, configure=fixed + LIM["point_bytes"] * (WG + 3))           # chunks that end inside a workgroup
    dev = lib.LocalMap(ctx)
    dev.configure(least - 1)
    es.play(ops[:-1], dev)
    kfs, pts = es.alive(ops)
    before = en.snapshot(dev, kfs, pts)
    with pytest.raises(lib.DrfeError) as e:
        es.call(dev, ops[-1], mode="device")
    assert e.value.rc == lib.ERR_CAPACITY
    en.gn.same_snapshot(before, en.snapshot(dev, kfs, pts))
    assert dev.essential_stats()["commit_calls"] == 0
    host = lib.LocalMap()
    es.play(ops[:-1], host)
    en.same_commit(es.call(dev, ops[-1], mode="batch"), es.call(host, ops[-1]))      # _batch runs it on the host
    assert dev.essential_stats()["device_calls"] == 0 and dev.essential_stats()["commit_calls"] == 1
    en.same_store(dev, host, kfs, pts)


def test_edges_scratch_and_one_byte_less(ctx):
    s = es.script(WAVE + 1, 4, seed=11, n_bad=1)
    ops, edges = s[:-3], s[-3]
    probe = lib.LocalMap()
    es.play(ops, probe)
    sc = probe.essential_scratch(sum(len(ms) for _, ms in edges[4]))
    assert sc["edges"] == sc["edges_fixed"] + LIM["edge_bytes"] * sc["edge_bound"]
    three_ways(ctx, ops + [edges], configure=sc["edges"])
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    dev.configure(sc["edges"] - 1)
    es.play(ops, dev)
    es.play(ops, host)
    with pytest.raises(lib.DrfeError) as e:
        es.call(dev, edges, mode="device")
    assert e.value.rc == lib.ERR_CAPACITY and dev.essential_stats()["edges_calls"] == 0
    en.same_edges(es.call(dev, edges, mode="batch"), es.call(host, edges))
    assert dev.essential_stats()["device_calls"] == 0


def test_commit_in_place_is_what_later_device_calls_read(ctx):
    s = es.script(9, 60, seed=4, n_bad=2)
    ops, edges, commit = s[:-3], s[-3], s[-2]
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    es.play(ops, dev)
    es.play(ops, host)
    pts = [r["handle"] for op in ops if op[0] == "points" for r in op[1]]
    root = next(r["handle"] for r in ops[0][1] if r["parent"] == -1 and not r["bad"])
    q = [dict(frame_id=77, points=pts[:9])]
    ln.same(dev.update(q, mode="device"), host.update(q, mode="host"))               # the image becomes resident
    en.same_edges(es.call(dev, edges, mode="device"), es.call(host, edges))          # the geometry and the loop edges too
    up0, le0 = dev.upload_bytes(), dev.essential_upload_bytes()
    assert up0["geometry"] > 0 and le0 > 0
    en.same_commit(es.call(dev, commit, mode="device"), es.call(host, commit))
    assert dev.upload_bytes() == up0 and dev.essential_upload_bytes() == le0         # everything it read was resident
    q[0]["frame_id"] = 78
    ln.same(dev.update(q, mode="device"), host.update(q, mode="host"))
    for st in (dev, host):
        st.set_gba_keyframes([root], st.get_poses([root])["Tcw"], [edges[2]])
    en.gn.same_gba(dev.gba(edges[2], [root], mode="device"), host.gba(edges[2], [root], mode="host"))
    up1 = dev.upload_bytes()
    assert all(up1[k] == up0[k] for k in ("rows", "graph", "geometry", "attributes")) and up1["gba"] > up0["gba"]
    en.same_edges(es.call(dev, edges, mode="device"), es.call(host, edges))          # the edges read the moved poses in place
    assert dev.upload_bytes() == up1 and dev.essential_upload_bytes() == le0
    dev.set_loop_edges([(root, [edges[2]])])                                         # an edit of the loop edges sends its block alone
    host.set_loop_edges([(root, [edges[2]])])
    en.same_edges(es.call(dev, edges, mode="device"), es.call(host, edges))
    assert dev.upload_bytes() == up1 and dev.essential_upload_bytes() > le0
    kfs, allpts = es.alive(ops)
    en.same_store(dev, host, kfs, allpts)


def test_a_loop_closure_chained_on_the_device(ctx):
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    r_dev, lcs, kfs, pts = chain(dev, mode="device")
    r_host, lcs_host, _, _ = chain(host)
    assert lcs == lcs_host
    same_results(r_dev, r_host)
    en.same_store(dev, host, kfs, pts)
    assert dev.essential_stats()["device_calls"] == 3


def test_batch_follows_the_crossovers(ctx):
    n_bad = 1
    ops = es.script(WAVE, WG + 1, seed=3, n_bad=n_bad)
    _, dev = three_ways(ctx, ops, mode="batch", restate=False)
    stored_kfs, stored_pts = dev.size()[:2]
    assert (stored_kfs, stored_pts) == (WAVE + n_bad, WG + 1)
    want = 2 * (LIM["edges_device_from"] <= stored_kfs) + (LIM["commit_device_from"] <= stored_pts)
    assert dev.essential_stats()["device_calls"] == want


def cheap_points(n, seed):
    """three key frames and n points without observations, a seventh of them bad: a commit that only moves"""
    rng = np.random.default_rng(seed)
    pts = list(range(1000, 1000 + n))
    ops = [("kfs", [es.kf(1, ch=[2, 3]), es.kf(2, parent=1), es.kf(3, parent=1)]), ("scales", es.SCALES),
           ("poses", [1, 2, 3], [es.rand_pose(rng) for _ in range(3)]),
           ("points", [es.ls.mp(p, bad=int(k % 7 == 3)) for k, p in enumerate(pts)])]
    X = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    ops.append(("geo", [es.geo(p, X[k], 1 + k % 3, by=3 if k % 2 else 0, byref=1 + k % 2) for k, p in enumerate(pts)]))
    commit = ("essential_commit", 3, [3, 1, 2], [es.rand_sim3(rng) for _ in range(3)], [es.rand_sim3(rng) for _ in range(3)])
    return ops, commit, pts


def test_commit_batch_takes_the_device_from_the_crossover_and_the_host_when_the_scratch_is_short(ctx):
    n = LIM["commit_device_from"]
    assert n < 2 ** 31 - 1, "profiles/essential_timing.jsonl gives a crossover: the device entry wins from it"
    for count, want in ((n - 1, 0), (n, 1)):
        ops, commit, pts = cheap_points(count, seed=5)
        dev, host = lib.LocalMap(ctx), lib.LocalMap()
        es.play(ops, dev)
        es.play(ops, host)
        en.same_commit(es.call(dev, commit, mode="batch"), es.call(host, commit))
        assert dev.essential_stats()["device_calls"] == want
        en.same_store(dev, host, [1, 2, 3], pts[:3] + pts[count // 2:count // 2 + 3] + pts[-3:])
    # the same call above the crossover with a scratch one byte short of one point slot: _batch runs it on the host
    ops, commit, pts = cheap_points(n, seed=6)
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    es.play(ops, dev)
    es.play(ops, host)
    dev.configure(dev.essential_scratch()["commit_least"] - 1)
    en.same_commit(es.call(dev, commit, mode="batch"), es.call(host, commit))
    assert dev.essential_stats()["device_calls"] == 0 and dev.essential_stats()["commit_calls"] == 1
    # and with room for a third of the points a chunk it runs on the device, in three chunks
    s = dev.essential_scratch()
    dev.configure(s["commit_fixed"] + LIM["point_bytes"] * ((n + 2) // 3))
    en.same_commit(es.call(dev, commit, mode="batch"), es.call(host, commit))
    assert dev.essential_stats()["device_calls"] == 1
    en.same_store(dev, host, [1, 2, 3], pts[:3] + pts[-3:])


@pytest.mark.parametrize("case", es.refusals(), ids=lambda c: c[0])
def test_refusals_on_the_device_entries(ctx, case):
    name, ops, op, rc, handle = case
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    es.play(ops, dev, mode="device")
    es.play(ops, host)
    kfs, pts = es.alive(ops)
    before, st, up = en.snapshot(dev, kfs, pts), dev.essential_stats(), dev.upload_bytes()
    with pytest.raises(lib.DrfeError) as e:
        es.call(dev, op, mode="device")
    with pytest.raises(lib.DrfeError) as f:
        es.call(host, op)
    assert e.value.rc == f.value.rc == RC[rc] and str(e.value).split(":", 1)[1] == str(f.value).split(":", 1)[1]
    if handle is not None:
        assert re.search(rf"\b{handle}\b", str(e.value).split(":", 1)[1])
    en.gn.same_snapshot(before, en.snapshot(dev, kfs, pts))
    assert dev.essential_stats() == st
    if name != "edges_capacity_short":                                               # that one is known only after the plan launches
        assert dev.upload_bytes() == up


def test_native_caller_on_the_device_entries():
    """tests/native/essential_caller.cpp with the adaptor forced onto the device entries"""
    exe = os.path.join(lib._HERE, "..", "tests", "native", "essential_caller")
    assert os.path.exists(exe), "build() makes it"
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout
