"""GPU tests of the device entry of LocalMapping::MapPointCulling and MapLineCulling (drfe_lmap_recent_cull_device,
dr_slam_amd/csrc/recent_kernels.hip): the same bytes, the same store afterwards (through the getters and a
following update, connect and cull on the device, which read the resident image the kernels stored into) and the same counters
as the host entry and as tests/recent_cull_numpy.py, on every hand-built store of tests/recent_cull_scenarios.py, on seeded
scripts with edits, and on shapes placed from drfe_lmap_recent_cull_limits(): lists of 0, 1, 63, 64, 65 and the workgroup's size
- 1, + 0, + 1 entries with all, none and every other entry culled; a handle twice across a wavefront seam and across a workgroup
seam; items with 0, 1, 64, 65 and 300 observers; erased observations of the erase tile's size - 1, + 0, + 1; the scratch budget
of one chunk, of two, of one entry a chunk, and one byte less; and the bytes that travel after a call."""
import numpy as np
import pytest

import cull_numpy as un
import recent_cull_numpy as rn
import recent_cull_scenarios as rs
from dr_slam_amd import lib
from test_recent_cull_cpu import rows_of, same_counters, same_results, same_store

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.recent_cull_limits()
T, ET, EB, WAVE = LIM["entry_tile"], LIM["erase_tile"], LIM["entry_bytes"], LIM["wavefront"]
POINT, LINE, CUR = rs.POINT, rs.LINE, rs.CUR


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def three_ways(ctx, ops, configure=None, mode="device"):
    """a script on the device, on the host and in the restatement: equal results, equal stores, equal counters; then a cull, an
    update and a connect on the device against the restatement's.  Returns the device's results and store."""
    host = lib.LocalMap()
    r_host = rs.play(ops, host)
    dev = lib.LocalMap(ctx)
    if configure:
        dev.configure(configure)
    r_dev = rs.play(ops, dev, mode=mode)
    same_results(r_dev, r_host)
    sd, sh = dev.recent_cull_stats(), host.recent_cull_stats()
    assert {k: v for k, v in sd.items() if k != "device_calls"} == {k: v for k, v in sh.items() if k != "device_calls"}
    n_calls = sum(1 for op in ops if op[0] == "rcull" and (len(op[2]) or len(op[3])))
    if mode == "device":
        assert sd["device_calls"] == n_calls and sh["device_calls"] == 0
    ref = rn.Store()
    same_results(r_dev, rs.play(ops, ref))
    same_counters(dev, ref)
    if configure:
        dev.configure(1 << 30)                                          # the budget was the script's; the calls below are not its subject
    called = [h for h in sorted(rows_of(ops)) if not ref.kf[h].bad and h != 1][:5]
    un.same_cull(dev.cull(called, mode="device"), ref.cull(called))
    same_store(dev, ref, mode="device")
    return r_dev, dev


@pytest.mark.parametrize("name", sorted(rs.HAND))
def test_hand_built(ctx, name):
    ops, expect, _ = rs.HAND[name]()
    r, _ = three_ways(ctx, ops)
    rs.check(r, expect)


@pytest.mark.parametrize("seed", [71, 73, 75])
def test_seeded_scripts(ctx, seed):
    three_ways(ctx, rs.random_script(seed))


def test_seeded_script_by_the_crossover(ctx):
    _, dev = three_ways(ctx, rs.random_script(72), mode="batch")
    assert dev.recent_cull_stats()["device_calls"] == 0                # no list reaches DRFE_LMAP_RECENT_DEVICE_FROM


def wide_world(n_kf, pad=0):
    """the origin 1 and its children 2 .. n_kf, each row starting with `pad` null entries"""
    w = rs.World()
    w.kf(1, 10, flags=un.ORIGIN, ch=list(range(2, n_kf + 1)))
    for h in range(2, n_kf + 1):
        w.kf(h, 10 * h, parent=1)
    for k in range(1, n_kf + 1):
        for _ in range(pad):
            w.entry(k, -1)
    return w


CULLED, STAYS = dict(found=1, visible=5), dict(found=4, visible=4)


def list_world(n, culls, n_kf=6):
    """n points and n lines, two observers each; culls(i) says whether item i is culled"""
    w = wide_world(n_kf)
    lists = {}
    for kind in (POINT, LINE):
        lists[kind] = [w.item(kind, [1 + i % n_kf, 1 + (i + 1) % n_kf], **(CULLED if culls(i) else STAYS)) for i in range(n)]
    return w, lists[POINT], lists[LINE]


@pytest.mark.parametrize("culls", ["all", "none", "alternating"])
@pytest.mark.parametrize("n", [0, 1, WAVE - 1, WAVE, WAVE + 1, T - 1, T, T + 1])
def test_list_lengths(ctx, n, culls):
    rule = {"all": lambda i: True, "none": lambda i: False, "alternating": lambda i: i % 2 == 0}[culls]
    w, pts, lns = list_world(n, rule)
    r, _ = three_ways(ctx, w.ops() + [("rcull", CUR, pts, lns, 0)])
    want = [2 if rule(i) else 0 for i in range(n)]
    assert r[0]["points"]["action"].tolist() == want and r[0]["lines"]["action"].tolist() == want
    assert r[0]["points"]["kept"].tolist() == [h for i, h in enumerate(pts) if not rule(i)]
    assert r[0]["lines"]["culled"].tolist() == [h for i, h in enumerate(lns) if rule(i)]


def test_a_handle_twice_across_the_seams(ctx):
    w, pts, lns = list_world(T + 20, lambda i: i in (0, 1))
    (c1, c2), (d1, d2) = pts[:2], lns[:2]
    pts, lns = pts[2:], lns[2:]
    pts[WAVE - 1] = pts[WAVE] = c1                                      # the last lane of a wavefront and the first of the next
    pts[T - 1] = pts[T] = c2                                            # the last lane of a workgroup and the first of the next
    # the line list starts at entry len(pts) of the flat entry space: its seams are placed in that space
    jt = (T - 1 - len(pts)) % T
    jw = (WAVE - 1 - len(pts)) % WAVE
    while abs(jw - jt) < 2:
        jw += WAVE
    assert (len(pts) + jt + 1) % T == 0 and (len(pts) + jw + 1) % WAVE == 0 and max(jt, jw) + 1 < len(lns)
    lns[jw] = lns[jw + 1] = d1
    lns[jt] = lns[jt + 1] = d2
    r, _ = three_ways(ctx, w.ops() + [("rcull", CUR, pts, lns, 0)])
    act = r[0]["points"]["action"]
    assert act[[WAVE - 1, WAVE, T - 1, T]].tolist() == [2, 1, 2, 1] and r[0]["points"]["culled"].tolist() == [c1, c2]
    act = r[0]["lines"]["action"]
    assert act[[jw, jw + 1, jt, jt + 1]].tolist() == [2, 1, 2, 1] and sorted(r[0]["lines"]["culled"].tolist()) == sorted([d1, d2])
    assert int((r[0]["points"]["action"] == 0).sum()) == len(pts) - 4 and int((r[0]["lines"]["action"] == 0).sum()) == len(lns) - 4


@pytest.mark.parametrize("culled", [True, False])
def test_items_with_0_1_64_65_and_300_observers(ctx, culled):
    w = wide_world(301)
    kw = CULLED if culled else STAYS
    pts = [w.rpoint(list(range(1, k + 1)), n_obs=9, **kw) for k in (300, 0, 65, 1, 64)]
    lns = [w.rline(list(range(301, 301 - k, -1)), n_obs=9, **kw) for k in (64, 300, 1, 65, 0)]
    r, _ = three_ways(ctx, w.ops() + [("rcull", CUR, pts, lns, 0)])
    if culled:
        assert [len(e) for e in r[0]["points"]["erased"]] == [300, 0, 65, 1, 64]
        assert [len(e) for e in r[0]["lines"]["erased"]] == [64, 300, 1, 65, 0]
        assert r[0]["lines"]["erased"][1][:3].tolist() == [[301, 1], [300, 1], [299, 1]]     # stored order, not slot order


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_erased_observations_around_the_erase_tile(ctx, delta):
    w = wide_world(120)
    last = ET + delta - 200
    assert 0 < last <= 120
    pts = [w.rpoint(list(range(1, k + 1)), n_obs=9, **CULLED) for k in (100, 100, last)]
    keep = w.rpoint([1, 2, 3, 4], **STAYS)
    r, dev = three_ways(ctx, w.ops() + [("rcull", CUR, pts[:2] + [keep, pts[2]], [], 0)])
    assert sum(len(e) for e in r[0]["points"]["erased"]) == ET + delta and r[0]["points"]["kept"].tolist() == [keep]


def chunk_ops():
    """42 entries: culled and kept items mixed, a culled handle again 20 entries on, a kept one again"""
    w, pts, lns = list_world(20, lambda i: i % 3 == 0)
    pts = pts + [pts[0]]
    lns = lns[:19] + [lns[0], lns[1]]
    return w.ops(), pts, lns


@pytest.mark.parametrize("chunks", [1, 2, 42])
def test_scratch_budgets(ctx, chunks):
    ops, pts, lns = chunk_ops()
    n = len(pts) + len(lns)
    probe = lib.LocalMap()
    rs.play(ops, probe)
    whole, least, fixed = probe.recent_cull_scratch(n)
    assert least == fixed + EB and whole == fixed + EB * n and n == 42
    r, _ = three_ways(ctx, ops + [("rcull", CUR, pts, lns, 0)], configure=fixed + EB * -(-n // chunks))
    assert r[0]["points"]["action"][-1] == 1 and r[0]["lines"]["action"][-2:].tolist() == [1, 0]


def test_one_byte_too_little_for_one_entry(ctx):
    ops, pts, lns = chunk_ops()
    dev = lib.LocalMap(ctx)
    rs.play(ops, dev)
    _, least, _ = dev.recent_cull_scratch(len(pts) + len(lns))
    dev.configure(least - 1)
    with pytest.raises(lib.DrfeError) as e:
        dev.recent_cull(CUR, pts, lns, mode="device")
    assert e.value.rc == lib.ERR_CAPACITY and dev.recent_cull_stats()["calls"] == 0
    host = lib.LocalMap()
    rs.play(ops, host)
    rn.same_recent(dev.recent_cull(CUR, pts, lns, mode="batch"), host.recent_cull(CUR, pts, lns, mode="host"))
    assert dev.recent_cull_stats()["device_calls"] == 0


def test_refused_device_calls_change_nothing(ctx):
    ops, expect, _ = rs.each_action()
    pts, lns = ops[-1][2], ops[-1][3]
    dev = lib.LocalMap(ctx)
    rs.play(ops[:-1], dev)
    line = dict([op for op in ops if op[0] == "recent"][0][2][-1])
    dev.set_recent_attributes([], [dict(line, visible=0)])
    with pytest.raises(lib.DrfeError) as e:
        dev.recent_cull(CUR, pts, lns, mode="device")
    assert e.value.rc == lib.ERR_STATE and "map line %d" % line["handle"] in str(e.value)
    dev.set_recent_attributes([], [line])
    with pytest.raises(lib.DrfeError) as e:
        dev.recent_cull(CUR, pts + [99999], lns, mode="device")
    assert e.value.rc == lib.ERR_INVALID
    need = [sum(len(x) for x in expect[0][k]["erased"]) for k in ("points", "lines")]
    for which in (0, 1):
        cap = list(need)
        cap[which] -= 1
        with pytest.raises(lib.DrfeError) as e:
            dev.recent_cull(CUR, pts, lns, mode="device", capacity=cap)
        assert e.value.rc == lib.ERR_CAPACITY
    assert dev.recent_cull_stats()["calls"] == 0
    # the exact capacities are below the bound (the kept items have observations too), and the call runs on the device
    r = dev.recent_cull(CUR, pts, lns, mode="device", capacity=need)
    rs.check([r], expect)
    assert dev.recent_cull_stats()["device_calls"] == 1
    ref = rn.Store()
    rs.play(ops, ref)
    same_store(dev, ref, mode="device")


def test_what_travels_after_a_call(ctx):
    """The device entry stores the bad flags and the nulled entries into the resident image itself: the call and the device call
    after it send no match rows and no graph block, only the observations with their offsets; a counter edit sends the four
    counter arrays of the recent-list block and nothing else."""
    pad = 3000
    w = wide_world(8, pad=pad)
    pts = [w.rpoint([1 + i % 8, 1 + (i + 3) % 8], **(CULLED if i % 2 else STAYS)) for i in range(40)]
    lns = [w.rline([1 + i % 8, 1 + (i + 3) % 8], **(CULLED if i % 2 else STAYS)) for i in range(40)]
    ops = w.ops()
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    rs.play(ops, dev)
    rs.play(ops, host)
    q, q2, q3 = ([dict(frame_id=f, points=pts, lines=lns)] for f in (77, 78, 79))
    dev.update(q, mode="device")                                        # the rows and the graph are resident now
    host.update(q, mode="host")
    b0, r0 = dev.upload_bytes(), dev.recent_upload_bytes()
    match_rows = 4 * 8 * pad
    assert b0["rows"] > match_rows and b0["graph"] > 0 and r0 == 0
    rn.same_recent(dev.recent_cull(CUR, pts, lns, mode="device"), host.recent_cull(CUR, pts, lns, mode="host"))
    b1, r1 = dev.upload_bytes(), dev.recent_upload_bytes()
    assert b1["rows"] == b0["rows"] and b1["graph"] == b0["graph"] and b1["geometry"] == b0["geometry"] and r1 > 0
    import lmap_numpy as ln
    ln.same(dev.update(q2, mode="device"), host.update(q2, mode="host"))  # reads the flags and entries the kernels stored
    b2 = dev.upload_bytes()
    tail = 4 * (len(w.pts) + 1) + 4 * 2 * 20 + 2 * 16                    # the offsets and the 20 kept points' observations
    assert 0 < b2["rows"] - b1["rows"] <= tail < match_rows and b2["graph"] == b1["graph"]
    ln.same(dev.update(q3, mode="device"), host.update(q3, mode="host"))
    b3 = dev.upload_bytes()
    assert b3 == b2
    # IncreaseFound / IncreaseVisible: the counters alone
    for s in (dev, host):
        s.recent_increase(POINT, pts[::2], [0] * 20, [40] * 20)          # the kept points drop below a quarter
        s.recent_increase(LINE, lns[:1], [0], [0])
    r2 = dev.recent_upload_bytes()
    res = dev.recent_cull(CUR, pts, lns, mode="device")
    rn.same_recent(res, host.recent_cull(CUR, pts, lns, mode="host"))
    assert res["points"]["action"].tolist() == [2, 1] * 20
    b4, r3 = dev.upload_bytes(), dev.recent_upload_bytes()
    counters = 4 * 2 * (len(w.pts) + len(w.lns))
    # what the first call cleared and no call has read since travels with this one too: the observation indices of the points at
    # the end of the attribute block, the line observations at the end of the recent-list block
    assert all(b4[k] == b3[k] for k in ("rows", "graph", "geometry", "gba"))
    assert 0 < b4["attributes"] - b3["attributes"] <= 4 * 2 * 20 + 16
    assert counters <= r3 - r2 <= counters + 4 * 16 + 4 * (len(w.lns) + 1) + 2 * 4 * 2 * 20 + 3 * 16
    ref = rn.Store()
    rs.play(ops, ref)
    ref.update(q)
    ref.recent_cull(CUR, pts, lns)
    ref.update(q2)
    ref.update(q3)
    for kind, hs, df, dv in ((POINT, pts[::2], [0] * 20, [40] * 20), (LINE, lns[:1], [0], [0])):
        ref.recent_increase(kind, hs, df, dv)
    ref.recent_cull(CUR, pts, lns)
    same_store(dev, ref, mode="device")


def test_a_host_call_reaches_the_device_with_few_and_with_many_nulled_entries(ctx):
    """after the host entry the flags and the nulled entries travel: one by one, or above 1 024 of them as the whole section"""
    import lmap_numpy as ln
    for n in (20, 200):                                                 # 160 and 1 600 nulled entries
        w = wide_world(8, pad=1000)
        pts = [w.rpoint(list(range(1, 9)), n_obs=9, **CULLED) for _ in range(n)] + [w.rpoint([1, 2], **STAYS)]
        dev, host = lib.LocalMap(ctx), lib.LocalMap()
        for s in (dev, host):
            rs.play(w.ops(), s)
        q, q2 = ([dict(frame_id=f, points=pts + [-1])] for f in (5, 6))
        ln.same(dev.update(q, mode="device"), host.update(q, mode="host"))
        b0 = dev.upload_bytes()
        rn.same_recent(dev.recent_cull(CUR, pts, [], mode="host"), host.recent_cull(CUR, pts, [], mode="host"))
        assert dev.recent_cull_stats()["nulled"] == 8 * n
        ln.same(dev.update(q2, mode="device"), host.update(q2, mode="host"))
        sent = dev.upload_bytes()["rows"] - b0["rows"]
        padding = 4 * 8 * 1000                                          # of the match rows, which dwarf 4 bytes per nulled entry
        assert (sent > padding) == (8 * n > 1024) and sent > 4 * 8 * n and dev.upload_bytes()["graph"] == b0["graph"]


def test_native_caller_on_the_device_entry():
    """tests/native/recent_cull_caller.cpp with every call forced onto the device entry: the same two worlds, and the store read
    back through a device UpdateLocalMap"""
    import subprocess
    import native_build
    exe = native_build.caller("recent_cull_caller")
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "recent_cull_caller ok (device, 8 calls, 390 culled" in p.stdout, (p.returncode, p.stdout, p.stderr)
