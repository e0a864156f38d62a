"""GPU tests of the device entry of LocalMapping::KeyFrameCulling (drfe_lmap_cull_device, dr_slam_amd/csrc/cull_kernels.hip,
DESIGN.md section 28): the same bytes, the same store afterwards (through the getters, a following connect and a following update,
both on the device, which read the image the commit left) and the same counters as the host entry and as tests/cull_numpy.py, on
every hand-built graph of tests/cull_scenarios.py, on seeded scripts with edits, and on shapes placed from
drfe_lmap_cull_limits(): match rows of the record tile's and of the walking workgroup's size - 1, + 0, + 1, of one entry and of
none; points with 0, 1, 3, 4 and 70 observers, all of them called, none of them called and mixed; calls of 1, 2, 64, 65 and 200
key frames; 0, 1 and 40 culls in one call; the scratch budget of one called key frame a chunk, of two, and one byte less.  The
device's record holds counts and no list of called observers, so there is no inline length to step past: the called observers are
read again from the image."""
import numpy as np
import pytest

import conn_numpy as cn
import cull_numpy as un
import cull_scenarios as us
import lmap_numpy as ln
from lmap_scenarios import kf as ls_kf
from dr_slam_amd import lib
from test_cull_cpu import same_results, same_store

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.cull_limits()
T, WT, EB = LIM["record_tile"], LIM["walk_threads"], LIM["entry_bytes"]


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def same_counters(dev, host):
    sd, sh = dev.cull_stats(), host.cull_stats()
    assert {k: v for k, v in sd.items() if k != "device_calls"} == {k: v for k, v in sh.items() if k != "device_calls"}
    return sd, sh


def three_ways(ctx, ops, configure=None, restate=True, mode="device"):
    """a script on the device, on the host and in the restatement: equal results, equal stores, equal counters; returns the
    device's results and store"""
    host = lib.LocalMap()
    r_host = us.play(ops, host)
    dev = lib.LocalMap(ctx)
    if configure:
        dev.configure(configure)
    r_dev = us.play(ops, dev, mode=mode)
    same_results(r_dev, r_host)
    sd, sh = same_counters(dev, host)
    n_calls = sum(1 for op in ops if op[0] == "cull" and len(op[1]))
    if mode == "device":
        assert sd["device_calls"] == n_calls and sh["device_calls"] == 0
    rows = {}
    for op in ops:
        if op[0] == "kfs":
            rows.update({r["handle"]: r for r in op[1]})
        elif op[0] == "remove" and op[1] == us.KEYFRAME:
            rows.pop(op[2], None)
    kfs = sorted(rows)
    # what the commit left on the device: an UpdateLocalMap and an UpdateConnections there against the host's
    q = [dict(frame_id=10 ** 6 + i, points=rows[h]["points"]) for i, h in enumerate(kfs[:6])]
    ln.same(dev.update(q, mode="device"), host.update(q, mode="host"))
    some = kfs[:12]
    cn.same_connect(dev.connect(some, mode="device"), host.connect(some, mode="host"))
    cn.same_state(dev, host, kfs)
    if restate:
        ref = un.Store()
        same_results(r_dev, us.play(ops, ref))
        assert all(sd[k] == v for k, v in ref.ucounts.items())
        ref.update(q)
        ref.connect(some)
        same_store(dev, ref)
    return r_dev, dev


@pytest.mark.parametrize("name", sorted(us.HAND))
def test_hand_built(ctx, name):
    ops, expect = us.HAND[name]()[:2]
    r, dev = three_ways(ctx, ops)
    us.check(r, expect, dev)


@pytest.mark.parametrize("seed", [61, 64, 67])
def test_seeded_scripts(ctx, seed):
    r, _ = three_ways(ctx, us.random_script(seed))
    assert sum(len(x["culled"]) for x in r if "culled" in x) >= 3


def test_seeded_script_by_the_crossover(ctx):
    three_ways(ctx, us.random_script(62), mode="batch")


def standers(w, n=3):
    """the origin 1 and n key frames that are never called"""
    w.kf(1, 10, flags=un.ORIGIN)
    for h in range(2, 2 + n):
        w.kf(h, 10 * h, parent=1)
    return list(range(2, 2 + n))


def rows_world(sizes, thin_every=2):
    """one called key frame per size with that many points of its own, all redundant; every thin_every-th key frame also gets a
    ninth as many points that nobody else sees often enough, which keeps it"""
    w = us.World()
    by = standers(w)
    called = []
    for i, s in enumerate(sizes):
        h = 10 + i
        w.kf(h, 1000 + 7 * i, parent=1)
        called.append(h)
        thin = (s // 9 + 1) if i % thin_every == 1 else 0
        w.redundant(h, by, s - thin)
        w.plain(h, by[0], thin)
    return w, called


def test_rows_around_the_tiles(ctx):
    sizes = (T - 1, T, T + 1, 1, 0, WT - 1, WT, WT + 1, 2 * WT + 3)
    w, called = rows_world(sizes)
    r, _ = three_ways(ctx, w.ops() + [("cull", called, 0)], restate=False)
    rec = r[0]["record"]
    assert rec[:, 0].tolist() == list(sizes) and set(rec[:, 3].tolist()) == {un.KEPT, un.CULLED}
    assert len(r[0]["points"]) > 2 * WT


def observers_world():
    """key frame 100's row holds points with 0, 1, 3, 4 and 70 observers beside itself, once with every observer called, once with
    none called, once mixed; the octaves alternate between counting and not, so that three counting observers come early, late
    or never"""
    w = us.World()
    standers(w)
    obs = list(range(10, 80))
    for h in obs + [100]:
        w.kf(h, 100 + 3 * h, parent=1)
    for count in (0, 1, 3, 4, 70):
        for pattern in ((0,), (3,), (0, 3), (3, 3, 3, 0), (3, 0, 0, 3, 0)):
            seen = obs[:count]
            w.point([(100, 1)] + [(k, pattern[i % len(pattern)]) for i, k in enumerate(seen)], n_obs=max(4, count + 1))
    return w, obs


@pytest.mark.parametrize("called", ["all", "none", "mixed"])
def test_points_with_0_1_3_4_and_70_observers(ctx, called):
    w, obs = observers_world()
    call = {"all": obs + [100], "none": [100], "mixed": obs[::2] + [100] + obs[1:8:2]}[called]
    r, _ = three_ways(ctx, w.ops() + [("cull", call, 0)])
    at = call.index(100)
    assert r[0]["record"][at, 0] == 25 and 0 < r[0]["record"][at, 1] < 25


def chain_world(n, every):
    """n called key frames in a chain of parents; every `every`-th (0 = none) is redundant in all its points, the others are not;
    neighbours in the chain share points, so a cull lowers what the next one counts"""
    w = us.World()
    by = standers(w)
    hs = list(range(10, 10 + n))
    for i, h in enumerate(hs):
        w.kf(h, 1000 + h, parent=1 if i == 0 else hs[i - 1])
        if i:
            w.kfs[hs[i - 1]]["children"].append(h)
    for i, h in enumerate(hs):
        if every and i % every == 0:
            w.redundant(h, by, 30)
        else:
            w.redundant(h, by, 3)
            w.plain(h, by[1], 3)
        if i + 1 < n:
            w.point([(h, 0), (hs[i + 1], 0), (by[0], 1, 1.0, 1)])
            w.link(h, hs[i + 1], 20 + i % 3)
    return w, hs


@pytest.mark.parametrize("n,every,culls", [(1, 1, 1), (2, 0, 0), (64, 0, 0), (65, 64, 2), (200, 5, 40), (200, 200, 1)])
def test_call_sizes_and_cull_counts(ctx, n, every, culls):
    w, hs = chain_world(n, every)
    r, _ = three_ways(ctx, w.ops() + [("cull", hs, 0)])
    assert len(r[0]["culled"]) == culls


def test_every_key_frame_of_a_long_call_is_culled(ctx):
    w, hs = chain_world(70, 1)
    r, _ = three_ways(ctx, w.ops() + [("cull", hs[::-1], 0)])
    assert len(r[0]["culled"]) == 70


@pytest.mark.parametrize("per_chunk", [1, 2])
def test_scratch_budgets(ctx, per_chunk):
    w, called = rows_world((300,) * 5, thin_every=3)
    ops = w.ops()
    probe = lib.LocalMap()
    us.play(ops, probe)
    whole, least, fixed = probe.cull_scratch(called)
    assert least == fixed + EB * 300 and whole == fixed + EB * 1500
    r, _ = three_ways(ctx, ops + [("cull", called, 0)], configure=fixed + per_chunk * EB * 300, restate=False)
    assert len(r[0]["culled"]) == 3


def test_a_row_that_does_not_fit_the_scratch(ctx):
    w, called = rows_world((300,) * 3)
    ops = w.ops()
    dev = lib.LocalMap(ctx)
    us.play(ops, dev)
    _, least, _ = dev.cull_scratch(called)
    dev.configure(least - 1)
    with pytest.raises(lib.DrfeError) as e:
        dev.cull(called, mode="device")
    assert e.value.rc == lib.ERR_CAPACITY and dev.cull_stats()["calls"] == 0
    host = lib.LocalMap()
    us.play(ops, host)
    un.same_cull(dev.cull(called, mode="batch"), host.cull(called, mode="host"))       # _batch runs it on the host
    assert dev.cull_stats()["device_calls"] == 0


def test_an_attribute_edit_does_not_send_the_graph_again(ctx):
    w, hs = chain_world(20, 0)
    ops = w.ops()
    dev = lib.LocalMap(ctx)
    us.play(ops, dev)
    r0 = dev.cull(hs, mode="device")
    assert len(r0["culled"]) == 0
    uploads = dev.stats()["uploads"]
    attr = [op for op in ops if op[0] == "attr"][0]
    kf = dict([r for r in attr[1] if r["handle"] == hs[3]][0], th_depth=np.float32(0.5))
    dev.set_cull_attributes([kf], [])
    r1 = dev.cull(hs, mode="device")
    assert dev.stats()["uploads"] == uploads                   # neither the rows nor the graph block went up again
    assert r1["record"][3, 0] < r0["record"][3, 0]             # and the edit was read: th_depth 0.5 skips the entries at depth 1
    host = lib.LocalMap()
    us.play(ops, host)
    host.set_cull_attributes([kf], [])
    un.same_cull(r1, host.cull(hs, mode="host"))


def test_a_call_that_culls_nothing_sends_nothing(ctx):
    w, hs = chain_world(20, 0)
    dev = lib.LocalMap(ctx)
    us.play(w.ops(), dev)
    dev.cull(hs, mode="device")
    uploads = dev.stats()["uploads"]
    dev.cull(hs[::-1], mode="device")
    dev.update([dict(frame_id=9, points=w.kfs[hs[0]]["points"])], mode="device")
    assert dev.stats()["uploads"] == uploads


def test_refused_device_call_changes_nothing(ctx):
    """5 is culled on the device, then 6 turns out to have no parent: the host takes back what it had applied"""
    ops, expect = us.HAND["earlier_cull_dooms_a_later_one"]()[:2]
    dev = lib.LocalMap(ctx)
    us.play(ops[:-1], dev)
    kf6 = [r for r in ops[0][1] if r["handle"] == 6][0]
    dev.set_keyframes([dict(kf6, parent=-1)])
    with pytest.raises(lib.DrfeError) as e:
        dev.cull([5, 6], mode="device")
    assert e.value.rc == lib.ERR_STATE and "no parent" in str(e.value)
    dev.set_keyframes([kf6])
    r = [dev.cull([5, 6], mode="device")]
    us.check(r, expect, dev)
    ref = un.Store()
    same_results(r, us.play(ops, ref))
    same_store(dev, ref)


def test_a_call_that_culled_sends_its_pieces_and_not_the_image(ctx):
    """after a call that culled, the next device call gets the bad flags, 4 bytes per nulled entry, the observations with their
    offsets, the graph block and the end of the attribute block: never the match rows, which are most of the image"""
    ops, expect = us.HAND["stereo_and_mono_cross_the_line"]()[:2]
    rows = {r["handle"]: r for r in ops[0][1]}
    entries = sum(len(r["points"]) for r in rows.values())
    n_obs_entries = sum(len(r["obs"]) for r in ops[1][1])
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    us.play(ops[:-1], dev)
    us.play(ops[:-1], host)
    r = dev.cull(ops[-1][1], mode="device")                    # the first device call: the whole image once
    us.check([r], expect, dev)
    host.cull(ops[-1][1], mode="host")
    first = dev.upload_bytes()
    assert first["rows"] >= 4 * (entries + n_obs_entries) and first["graph"] > 0 and first["attributes"] >= 9 * entries
    q = [dict(frame_id=5, points=rows[2]["points"])]
    ln.same(dev.update(q, mode="device"), host.update(q, mode="host"))
    sent = {k: v - first[k] for k, v in dev.upload_bytes().items()}
    nulled = sum(len(x) for x in r["nulled"])
    assert nulled == 2 and len(r["points"]) == 22
    assert 4 * nulled < sent["rows"] <= first["rows"] - 4 * entries           # no match row went up again
    assert sent["graph"] == first["graph"] and sent["geometry"] == 0
    some = sorted(rows)
    cn.same_connect(dev.connect(some, mode="device"), host.connect(some, mode="host"))
    r2 = dev.cull([2], mode="device")
    assert len(r2["culled"]) == 0
    sent2 = {k: v - first[k] for k, v in dev.upload_bytes().items()}
    assert 0 < sent2["attributes"] <= first["attributes"] - 9 * entries       # counters and indices, not octave, depth and stereo
    assert sent2["rows"] == sent["rows"]
    un.same_cull(r2, host.cull([2], mode="host"))
    ln.same(dev.update([dict(frame_id=6, points=rows[3]["points"])], mode="device"),
            host.update([dict(frame_id=6, points=rows[3]["points"])], mode="host"))
    assert dev.upload_bytes()["rows"] - first["rows"] == sent["rows"]         # and nothing more after that


def block_bytes(*sections):
    """a resident block of (elements, element bytes) sections, each rounded up to 16 bytes"""
    return sum((n * e + 15) // 16 * 16 for n, e in sections)


def test_every_kind_of_edit_reaches_the_device(ctx):
    """one store through all five entries with every kind of edit in between, next to a host twin: equal results and equal stores
    after every call, and of the five resident blocks (rows, graph, geometry, attributes, adjustment state) exactly those go up
    that an edit touched since the last device call that used them - whole, with sizes restated here from the arrays, where the
    slots moved or the block is rebuilt, and in pieces after set_bad and after the cull"""
    import gba_propagate_numpy as gn
    import loop_correct_numpy as rn
    ops, expect = us.HAND["stereo_and_mono_cross_the_line"]()[:2]
    rows = {r["handle"]: r for r in ops[0][1]}
    kfs, pts = sorted(rows), sorted(r["handle"] for r in ops[1][1])
    E = sum(len(r["points"]) for r in rows.values())
    n_obs = sum(len(r["obs"]) for r in ops[1][1])
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    pose = lambda h, d=0.0: np.array([[1, 0, 0, 0.1 * h + d], [0, 1, 0, -0.2 * h], [0, 0, 1, 0.05 * h], [0, 0, 0, 1]], np.float32)
    for s in (dev, host):
        us.play(ops[:-1], s)
        s.set_scales([1.0, 1.2, 1.44])
        s.set_poses(kfs, [pose(h) for h in kfs])
        s.set_point_geometry([dict(handle=p, world=(0.01 * i, 0.5, 2.0 + 0.1 * i), ref_kf=2, ref_level=i % 3) for i, p in enumerate(pts)])
        s.set_gba_keyframes([1, 2], [pose(1, 0.5), pose(2, 0.25)], [7, 7])
        s.set_gba_points(pts[2:5], [(1, 2, 3), (4, 5, 6), (7, 8, 9)], [7, 7, 7])
    S = np.array([0, 0, 0, 1, 0.5, 0, 0, 1.0])
    K, P = len(kfs), len(pts)
    rows_whole = lambda k, obs: block_bytes((k, 1), (P, 1), (0, 1), (k + 1, 4), (E, 4), (k + 1, 4), (0, 4), (P + 1, 4), (obs, 4))
    geo_whole = lambda k: block_bytes((3, 4), (16 * k, 4), (3 * k, 4), (3 * P, 4), (P, 4), (P, 4), (P, 4), (P, 4))
    attr_whole = lambda k, obs: block_bytes((k, 4), (k, 1), (E, 4), (E, 4), (E, 1), (P, 4), (obs, 4))
    gba_whole = lambda k: block_bytes((16 * k, 4), (16 * k, 4), (3 * P, 4), (k, 4), (P, 4), (k, 1))

    def graph_whole(k):
        g = host.get_connections(sorted(rows))
        cw, co, ch = (sum(len(x) for x in g[n]) for n in ("weights", "ordered", "children"))
        return block_bytes((k, 4), (10 * k, 4), (k + 1, 4), (ch, 4), (k, 1), (k + 1, 4), (cw, 4), (cw, 4), (k + 1, 4), (co, 4), (co, 4))

    def stores_agree():
        cn.same_state(dev, host, sorted(rows))
        un.same_attributes(dev, host, kfs, pts)
        rn.same_geometry(dev, host, sorted(rows), pts)
        gn.same_store(dev, host, sorted(rows), pts)

    def call(what, same, fn, **sent):
        """fn on both stores; every block not named in `sent` went up by 0 bytes, a named one by that figure (or passes that test)"""
        before = dev.upload_bytes()
        r_dev, r_host = fn(dev, "device"), fn(host, "host")
        same(r_dev, r_host)
        stores_agree()
        delta = {k: v - before[k] for k, v in dev.upload_bytes().items()}
        print(what, delta)
        for k, v in delta.items():
            want = sent.get(k, 0)
            assert want(v) if callable(want) else v == want, (what, k, v, delta)
        return r_dev

    def edit(fn):
        fn(dev)
        fn(host)

    q = lambda i, h: [dict(frame_id=i, points=rows[h]["points"])]
    call("update", ln.same, lambda s, m: s.update(q(1, 2), mode=m), rows=rows_whole(K, n_obs), graph=graph_whole(K))
    edit(lambda s: s.set_bad(us.POINT, [pts[7]], [1]))
    call("update after set_bad", ln.same, lambda s, m: s.update(q(2, 2), mode=m), rows=lambda v: 0 < v < 4 * E)
    call("connect", cn.same_connect, lambda s, m: s.connect(kfs, mode=m))
    r = call("cull", un.same_cull, lambda s, m: s.cull([5], mode=m), graph=graph_whole(K), attributes=attr_whole(K, n_obs))
    assert list(r["culled"]) == [5]
    obs_left = sum(len(x) for x in r["obs"])
    assert len(r["points"]) == P and obs_left < n_obs
    corr = lambda s, m: s.correct(2, S, [1, 2, 3], mode=m)
    call("correct", rn.same_correct, corr, rows=lambda v: 0 < v <= rows_whole(K, obs_left) - 4 * E, graph=graph_whole(K), geometry=geo_whole(K))
    call("gba", gn.same_gba, lambda s, m: s.gba(7, [1], mode=m), gba=gba_whole(K))
    edit(lambda s: s.set_poses([3], [pose(3, 1.0)]))
    call("correct after set_poses", rn.same_correct, corr, geometry=geo_whole(K))
    edit(lambda s: s.set_gba_points([pts[9]], [(3, 2, 1)], [8]))
    call("gba after set_gba_points", gn.same_gba, lambda s, m: s.gba(8, [1], mode=m), gba=gba_whole(K))
    new = ls_kf(6, 60, parent=1)
    rows[6] = new
    edit(lambda s: (s.set_keyframes([new]), s.set_poses([6], [pose(6)])))
    call("update after set_keyframes", ln.same, lambda s, m: s.update(q(3, 3), mode=m), rows=rows_whole(K + 1, obs_left), graph=graph_whole(K + 1))
    # the slots moved for every block: each goes up whole at the first call that uses it, and only then
    call("correct after set_keyframes", rn.same_correct, corr, geometry=geo_whole(K + 1))
    r = call("cull after set_keyframes", un.same_cull, lambda s, m: s.cull([2], mode=m), attributes=attr_whole(K + 1, obs_left))
    assert len(r["culled"]) == 0
    call("gba after set_keyframes", gn.same_gba, lambda s, m: s.gba(9, [1], mode=m), gba=gba_whole(K + 1))
    call("update at the end", ln.same, lambda s, m: s.update(q(4, 4), mode=m))


def test_native_caller_on_the_device_entry():
    """tests/native/cull_caller.cpp with the adaptor forced onto the device entry"""
    import subprocess
    import native_build
    exe = native_build.caller("cull_caller")
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "cull_caller ok (device, 6 calls, 7 culled" in p.stdout, (p.returncode, p.stdout, p.stderr)
