"""GPU tests of KeyFrame::UpdateConnections' device entry (drfe_lmap_connect_device, dr_slam_amd/csrc/conn_kernels.hip, DESIGN.md
section 26): the same bytes, the same store afterwards (drfe_lmap_get_connections and a following UpdateLocalMap on the host) and
the same counters as the host entry and as tests/conn_numpy.py, on every hand-built graph of tests/conn_scenarios.py, on seeded
scripts with edits, and on shapes placed from drfe_lmap_limits() and drfe_lmap_connect_limits(): match rows of the vote
workgroup's size - 1, + 0, + 1 and of one entry; points with 0, 1 and 70 observations; stores at the LDS histogram's limit and
one key frame above it; listed counts around a wavefront and one past each tile of the list sort; a key frame that 1, 64 and 65
edges land on; calls of 1, 2 and 200 key frames; the scratch budget of one and of two called key frames per vote launch."""
import numpy as np
import pytest

import conn_numpy as cn
import conn_scenarios as cs
import lmap_numpy as ln
import lmap_scenarios as ls
from dr_slam_amd import lib

pytestmark = pytest.mark.gpu

LIM = lib.LocalMap.limits()
CLIM = lib.LocalMap.connect_limits()
TH = CLIM["threshold"]


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        (cn.same_connect if "touched" in x else ln.same)(x, y)


def three_ways(ctx, ops, configure=None, restate=True):
    """a script on the device, on the host and in the restatement: equal results, equal stores, equal counters; returns the
    device's results and store"""
    host = lib.LocalMap()
    r_host = cs.play(ops, host)
    dev = lib.LocalMap(ctx)
    if configure:
        dev.configure(configure)
    r_dev = cs.play(ops, dev, mode="device")
    same_results(r_dev, r_host)
    sd, sh = dev.connect_stats(), host.connect_stats()
    n_calls = sum(1 for op in ops if op[0] == "connect" and len(op[1]))
    assert sd["device_calls"] == n_calls and sh["device_calls"] == 0
    assert {k: v for k, v in sd.items() if k != "device_calls"} == {k: v for k, v in sh.items() if k != "device_calls"}
    handles = sorted({r["handle"] for op in ops if op[0] == "kfs" for r in op[1]} - {op[2] for op in ops if op[0] == "remove" and op[1] == ls.KEYFRAME})
    cn.same_state(dev, host, handles)
    rows = {}
    for op in ops:
        if op[0] == "kfs":
            rows.update({r["handle"]: r for r in op[1]})
    q = [dict(frame_id=10 ** 6 + i, points=rows[h]["points"]) for i, h in enumerate(handles[:6])]
    after = dev.update(q, mode="host")
    ln.same(after, host.update(q, mode="host"))
    if restate:
        ref = cn.Store()
        same_results(r_dev, cs.play(ops, ref))
        assert all(sd[k] == v for k, v in ref.ccounts.items())
        cn.same_state(dev, ref, handles)
        ln.same(after, ref.update(q))
    return r_dev, dev


@pytest.mark.parametrize("name", sorted(cs.HAND))
def test_hand_built(ctx, name):
    ops, expect, _ = cs.HAND[name]()
    r, dev = three_ways(ctx, ops)
    cs.check(r, expect, dev)


@pytest.mark.parametrize("seed", [3, 14, 102])
def test_seeded_scripts(ctx, seed):
    three_ways(ctx, cs.random_script(seed))


def test_match_rows_around_the_vote_workgroup(ctx):
    T = LIM["vote_threads"]
    rng = np.random.default_rng(6)
    sizes = (T - 1, T, T + 1, 1, 2 * T + 3)
    n_mp = 120
    kfs = [ls.kf(h, 100 - h, pts=[int(p) for p in rng.integers(-1, n_mp, s)]) for h, s in enumerate(sizes)]
    kfs += [ls.kf(h, 200 + 3 * h) for h in range(5, 12)]
    pts = [ls.mp(p, obs=[int(k) for k in rng.permutation(12)[:int(rng.integers(0, 6))]], bad=int(rng.random() < 0.1)) for p in range(n_mp)]
    r, _ = three_ways(ctx, [("kfs", kfs), ("points", pts), ("conn", [cs.conn(h, first=1) for h in range(5)]), ("connect", [3, 0, 4, 1, 2])])
    rec = r[0]["record"]
    assert (rec[:, 1] > 1).any() and (rec[:, 2] >= TH).any() and (rec[:, 2] < TH).any()


def test_observation_counts(ctx):
    """points with no observation, one, and 70 (more than a wavefront)"""
    kfs = [ls.kf(h, 1000 - h) for h in range(70)] + [ls.kf(100, 5, pts=[0]), ls.kf(101, 6, pts=[1] * TH), ls.kf(102, 7, pts=[2] * (TH - 1) + [1, 0]),
                                                      ls.kf(103, 8, pts=[2, 1, 0, 2] * 8)]
    pts = [ls.mp(0), ls.mp(1, [33]), ls.mp(2, list(range(70)))]
    r, _ = three_ways(ctx, [("kfs", kfs), ("points", pts), ("connect", [100, 101, 102, 103])])
    assert r[0]["record"].tolist() == [[0, 0, 0, -1], [1, 1, TH, 33], [70, 1, TH, 33], [70, 70, 24, 33]]
    assert cs.pairs(r[0]["ordered"][list(r[0]["touched"]).index(103)])[:2] == [(33, 24), (0, 16)]


@pytest.mark.parametrize("extra", [0, 1])
def test_histogram_at_the_lds_limit(ctx, extra):
    """the limit's count of stored key frames (rows over slots in LDS) and one more (rows of global scratch); the votes reach the
    first and the last slot; with the smallest scratch budget the call runs with, the vote runs one called key frame per launch,
    with 4 bytes x stored key frames more two per launch; one byte less and _device refuses while _batch runs the call on the host"""
    n = LIM["lds_keyframes"] + extra
    kfs = [ls.kf(h, h + 1) for h in range(n)]
    for h, k in ((5, 18), (n - 1, 16), (n // 2, 3)):
        kfs[h]["points"] = list(range(k)) + [20]
    pts = [ls.mp(p, obs=[0, n - 1, 5, n // 2 + p]) for p in range(20)] + [ls.mp(20, obs=[7])]
    ops = [("kfs", kfs), ("points", pts), ("conn", [cs.conn(5, first=1), cs.conn(0, weights=[(5, 18), (n - 1, 2)], ordered=[(5, 18)])]),
           ("connect", [n - 1, 5, n // 2])]
    whole, dev = three_ways(ctx, ops, restate=False)
    assert whole[0]["touched"].tolist()[0] == 0 and whole[0]["record"][:, 0].tolist() == [19, 21, 6]     # n // 2 is itself among its points' observers
    ref = cn.Store()
    same = cs.play(ops, ref)
    cn.same_connect(whole[0], same[0])
    if not extra:
        return
    lo, hi = 1, 1 << 30                     # lo refuses, hi runs
    while hi - lo > 1:
        mid = (lo + hi) // 2
        dev.configure(mid)
        try:
            dev.connect([n - 1, 5, n // 2], mode="device")
            hi = mid
        except lib.DrfeError as e:
            assert e.rc == lib.ERR_CAPACITY
            lo = mid
    for budget in (hi, hi + 4 * n, hi + 8 * n):
        r, _ = three_ways(ctx, ops, configure=budget, restate=False)
        cn.same_connect(r[0], whole[0])
    dev.configure(lo)
    before = dev.connect_stats()
    with pytest.raises(lib.DrfeError) as e:
        dev.connect([n - 1, 5, n // 2], mode="device")
    assert e.value.rc == lib.ERR_CAPACITY and dev.connect_stats() == before


def listed_group(rng, base, listed):
    """a called key frame `base` and `listed` key frames that each get between 15 and 25 of its votes"""
    kfs = [ls.kf(base, int(rng.integers(1, 2 ** 40)) * 8192 + base)] + [ls.kf(base + 1 + i, int(rng.integers(1, 2 ** 40)) * 8192 + base + 1 + i) for i in range(listed)]
    pts = []
    for i in range(TH + 10):
        obs = [base + 1 + j for j in range(listed) if i < TH or (j + 1) % (i - TH + 2) == 0]
        pts.append(ls.mp(base * 64 + i, obs))
    kfs[0]["points"] = [p["handle"] for p in pts]
    return kfs, pts


def test_listed_counts_around_a_wavefront_and_the_sort_tile(ctx):
    tile = CLIM["sort_tile"]
    counts = (1, 63, 64, 65, tile, tile + 1, 2 * tile + 1)
    rng = np.random.default_rng(12)
    kfs, pts, heads, base = [], [], [], 0
    for c in counts:
        k, p = listed_group(rng, base, c)
        kfs, pts = kfs + k, pts + p
        heads.append(base)
        base += c + 1
    ops = [("kfs", kfs), ("points", pts), ("conn", [cs.conn(h, first=1) for h in heads]), ("connect", heads), ("connect", heads[::-1])]
    r, _ = three_ways(ctx, ops)
    assert r[0]["record"][:, 1].tolist() == list(counts) and len(set(cs.pairs(r[0]["ordered"][list(r[0]["touched"]).index(heads[-1])]))) == counts[-1]
    assert not r[1]["flags"].any()                          # the second call meets its own weights everywhere


def test_one_64_and_65_edges_onto_a_key_frame(ctx):
    rng = np.random.default_rng(13)
    g = cs.Graph()
    for h in range(65):
        g.kf(h, int(rng.integers(1, 2 ** 40)) * 128 + h)
    for t in (100, 101, 102, 103):
        g.kf(t, int(rng.integers(1, 2 ** 40)) * 128 + t)
    for h in range(65):
        g.see(h, [102], TH + h % 5)
        if h < 64:
            g.see(h, [101], TH + h % 3)
        if h == 0:
            g.see(h, [100], TH)
        g.see(h, [103], h % 4)
    stored = [cs.conn(101, weights=[(h, TH + h % 3 + (h % 2)) for h in range(0, 64, 2)], ordered=[(0, TH)]), cs.conn(102, weights=[(103, 4)], ordered=[(103, 4)])]
    ops = g.ops() + [("conn", stored), ("connect", [int(h) for h in rng.permutation(65)])]
    r, _ = three_ways(ctx, ops)
    t = r[0]["touched"].tolist()
    assert [len(r[0]["weights"][t.index(h)]) for h in (100, 101, 102)] == [1, 64, 66]


def test_calls_of_1_2_and_200_key_frames(ctx):
    rng = np.random.default_rng(14)
    kfs, pts = cs.clustered(rng, 220, 60)
    order = [int(h) for h in rng.permutation(220)]
    ops = [("kfs", list(kfs.values())), ("points", pts), ("conn", [cs.conn(h, first=1) for h in range(1, 220)]), ("connect", order[:1]),
           ("connect", order[1:3]), ("connect", order[3:203]), ("connect", order[100:220])]
    r, _ = three_ways(ctx, ops)
    assert (r[2]["record"][:, 1] > 1).any() and (r[2]["new_parent"] >= 0).sum() > 100 and r[3]["flags"].any() and not r[3]["flags"].all()


def test_host_device_and_batch_calls_in_turn(ctx):
    ops = cs.random_script(18, calls=9)
    ref, dev = cn.Store(), lib.LocalMap(ctx)
    k = 0
    for op in ops:
        r = cs.play([op], ref)
        d = cs.play([op], dev, mode=("device", "host", "batch")[k % 3] if op[0] == "connect" else "host")
        if op[0] == "connect":
            k += 1
        same_results(d, r)
    st = dev.connect_stats()
    assert st["calls"] == 9 and st["device_calls"] >= 3
    cn.same_state(dev, ref, sorted(ref.kf))


def test_update_device_between_two_connect_device_calls(ctx):
    """a connect commits into the rows, so the next device call of either kind uploads the image once; a call that follows without
    an edit uploads nothing"""
    rng = np.random.default_rng(15)
    kfs, pts = cs.clustered(rng, 40, 60)
    ops = [("kfs", list(kfs.values())), ("points", pts), ("conn", [cs.conn(h, first=1) for h in range(1, 40)])]
    dev, ref = lib.LocalMap(ctx), cn.Store()
    cs.play(ops, dev), cs.play(ops, ref)
    cn.same_connect(dev.connect([3, 4, 5], mode="device"), ref.connect([3, 4, 5]))
    assert dev.stats()["uploads"] == 1
    q = [dict(frame_id=1, points=kfs[4]["points"])]
    ln.same(dev.update(q, mode="device"), ref.update(q))
    assert dev.stats()["uploads"] == 2
    q = [dict(frame_id=2, points=kfs[9]["points"])]
    ln.same(dev.update(q, mode="device"), ref.update(q))
    assert dev.stats()["uploads"] == 2
    cn.same_connect(dev.connect([9, 4, 10], mode="device"), ref.connect([9, 4, 10]))
    assert dev.stats()["uploads"] == 2
    cn.same_connect(dev.connect([11], mode="device"), ref.connect([11]))
    assert dev.stats()["uploads"] == 3 and dev.connect_stats()["device_calls"] == 3


def test_batch_entry_follows_the_crossover(ctx):
    n = CLIM["device_from"]
    rng = np.random.default_rng(16)
    kfs, pts = cs.clustered(rng, 300, 60)
    ops = [("kfs", list(kfs.values())), ("points", pts)]
    dev, host = lib.LocalMap(ctx), lib.LocalMap()
    cs.play(ops, dev), cs.play(ops, host)
    cn.same_connect(dev.connect([1], mode="batch"), host.connect([1], mode="host"))
    assert dev.connect_stats()["device_calls"] == (1 if n <= 1 else 0)
    many = list(range(10, 10 + min(n, 280)))
    cn.same_connect(dev.connect(many, mode="batch"), host.connect(many, mode="host"))
    assert dev.connect_stats()["device_calls"] == (1 if n <= 1 else 0) + (1 if n <= 280 else 0)


def test_dangling_connection_refused_before_anything_runs(ctx):
    dev = lib.LocalMap(ctx)
    dev.set_keyframes([ls.kf(1, 1)])
    dev.set_connections([cs.conn(1, weights=[(5, 3)])])
    with pytest.raises(lib.DrfeError) as e:
        dev.connect([1], mode="device")
    assert e.value.rc == lib.ERR_STATE and "5" in str(e.value) and dev.stats()["uploads"] == 0


def test_native_caller_on_the_device_entry():
    """tests/native/conn_caller.cpp with every call forced to the device entry"""
    import subprocess
    import native_build
    exe = native_build.caller("conn_caller")
    p = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "conn_caller ok (device, 40 single calls, 1 call of 30, device calls 41)" in p.stdout, (p.returncode, p.stdout, p.stderr)
