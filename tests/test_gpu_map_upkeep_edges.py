"""-m gpu tests that hold device map-point and map-line upkeep to the hand-built items of
tests/map_upkeep_scenarios.py.  The device's descriptor kernels are another algorithm than the host's (a rank selection by
bisection on the value, then the minimum of (median << 16) | row over a lane group, a wavefront or a workgroup), so they get:
every hand-built case alone, points and lines, each half and both; items of 1 .. 2048 rows on both sides of every bucket
boundary whose winner is stated by construction (the last row, row 0 of identical rows, the lower of two tied rows in different
wavefronts or in one thread's stride, the first complement row with medians 256 and 0, random rows), each behind an
observation on a bad keyframe so that a row's index is never its observation's; items whose observation
count and row count lie in different buckets, with the counters; one call that interleaves all four buckets with partly full
last workgroups; and the NaN normals of a zero-length viewing ray.  Floats are compared by the rule of
pose_opt_numpy.tables_equal: a NaN equals a NaN, everything else bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_upkeep_numpy as MU  # noqa: E402
import map_upkeep_scenarios as MS  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("best_obs", "desc", "normal", "max_distance", "min_distance", "status", "frustum")
BUCKETS = ("desc_b4", "desc_b16", "desc_b64", "desc_wg", "desc_host")
NUMPY_ROWS = 257                       # numpy is the truth up to here, the host entry above (the numpy N^2 at 2048 is too slow)


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


def _differs(x, y):
    """a NaN equals a NaN whatever its sign and payload, everything else is compared by bits; structured records field by
    field"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return True
    if x.dtype.names:
        return any(_differs(x[f], y[f]) for f in x.dtype.names)
    if x.dtype.kind == "f":
        u = f"u{x.dtype.itemsize}"
        return not ((np.isnan(x) & np.isnan(y)) | (x.view(u) == y.view(u))).all()
    return x.tobytes() != y.tobytes()


def _assert_same(got, want, what=""):
    for k in KEYS:
        assert not _differs(got[k], want[k]), (what, k)


def _item(r, i):
    return {k: r[k][i:i + 1] for k in KEYS}


def _host(scene, line, what=3):
    from dr_slam_amd import lib
    return (lib.map_line_upkeep_host if line else lib.map_point_upkeep_host)(scene, what)


def _device(ctx, scene, line, what=3):
    return (ctx.map_line_upkeep_batch if line else ctx.map_point_upkeep_batch)(scene, what)


def _moved(ctx, before):
    st = ctx.map_upkeep_stats()
    return [st[b] - before[b] for b in BUCKETS]


@pytest.mark.parametrize("line", [False, True])
def test_hand_built_cases_alone(ctx, line):
    cases = MS.cases(line)
    assert len(cases) >= 14
    for name, s, expect in cases:
        for what in (1, 2, 3):
            dev = _device(ctx, s, line, what)
            _assert_same(dev, _host(s, line, what), (name, what))
            _assert_same(dev, MU.upkeep(s, what=what, line=line), (name, what))
            MS.holds(expect, dev, what=what)


@pytest.mark.parametrize("line", [False, True])
@pytest.mark.parametrize("nr", MS.BUCKET_ROWS)
def test_items_of_every_bucket(ctx, line, nr):
    """the items of nr rows in one call: the winner stated by construction, device == numpy (the host entry above 257 rows),
    and the bucket's counter moves by the number of items"""
    items = MS.bucket_items(nr)
    names = [n for n, _, _ in items]
    assert "identical" in names and "random" in names and (nr % 2 == 0 or "complement" in names)
    assert nr < 2 or sum(n.startswith("tied") for n in names) == (2 if nr > 256 else 1)
    assert 2 <= nr <= 4 or "last_least" in names
    # every item's first observation is on a bad keyframe (a row that is no item's), so row r is observation r + 1
    extra = np.bitwise_not(MS.BASE)
    s = MS.merge([MS.scene([extra] + list(rows), kf_bad=[1] + [0] * nr, line=line, ref_kf=1 + q % nr, ref_level=q % 8)
                  for q, (_, rows, _) in enumerate(items)], line)
    before = ctx.map_upkeep_stats()
    dev = _device(ctx, s, line)
    want = [0, 0, 0, 0, 0]
    want[0 if nr <= 4 else 1 if nr <= 16 else 2 if nr <= 64 else 3] = len(items)
    assert _moved(ctx, before) == want
    truth = MU.upkeep(s, line=line) if nr <= NUMPY_ROWS else _host(s, line)
    for q, (name, rows, win) in enumerate(items):
        if win is not None:
            assert truth["best_obs"][q] == win + 1, (name, "reference")
            assert dev["best_obs"][q] == win + 1 and dev["desc"][q].tobytes() == rows[win].tobytes(), name
    _assert_same(dev, truth, nr)


@pytest.mark.parametrize("line", [False, True])
def test_bucket_is_chosen_by_rows_not_by_observations(ctx, line):
    """70 observations with 4 rows, 20 with 16, 2100 (above the device cap) with 60: the four-lane, sixteen-lane and wavefront
    kernels take them, nothing goes to the workgroup kernel or the host, and best_obs indexes the caller's list"""
    shapes = [(70, 4)] * 3 + [(20, 16)] * 2 + [(2100, 60)] + [(70, 4), (20, 16)]
    scenes = [MS.with_bad_keyframes(o, g, seed=q, line=line) for q, (o, g) in enumerate(shapes)]
    s = MS.merge(scenes, line)
    before = ctx.map_upkeep_stats()
    dev = _device(ctx, s, line)
    assert _moved(ctx, before) == [4, 3, 1, 0, 0]
    _assert_same(dev, _host(s, line))
    _assert_same(dev, MU.upkeep(s, line=line))
    for q, (one, (n_obs, n_good)) in enumerate(zip(scenes, shapes)):
        b = int(dev["best_obs"][q])
        assert 0 <= b < n_obs and one["kf_bad"][b] == 0 and dev["desc"][q].tobytes() == one["obs_desc"][b].tobytes()
        assert int((one["kf_bad"] == 0).sum()) == n_good
        _assert_same(_device(ctx, one, line), _item(dev, q), q)
    # the row of a bad keyframe would have won: with every keyframe good the winner is another row
    allgood = dict(scenes[0], kf_bad=np.zeros_like(scenes[0]["kf_bad"]))
    assert scenes[0]["kf_bad"][int(_host(allgood, line)["best_obs"][0])] == 1


@pytest.mark.parametrize("line", [False, True])
def test_all_buckets_interleaved_in_one_call(ctx, line):
    """65 items of the four-lane bucket, 17 of the sixteen-lane one, 5 of the wavefront one and 3 of the workgroup one (the last
    workgroup of every group kernel partly full), a bad item, one without observations and one whose keyframes are all bad,
    shuffled: device == host, and every item equals its single-call result"""
    rng = np.random.default_rng(51 + line)
    nrs = [1 + q % 4 for q in range(65)] + [5 + q % 12 for q in range(17)] + [17, 33, 63, 64, 40] + [65, 100, 300]
    scenes = []
    for q, nr in enumerate(nrs):
        c = rng.integers(0, 256, 32, dtype=np.uint8)
        rows = MS.around(rng, c, nr, int(rng.integers(1, 12)))
        world = rng.normal(0, 3, (1, 6)) if line else rng.normal(0, 3, (1, 3)).astype(np.float32)
        lead = q % 3                      # observations on bad keyframes ahead of the rows: best_obs is not the row's index
        scenes.append(MS.scene([MS.BASE] * lead + rows, kf_bad=[1] * lead + [0] * nr, line=line, world=world,
                               ref_kf=int(rng.integers(0, nr)), ref_level=q % 8))
    two = [MS.BASE, MS.flip(MS.BASE, [1, 2])]
    scenes += [MS.scene(two, bad=1, line=line), MS.scene(np.zeros((0, 32), np.uint8), line=line),
               MS.scene(two, kf_bad=[1, 1], line=line)]
    order = rng.permutation(len(scenes))
    scenes = [scenes[q] for q in order]
    s = MS.merge(scenes, line)
    before = ctx.map_upkeep_stats()
    dev = _device(ctx, s, line)
    assert _moved(ctx, before) == [65, 17, 5, 3, 0]
    _assert_same(dev, _host(s, line))
    assert dev["status"].tolist().count(0) == 2 and dev["status"].tolist().count(2) == 1
    for q, one in enumerate(scenes):
        _assert_same(_device(ctx, one, line), _item(dev, q), q)


@pytest.mark.parametrize("line", [False, True])
def test_nan_normals(ctx, line, capsys):
    """a keyframe centre on the point (on the line's middle): the normal is NaN in every component on device, host and numpy,
    and nowhere else; alone and between two ordinary items.  The NaN's sign and payload are reported, not compared."""
    nan = MS.zero_ray_scene(line)
    plain = MS.scene(MS.tie_rows(), line=line)
    for s, at in ((nan, 0), (MS.merge([plain, nan, plain], line), 1)):
        dev, host = _device(ctx, s, line), _host(s, line)
        _assert_same(dev, host)
        _assert_same(dev, MU.upkeep(s, line=line))
        for r in (dev, host):
            where = np.isnan(r["normal"])
            assert where[at].all() and where.sum() == 3
            assert np.isnan(r["frustum"]["normal"][at]).all() and np.isnan(r["frustum"]["normal"]).sum() == 3
            for k in ("max_distance", "min_distance"):
                assert not np.isnan(r[k]).any() and not np.isnan(r["frustum"][k]).any()
            assert not np.isnan(r["frustum"]["world"]).any()
        u = "u8" if line else "u4"
        with capsys.disabled():
            print(f"\nNaN normal ({'line' if line else 'point'}): device {[hex(v) for v in dev['normal'][at].view(u)]}, "
                  f"host {[hex(v) for v in host['normal'][at].view(u)]}")
