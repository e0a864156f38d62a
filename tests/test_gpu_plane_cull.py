"""-m gpu tests of LocalMapping::MapPlaneCulling on the resident plane maps: on every hand-built scene
drfe_plane_map_cull_batch, with the device forced and once through the dispatch, equals drfe_plane_map_cull_host byte for byte;
the resident map afterwards gives the clouds and the association results of a host map edited by the host entry's outputs,
with nothing re-uploaded; the counters of the rounds; a second resident map stays untouched; the native caller."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_cull_scenarios as us  # noqa: E402
import plane_match_numpy as PN  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
SCENARIOS = us.all_scenarios()
same = us.same
_HOST = {}


def host_result(name):
    """the host entry's result of a scene, computed once"""
    from dr_slam_amd import lib
    if name not in _HOST:
        _HOST[name] = lib.plane_map_cull_host(SCENARIOS[name]["scene"])
    return _HOST[name]


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


def as_map(scene):
    return dict(coefs=scene["coefs"], bad=scene["bad"], clouds=scene["clouds"], points=np.zeros((0, 3), f32))


def edited(scene, r):
    """the host's map after the call: the entry's flags and rebuilt clouds over the scene's"""
    clouds = [np.asarray(c, f32).reshape(-1, 3) for c in scene["clouds"]]
    for j, c in r["clouds"].items():
        clouds[j] = c
    return r["bad"], clouds


def check_resident(c, map_id, scene, bad, clouds, seed=5):
    """the resident clouds, and an association batch against the resident map next to the host entry on the host's map"""
    from dr_slam_amd import lib
    P = len(scene["coefs"])
    for j in range(P):
        got = c.plane_map_cloud_download(map_id, j)
        assert got.shape == clouds[j].shape and np.array_equal(got.view(np.uint32), clouds[j].view(np.uint32)), j
    if P == 0:
        return
    rng = np.random.default_rng(seed)
    T = np.eye(4, dtype=f32)
    pick = rng.choice(P, min(P, 6), replace=False)
    cf = scene["coefs"][pick].copy()
    cf[:, 3] += rng.normal(0, 0.02, len(cf)).astype(f32)
    for params in (PN.DEFAULTS, (f32(200.0),) + PN.DEFAULTS[1:]):
        c.plane_match_batch([map_id], T[None], [cf], flag_points=False, params=params)
        mi, pi, vi, n, _ = c.plane_match_download(0)
        h = lib.plane_match_host(T, cf, scene["coefs"], bad, clouds, params=params)
        assert np.array_equal(mi, h[0]) and np.array_equal(pi, h[1]) and np.array_equal(vi, h[2]) and n == h[3]


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_device_equals_host(ctx, name):
    from dr_slam_amd import lib
    scene = SCENARIOS[name]["scene"]
    ref = host_result(name)
    P = len(scene["coefs"])
    ctx.plane_map_upload([as_map(scene)])
    got = ctx.plane_map_cull_batch(0, scene, mode=lib.PLANE_CULL_DEVICE)
    same(got, ref)
    up, cu = ctx.plane_map_update_stats(), ctx.plane_map_cull_stats()
    assert cu["calls"] == 1 and cu["device_calls"] == 1
    assert up["device_jobs"] + up["host_jobs"] == ref["counters"]["rebuilds"]
    assert up["host_jobs"] >= SCENARIOS[name].get("host_jobs", 0)
    assert up["rounds"] == cu["rebuild_calls"] and ref["counters"]["stale_columns"] <= cu["rebuild_calls"] <= max(ref["counters"]["rebuilds"], 0)
    assert (P >= 2) <= cu["dist_launches"] <= 1 + ref["counters"]["stale_columns"]
    check_resident(ctx, 0, scene, *edited(scene, ref))
    # a second call on the culled map: the host entry on the edited map
    s2 = dict(scene, bad=ref["bad"], clouds=edited(scene, ref)[1], n_obs=ref["n_obs"], found=ref["found"], visible=ref["visible"])
    if len(ref["events"]) == 0:
        same(ctx.plane_map_cull_batch(0, s2, mode=lib.PLANE_CULL_DEVICE), lib.plane_map_cull_host(s2))


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_dispatch_equals_host(ctx, name):
    """mode 0: below DRFE_PLANE_CULL_DEVICE_FROM the host walk runs on the downloaded clouds and still commits"""
    from dr_slam_amd import lib
    scene = SCENARIOS[name]["scene"]
    ref = host_result(name)
    ctx.plane_map_upload([as_map(scene)])
    same(ctx.plane_map_cull_batch(0, scene), ref)
    cu = ctx.plane_map_cull_stats()
    assert cu["device_calls"] == int(len(scene["coefs"]) >= lib.plane_map_cull_limits()["device_from"])
    check_resident(ctx, 0, scene, *edited(scene, ref))


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_modes_agree(ctx, mode):
    """the forced device, the host walk and the one-row tile give the same bytes on a random map"""
    name = f"random_{us.RANDOM_SEEDS[0]}"
    scene = SCENARIOS[name]["scene"]
    ctx.plane_map_upload([as_map(scene)])
    same(ctx.plane_map_cull_batch(0, scene, mode=mode), host_result(name))


def test_other_map_untouched(ctx):
    a, b = SCENARIOS[f"random_{us.RANDOM_SEEDS[1]}"]["scene"], SCENARIOS["stale_column_grows"]["scene"]
    ctx.plane_map_upload([as_map(a), as_map(b), as_map(a)])
    from dr_slam_amd import lib
    ref = host_result("stale_column_grows")
    same(ctx.plane_map_cull_batch(1, b, mode=lib.PLANE_CULL_DEVICE), ref)
    check_resident(ctx, 1, b, *edited(b, ref))
    for m in (0, 2):
        check_resident(ctx, m, a, a["bad"], [np.asarray(c, f32) for c in a["clouds"]])
    # and the first map culled afterwards, as if alone
    same(ctx.plane_map_cull_batch(0, a, mode=lib.PLANE_CULL_DEVICE), host_result(f"random_{us.RANDOM_SEEDS[1]}"))
    check_resident(ctx, 2, a, a["bad"], [np.asarray(c, f32) for c in a["clouds"]])


def test_refused(ctx):
    from dr_slam_amd import lib
    a, b = SCENARIOS["stale_column_grows"]["scene"], SCENARIOS["row_tiles"]["scene"]
    ctx.plane_map_upload([as_map(a)])
    with pytest.raises(lib.DrfeError, match="plane count"):
        ctx.plane_map_cull_batch(0, b)
    with pytest.raises(lib.DrfeError):
        ctx.plane_map_cull_batch(1, a)
    with pytest.raises(lib.DrfeError):
        ctx.plane_map_cull_batch(0, a, mode=7)
    check_resident(ctx, 0, a, a["bad"], [np.asarray(c, f32) for c in a["clouds"]])     # a refused call changes nothing
    # rebuilt_capacity too small: DRFE_ERR_CAPACITY, the map committed all the same
    with pytest.raises(lib.DrfeError, match="rebuilt_capacity"):
        ctx.plane_map_cull_batch(0, a, mode=lib.PLANE_CULL_DEVICE, rebuilt_capacity=1)
    check_resident(ctx, 0, a, *edited(a, host_result("stale_column_grows")))


def test_native_caller():
    """drfe::MapPlaneCulling of include/drfe_adaptor.hpp over mock MapPlane / KeyFrame classes (tests/native/plane_cull_caller.cpp)"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "plane_cull_caller")
    assert os.path.exists(exe), "tests/native/plane_cull_caller is built by build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plane_cull_caller ok" in r.stdout
