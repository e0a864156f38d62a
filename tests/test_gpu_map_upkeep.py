"""-m gpu tests of map-point and map-line upkeep on the device: drfe_map_point_upkeep_batch and
drfe_map_line_upkeep_batch equal the host entries bit for bit on batches that cover every bucket boundary (N and N + 1 at 4,
16, 64 and the device row cap), on items handed back to the host above the cap, on observation lists built from descriptors
extracted from the synthetic room sequence, on an empty call and on repeated calls on one context; and the device's frustum
records and descriptors feed drfe_frame_is_in_frustum + drfe_search_by_projection_map exactly as records built from the host
entry's results do."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_upkeep_numpy as MU  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("best_obs", "desc", "normal", "max_distance", "min_distance", "status", "frustum")
BOUNDS = (1, 2, 4, 5, 16, 17, 64, 65, 300)


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


def _assert_same(got, want):
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k


def _host(scene, line, what=3):
    from dr_slam_amd import lib
    return (lib.map_line_upkeep_host if line else lib.map_point_upkeep_host)(scene, what)


def _device(ctx, scene, line, what=3):
    return (ctx.map_line_upkeep_batch if line else ctx.map_point_upkeep_batch)(scene, what)


def _counts(rng, n, tail):
    """mostly 2-10 observations, every bucket boundary a few times, a heavy tail"""
    c = np.concatenate([rng.integers(2, 11, n), np.repeat(BOUNDS, 6), [0, 0, 0], rng.integers(11, tail + 1, n // 100)])
    rng.shuffle(c)
    return c


@pytest.mark.parametrize("line,n", [(False, 10000), (True, 2000)])
def test_device_equals_host_on_bucket_boundaries(ctx, line, n):
    rng = np.random.default_rng(11 + line)
    scene = MU.random_scene(rng, _counts(rng, n, 400), line=line, n_kf=512, flips=(0, 12))
    before = ctx.map_upkeep_stats()
    got = _device(ctx, scene, line)
    _assert_same(got, _host(scene, line))
    st = ctx.map_upkeep_stats()
    for b in ("desc_b4", "desc_b16", "desc_b64", "desc_wg"):
        assert st[b] > before[b], b
    assert st["desc_host"] == before["desc_host"] and st["normals"] - before["normals"] == int((got["status"] & 2 != 0).sum())
    for what in (1, 2):
        _assert_same(_device(ctx, scene, line, what), _host(scene, line, what))


@pytest.mark.parametrize("line", [False, True])
def test_items_above_the_cap_are_handed_back(ctx, line):
    from dr_slam_amd import lib
    cap = lib.UPKEEP_DEVICE_ROWS
    rng = np.random.default_rng(21 + line)
    counts = np.array([3, cap, cap + 1, 7, cap + 40, 65], np.int64)
    scene = MU.random_scene(rng, counts, line=line, n_kf=4096, p_bad_kf=0.0, p_bad_item=0.0, flips=(0, 40))
    before = ctx.map_upkeep_stats()
    got = _device(ctx, scene, line)
    st = ctx.map_upkeep_stats()
    assert st["desc_host"] - before["desc_host"] == 2 and st["desc_wg"] - before["desc_wg"] == 2
    _assert_same(got, _host(scene, line))


def test_empty_call_and_repeated_calls(ctx):
    empty = dict(kf_center=np.zeros((0, 3), np.float32), scale_factors=MU.scale_factors(), obs_offsets=np.zeros(1, np.int32),
                 obs_kf=np.zeros(0, np.int32), obs_desc=np.zeros((0, 32), np.uint8), world=np.zeros((0, 3), np.float32),
                 ref_kf=np.zeros(0, np.int32), ref_level=np.zeros(0, np.int32))
    calls = ctx.map_upkeep_stats()["calls"]
    assert len(ctx.map_point_upkeep_batch(empty)["status"]) == 0
    assert ctx.map_upkeep_stats()["calls"] == calls + 1
    rng = np.random.default_rng(31)
    for k in range(6):
        line = k % 2 == 1
        scene = MU.random_scene(rng, _counts(rng, int(rng.integers(50, 3000)), 120), line=line)
        _assert_same(_device(ctx, scene, line), _host(scene, line))


def _room_map(n_frames=8):
    """map points from frame 0's keypoints with depth; every frame observes a point through its best Hamming match (keyframe
    f, keypoint idx), so the observation lists hold real extracted descriptors at realistic distances"""
    import torch
    from dr_slam_amd import synth
    from dr_slam_amd.pipeline import FrontEnd
    cam = synth.TUM3
    frames = list(synth.sequence(2, n_frames, cam=cam))
    fe = FrontEnd(cam, max_batch=n_frames)
    gray = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    depth = torch.from_numpy(np.stack([f[1] for f in frames]).view(np.int16)).cuda()
    Twc = np.stack([f[2] for f in frames]).astype(np.float32)
    Tcw = np.linalg.inv(Twc.astype(np.float64)).astype(np.float32)
    fe.process(gray, depth, Tcw, Twc, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    kd = [fe.keypoints(s) for s in range(n_frames)]
    _, z = fe.ctx.download_stereo(0)
    kps0, d0 = kd[0]
    n0 = len(kps0)
    z = z[:n0]
    keep = np.flatnonzero(z > 0)[:600]
    x = np.stack([(kps0["x"][keep] - cam.cx) * z[keep] / cam.fx, (kps0["y"][keep] - cam.cy) * z[keep] / cam.fy, z[keep]], 1)
    world = (x.astype(np.float64) @ Twc[0][:3, :3].T.astype(np.float64) + Twc[0][:3, 3]).astype(np.float32)
    bits = [np.unpackbits(d, axis=1) for _, d in kd]
    obs_kf, obs_desc, off, level = [], [], [0], []
    for j, i in enumerate(keep):
        q = np.unpackbits(d0[i])
        for f in range(n_frames):
            dist = (bits[f] != q).sum(1)
            m = int(np.argmin(dist))
            if f == 0 or dist[m] <= 80:
                obs_kf.append(f)
                obs_desc.append(kd[f][1][m])
        off.append(len(obs_kf))
        level.append(int(kps0["octave"][i]))
    n = len(keep)
    scene = dict(kf_center=Twc[:, :3, 3].copy(), kf_bad=np.zeros(n_frames, np.uint8), scale_factors=MU.scale_factors(),
                 bad=np.zeros(n, np.uint8), obs_offsets=np.int32(off), obs_kf=np.int32(obs_kf), obs_desc=np.array(obs_desc, np.uint8),
                 world=world, ref_kf=np.zeros(n, np.int32), ref_level=np.int32(level))
    return fe, Tcw, scene, [len(k) for k, _ in kd]


def test_real_descriptors_and_chaining_into_the_matchers(ctx):
    from dr_slam_amd import lib
    fe, Tcw, scene, nkp = _room_map()
    try:
        n = len(scene["obs_offsets"]) - 1
        assert n > 300 and len(scene["obs_kf"]) > 3 * n
        scene["kf_bad"][5] = 1
        host = _host(scene, False)
        dev = _device(ctx, scene, False)
        _assert_same(dev, host)
        assert len(set(host["best_obs"].tolist())) > 3
        # records as drfe_adaptor.hpp's frustum_of builds them from the host results
        rec = np.zeros(n, lib.FRUSTUM_POINT_DTYPE)
        rec["world"] = scene["world"]
        rec["normal"] = host["normal"]
        rec["min_distance"] = (np.float32(0.8) * host["min_distance"]).astype(np.float32)
        rec["max_distance"] = (np.float32(1.2) * host["max_distance"]).astype(np.float32)
        assert rec.tobytes() == dev["frustum"].tobytes()
        slot = 3
        outs = []
        for records, desc in ((rec, host["desc"]), (dev["frustum"], dev["desc"])):
            tp = fe.ctx.is_in_frustum(Tcw[slot], fe.cam, records, 0.5)
            tp["desc"] = desc
            tp["obs_positive"] = 1
            outs.append((tp.copy(), fe.ctx.search_by_projection_map(slot, tp, nkp[slot], 3.0, 0.8)))
        (ta, (na, ma)), (tb, (nb, mb)) = outs
        assert ta.tobytes() == tb.tobytes() and na == nb and np.array_equal(ma, mb)
        assert ta["track_in_view"].sum() > 100 and na > 50
    finally:
        fe.ctx.close()
