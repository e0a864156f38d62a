"""-m gpu tests of device plane association: drfe_plane_map_upload + drfe_plane_match_batch +
drfe_plane_match_download / drfe_plane_flags_download equal the host entries (drfe_plane_match_host,
drfe_plane_flag_points_host) bit for bit - indices, counts and flags - on maps built from the plane pipeline's own output,
on synthetic maps whose clouds span many work items, with many maps in one call, frames without planes and all-bad maps;
two device frames also equal the numpy restatement (tests/plane_match_numpy.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_match_numpy as PN  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def _run(maps, frames, numpy_frames=(), params=None, repeat=1):
    """maps: dicts(coefs, bad, clouds, points); frames: dicts(map, Tcw, coefs, priors (3 arrays or None)).  Device batch vs
    host entries on every frame; flags of each map vs the OR of the host entry over that map's frames."""
    import torch
    from dr_slam_amd import lib
    prm = PN.DEFAULTS if params is None else params
    c = lib.Context()
    totals = np.zeros(3, int)
    try:
        c.plane_map_upload(maps)
        stream = torch.cuda.current_stream().cuda_stream
        pri = [[(fr.get("priors") or (None, None, None))[k] for fr in frames] for k in range(3)]
        for _ in range(repeat):                    # a second call on the same buffers: the accumulators are reset
            c.plane_match_batch([fr["map"] for fr in frames], np.stack([fr["Tcw"] for fr in frames]), [fr["coefs"] for fr in frames],
                                *pri, flag_points=True, params=np.array(prm, f32), stream=stream)
        want_flags = [np.zeros(len(m["points"]), np.uint8) for m in maps]
        for f, fr in enumerate(frames):
            m = maps[fr["map"]]
            mi, pi, vi, n, npair = c.plane_match_download(f)
            h = lib.plane_match_host(fr["Tcw"], fr["coefs"], m["coefs"], m["bad"], m["clouds"], *(fr.get("priors") or (None,) * 3),
                                     params=np.array(prm, f32))
            assert np.array_equal(mi, h[0]) and np.array_equal(pi, h[1]) and np.array_equal(vi, h[2]) and n == h[3], (f, mi, h)
            fl, hp = lib.plane_flag_points_host(fr["Tcw"], fr["coefs"], h[0], m["points"], want_flags[fr["map"]])
            want_flags[fr["map"]] = fl
            assert npair == hp, (f, npair, hp)
            if f in numpy_frames:
                w = PN.search_map_by_coefficients(fr["Tcw"], fr["coefs"], m["coefs"], m["bad"], m["clouds"],
                                                  *(fr.get("priors") or (None,) * 3), params=prm)
                assert all(np.array_equal(a, b) for a, b in zip((mi, pi, vi), w[:3])) and n == w[3]
                assert npair == PN.flag_matched_plane_points(fr["Tcw"], fr["coefs"], mi, m["points"])[1]
            totals += [n, npair, (pi >= 0).sum()]
        for s in range(len(maps)):
            assert np.array_equal(c.plane_flags_download(s), want_flags[s]), s
    finally:
        c.close()
    return totals


def _pipeline_map(cam, kind, seed, n_frames):
    """planes_ahc + planes_ahc_postprocess (accepted coefficients, voxel clouds) of n_frames synthetic frames; the map holds
    the planes of the even frames moved into world by their poses, the odd frames observe it"""
    from dr_slam_amd import lib, synth
    seq = list(synth.sequence(seed, n_frames, cam=cam, kind=kind))
    inv = float(np.float32(1.0) / np.float32(cam.depth_factor))
    K4 = np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float32)
    c = lib.Context(max_width=cam.w, max_height=cam.h)
    obs = []
    try:
        for _, d, Twc in seq:
            g = c.planes_ahc_postprocess(d, K4, inv, c.planes_ahc(d, K4, inv), 9.0, 0.10)
            acc = np.flatnonzero(g["post"]["accepted"])
            obs.append((np.linalg.inv(Twc).astype(f32), Twc, g["post"]["coef"][acc].astype(f32), [g["voxels"][i] for i in acc]))
    finally:
        c.close()
    coefs, clouds, points = [], [], []
    for Tcw, Twc, cf, vox in obs[0::2]:
        for k in range(len(cf)):
            coefs.append(PN.world_coef(Tcw, cf[k]))
            w = (Twc[:3, :3] @ vox[k].astype(np.float64).T).T + Twc[:3, 3]
            clouds.append(w.astype(f32))
            points.append(w[::7])
    rng = np.random.default_rng(seed)
    pts = np.vstack(points + [rng.uniform(-3, 3, (5000, 3))]).astype(f32)
    bad = np.zeros(len(coefs), np.uint8)
    bad[::5] = 1
    mp = dict(coefs=np.asarray(coefs, f32).reshape(-1, 4), bad=bad, clouds=clouds, points=pts)
    frames = [dict(map=0, Tcw=Tcw, coefs=cf) for Tcw, _, cf, _ in obs]
    return mp, frames


@pytest.mark.timeout(600)
@pytest.mark.parametrize("camname,kind,seed", [("TUM3", "room_boxes", 2), ("ICL", "living_room", 3)])
def test_device_equals_host_on_pipeline_maps(camname, kind, seed):
    from dr_slam_amd import synth
    mp, frames = _pipeline_map(getattr(synth, camname), kind, seed, 8)
    assert len(mp["coefs"]) >= 4 and sum(len(f["coefs"]) for f in frames) >= 8
    tot = _run([mp], frames, numpy_frames=(1, 3), repeat=2)
    assert tot[0] > 0 and tot[1] > 0


def _observe(map_coefs, rng, P):
    """a random pose and P camera-frame planes near planes of the map (pM = Tcw^T c)"""
    a = rng.normal(0, 0.3, 3)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Tcw = np.eye(4)
    Tcw[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    Tcw[:3, 3] = rng.normal(0, 1, 3)
    Tcw = Tcw.astype(f32)
    w = map_coefs[rng.integers(0, len(map_coefs), P)].astype(np.float64)
    w[:, :3] += rng.normal(0, 0.02, (P, 3))
    w[:, 3] += rng.normal(0, 0.08, P)
    return Tcw, (np.linalg.inv(Tcw.astype(np.float64)).T @ w.T).T.astype(f32)


@pytest.mark.timeout(900)
def test_device_equals_host_with_clouds_spanning_many_work_items():
    """clouds up to 20 k points (10 work items of 2 048), 100 k map points, 200 map planes"""
    rng = np.random.default_rng(7)
    Tcw, coefs, mc, bad, clouds, pts = PN.random_scene(11, n_map=200, n_planes=10, cloud=20000, n_points=100000)
    clouds[1] = np.vstack([clouds[1], rng.uniform(-2, 2, (20000, 3)).astype(f32)])   # one cloud past 20 k
    mp = dict(coefs=mc, bad=bad, clouds=clouds, points=pts)
    frames = [dict(map=0, Tcw=Tcw, coefs=coefs)]
    for k in range(5):
        T2, c2 = _observe(mc, rng, 10)
        frames.append(dict(map=0, Tcw=T2, coefs=c2))
    tot = _run([mp], frames, numpy_frames=(0,))
    assert tot[0] > 0 and tot[1] > 0


@pytest.mark.timeout(900)
def test_many_maps_in_one_call_with_empty_frames_and_all_bad_maps():
    rng = np.random.default_rng(3)
    maps, frames = [], []
    for s in range(8):
        Tcw, coefs, mc, bad, clouds, pts = PN.random_scene(40 + s, n_map=30 + 5 * s, n_planes=8, cloud=3000, n_points=20000 + 1000 * s)
        if s == 5:
            bad = np.ones_like(bad)                # an all-bad map: nothing is matched, nothing parallel or vertical
        maps.append(dict(coefs=mc, bad=bad, clouds=clouds, points=pts))
    for f in range(64):
        s = f % 8
        P = int(rng.integers(0, 9)) if f % 5 else 0               # every fifth frame has no planes
        Tcw, coefs = _observe(maps[s]["coefs"], rng, P)
        pri = None
        if f % 3 == 0:
            pri = tuple(np.where(rng.random(P) < 0.5, rng.integers(0, len(maps[s]["coefs"]), P), -1).astype(np.int32)
                        for _ in range(3))
        frames.append(dict(map=s, Tcw=Tcw, coefs=coefs, priors=pri))
    tot = _run(maps, frames, numpy_frames=(2, 13), repeat=2)
    assert tot[0] > 0 and tot[1] > 0 and tot[2] > 0


@pytest.mark.timeout(300)
def test_device_rejects_bad_arguments():
    from dr_slam_amd import lib
    c = lib.Context()
    try:
        with pytest.raises(lib.DrfeError):
            c.plane_match_batch([0], np.eye(4, dtype=f32)[None], [np.zeros((1, 4), f32)])      # nothing uploaded
        c.plane_map_upload([dict(coefs=np.zeros((1, 4), f32), bad=[0], clouds=[np.zeros((3, 3), f32)], points=np.zeros((2, 3), f32))])
        with pytest.raises(lib.DrfeError):
            c.plane_match_batch([1], np.eye(4, dtype=f32)[None], [np.zeros((1, 4), f32)])      # no map 1
    finally:
        c.close()
