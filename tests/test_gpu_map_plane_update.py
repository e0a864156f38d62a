"""-m gpu tests of map-plane upkeep on the device: drfe_plane_map_update_batch,
drfe_plane_map_rebuild_batch and drfe_plane_map_edit on the resident maps of drfe_plane_map_upload equal the host entries
(drfe_map_plane_update_host, drfe_map_plane_rebuild_host, drfe_plane_match_host) bit for bit: a live match -> update -> match
sequence with nothing re-uploaded, many maps and several frames per map in one call, one map plane hit twice in a frame,
clouds that outgrow their slots and the uploaded total, appended planes rebuilt from observations, and a job the device hands
back to the host."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_plane_numpy as MN  # noqa: E402
import plane_match_numpy as PN  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def _same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_clouds(c, maps, host):
    for s, m in enumerate(maps):
        for j in range(len(m["coefs"])):
            assert _same(c.plane_map_cloud_download(s, j), host[s][j]), (s, j)


def _host_updates(host, frame_map, Tcw, fclouds, map_idx):
    """the per-frame form in call order on host-held clouds"""
    from dr_slam_amd import lib
    for f, s in enumerate(frame_map):
        for q, j in enumerate(map_idx[f]):
            if j >= 0:
                host[s][j] = lib.map_plane_update_host(Tcw[f], fclouds[f][q], host[s][j])


def _pipeline_scene(cam, kind, seed, n_frames):
    """planes_ahc + planes_ahc_postprocess of n_frames synthetic frames: a map from the even frames' planes moved into world,
    and every frame's (Tcw, coefficients, camera-frame voxel clouds)"""
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
            obs.append((np.linalg.inv(Twc).astype(f32), Twc, g["post"]["coef"][acc].astype(f32), [g["voxels"][i].copy() for i in acc]))
    finally:
        c.close()
    coefs, clouds, points = [], [], []
    for Tcw, Twc, cf, vox in obs[0::2]:
        for k in range(len(cf)):
            coefs.append(PN.world_coef(Tcw, cf[k]))
            w = (Twc[:3, :3] @ vox[k].astype(np.float64).T).T + Twc[:3, 3]
            clouds.append(w.astype(f32))
            points.append(w[::7])
    bad = np.zeros(len(coefs), np.uint8)
    bad[::5] = 1
    mp = dict(coefs=np.asarray(coefs, f32).reshape(-1, 4), bad=bad, clouds=clouds, points=np.vstack(points).astype(f32))
    frames = [dict(Tcw=Tcw, coefs=cf, clouds=vox) for Tcw, _, cf, vox in obs]
    return mp, frames


@pytest.mark.timeout(900)
@pytest.mark.parametrize("camname,kind,seed", [("TUM3", "room_boxes", 2), ("ICL", "living_room", 3)])
def test_live_sequence_match_update_match(camname, kind, seed):
    """match, then update with map_idx NULL (the device's own decisions), then match the next frame: per frame the indices,
    counts and flags equal the host loop's, and the final clouds are equal bit for bit"""
    import torch
    from dr_slam_amd import lib, synth
    mp, frames = _pipeline_scene(getattr(synth, camname), kind, seed, 10)
    assert len(mp["coefs"]) >= 4 and len(frames) >= 8
    host = [[cl.copy() for cl in mp["clouds"]]]
    c = lib.Context()
    stream = torch.cuda.current_stream().cuda_stream
    updated = 0
    try:
        c.plane_map_upload([mp])
        for f, fr in enumerate(frames):
            c.plane_match_batch([0], fr["Tcw"][None], [fr["coefs"]], flag_points=True, stream=stream)
            mi, pi, vi, n, npair = c.plane_match_download(0)
            h = lib.plane_match_host(fr["Tcw"], fr["coefs"], mp["coefs"], mp["bad"], host[0])
            assert np.array_equal(mi, h[0]) and np.array_equal(pi, h[1]) and np.array_equal(vi, h[2]) and n == h[3], f
            fl, hp = lib.plane_flag_points_host(fr["Tcw"], fr["coefs"], h[0], mp["points"])
            assert npair == hp and np.array_equal(c.plane_flags_download(0), fl), f
            c.plane_map_update_batch([0], fr["Tcw"][None], [fr["clouds"]], map_idx=None, stream=stream)
            _host_updates(host, [0], [fr["Tcw"]], [fr["clouds"]], [h[0]])
            updated += int((h[0] >= 0).sum())
        _check_clouds(c, [mp], host)
        st = c.plane_map_update_stats()
        assert updated > 0 and st["device_jobs"] + st["host_jobs"] == updated
    finally:
        c.close()
    assert any(len(host[0][j]) != len(mp["clouds"][j]) for j in range(len(mp["clouds"])))


def _scene_maps(rng, n_maps, cloud=1500):
    maps = []
    for s in range(n_maps):
        _, _, mc, bad, clouds, pts = PN.random_scene(200 + s, n_map=12 + s, n_planes=4, cloud=cloud, n_points=1000, special=False)
        maps.append(dict(coefs=mc, bad=bad, clouds=clouds, points=pts))
    return maps


def _frame_clouds(rng, n, size=(200, 2500), extent=1.5):
    return [MN.plane_cloud(rng, int(rng.integers(*size)), center=rng.normal(0, 1, 3) + [0, 0, 2], normal=rng.normal(0, 1, 3),
                           extent=extent) for _ in range(n)]


@pytest.mark.timeout(900)
def test_many_maps_several_frames_per_map_and_a_plane_hit_twice():
    """8 maps, 3 frames of each in one call (interleaved), explicit map_idx with -1 entries and one map plane named twice
    within a frame: the updates chain in (frame, frame plane) order"""
    import torch
    from dr_slam_amd import lib
    rng = np.random.default_rng(11)
    maps = _scene_maps(rng, 8)
    host = [[cl.copy() for cl in m["clouds"]] for m in maps]
    frame_map, Tcw, fclouds, midx = [], [], [], []
    for r in range(3):
        for s in range(8):
            P = 4 if (r, s) == (0, 2) else int(rng.integers(0, 6)) if (r + s) % 4 else 0
            M = len(maps[s]["coefs"])
            mi = np.where(rng.random(P) < 0.75, rng.integers(0, M, P), -1).astype(np.int32)
            if P >= 2 and s % 2 == 0:
                mi[-1] = mi[0] = int(rng.integers(0, M))       # one map plane twice in this frame
            frame_map.append(s)
            Tcw.append(MN.random_pose(rng))
            fclouds.append(_frame_clouds(rng, P))
            midx.append(mi)
    c = lib.Context()
    try:
        c.plane_map_upload(maps)
        c.plane_map_update_batch(frame_map, np.stack(Tcw), fclouds, map_idx=midx, stream=torch.cuda.current_stream().cuda_stream)
        _host_updates(host, frame_map, Tcw, fclouds, midx)
        _check_clouds(c, maps, host)
        st = c.plane_map_update_stats()
        assert st["rounds"] >= 2 and st["device_jobs"] + st["host_jobs"] == sum(int((m >= 0).sum()) for m in midx)
        # a match over the updated clouds equals the host entry on the host's clouds
        fr = [(s, *PN.random_scene(300 + s, n_map=len(maps[s]["coefs"]), n_planes=6)[:2]) for s in range(8)]
        c.plane_match_batch([s for s, _, _ in fr], np.stack([T for _, T, _ in fr]), [cf for _, _, cf in fr], flag_points=False)
        for f, (s, T, cf) in enumerate(fr):
            mi, pi, vi, n, _ = c.plane_match_download(f)
            h = lib.plane_match_host(T, cf, maps[s]["coefs"], maps[s]["bad"], host[s])
            assert np.array_equal(mi, h[0]) and np.array_equal(pi, h[1]) and np.array_equal(vi, h[2]) and n == h[3], f
    finally:
        c.close()


@pytest.mark.timeout(900)
def test_clouds_outgrow_their_slots_and_the_upload_then_match():
    """tiny uploaded clouds, wide frame clouds: every updated cloud and the total outgrow the upload (the arena is repacked),
    and a match over the grown clouds still equals the host entry"""
    from dr_slam_amd import lib
    rng = np.random.default_rng(12)
    _, _, mc, bad, clouds, pts = PN.random_scene(77, n_map=40, n_planes=6, cloud=20, n_points=3000, special=False)
    mp = dict(coefs=mc, bad=bad, clouds=clouds, points=pts)
    total0 = sum(len(cl) for cl in clouds)
    host = [[cl.copy() for cl in clouds]]
    c = lib.Context()
    try:
        c.plane_map_upload([mp])
        for step in range(3):
            P = 12
            Tcw = MN.random_pose(rng)
            fcl = _frame_clouds(rng, P, size=(8000, 20000), extent=4.0)
            mi = rng.choice(len(mc), P, replace=False).astype(np.int32)
            c.plane_map_update_batch([0], Tcw[None], [fcl], map_idx=[mi])
            _host_updates(host, [0], [Tcw], [fcl], [mi])
        _check_clouds(c, [mp], host)
        assert sum(len(cl) for cl in host[0]) > 10 * total0 and max(len(cl) for cl in host[0]) > 20000
        assert c.plane_map_update_stats()["repacks"] >= 1
        frames = []
        for _ in range(4):
            T = MN.random_pose(rng, 0.1)
            w = mc[rng.integers(0, len(mc), 8)].astype(np.float64)
            frames.append((T, (np.linalg.inv(T.astype(np.float64)).T @ w.T).T.astype(f32)))
        c.plane_match_batch([0] * 4, np.stack([T for T, _ in frames]), [cf for _, cf in frames], flag_points=False)
        nm = 0
        for f, (T, cf) in enumerate(frames):
            mi, pi, vi, n, _ = c.plane_match_download(f)
            h = lib.plane_match_host(T, cf, mc, bad, host[0])
            assert np.array_equal(mi, h[0]) and np.array_equal(pi, h[1]) and np.array_equal(vi, h[2]) and n == h[3], f
            nm += n
        assert nm > 0
    finally:
        c.close()


@pytest.mark.timeout(900)
def test_edit_append_rebuild_then_match():
    """append planes (empty clouds), set coefficients and a bad flag, rebuild appended and existing planes from keyframe
    observations, then match: clouds and decisions equal the host"""
    from dr_slam_amd import lib
    rng = np.random.default_rng(13)
    maps = _scene_maps(rng, 3)
    host = [[cl.copy() for cl in m["clouds"]] for m in maps]
    coefs = [m["coefs"].copy() for m in maps]
    bad = [m["bad"].copy() for m in maps]
    c = lib.Context()
    try:
        c.plane_map_upload(maps)
        M1 = len(coefs[1])
        new = np.array([[0, 0, 1, -2], [1, 0, 0, 0.5], [0, 1, 0, 1]], f32)
        c.plane_map_edit(1, [M1, M1 + 1, M1 + 2], coefs=new)                       # appended, empty
        c.plane_map_edit(1, [0, 2], coefs=new[:2], bad=[1, 0])                   # SetWorldPos + SetBadFlag
        c.plane_map_edit(0, [1], bad=[1])
        coefs[1] = np.vstack([coefs[1], new])
        coefs[1][[0, 2]] = new[:2]
        bad[1] = np.r_[bad[1], [0, 0, 0]].astype(np.uint8)
        bad[1][[0, 2]] = [1, 0]
        bad[0][1] = 1
        host[1] += [np.zeros((0, 3), f32)] * 3
        for j in range(M1, M1 + 3):
            assert c.plane_map_cloud_download(1, j).shape == (0, 3)
        jobs = []
        for s, j in [(1, M1), (1, M1 + 1), (1, M1 + 2), (0, 3), (2, 0), (1, M1)]:     # (1, M1) twice: the last one wins
            k = int(rng.integers(0, 5))
            obs = [(MN.random_pose(rng), MN.plane_cloud(rng, int(rng.integers(100, 3000)), extent=1.0)) for _ in range(k)]
            jobs.append((s, j, obs))
            host[s][j] = lib.map_plane_rebuild_host([o[0] for o in obs], [o[1] for o in obs])
        c.plane_map_rebuild_batch(jobs)
        ms = [dict(coefs=coefs[s]) for s in range(3)]
        _check_clouds(c, ms, host)
        fr = []
        for s in range(3):
            T = MN.random_pose(rng, 0.1)
            w = coefs[s][rng.integers(0, len(coefs[s]), 6)].astype(np.float64)
            fr.append((s, T, (np.linalg.inv(T.astype(np.float64)).T @ w.T).T.astype(f32)))
        c.plane_match_batch([s for s, _, _ in fr], np.stack([T for _, T, _ in fr]), [cf for _, _, cf in fr], flag_points=False)
        for f, (s, T, cf) in enumerate(fr):
            mi, pi, vi, n, _ = c.plane_match_download(f)
            h = lib.plane_match_host(T, cf, coefs[s], bad[s], host[s])
            assert np.array_equal(mi, h[0]) and np.array_equal(pi, h[1]) and np.array_equal(vi, h[2]) and n == h[3], f
    finally:
        c.close()


@pytest.mark.timeout(600)
def test_job_handed_back_to_the_host():
    """a frame cloud spread wide enough to overflow the voxel grid's int32 leaf index: the device hands the job back, the host
    redoes it (PCL returns the input), the next round chains on it, and the counter shows it"""
    from dr_slam_amd import lib
    rng = np.random.default_rng(14)
    maps = _scene_maps(rng, 1)
    host = [[cl.copy() for cl in maps[0]["clouds"]]]
    wide = rng.uniform(-800, 800, (60, 3)).astype(f32)
    T = [MN.random_pose(rng), MN.random_pose(rng)]
    fcl = [[wide, MN.plane_cloud(rng, 900)], [MN.plane_cloud(rng, 500)]]
    mi = [np.array([2, 5], np.int32), np.array([2], np.int32)]
    c = lib.Context()
    try:
        c.plane_map_upload(maps)
        c.plane_map_update_batch([0, 0], np.stack(T), fcl, map_idx=mi)
        _host_updates(host, [0, 0], T, fcl, mi)
        _check_clouds(c, maps, host)
        st = c.plane_map_update_stats()
        assert st["host_jobs"] == 2 and st["device_jobs"] == 1 and st["rounds"] == 2
        assert len(host[0][2]) == 500 + 60 + len(maps[0]["clouds"][2])          # both times the input came back whole
    finally:
        c.close()


@pytest.mark.timeout(300)
def test_bad_arguments_are_rejected():
    from dr_slam_amd import lib
    rng = np.random.default_rng(15)
    T = np.eye(4, dtype=f32)[None]
    cl = [[np.zeros((3, 3), f32)]]
    c = lib.Context()
    try:
        with pytest.raises(lib.DrfeError):
            c.plane_map_update_batch([0], T, cl, map_idx=[[0]])                    # nothing uploaded
        maps = _scene_maps(rng, 1)
        M = len(maps[0]["coefs"])
        c.plane_map_upload(maps)
        with pytest.raises(lib.DrfeError):
            c.plane_map_update_batch([1], T, cl, map_idx=[[0]])                    # no map 1
        with pytest.raises(lib.DrfeError):
            c.plane_map_update_batch([0], T, cl, map_idx=[[M]])                    # no such plane
        with pytest.raises(lib.DrfeError):
            c.plane_map_update_batch([0], T, cl, map_idx=None)                     # no match batch to take decisions from
        c.plane_match_batch([0], T, [np.zeros((2, 4), f32)], flag_points=False)
        with pytest.raises(lib.DrfeError):
            c.plane_map_update_batch([0], T, cl, map_idx=None)                     # other frame planes than that batch
        with pytest.raises(lib.DrfeError):
            c.plane_map_edit(0, [M + 1], coefs=np.zeros((1, 4), f32))              # past the end
        with pytest.raises(lib.DrfeError):
            c.plane_map_edit(0, [M], bad=[1])                                       # appending needs coefficients
        with pytest.raises(lib.DrfeError):
            c.plane_map_rebuild_batch([(0, M, [])])
        with pytest.raises(lib.DrfeError):
            c.plane_map_cloud_download(0, M)
        assert c.plane_map_cloud_download(0, 0).shape == maps[0]["clouds"][0].shape
    finally:
        c.close()
