"""-m gpu tests of map-point and map-line triangulation on the device: drfe_triangulate_points_batch and
drfe_triangulate_lines_batch equal the host entries bit for bit at 0, 1, 63, 64, 65 and 100 000 matches, across many pairs in one
call; the counters add up; and on keyframes extracted from the synthetic room
sequence the chain SearchForTriangulation -> triangulation -> map-point upkeep (and its line counterpart) agrees on device, host
and numpy, with the accepted points on the scene's surfaces."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulate_numpy as TN  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("status", "branch", "x3d", "pair_skipped", "accepted")


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


def _same(got, want):
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k


def _first(scene, n):
    """the scene's first n matches (later pairs emptied)"""
    s = dict(scene)
    s["match_offsets"] = np.minimum(scene["match_offsets"], n).astype(np.int32)
    s["matches"] = scene["matches"][:n]
    return s


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(11)
    return {line: TN.random_scene(rng, n_kf=12, n_feat=1500, n_pairs=2200, line=line) for line in (False, True)}


@pytest.mark.parametrize("line", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100000])
def test_device_equals_host(ctx, big, line, n):
    from dr_slam_amd import lib
    scene = big[line]
    assert int(scene["match_offsets"][-1]) >= 100000
    s = _first(scene, n)
    host = (lib.triangulate_lines_host if line else lib.triangulate_points_host)(s)
    dev = (ctx.triangulate_lines_batch if line else ctx.triangulate_points_batch)(s)
    _same(dev, host)
    if n == 100000:
        assert len(set(host["status"].tolist())) >= 7 and (host["accepted"] > 0).sum() > 100


@pytest.mark.parametrize("line", [False, True])
def test_many_pairs_equal_numpy(ctx, line):
    """many small pairs in one call, device == host == numpy"""
    from dr_slam_amd import lib
    scene = TN.random_scene(np.random.default_rng(5), n_kf=8, n_feat=200, n_pairs=40, line=line)
    dev = (ctx.triangulate_lines_batch if line else ctx.triangulate_points_batch)(scene)
    _same(dev, (lib.triangulate_lines_host if line else lib.triangulate_points_host)(scene))
    _same(dev, TN.triangulate(scene, line))


def test_stats_count_the_calls():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    try:
        assert c.triangulate_stats() == dict.fromkeys(lib.TRI_STATS, 0)
        rng = np.random.default_rng(3)
        sp, sl = TN.random_scene(rng), TN.random_scene(rng, line=True)
        rp, rl = c.triangulate_points_batch(sp), c.triangulate_lines_batch(sl)
        c.triangulate_points_batch(_first(sp, 0))
        st = c.triangulate_stats()
        both = (rp, rl)
        assert st["calls"] == 3
        assert st["pairs"] == 2 * len(sp["kf1"]) + len(sl["kf1"])
        assert st["pairs_skipped"] == sum(int(r["pair_skipped"].sum()) for r in both) + int(rp["pair_skipped"].sum())
        assert st["matches"] == len(sp["matches"]) + len(sl["matches"])
        for key, b in (("svd", 1), ("stereo1", 2), ("stereo2", 3)):
            assert st[key] == sum(int((r["branch"] == b).sum()) for r in both)
        assert st["accepted"] == sum(int(r["accepted"].sum()) for r in both)
        assert st["svd"] > 0 and st["stereo1"] > 0 and st["stereo2"] > 0
    finally:
        c.close()


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


@pytest.fixture(scope="module")
def room():
    """three keyframes of the seed-2 room_boxes sequence, 0.1 m apart (above the stereo baseline mb = 0.075 m)"""
    from dr_slam_amd import synth
    return [next(synth.sequence(2, 1, start=k)) for k in (0, 10, 20)]


def test_chain_on_room_keyframes(room, oracle_mod):
    """extract, glue, BoW-transform, SearchForTriangulation, then triangulate (device == host == numpy), then map-point upkeep
    of the accepted points (device == host); the points lie on the rendered surfaces"""
    import torch
    from dr_slam_amd import lib, synth, vocabulary as V
    from dr_slam_amd.pipeline import FrontEnd
    cam = synth.TUM3
    fe = FrontEnd(cam, max_batch=4)
    try:
        gray = torch.from_numpy(np.stack([f[0] for f in room])).cuda()
        depth = torch.from_numpy(np.stack([f[1] for f in room]).view(np.int16)).cuda()
        fe.process(gray, depth, None, None, stream=torch.cuda.current_stream().cuda_stream)
        c = fe.ctx
        voc = V.make_synthetic(10, 4, seed=5, stop_fraction=0.02)
        voc.upload(c)
        c.bow_transform_batch(2, 3)
        scale, _, sigma2, _ = c.scale_tables()
        K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], np.float64)
        feats, kfs, desc = [], [], []
        for s, (_, _, Twc) in enumerate(room):
            kps, d = c.orb_download(s)
            n = len(kps)
            un = c.download_keys_un(s, n)
            ur, z = c.download_stereo(s)
            Tcw = np.linalg.inv(Twc.astype(np.float64))
            kfs.append(TN.keyframe(Tcw[:3, :3], Tcw[:3, 3], cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, 1.2))
            feats.append(dict(un=np.stack([un["x"], un["y"]], 1), raw=np.stack([kps["x"], kps["y"]], 1), octave=un["octave"],
                              u_right=ur[:n], depth=z[:n]))
            desc.append(d)
        offsets = np.concatenate([[0], np.cumsum([len(f["octave"]) for f in feats])]).astype(np.int32)
        scene = dict(kf=np.array(kfs), scale_factors=np.tile(scale, (3, 1)), level_sigma2=np.tile(sigma2, (3, 1)), offsets=offsets)
        for key in feats[0]:
            scene[key] = np.concatenate([f[key] for f in feats])
        kf1, kf2, mo, mt = [], [], [0], []
        for s1, s2 in ((0, 1), (1, 2), (0, 2), (2, 0)):
            Twc1, Twc2 = room[s1][2].astype(np.float64), room[s2][2].astype(np.float64)
            T1w, T2w = np.linalg.inv(Twc1), np.linalg.inv(Twc2)
            R12 = T1w[:3, :3] @ T2w[:3, :3].T
            t12 = -R12 @ T2w[:3, 3] + T1w[:3, 3]
            F12 = (np.linalg.inv(K).T @ _skew(t12) @ R12 @ np.linalg.inv(K)).astype(np.float32)
            none1 = np.full(offsets[s1 + 1] - offsets[s1], -1, np.int32)
            none2 = np.full(offsets[s2 + 1] - offsets[s2], -1, np.int32)
            n, m12 = c.search_for_triangulation(s1, s2, none1, none2, F12, Twc1[:3, 3].astype(np.float32),
                                                T2w.astype(np.float32), fe.cam, False, True)
            pairs = [(i, int(m12[i])) for i in range(len(m12)) if m12[i] >= 0]
            assert len(pairs) == n > 30
            kf1.append(s1)
            kf2.append(s2)
            mt += pairs
            mo.append(len(mt))
        scene.update(kf1=np.int32(kf1), kf2=np.int32(kf2), match_offsets=np.int32(mo), matches=np.int32(mt).reshape(-1, 2))
        dev = c.triangulate_points_batch(scene)
        host = lib.triangulate_points_host(scene)
        _same(dev, host)
        _same(dev, TN.triangulate(scene, False))
        assert not dev["pair_skipped"].any() and (dev["accepted"] > 20).all()
        ok = np.nonzero(dev["status"] == 0)[0]
        # on the surfaces: the point's depth in KF1 against the rendered depth at its keypoint
        near = 0
        for m in ok:
            p = np.searchsorted(mo, m, side="right") - 1
            s1 = kf1[p]
            T = np.linalg.inv(room[s1][2].astype(np.float64))
            Xc = T[:3, :3] @ dev["x3d"][m].astype(np.float64) + T[:3, 3]
            i1 = mt[m][0]
            u, v = feats[s1]["un"][i1]
            # keypoints sit on corners and edges: the nearest rendered depth within two pixels
            iu, iv = int(round(u)), int(round(v))
            zr = room[s1][1][max(iv - 2, 0):iv + 3, max(iu - 2, 0):iu + 3].astype(np.float64).ravel() / cam.depth_factor
            zr = zr[zr > 0]
            near += zr.size > 0 and np.abs(Xc[2] - zr).min() < 0.05 * Xc[2]
        # matches along the epipolar line of a repeated texture triangulate off the surface and still pass every gate, as in
        # the reference; a wrong pose or SVD would put almost none on it
        assert near >= 0.4 * len(ok)
        # the accepted points into drfe_map_point_upkeep_batch: observations (KF1, idx1), (KF2, idx2), reference KF1
        obs_kf, obs_desc, ref_level = [], [], []
        for m in ok:
            p = np.searchsorted(mo, m, side="right") - 1
            i1, i2 = mt[m]
            obs_kf += [kf1[p], kf2[p]]
            obs_desc += [desc[kf1[p]][i1], desc[kf2[p]][i2]]
            ref_level.append(feats[kf1[p]]["octave"][i1])
        up = dict(kf_center=np.stack([k["Ow"] for k in kfs]), kf_bad=None, scale_factors=scale, bad=None,
                  obs_offsets=np.arange(0, 2 * len(ok) + 1, 2, dtype=np.int32), obs_kf=np.int32(obs_kf),
                  obs_desc=np.array(obs_desc, np.uint8), world=dev["x3d"][ok],
                  ref_kf=np.int32([kf1[np.searchsorted(mo, m, side="right") - 1] for m in ok]), ref_level=np.int32(ref_level))
        ud = c.map_point_upkeep_batch(up)
        uh = lib.map_point_upkeep_host(up)
        for k in ud:
            assert ud[k].tobytes() == uh[k].tobytes(), k
        assert (ud["status"] == 3).all()
    finally:
        fe.ctx.close()


def test_line_chain_on_room_keyframes(ctx, room):
    """LSD extraction, Frame::isLineGood's 3-D lines (the intended double read of mK), LSDmatcher::SearchForTriangulation, then
    line triangulation (device == host == numpy) and map-line upkeep of the accepted lines (device == host)"""
    from dr_slam_amd import lib, synth
    cam = synth.TUM3
    K9 = np.array([cam.fx, 0, cam.cx, 0, cam.fy, cam.cy, 0, 0, 1], np.float32)
    invfx, invfy = float(np.float32(1) / np.float32(cam.fx)), float(np.float32(1) / np.float32(cam.fy))
    feats, kfs, desc = [], [], []
    for g, dpt, Twc in room:
        a = ctx.lsd_extract(g)
        L = a["lines"]
        dl, l3, _, _ = lib.lines_is_good(L, dpt.astype(np.float32) / np.float32(cam.depth_factor), K9, cam.cx, cam.cy, invfx, invfy,
                                         k_as_f64=True)
        Tcw = np.linalg.inv(Twc.astype(np.float64))
        kfs.append(TN.keyframe(Tcw[:3, :3], Tcw[:3, 3], cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, 1.2))
        feats.append(dict(ends=np.stack([L["start_point_x"], L["start_point_y"], L["end_point_x"], L["end_point_y"]], 1),
                          octave=L["octave"].astype(np.int32), depth=dl, lines3d=l3))
        desc.append(a["desc"])
    assert sum(int((f["depth"] > 0).sum()) for f in feats) > 20
    sc, sg = TN.scale_tables()
    offsets = np.concatenate([[0], np.cumsum([len(f["octave"]) for f in feats])]).astype(np.int32)
    scene = dict(kf=np.array(kfs), scale_factors=np.tile(sc, (3, 1)), level_sigma2=np.tile(sg, (3, 1)), offsets=offsets)
    for key in feats[0]:
        scene[key] = np.concatenate([f[key] for f in feats])
    kf1, kf2, mo, mt = [], [], [0], []
    for s1, s2 in ((0, 1), (1, 2), (0, 2), (2, 0)):
        h1 = np.zeros(len(desc[s1]), np.uint8)
        h2 = np.zeros(len(desc[s2]), np.uint8)
        n, m12 = ctx.lsd_search_for_triangulation(desc[s1], desc[s2], h1, h2)
        pairs = [(i, int(m12[i])) for i in range(len(m12)) if m12[i] >= 0]
        kf1.append(s1)
        kf2.append(s2)
        mt += pairs
        mo.append(len(mt))
    scene.update(kf1=np.int32(kf1), kf2=np.int32(kf2), match_offsets=np.int32(mo), matches=np.int32(mt).reshape(-1, 2))
    dev = ctx.triangulate_lines_batch(scene)
    _same(dev, lib.triangulate_lines_host(scene))
    _same(dev, TN.triangulate(scene, True))
    ok = np.nonzero((dev["status"] & 0x7F) == 0)[0]
    assert len(ok) > 5
    obs_kf, obs_desc, ref_level, ref_kf = [], [], [], []
    for m in ok:
        p = np.searchsorted(mo, m, side="right") - 1
        i1, i2 = mt[m]
        obs_kf += [kf1[p], kf2[p]]
        obs_desc += [desc[kf1[p]][i1], desc[kf2[p]][i2]]
        ref_kf.append(kf1[p])
        ref_level.append(feats[kf1[p]]["octave"][i1])
    up = dict(kf_center=np.stack([k["Ow"] for k in kfs]), kf_bad=None, scale_factors=sc, bad=None,
              obs_offsets=np.arange(0, 2 * len(ok) + 1, 2, dtype=np.int32), obs_kf=np.int32(obs_kf),
              obs_desc=np.array(obs_desc, np.uint8), world=dev["x3d"][ok].astype(np.float64), ref_kf=np.int32(ref_kf),
              ref_level=np.int32(ref_level))
    ud = ctx.map_line_upkeep_batch(up)
    uh = lib.map_line_upkeep_host(up)
    for k in ud:
        assert ud[k].tobytes() == uh[k].tobytes(), k
    assert (ud["status"] == 3).all()
