"""-m gpu tests of the device Manhattan-frame tracker: drfe_manhattan_track_batch over the records the
surface-normal batch left on the device, then drfe_manhattan_download, equals drfe_manhattan_track_host fed the downloaded
records and chained frame to frame the same way, bit for bit (R, info, record and line bits); two device frames also equal
the numpy restatement of the reference (tests/manhattan_numpy.py)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manhattan_numpy as MN  # noqa: E402

pytestmark = pytest.mark.gpu


def _rot(ax, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


_FRAMES = {}


def _frames(cam, kind, seed, n):
    key = (cam.fx, cam.w, cam.h, kind, seed, n)
    if key not in _FRAMES:
        from dr_slam_amd import synth
        _FRAMES[key] = list(synth.sequence(seed, n, cam=cam, kind=kind))
    return _FRAMES[key]


def _run(frames, cam, nseq, seq_len, R0, dirs=None, loff=None, numpy_frames=()):
    """device batch vs chained host entry on every frame; frame i of the batch is frames[i % len(frames)]"""
    import torch
    from dr_slam_amd import lib
    nf = nseq * seq_len
    depth = torch.from_numpy(np.stack([frames[i % len(frames)][1] for i in range(nf)]).view(np.int16)).cuda()
    K4 = (cam.fx, cam.fy, cam.cx, cam.cy)
    inv = np.float32(1.0) / np.float32(cam.depth_factor)
    c = lib.Context(max_width=cam.w, max_height=cam.h)
    lost = 0
    try:
        stream = torch.cuda.current_stream().cuda_stream
        c.surface_normals_batch_ptr(depth.data_ptr(), cam.w * cam.h, cam.w, cam.w, cam.h, K4, inv, 9.0, nf, stream)
        c.manhattan_track_batch(R0, nseq, seq_len, dirs, loff, 3, stream)
        for s in range(nseq):
            R = np.asarray(R0, np.float32).reshape(nseq, 3, 3)[s]
            for t in range(seq_len):
                f = s * seq_len + t
                recs = c.surface_normals_download(f)
                d = None if dirs is None else dirs[loff[f]:loff[f + 1]]
                Rd, infod, rbd, lbd = c.manhattan_download(f, len(recs))
                Rh, infoh, rbh, lbh = lib.manhattan_track_host(R, recs, d, 3)
                assert np.array_equal(Rd.view(np.uint32), Rh.view(np.uint32)), (f, Rd, Rh)
                assert infod.tobytes() == infoh.tobytes(), f
                assert np.array_equal(rbd, rbh) and np.array_equal(lbd, lbh), f
                if f in numpy_frames:
                    Rn, infos, rbn, lbn, _ = MN.track(R, recs["normal"], d, 3)
                    MN.assert_equal_to_product(Rn, infos, rbn, lbn, Rd, infod, rbd, lbd)
                lost += int(infod["call"]["svd"][:3].min() == 0)
                R = Rd
    finally:
        c.close()
    return lost


def test_batch_one_sequence_of_64_equals_host():
    from dr_slam_amd import synth
    cam = synth.TUM3
    frames = _frames(cam, "room_boxes", 2, 64)
    R0 = np.linalg.inv(frames[0][2])[:3, :3].astype(np.float32)[None]
    _run(frames, cam, 1, 64, R0, numpy_frames=(0, 37))


def test_batch_eight_sequences_of_16_equals_host():
    from dr_slam_amd import synth
    cam = synth.TUM3
    frames = _frames(cam, "living_room", 3, 16)
    Rcw = np.linalg.inv(frames[0][2])[:3, :3]
    R0 = np.stack([(Rcw @ _rot(s % 3, 1.5 * s)).astype(np.float32) for s in range(8)])
    _run(frames, cam, 8, 16, R0)


def test_batch_1280x960_equals_host():
    from dr_slam_amd import synth
    cam = synth.REALSENSE.scaled(2.0)
    frames = _frames(cam, "corridor", 5, 3)
    R0 = np.stack([np.linalg.inv(frames[0][2])[:3, :3].astype(np.float32)] * 2)
    _run(frames, cam, 2, 3, R0)


def test_batch_with_line_directions_equals_host():
    from dr_slam_amd import synth
    cam = synth.TUM3
    frames = _frames(cam, "corridor", 4, 8)
    Rcw = np.linalg.inv(frames[0][2])[:3, :3]
    rng = np.random.default_rng(11)
    counts = [0, 3, 17, 1, 40, 0, 9, 300, 5, 2, 0, 12, 7, 60, 4, 1]
    dirs = []
    for n in counts:
        ax = Rcw[:, rng.integers(0, 3, n)].T * np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)
        v = ax + rng.normal(0, 0.08, (n, 3))
        dirs.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    dirs = np.concatenate(dirs)
    loff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    R0 = np.stack([Rcw.astype(np.float32), (Rcw @ _rot(2, 2.0)).astype(np.float32)])
    _run(frames, cam, 2, 8, R0, dirs, loff, numpy_frames=(9,))


def test_batch_where_frames_lose_tracking_equals_host():
    """frames without depth (every normal NaN) find no axis: R passes through unchanged, no SVD, and the next frame resumes"""
    from dr_slam_amd import synth
    cam = synth.TUM3
    frames = list(_frames(cam, "room_boxes", 2, 16)[:6])
    for k in (2, 3):
        frames[k] = (frames[k][0], np.zeros_like(frames[k][1]), frames[k][2])
    Rcw = np.linalg.inv(frames[0][2])[:3, :3]
    R0 = np.stack([Rcw.astype(np.float32), (Rcw @ _rot(2, 3.0)).astype(np.float32)])
    assert _run(frames, cam, 2, 6, R0) == 4


def test_batch_needs_a_normals_batch():
    from dr_slam_amd import lib
    c = lib.Context()
    try:
        with pytest.raises(lib.DrfeError):
            c.manhattan_track_batch(np.eye(3, dtype=np.float32)[None], 1, 1)
    finally:
        c.close()
