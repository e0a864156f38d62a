"""-m gpu tests of Frame::isLineGood's batch entry: drfe_lines_is_good_batch equals the host entry
drfe_lines_is_good byte for byte on the hand-built scene of line3d_scenarios.py (seeds 1, 2, 4 and 8, in one call and in four),
wherever a frame stands in a call, at 0, 1 and cap key lines, with an empty frame between full ones, in the as-shipped mode that
rejects everything, with the depth already on the device, with padded rows, across a chunk boundary and on two synthetic frames
behind the line extractor; the counters show that the scene reaches the branches it was built for; invalid arguments are
refused; the native caller tests/native/line3d_caller.cpp holds drfe::Line3DBatch's device path to its host path."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line3d_scenarios as sc  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 4, 8)
CAM = (sc.K9, sc.CX, sc.CY, sc.INVFX, sc.INVFY)
INVALID = -1                         # DRFE_ERR_INVALID


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def depth():
    d = sc.depth_image()
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _lines(count=len(sc.SEGMENTS)):
    from dr_slam_amd import lib
    kl = sc.key_lines(lib.KEYLINE_DTYPE, count=count)
    kl.setflags(write=False)
    return kl


@functools.lru_cache(maxsize=None)
def _host(seed, count=len(sc.SEGMENTS), k_as_f64=True):
    """the host entry on the scene: the truth, computed once per (seed, line count, mode)"""
    from dr_slam_amd import lib
    r = lib.lines_is_good(_lines(count), sc.depth_image(), *CAM, k_as_f64=k_as_f64, seed=seed)
    for a in r[:3]:
        a.setflags(write=False)
    return r


def _frame_equals(got, f, n, want):
    """frame f of a batch result against a host result, byte for byte over the frame's n lines; the rest untouched"""
    dl, l3, ni, good = got
    assert dl[f, :n].tobytes() == want[0].tobytes(), f"depth_line differs in frame {f}"
    assert l3[f, :n].tobytes() == want[1].tobytes(), f"lines3d differs in frame {f}"
    assert ni[f, :n].tobytes() == want[2].tobytes(), f"n_inliers differs in frame {f}"
    assert good[f] == want[3], f"n_good differs in frame {f}"
    assert (dl[f, n:] == -1).all() and (l3[f, n:] == 0).all() and (ni[f, n:] == 0).all()


def _batch(ctx, depth, seeds, counts=None, cap=None, **kw):
    """one call over len(seeds) copies of the scene; counts: key lines per frame (default: the twelve)"""
    counts = [len(sc.SEGMENTS)] * len(seeds) if counts is None else counts
    cap = max(max(counts), 1) if cap is None else cap
    lines = np.stack([_lines(cap)] * len(seeds))
    d = np.broadcast_to(depth, (len(seeds),) + depth.shape)
    return ctx.lines_is_good_batch(lines, counts, d, *CAM, seeds=seeds, **kw)


def test_device_equals_host_in_one_call_and_in_four(ctx, depth):
    got = _batch(ctx, depth, SEEDS)
    for f, s in enumerate(SEEDS):
        _frame_equals(got, f, 12, _host(s))
        _frame_equals(_batch(ctx, depth, [s]), 0, 12, _host(s))
    assert len({got[1][f].tobytes() for f in range(4)}) == 4          # the seeds matter
    assert all(_host(s)[3] == 3 for s in SEEDS)
    h = _host(1)
    assert h[2][0] != h[2][11]                                       # one line twice in a frame: the draws go on


def test_position_in_the_call_does_not_matter(ctx, depth):
    a = _batch(ctx, depth, [1, 2, 4, 8, 4])
    b = _batch(ctx, depth, [4, 1, 1, 2])
    _frame_equals(a, 2, 12, _host(4))
    _frame_equals(a, 4, 12, _host(4))
    _frame_equals(b, 0, 12, _host(4))
    _frame_equals(b, 1, 12, _host(1))
    _frame_equals(b, 2, 12, _host(1))
    _frame_equals(b, 3, 12, _host(2))


def test_default_seed_is_one(ctx, depth):
    got = ctx.lines_is_good_batch(_lines()[None], [12], depth[None], *CAM, seeds=None)
    _frame_equals(got, 0, 12, _host(1))


def test_counters_after_the_seed_1_frame(depth):
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    try:
        _batch(c, depth, [1])
        st = c.line3d_stats()
    finally:
        c.close()
    print(st)
    assert st["calls"] == 1 and st["frames"] == 1 and st["lines"] == 12
    assert st["lines"] - st["ransac_lines"] >= 1                     # a line with fewer than 10 samples drew nothing
    assert st["ransac_lines"] < st["iterations"] < 10 * st["ransac_lines"]
    assert st["coincident_pairs"] >= 1 and st["verify_rejections"] >= 1
    assert st["accepted"] == 3
    # what an instrumented copy of the host code counted on this frame
    assert (st["ransac_lines"], st["iterations"], st["coincident_pairs"], st["verify_rejections"]) == (10, 88, 1, 51)


@pytest.mark.parametrize("counts", [[0], [1], [40], [40, 0, 40]])
def test_line_counts(ctx, depth, counts):
    seeds = [1, 2, 4][:len(counts)]
    got = _batch(ctx, depth, seeds, counts=counts, cap=40)
    for f, (s, n) in enumerate(zip(seeds, counts)):
        _frame_equals(got, f, n, _host(s, n))
    if counts == [40]:
        assert _host(1, 40)[3] > 3


def test_as_shipped_rejects_everything_as_the_host_does(ctx, depth):
    got = _batch(ctx, depth, [1, 8], k_as_f64=False)
    for f, s in enumerate((1, 8)):
        want = _host(s, k_as_f64=False)
        assert (want[0] == -1).all() and (want[1] == 0).all() and (want[2] == 0).all() and want[3] == 0
        _frame_equals(got, f, 12, want)


def test_depth_on_the_device(ctx, depth):
    import torch
    d = torch.from_numpy(np.stack([depth] * 3)).cuda()
    lines = np.stack([_lines()] * 3)
    got = ctx.lines_is_good_batch(lines, [12, 12, 12], d, *CAM, seeds=[2, 1, 8])
    torch.cuda.synchronize()
    for f, s in enumerate((2, 1, 8)):
        _frame_equals(got, f, 12, _host(s))


def test_padded_rows(ctx, depth):
    d = np.full((2, sc.H, sc.W + 24), 9.0, np.float32)            # padding that would be accepted if it were read
    d[:, :, :sc.W] = depth
    lines = np.stack([_lines()] * 2)
    got = ctx.lines_is_good_batch(lines, [12, 12], d, *CAM, seeds=[1, 4], w=sc.W)
    _frame_equals(got, 0, 12, _host(1))
    _frame_equals(got, 1, 12, _host(4))


def test_a_call_larger_than_one_chunk(ctx, depth):
    from dr_slam_amd import lib
    chunk = lib.line3d_chunk_frames(40)
    assert 1 <= chunk <= 1024
    F = chunk + 1
    got = _batch(ctx, depth, list(range(1, F + 1)), counts=[40] * F, cap=40)
    for f in sorted({0, 1, chunk - 1, chunk, *np.random.default_rng(0).integers(0, F, 12).tolist()}):
        _frame_equals(got, f, 40, _host(f + 1, 40))


def test_synthetic_frames_behind_the_line_extractor(ctx, oracle_mod):
    from dr_slam_amd import lib, synth
    cam = synth.TUM3
    K9 = np.array([cam.fx, 0, cam.cx, 0, cam.fy, cam.cy, 0, 0, 1], np.float32)
    inv = (np.float32(1) / np.float32(cam.fx), np.float32(1) / np.float32(cam.fy))
    frames = [next(synth.sequence(seed, 1, kind=kind)) for seed, kind in ((2, "room_boxes"), (5, "corridor"))]
    ext = ctx.lsd_extract_batch(np.stack([g for g, _, _ in frames]), max_lines=40)
    depth = np.stack([oracle_mod.depth_to_float(d16, np.float32(1.0) / np.float32(cam.depth_factor)) for _, d16, _ in frames])
    lines = np.zeros((2, 40), lib.KEYLINE_DTYPE)
    counts = [len(e["lines"]) for e in ext]
    for f, e in enumerate(ext):
        lines[f, :counts[f]] = e["lines"]
    got = ctx.lines_is_good_batch(lines, counts, depth, K9, cam.cx, cam.cy, inv[0], inv[1], seeds=[1, 1])
    total = 0
    for f in range(2):
        want = lib.lines_is_good(lines[f, :counts[f]], depth[f], K9, cam.cx, cam.cy, inv[0], inv[1], k_as_f64=True, seed=1)
        _frame_equals(got, f, counts[f], want)
        total += want[3]
    assert min(counts) >= 20 and total >= 10


def test_invalid_arguments_are_refused(ctx, depth):
    from dr_slam_amd import lib
    before = ctx.line3d_stats()

    def call(edit_frames=None, edit_out=None):
        lines = np.stack([_lines()] * 2)
        fr, out, _, keep = lib.line3d_frames(lines, [12, 12], np.stack([depth] * 2), *CAM, seeds=[1, 2])
        if edit_frames:
            edit_frames(fr, keep)
        if edit_out:
            edit_out(out)
        return ctx.L.drfe_lines_is_good_batch(ctx.h, C.byref(fr), C.byref(out), None)

    def too_many(fr, keep):
        keep[1][1] = 13

    assert call() == 0
    assert call(lambda fr, keep: setattr(fr, "nframes", -1)) == INVALID
    assert call(too_many) == INVALID
    assert b"n_lines" in ctx.L.drfe_last_error(ctx.h)
    assert call(lambda fr, keep: setattr(fr, "stride", sc.W - 1)) == INVALID
    assert b"stride" in ctx.L.drfe_last_error(ctx.h)
    assert call(lambda fr, keep: setattr(fr, "cap", lib.LINE3D_MAX_CAP + 1)) == INVALID
    assert call(lambda fr, keep: setattr(fr, "depth", None)) == INVALID
    for field in ("depth_line", "lines3d", "n_good"):
        assert call(edit_out=lambda out, field=field: setattr(out, field, None)) == INVALID
    assert ctx.L.drfe_lines_is_good_batch(ctx.h, None, None, None) == INVALID
    after = ctx.line3d_stats()
    assert after["frames"] == before["frames"] + 2 and after["calls"] == before["calls"] + 1   # the refused calls launched nothing


def test_native_caller_over_the_adaptor():
    """tests/native/line3d_caller.cpp: nine Frame-like objects through drfe::Line3DBatch on the device and on the host"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "line3d_caller")
    assert os.path.exists(exe), "build() compiles tests/native/line3d_caller"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "line3d_caller ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
