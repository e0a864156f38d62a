"""-m gpu: the bordered pyramid byte for byte against the oracle, aimed at the tiled resize (k_pyr_resize_tile).

Frame widths cover every residue mod 8 and, through the levels they produce, many residues mod 64 of the bordered width
(which sets how far a frame's last block overhangs and how many border rows are computed directly); strided input,
batches of distinct frames in one launch, and a geometry whose first level falls back to k_pyr_resize.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _check_levels(c, slot, o, nlevels, what):
    for l in range(nlevels):
        assert np.array_equal(c.pyramid_level(slot, l), o.pyramid(l)), f"{what}: pyramid level {l}"


@pytest.mark.parametrize("w,h", [(600, 451), (601, 449), (602, 460), (603, 470), (604, 455), (605, 441), (606, 463),
                                 (607, 477), (577, 433), (663, 497)])
def test_widths_mod_8_and_64(oracle_mod, w, h):
    from dr_slam_amd import lib, synth
    g = synth.noise_frame(w + h, w, h)
    c = lib.Context(nfeatures=600, max_width=w, max_height=h)
    try:
        c.orb_extract(g)
        o = oracle_mod.OrbOracle(600, 1.2, 8, 20, 7)
        o(g)
        _check_levels(c, 0, o, 8, f"{w}x{h}")
    finally:
        c.close()


def test_strided_batch_of_distinct_frames(oracle_mod):
    """Four different frames in one launch, rows 704 bytes apart in a padded device buffer."""
    import torch
    from dr_slam_amd import lib, synth
    w, h, n, stride = 640, 480, 4, 704
    frames = [synth.noise_frame(100 + s, w, h) for s in range(n)]
    buf = np.zeros((n, h, stride), np.uint8)
    for s in range(n):
        buf[s, :, :w] = frames[s]
    d = torch.from_numpy(buf).cuda()
    c = lib.Context(nfeatures=1000, max_batch=n)
    try:
        c.orb_extract_batch_ptr(d.data_ptr(), h * stride, stride, w, h, n, torch.cuda.current_stream().cuda_stream)
        c.orb_counts(n)
        for s in range(n):
            o = oracle_mod.OrbOracle()
            o(frames[s])
            _check_levels(c, s, o, 8, f"slot {s}")
    finally:
        c.close()


@pytest.mark.parametrize("w,h,scale,nlevels", [(1280, 960, 2.0, 3), (1600, 1200, 2.0, 3), (640, 480, 1.7, 4)])
def test_large_scale_factors_and_fallback(oracle_mod, w, h, scale, nlevels):
    """1600x1200 at scale 2: level 1 runs k_pyr_resize (its tile would need more than eight loads per thread), level 2 the
    tiled kernel."""
    from dr_slam_amd import lib, synth
    g = synth.noise_frame(w ^ h, w, h)
    c = lib.Context(nfeatures=800, scale_factor=scale, nlevels=nlevels, max_width=w, max_height=h)
    try:
        c.orb_extract(g)
        o = oracle_mod.OrbOracle(800, scale, nlevels, 20, 7)
        o(g)
        _check_levels(c, 0, o, nlevels, f"{w}x{h} scale {scale}")
    finally:
        c.close()
