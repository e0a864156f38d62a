"""-m gpu: pyramid level 0 read in place from the caller's frames (dr_slam_amd/csrc/level0_view.h).

Where a batch is eligible the two level-0 copy kernels do not run and level 1's resize, FAST, the blur and the descriptor's raw
patch address the caller's image.  Every output - bordered pyramid, blurred levels, FAST candidates, keypoints, descriptors -
must be byte for byte the oracle's and the copy path's, whatever the row and frame padding holds, and the query must say which
path ran so that nothing here passes on the fallback by accident.

Shapes.  256x128: blur tiles (128 x 64) end exactly on the image edge.  208x122 in rows of 256 bytes with frame padding: two blur
tiles across, the second overhanging in x, and two down, the second overhanging in y.  A batch of 2 at 640x480.
The small shapes run two levels: a third one is refused by the context at 256x128 (its single FAST cell row is taller than the
60-px window limit) and at 208x122 takes the geometry off k_fast_cells_cols (more than 12 rows per lane), which is one of the
conditions of reading in place.  208x112 with three levels is such a geometry (level 0 already needs 14 rows per lane): it is
kept here as a fallback case.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {
    # name: (w, h, row stride, frame padding, nlevels, nfeatures, batch)
    "256x128": (256, 128, 256, 0, 2, 300, 1),
    "208x122": (208, 122, 256, 48, 2, 300, 1),
    "640x480x2": (640, 480, 704, 64, 8, 1000, 2),
}


def _image(kind, seed, w, h):
    from dr_slam_amd import synth
    if kind == "noise":
        return synth.noise_frame(seed, w, h)
    if kind == "constant":
        return np.full((h, w), 128, np.uint8)
    rng = np.random.default_rng(seed)
    if kind == "rim":
        # the only strong corners and edges lie within 3 px of each border and in the four image corners
        g = np.full((h, w), 128, np.uint8)
        for x in range(0, w, 12):
            g[0:3, x:x + 6] = 255 if (x // 12) % 2 else 0
            g[h - 3:h, x:x + 6] = 0 if (x // 12) % 2 else 255
        for y in range(0, h, 12):
            g[y:y + 6, 0:3] = 255 if (y // 12) % 2 else 0
            g[y:y + 6, w - 3:w] = 0 if (y // 12) % 2 else 255
        for ys, xs in ((slice(0, 5), slice(0, 5)), (slice(0, 5), slice(w - 5, w)), (slice(h - 5, h), slice(0, 5)),
                       (slice(h - 5, h), slice(w - 5, w))):
            g[ys, xs] = 255
        return g
    if kind == "border_values":
        # distinct values in every border row and column over a textured interior: a wrong reflection changes the blur
        g = synth.noise_frame(seed, w, h).copy()
        xs, ys = np.arange(w), np.arange(h)
        for k in range(4):
            g[k, :] = (xs * (3 + 2 * k) + 17 * k) % 251
            g[h - 1 - k, :] = (xs * (5 + 2 * k) + 29 * k + 7) % 241
        for k in range(4):
            g[:, k] = (ys * (7 + 2 * k) + 31 * k + 3) % 239
            g[:, w - 1 - k] = (ys * (11 + 2 * k) + 37 * k + 5) % 233
        g[0, 0], g[0, w - 1], g[h - 1, 0], g[h - 1, w - 1] = rng.integers(0, 256, 4)
        return g
    raise ValueError(kind)


def _run(c, frames, stride, frame_pad, nlevels, fill, ptr_off=0):
    """One batch from a padded device buffer whose padding holds `fill`; everything the context exposes, per slot.  The buffer
    stays alive until the bordered level 0 has been fetched (after an in-place batch it is built from the frames on demand)."""
    import torch
    n = len(frames)
    h, w = frames[0].shape
    fstride = h * stride + frame_pad
    buf = np.full(ptr_off + n * fstride + 64, fill, np.uint8)
    for s, g in enumerate(frames):
        v = buf[ptr_off + s * fstride: ptr_off + s * fstride + h * stride].reshape(h, stride)
        v[:, :w] = g
    d = torch.from_numpy(buf).cuda()
    c.orb_extract_batch_ptr(d.data_ptr() + ptr_off, fstride, stride, w, h, n, torch.cuda.current_stream().cuda_stream)
    in_place = c.orb_level0_in_place()
    c.orb_counts(n)
    out = []
    for s in range(n):
        kps, desc = c.orb_download(s)
        out.append(dict(pyr=[c.pyramid_level(s, l) for l in range(nlevels)], blur=[c.blurred_level(s, l) for l in range(nlevels)],
                        cand=[c.candidates(s, l) for l in range(nlevels)], kps=kps, desc=desc))
    del d
    return in_place, out


def _same(a, b, what):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        for key in ("pyr", "blur", "cand"):
            for l, (p, q) in enumerate(zip(x[key], y[key])):
                assert np.array_equal(p, q), f"{what}: slot {s} {key} level {l}"
        assert np.array_equal(x["kps"].view(np.uint8), y["kps"].view(np.uint8)), f"{what}: slot {s} keypoints"
        assert np.array_equal(x["desc"], y["desc"]), f"{what}: slot {s} descriptors"


def _against_oracle(oracle_mod, frames, out, nfeatures, nlevels, need_blur0, what):
    for s, g in enumerate(frames):
        o = oracle_mod.OrbOracle(nfeatures, 1.2, nlevels, 20, 7)
        okps, odesc = o(g)
        for l in range(nlevels):
            assert np.array_equal(out[s]["pyr"][l], o.pyramid(l)), f"{what}: slot {s} pyramid level {l}"
            ob = o.blurred(l)
            if l == 0 and need_blur0:
                assert ob is not None, f"{what}: the oracle has no blurred level 0 to compare"
            if ob is not None:
                assert np.array_equal(out[s]["blur"][l], ob), f"{what}: slot {s} blur level {l}"
            assert np.array_equal(out[s]["cand"][l], o.candidates(l)), f"{what}: slot {s} FAST candidates level {l}"
        assert np.array_equal(out[s]["kps"].view(np.uint8), okps.view(np.uint8)), f"{what}: slot {s} keypoints"
        assert np.array_equal(out[s]["desc"], odesc), f"{what}: slot {s} descriptors"


@pytest.mark.parametrize("kind", ["noise", "constant", "rim", "border_values"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_in_place_equals_oracle_and_copy_path(oracle_mod, shape, kind):
    from dr_slam_amd import lib
    w, h, stride, fpad, nlevels, nfeatures, n = SHAPES[shape]
    frames = [_image(kind, 11 + 7 * s + w, w, h) for s in range(n)]
    c = lib.Context(nfeatures=nfeatures, nlevels=nlevels, max_width=w, max_height=h, max_batch=n)
    try:
        ip0, a0 = _run(c, frames, stride, fpad, nlevels, 0x00)
        assert ip0, "the batch did not read level 0 in place"
        ip1, a1 = _run(c, frames, stride, fpad, nlevels, 0xFF)
        assert ip1
        _same(a0, a1, "padding 0x00 against 0xFF")
        c.orb_configure_level0(False)
        ipc, b = _run(c, frames, stride, fpad, nlevels, 0x00)
        assert not ipc, "the switch did not force the copy path"
        _same(a0, b, "in place against the copy path")
        c.orb_configure_level0(True)
        ip2, a2 = _run(c, frames, stride, fpad, nlevels, 0xFF)
        assert ip2
        _same(a2, b, "in place again after the copy path")
        _against_oracle(oracle_mod, frames, a0, nfeatures, nlevels, kind in ("noise", "border_values"), f"{shape} {kind}")
    finally:
        c.close()


@pytest.mark.parametrize("case", ["641x479", "640x480+4", "208x112"])
def test_ineligible_input_takes_the_copy_path(oracle_mod, case):
    from dr_slam_amd import lib
    w, h, stride, nlevels, nfeatures, off = {"641x479": (641, 479, 656, 8, 1000, 0), "640x480+4": (640, 480, 640, 8, 1000, 4),
                                             "208x112": (208, 112, 256, 3, 300, 0)}[case]
    frames = [_image("noise", 5 + w, w, h)]
    c = lib.Context(nfeatures=nfeatures, nlevels=nlevels, max_width=w, max_height=h, max_batch=1)
    try:
        ip, a = _run(c, frames, stride, 0, nlevels, 0xFF, ptr_off=off)
        assert not ip, "an ineligible batch was read in place"
        _against_oracle(oracle_mod, frames, a, nfeatures, nlevels, True, case)
    finally:
        c.close()


def test_single_frame_entries_keep_the_copy(oracle_mod):
    """drfe_orb_extract stages the frame in a buffer the next call overwrites: level 0 is copied, and the bordered level 0 of
    slot 0 comes from the arena even after an in-place batch filled the slot before."""
    from dr_slam_amd import lib, synth
    w, h = 640, 480
    g0, g1 = synth.noise_frame(1, w, h), synth.noise_frame(2, w, h)
    c = lib.Context(max_batch=1)
    try:
        ip, _ = _run(c, [g0], w, 0, 8, 0)
        assert ip
        c.orb_extract(g1)
        assert not c.orb_level0_in_place()
        o = oracle_mod.OrbOracle()
        o(g1)
        assert np.array_equal(c.pyramid_level(0, 0), o.pyramid(0))
    finally:
        c.close()
