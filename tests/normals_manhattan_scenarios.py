"""Hand-built depth images, start rotations and line directions for the device chain surface normals -> Manhattan-frame
tracking (DESIGN.md sections 9 and 11; normals_kernels.hip, manhattan_kernels.hip), placed on the seams of the kernels: the
workgroup sizing of the row-skewed recurrences, the float thresholds of the depth-change map, the chamfer pass's read across a
row end, the window sizes, the strides of the batch entry, non-finite depth; the compaction chunks of 1 024 entries, the
record / line seam of the entry index space, the `n_selected > threshold` gate, the two-axis assembly with its determinant
flip, the zero-singular-value branch of the SVD, 1 to 5 calls, sequences side by side.  Pure numpy: nothing here imports the
project, and where noise is used the seed is fixed.

The module also restates in plain numpy the three things the oracle has no tap for: the subsampled depth (cloud_z), the
depth-change seeds (seeds) and the two raster passes of the 3-4 chamfer transform (chamfer), written from
oracle/post_oracle.cpp and DESIGN.md section 9.  tests/test_normals_manhattan_edges_cpu.py proves on the host that every
scenario reaches what it names; tests/test_gpu_normals_manhattan_edges.py holds the device to the same scenarios.

What the depth-change rule does not allow (stated here because the scenarios work around it): a jump always clears both ends of
a pair, so the smallest seed set is one pair, never one pixel; vertical pairs are not tested in the last cloud column, so a seed
in column W-1 always comes with its left neighbour in column W-2.  Records within 10 cloud points of the border never carry a
normal, so no selected record is adjacent to the record / line seam of the entry space: the entries before it are NaN records."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
DEPTH_FACTOR = 5000
INV = f32(1.0) / f32(DEPTH_FACTOR)          # the depth-map factor of the batch entry, as the reference computes it
MAXD = f32(9.0)
BORDER = 10                                 # NormalSmoothingSize: no normal within 10 cloud points of the border
MF_CHUNK = 1024                             # entries per barrier pair of k_manhattan's compaction


class Cam:
    """a pinhole camera for a w x h image (a field of view like the synthetic cameras')"""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.fx = self.fy = float(f32(0.82 * w))
        self.cx, self.cy = (w - 1) / 2.0, (h - 1) / 2.0
        self.depth_factor = DEPTH_FACTOR

    @property
    def K4(self):
        return np.array([self.fx, self.fy, self.cx, self.cy], f32)


def cloud_size(w, h):
    """(W, H) of the 3x-subsampled cloud"""
    return (w + 2) // 3, (h + 2) // 3


def n_records(w, h):
    W, H = cloud_size(w, h)
    return (W // 2) * (H // 2)


def to_metres(d16):
    """imDepth.convertTo(CV_32F, factor): float(raw) * factor in float32"""
    return (np.asarray(d16, np.uint16).astype(f32) * INV).astype(f32)


def block(img, r, c, v):
    """sets cloud point (r, c): the image pixel (3r, 3c) the cloud reads and the two rows / columns after it"""
    img[3 * r:3 * r + 3, 3 * c:3 * c + 3] = v


# ---- plain restatements: subsampled depth, depth-change seeds, chamfer distance ------------------------------------

def cloud_z(depth_m, maxd):
    """z of the cloud: every third pixel, depths beyond Point.MaxDistance zeroed (NaN compares false and stays)"""
    z = np.array(np.asarray(depth_m, f32)[::3, ::3], f32)
    with np.errstate(invalid="ignore"):
        z[z > f32(maxd)] = 0
    return z


def jump(d, dn):
    """|d - dn| > max_depth_change_factor * (|d| + 1) * 2 in float32, or either depth not finite"""
    with np.errstate(invalid="ignore"):
        lim = (f32(0.05) * (np.abs(d) + f32(1.0))) * f32(2.0)
        return (np.abs(d - dn) > lim) | ~np.isfinite(d) | ~np.isfinite(dn)


def seeds(z):
    """the depth-change map: pairs (r, c) - (r, c + 1) and (r, c) - (r + 1, c) for r < H - 1, c < W - 1 clear both ends"""
    H, W = z.shape
    s = np.zeros((H, W), bool)
    a = z[:H - 1, :W - 1]
    jr, jd = jump(a, z[:H - 1, 1:]), jump(a, z[1:, :W - 1])
    s[:H - 1, :W - 1] |= jr | jd
    s[:H - 1, 1:] |= jr
    s[1:, :W - 1] |= jd
    return s


def chamfer(seed, wrap=True):
    """the two raster passes of the 3-4 chamfer transform (weights 1.0 and 1.4, float32) from seeds at 0 and W + H elsewhere.
    wrap=True keeps PCL's read one element past the row end: the forward pass at the last column reads previous_row[W], which
    is current_row[0]; the backward pass at column 0 reads next_row[-1], which is current_row[W - 1].  wrap=False leaves that
    neighbour out (what a transform without the quirk would do)."""
    H, W = seed.shape
    d = np.where(seed, f32(0), f32(W + H)).astype(f32)
    a, b = f32(1.0), f32(1.4)
    for r in range(1, H):
        prev, cur = d[r - 1], d[r]
        for c in range(1, W):
            mv = min(prev[c - 1] + b, prev[c] + a, cur[c - 1] + a)
            if c + 1 < W:
                mv = min(mv, prev[c + 1] + b)
            elif wrap:
                mv = min(mv, cur[0] + b)
            if mv < cur[c]:
                cur[c] = mv
    for r in range(H - 2, -1, -1):
        nxt, cur = d[r + 1], d[r]
        for c in range(W - 2, -1, -1):
            mv = min(nxt[c] + a, nxt[c + 1] + b, cur[c + 1] + a)
            if c >= 1:
                mv = min(mv, nxt[c - 1] + b)
            elif wrap:
                mv = min(mv, cur[W - 1] + b)
            if mv < cur[c]:
                cur[c] = mv
    return d


_DIST = {}


def scenario_dist(sc):
    """chamfer distance of a normals scenario by the restatement above, computed once"""
    if sc["name"] not in _DIST:
        _DIST[sc["name"]] = chamfer(seeds(cloud_z(sc["depth_m"], sc["maxd"])))
    return _DIST[sc["name"]]


def window(dist):
    """the smoothing window (int) min(dist, 10) where that is > 2, else 0 (no normal)"""
    sm = np.minimum(dist, f32(BORDER))
    return np.where(sm > f32(2.0), sm.astype(np.int32), 0)


def interior(W, H):
    m = np.zeros((H, W), bool)
    m[BORDER:H - BORDER, BORDER:W - BORDER] = True
    return m


# ---- A. depth images for the surface normals -----------------------------------------------------------------------

SIZING = [(w, h) for h in (189, 192, 195, 384) for w in (192, 195, 258)]     # cloud heights 63, 64, 65, 128 x widths 64, 65, 86


def plane_box(w, h, mirror=False):
    """a tilted plane from 1.5 m with one box 0.6 m in front of it (the jump limit there is about 0.25 m): smooth regions and
    depth discontinuities in one frame"""
    y, x = np.mgrid[:h, :w]
    raw = 7500 + 2 * x + y
    box = (y >= h // 3) & (y < h // 2) & (x >= w // 4) & (x < w // 2)
    raw = np.where(box, raw - 3000, raw).astype(np.uint16)
    return np.ascontiguousarray(raw[::-1, ::-1]) if mirror else raw


def tilted(w, h, base=10000, sx=2, sy=1):
    y, x = np.mgrid[:h, :w]
    return (base + sx * x + sy * y).astype(np.uint16)


def threshold_pair():
    """(a, k): raw depths a and a + k (factor 1/5000) whose float32 difference equals sn_jump's float32 limit at a exactly, so
    that the pair is no jump and (a, a + k + 1) is one"""
    a = np.arange(5000, 20000)
    da = a.astype(f32) * INV
    lim = (f32(0.05) * (np.abs(da) + f32(1.0))) * f32(2.0)
    k0 = np.floor(lim.astype(f64) * DEPTH_FACTOR).astype(np.int64)
    for dk in (-1, 0, 1, 2):
        k = k0 + dk
        eq = np.abs(da - (a + k).astype(f32) * INV) == lim
        if eq.any():
            i = int(np.flatnonzero(eq)[0])
            return int(a[i]), int(k[i])
    raise AssertionError("no raw pair sits on the jump limit")


def _nsc(name, what, cam, maxd=MAXD, d16=None, depth_m=None, **kw):
    return dict(name=name, what=what, cam=cam, maxd=f32(maxd), d16=d16, depth_m=to_metres(d16) if depth_m is None else depth_m, **kw)


def jump_threshold_frame():
    a, k = threshold_pair()
    d = np.full((120, 120), a, np.uint16)
    block(d, 15, 15, a + k)              # exactly on the limit towards its left and upper neighbour: no jump
    block(d, 15, 25, a + k + 1)          # one raw unit further: a jump from the left and from above
    want = np.zeros((40, 40), bool)
    want[15, 25] = want[15, 24] = want[14, 25] = True
    return _nsc("jump_threshold", "sn_jump's float32 limit met exactly (no jump) and exceeded by one raw unit, as horizontal and as "
                "vertical neighbours", Cam(120, 120), d16=d, seeds=want)


def max_distance_frames():
    """a ramp through Point.MaxDistance = float32(15000) * factor: raw 15000 is kept, raw 15001 and above is zeroed; on the float
    entry also the next float above the limit"""
    y, x = np.mgrid[:120, :120]
    d = (14400 + 20 * (x // 3) + 2 * (y // 3)).astype(np.uint16)
    maxd = f32(15000) * INV
    cam = Cam(120, 120)
    dm = to_metres(d)
    block(dm, 5, 5, maxd)
    block(dm, 5, 8, np.nextafter(maxd, f32(np.inf)))
    return [_nsc("max_distance_u16", "depth exactly at Point.MaxDistance is kept, one raw unit above is zeroed", cam, maxd, d16=d),
            _nsc("max_distance_f32", "depth exactly at Point.MaxDistance is kept, the next float above is zeroed", cam, maxd, depth_m=dm,
                 kept=(5, 5), zeroed=(5, 8))]


def _three_levels(W3, H3):
    """background 2.25 m; 2.03 m and 2.47 m are each within the limit of the background and a jump from one another"""
    return np.full((3 * H3, 3 * W3), 11250, np.uint16), 10150, 12350


def chamfer_frames():
    W3, H3 = 64, 48
    cam = Cam(3 * W3, 3 * H3)
    out = []
    d, lo, hi = _three_levels(W3, H3)
    for r in range(H3):
        block(d, r, 0, lo if r < 20 else hi)
    want = np.zeros((H3, W3), bool)
    want[19, 0] = want[20, 0] = True
    out.append(_nsc("seeds_col0", "the only seeds are a vertical pair in cloud column 0: the forward pass reads them across the row "
                    "end", cam, d16=d, seeds=want, wrap_matters=True))
    d, lo, hi = _three_levels(W3, H3)
    block(d, 20, W3 - 2, lo)
    block(d, 20, W3 - 1, hi)
    want = np.zeros((H3, W3), bool)
    want[20, W3 - 2] = want[20, W3 - 1] = True
    out.append(_nsc("seeds_last_col", "the only seeds are the pair in cloud columns W-2 and W-1: the backward pass reads the last "
                    "column across the row start", cam, d16=d, seeds=want, wrap_matters=True))
    d = tilted(3 * W3, 3 * H3, 11000, 2, 1)
    block(d, 24, 32, int(d[72, 96]) - 1100)
    block(d, 24, 33, int(d[72, 99]) + 1100)
    want = np.zeros((H3, W3), bool)
    want[24, 32] = want[24, 33] = True
    out.append(_nsc("seed_interior", "one interior pair of seeds on a tilted plane: dist 1.0, 1.4, 2.0, 2.4, ... around it, NaN up to "
                    "2.0, every window size from 2 to 10", cam, d16=d, seeds=want, all_windows=True))
    return out


def nonfinite_frame():
    cam = Cam(192, 144)
    dm = to_metres(tilted(192, 144, 9000, 2, 1))
    block(dm, 20, 20, f32(np.nan))
    block(dm, 20, 40, f32(np.inf))               # above Point.MaxDistance: zeroed like any far depth
    dm[90:99, 84:93] = f32(np.nan)               # cloud rows 30..32, columns 28..30
    block(dm, 35, 50, f32(-np.inf))
    return _nsc("nonfinite", "NaN, +inf, -inf and a 3 x 3 block of NaN on the float entry: the isfinite branches of the seeds, of the "
                "integral images' finite counts and of the normal", cam, depth_m=dm)


_NORMALS = []


def normals_scenarios():
    """every depth frame of part A; d16 is None where the depth is not uint16-representable (float entry only)"""
    if not _NORMALS:
        for w, h in SIZING:
            W3, H3 = cloud_size(w, h)
            _NORMALS.append(_nsc(f"sizing_{W3}x{H3}", f"cloud {W3} x {H3}: workgroup of {(H3 + 63) // 64 * 64} lanes, record grid "
                                 f"{W3 // 2} x {H3 // 2}", Cam(w, h), d16=plane_box(w, h), sizing=True))
        # interior = cloud rows and columns 10 .. size - 11; records are the odd rows and columns
        for s, n, nr in ((60, 0, 0), (63, 1, 0), (66, 4, 1), (69, 9, 1)):
            _NORMALS.append(_nsc(f"smallest_{(s + 2) // 3}", f"a {(s + 2) // 3} x {(s + 2) // 3} cloud: {n} point(s) and {nr} record(s) "
                                 "carry a normal", Cam(s, s), d16=tilted(s, s, 10000, 3, 2), n_normals=n, n_record_normals=nr))
        _NORMALS.append(jump_threshold_frame())
        _NORMALS.extend(max_distance_frames())
        _NORMALS.extend(chamfer_frames())
        _NORMALS.append(nonfinite_frame())
    return _NORMALS


def padded(frames, pad_row=5, pad_frame=7, fill=65535):
    """frames [n, h, w] uint16 laid out with row_stride = w + 5 and frame_stride = row_stride * h + 7, the padding filled with
    65535 -> (flat buffer, frame_stride, row_stride)"""
    n, h, w = frames.shape
    rs = w + pad_row
    fs = rs * h + pad_frame
    buf = np.full(n * fs, fill, np.uint16)
    for f in range(n):
        buf[f * fs:f * fs + rs * h].reshape(h, rs)[:, :w] = frames[f]
    return buf, fs, rs


# ---- B. Manhattan tracking ----------------------------------------------------------------------------------------

def rot(ax, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


R1 = (rot(1, 3.0) @ rot(0, -2.0)).astype(f32)
I3 = np.eye(3, dtype=f32)
NO_LINES = np.zeros((0, 3), f64)


def near(v, n, rng, sigma=0.03):
    """n unit directions around +-v, Gaussian tilt"""
    d = np.asarray(v, f64)[None, :] * np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0) + rng.normal(0, sigma, (n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def offsets(per_frame):
    return np.concatenate([[0], np.cumsum([len(d) for d in per_frame])]).astype(np.int32)


def _call(R0, per_frame, nseq, seq_len, n_calls=3, expect=None):
    """one manhattan_track_batch call: per_frame = the line directions of every frame; expect = {frame: fields of call 0}"""
    assert len(per_frame) == nseq * seq_len
    return dict(R0=np.ascontiguousarray(R0, f32).reshape(nseq, 3, 3), nseq=nseq, seq_len=seq_len, n_calls=n_calls,
                dirs=np.concatenate([np.asarray(d, f64).reshape(-1, 3) for d in per_frame]), loff=offsets(per_frame),
                expect=expect or {})


def _msc(name, what, cam, depth, calls, hits=(), **kw):
    return dict(name=name, what=what, cam=cam, depth=np.ascontiguousarray(depth, np.uint16), calls=calls, hits=tuple(hits), **kw)


def lines_decide():
    """zero depth: every normal NaN, the deficiency rule sets the threshold to 0, and the lines decide what is found"""
    cam = Cam(192, 144)
    rng = np.random.default_rng(21)
    R = R1.astype(f64)
    sets, R0, expect = [], [], {}
    for axes, mask in (((0,), 1), ((1,), 2), ((2,), 4), ((0, 1), 3), ((1, 2), 6), ((0, 2), 5), ((0, 1, 2), 7)):
        sets.append(np.concatenate([near(R[:, a], 6, rng) for a in axes]))
        R0.append(R1)
        expect[len(sets) - 1] = dict(found=mask, svd=int(len(axes) >= 2), threshold=0, deficient=1)
    sets.append(np.array([[0.0, 0.0, 1.0]]))                 # exactly on z under R = I: lambda == 0, pushed and dropped
    R0.append(I3)
    expect[7] = dict(found=0, svd=0, n_selected=[0, 0, 0], pushed=[(n_records(cam.w, cam.h), 2)])
    sets.append(np.concatenate([[[np.nan, 0.0, 1.0]], near(R[:, 2], 3, rng), [[np.nan] * 3]]))
    R0.append(R1)
    expect[8] = dict(found=4, svd=0, n_selected=[0, 0, 3])
    sets.append(NO_LINES)
    R0.append(R1)
    expect[9] = dict(found=0, svd=0, n_selected=[0, 0, 0], unchanged=True)
    return _msc("lines_decide", "found masks 1, 2, 4, 3, 6, 5, 7 from lines alone; the determinant flip; a line with lambda == 0; NaN "
                "directions; a frame without lines", cam, np.zeros((10, cam.h, cam.w)), [_call(R0, sets, 10, 1, expect=expect)],
                hits=("found_1", "pair_3", "pair_6", "pair_5", "found_3", "det_flip", "zero_lambda_dropped", "deficiency", "found_0"))


def gate_at_zero():
    cam = Cam(192, 144)
    one = near(R1.astype(f64)[:, 2], 1, np.random.default_rng(22), 0.02)
    expect = {0: dict(found=0, n_selected=[0, 0, 0], threshold=0), 1: dict(found=4, n_selected=[0, 0, 1], threshold=0)}
    return _msc("gate_at_zero", "n_selected == threshold == 0 is not taken, n_selected == 1 is", cam, np.zeros((2, cam.h, cam.w)),
                [_call([R1, R1], [NO_LINES, one], 2, 1, expect=expect)], hits=("deficiency",))


def corner(cam, yaw_deg=9.0, floor=0.35, back=2.5, left=0.6):
    """a room corner seen from the room's origin: floor y = floor, back wall z = back, left wall x = -left in room axes, which
    are the camera's turned by yaw about y.  Returns (raw depth, R_cm whose columns are the room axes)."""
    R = rot(1, yaw_deg)
    u, v = np.meshgrid(np.arange(cam.w), np.arange(cam.h))
    rays = np.stack([(u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy, np.ones(u.shape)], -1) @ R
    with np.errstate(divide="ignore"):
        t = np.stack([np.where(rays[..., 1] > 1e-9, floor / rays[..., 1], np.inf), np.where(rays[..., 2] > 1e-9, back / rays[..., 2], np.inf),
                      np.where(rays[..., 0] < -1e-9, -left / rays[..., 0], np.inf)]).min(0)
    return np.rint(t * DEPTH_FACTOR).astype(np.uint16), R.astype(f32)


def cut_corner(cam, cut):
    """the corner with the cloud points listed in `cut` (row, column) zeroed"""
    d, R = corner(cam)
    for r, c in cut:
        block(d, r, c, 0)
    return d, R


CORNER_CAM = Cam(258, 195)                   # 86 x 65 cloud, 1 376 records, threshold 1376 / 20 = 68
# the left wall (axis x) without cloud columns 0..25: 66 of its normals are left, two below the threshold
CUT_WALL = [(r, c) for c in range(26) for r in range(65)]
# and the floor (axis y) without the cloud rows below 52 and the end of row 52: its in-cone count becomes the middle one, at 68 / 67
CUT_FLOOR_68 = CUT_WALL + [(r, c) for r in range(53, 65) for c in range(26, 86)] + [(52, c) for c in range(53, 86)]
CUT_FLOOR_67 = CUT_FLOOR_68 + [(52, 52), (52, 51)]


def gate_positive():
    """the room corner with R0 on the room's axes: two walls and the floor each give more than 68 normals.  Frames 0, 1: the left
    wall is cut down to 66 selected normals, and 2 / 3 lines in its mean-shift cone make n_selected 68 == threshold (not taken)
    and 69 (taken).  Frames 2, 3: the floor's in-cone count is the middle one and sits at 68 (the threshold stays 68, which the
    floor's 68 only equals: z alone is found) and at 67 (the deficiency rule: threshold (66 + 67) / 2 = 66, which the wall's 66
    only equals and the floor's 67 exceeds: y and z are found)."""
    cam = CORNER_CAM
    wall, R = cut_corner(cam, CUT_WALL)
    Rd = R.astype(f64)
    x = [Rd[:, 0] + 0.02 * Rd[:, 1], Rd[:, 0] - 0.02 * Rd[:, 1], Rd[:, 0] + 0.02 * Rd[:, 2]]
    x = np.array([v / np.linalg.norm(v) for v in x])
    depth = np.stack([wall, wall, cut_corner(cam, CUT_FLOOR_68)[0], cut_corner(cam, CUT_FLOOR_67)[0]])
    expect = {0: dict(n_selected0=68, threshold=68, deficient=0, found=6, svd=1),
              1: dict(n_selected0=69, threshold=68, deficient=0, found=7, svd=1),
              2: dict(in_cone=[66, 68, 238], threshold=68, deficient=0, n_selected=[66, 68, 238], found=4, svd=0),
              3: dict(in_cone=[66, 67, 238], threshold=66, deficient=1, n_selected=[66, 67, 238], found=6, svd=1)}
    return _msc("gate_positive", "n_selected == threshold == 68 and threshold + 1; the deficiency rule with the middle count at "
                "records / 20 and one below", cam, depth, [_call([R] * 4, [x[:2], x, NO_LINES, NO_LINES], 4, 1, expect=expect)],
                hits=("deficiency", "pair_6", "det_flip", "found_3"))


def _interleave(n, z, other):
    """n lines, `z z other z z other ...` shifted so that the last two are z lines"""
    shift = (-(n - 2)) % 3
    zi, oi, out = 0, 0, []
    for l in range(n):
        if (l + shift) % 3 < 2:
            out.append(z[zi]); zi += 1
        else:
            out.append(other[oi]); oi += 1
    return np.array(out)


def compaction_seams(w, h, counts):
    """a slightly tilted wall under R0 = I: every record with a normal is selected on z (lambda != 0), then lines so that
    records + lines is one below, at and one above a multiple of the 1 024-entry chunk; z lines first, last and interleaved
    with lines of the other axes"""
    cam = Cam(w, h)
    nrec = n_records(w, h)
    rng = np.random.default_rng(23 + w)
    z = near([0, 0, 1], 700, rng)
    xs, ys = near([1, 0, 0], 300, rng), near([0, 1, 0], 300, rng)
    n0, n1, n2 = counts
    sets = [np.concatenate([z[:n0 - 100], xs[:100]]), np.concatenate([ys[:100], z[:n1 - 100]]),
            _interleave(n2, z, np.stack([xs[:150], ys[:150]], 1).reshape(-1, 3))]
    assert [len(s) for s in sets] == list(counts)
    expect = {0: dict(found=5, pushed=[(nrec, 2), (nrec + n0 - 101, 2), (nrec + n0 - 1, 0)]),
              1: dict(found=6, pushed=[(nrec, 1), (nrec + n1 - 1, 2)]),
              2: dict(found=7, pushed=[(nrec + n2 - 2, 2), (nrec + n2 - 1, 2)])}
    depth = np.stack([tilted(w, h, 10000, 2, 1)] * 3)
    return _msc(f"compaction_seams_{nrec}", f"{nrec} records + {n0}, {n1}, {n2} lines: selected entries on both sides of every 1 024-"
                "entry chunk boundary and of the record / line seam", cam, depth, [_call([I3] * 3, sets, 3, 1, expect=expect)],
                seams=True)


def degenerate_start():
    cam = Cam(192, 144)
    rng = np.random.default_rng(24)
    R = R1.astype(f64)
    Rnan = R1.copy()
    Rnan[0, 1] = np.nan
    sets = [near([0, 1, 0], 40, rng, 0.02), np.concatenate([near([1, 0, 0], 6, rng), near([0, 1, 0], 6, rng)]),
            np.concatenate([near(R[:, a], 6, rng) for a in range(3)])]
    R0 = [np.array([[1, 1, 0], [0, 0, 0], [0, 0, 1]], f32), np.diag([1, 1, -1]).astype(f32), Rnan]
    # the NaN sits in column 1: lambda of axes x and y is NaN (never in a cone); axis z is projected from columns 2 and 0, so its
    # lines are in the cone and pushed, but m_j divides by the NaN third component and every one is dropped
    expect = {0: dict(found=7, svd=1), 1: dict(found=3, svd=1), 2: dict(found=0, svd=0, n_selected=[0, 0, 0], unchanged=True)}
    return _msc("degenerate_start", "a rank-deficient R0 (the SVD's zero-singular-value branch with its cv::RNG arithmetic), a "
                "reflection, and an R0 with a NaN entry", cam, np.zeros((3, cam.h, cam.w)), [_call(R0, sets, 3, 1, expect=expect)],
                hits=("svd_zero_singular_value", "pair_3"))


def constant_depth():
    """2.0 m everywhere under R0 = I: the normals are exactly (0, 0, -1), every one is in the z cone with lambda == 0, pushed
    and dropped; nothing is selected and R comes back unchanged"""
    cam = Cam(192, 144)
    expect = {0: dict(in_cone=[0, 0, 308], n_selected=[0, 0, 0], threshold=0, deficient=1, found=0, svd=0, unchanged=True)}
    return _msc("constant_depth", "every record in the cone, none selected (lambda == 0), R unchanged", cam,
                np.full((1, cam.h, cam.w), 10000), [_call([I3], [NO_LINES], 1, 1, expect=expect)], hits=("zero_lambda_dropped", "found_0"))


def calls_and_sequences():
    """three sequences of four frames (room corner, room corner, zero depth, room corner) with different R0; the line counts
    0, 300, 0, 7 (5, 0, 0, 300 in the middle sequence) make the largest frame size the scratch; the zero-depth frame without
    lines passes R through and the next frame resumes.  Then, on the same normals batch and context: 2 x 3 frames with 5 calls,
    and 2 x 1 frames with 1 call (the smaller call after the larger one on the same buffers)."""
    cam = CORNER_CAM
    full, R = corner(cam)
    wall = cut_corner(cam, CUT_WALL)[0]
    zero = np.zeros_like(full)
    depth = np.stack([full, full, zero, full, wall, wall, zero, wall, full, full, zero, full])
    Rd = R.astype(f64)
    rng = np.random.default_rng(25)

    def room_lines(n):
        return np.concatenate([near(Rd[:, a], n // 3 + (a < n % 3), rng) for a in range(3)]) if n else NO_LINES

    counts = [0, 300, 0, 7, 5, 0, 0, 300, 0, 300, 0, 7]
    R0 = [R, (Rd @ rot(2, 2.0)).astype(f32), (Rd @ rot(0, 3.0)).astype(f32)]
    passes = dict(found=0, svd=0, n_selected=[0, 0, 0], unchanged=True)
    expect = {2: passes, 6: passes, 10: passes, 0: dict(found=7), 3: dict(found=7), 5: dict(found=6), 7: dict(found=7), 11: dict(found=7)}
    calls = [_call(R0, [room_lines(n) for n in counts], 3, 4, 3, expect),
             _call([R0[1], R0[0]], [room_lines(n) for n in (3, 0, 0, 40, 0, 2)], 2, 3, 5, {2: dict(found=0, svd=0)}),
             _call([R0[2], R0[0]], [room_lines(4), room_lines(4)], 2, 1, 1, {0: dict(found=7), 1: dict(found=7)})]
    return _msc("calls_and_sequences", "1, 3 and 5 calls; sequences side by side; scratch sized by the frame with most lines; a frame "
                "that loses tracking mid-sequence; a smaller call after a larger one", cam, depth, calls, hits=("found_0", "found_3"))


_MANHATTAN = []


def manhattan_scenarios():
    if not _MANHATTAN:
        _MANHATTAN.extend([lines_decide(), gate_at_zero(), gate_positive(), compaction_seams(258, 195, (671, 672, 673)),
                           compaction_seams(192, 144, (255, 256, 257)), degenerate_start(), constant_depth(), calls_and_sequences()])
    return _MANHATTAN
