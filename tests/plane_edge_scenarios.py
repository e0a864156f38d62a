"""Hand-built depth images that drive the device plane extractors (k_ahc_cluster / k_ahc_refine / k_ahc_labels_* and k_cape_frame)
into the branches the rendered scenes do not reach: fixed capacities, ties between queue keys, the edges of the block grid, the
switch between the small and the big kernel forms, the support threshold, contended flood-fill pixels, hand-backs inside a
batch.  Pure numpy: every builder returns a depth image with its own K4 (uint16 counts for AHC, float32 metres for CAPE), its
docstring names the branch it aims at, and a precondition function beside it proves from the CPU oracle's outputs alone
(oracle.ahc_planes / oracle.cape_planes) that the image has the property claimed.  Nothing here reads the product.

What shapes the AHC frames (measured with the oracle): the reference feeds metres into PEAC's millimetre thresholds, so the merge
MSE bound never binds and ONLY the 60-degree normal gate stops a merge; a depth step does not stop a merge either, it
invalidates the block left of / above it (T_dz = 0.04 z + 0.02 "mm", read as metres); and a plane survives refineDetails only if
one of its blocks has all four neighbours in its own set, so facets are at least three blocks wide and tall."""
import functools
from dataclasses import dataclass, field

import numpy as np

WIN = 10                                   # PEAC's block: 10 x 10 pixels
FACTOR = 5000.0                            # depth counts per metre
INV = float(np.float32(1.0) / np.float32(FACTOR))
K_TUM3 = np.array([535.4, 539.2, 320.1, 247.6], np.float32)
K_CENTRED = np.array([525.0, 525.0, 319.5, 239.5], np.float32)   # principal point half-way between two pixels: the wall's block sums tie


def scaled_k(w, h, base=K_TUM3):
    """The base 640 x 480 intrinsics scaled to a w x h image."""
    return (base * np.array([w / 640.0, h / 480.0, w / 640.0, h / 480.0])).astype(np.float32)


@dataclass
class AhcFrame:
    name: str
    depth: np.ndarray                      # [h, w] uint16
    K4: np.ndarray
    to_host: int = 0                       # 1: designed to exceed a capacity of the device extractor
    truth: tuple = None                    # (planes [(unit normal, d)], label image) where the scene has a closed form
    info: dict = field(default_factory=dict)
    pre: object = None                     # the precondition function: pre(frame, oracle.ahc_planes(...)) -> measured values

    @property
    def size(self):
        return self.depth.shape[1], self.depth.shape[0]


def _rays(K4, w, h):
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return np.stack([(u - float(K4[2])) / float(K4[0]), (v - float(K4[3])) / float(K4[1]), np.ones_like(u)], -1)


def tilt(deg, axis):
    """Unit normal of a fronto-parallel plane turned by deg about the vertical ("y": the depth then changes along x) or the
    horizontal ("x") image axis."""
    a = np.deg2rad(float(deg))
    return np.array([np.sin(a), 0.0, np.cos(a)]) if axis == "y" else np.array([0.0, np.sin(a), np.cos(a)])


def facet_depth(w, h, K4, label, normals, anchors, z0):
    """Depth in metres of a facet field: pixel p shows the plane of facet label[p] (-1: no depth), which has unit normal
    normals[k] and passes through the point seen by pixel anchors[k] = (u, v) at depth z0 - so facets that share an anchor depth
    stay continuous where their anchors' mid-lines meet."""
    r = _rays(K4, w, h)
    normals, anchors = np.asarray(normals, np.float64), np.asarray(anchors, np.float64)
    ra = np.stack([(anchors[:, 0] - float(K4[2])) / float(K4[0]), (anchors[:, 1] - float(K4[3])) / float(K4[1]), np.ones(len(anchors))], -1)
    num = z0 * np.einsum("ij,ij->i", normals, ra)
    k = np.where(label < 0, 0, label)
    z = num[k] / np.einsum("hwj,hwj->hw", normals[k], r)
    return np.where(label < 0, 0.0, z)


def to_counts(z, noise=0, seed=0):
    d = np.rint(np.asarray(z) * FACTOR)
    if noise:
        d = d + np.where(d > 0, np.random.default_rng(seed).integers(-noise, noise + 1, d.shape), 0)
    return np.clip(d, 0, 65535).astype(np.uint16)


def block_grid(w, h):
    return w // WIN, h // WIN


def block_labels_to_pixels(bl, w, h):
    """[Nh, Nw] block labels -> [h, w] pixel labels; the spare pixels right of / below the grid repeat the last block's."""
    Nw, Nh = block_grid(w, h)
    iy, ix = np.minimum(np.arange(h) // WIN, Nh - 1), np.minimum(np.arange(w) // WIN, Nw - 1)
    return bl[np.ix_(iy, ix)]


def tele_k(w, h):
    """A narrow field of view (rays within 0.16 .. 0.32 of the axis): +-65 degree tilts stay far from grazing, and the depth steps
    between facets stay below T_dz.  The principal point lies half-way between the two middle pixels, as K_CENTRED's does."""
    return np.array([2000.0, 2000.0, w / 2 - 0.5, h / 2 - 0.5], np.float32)


K_TELE = tele_k(640, 480)


class _Cam:
    def __init__(self, w, h, K4):
        self.w, self.h = w, h
        self.fx, self.fy, self.cx, self.cy = (float(v) for v in K4)
        self.depth_factor = FACTOR


# ---------------------------------------------------------------------------------------------------------------------------
# AHC

GRID_EDGE_SIZES = [(19, 400), (400, 19), (20, 310), (30, 310), (310, 20), (310, 30), (649, 489), (70, 70)]


def grid_edge(w, h, seed=3):
    """initGraph's skip pattern at the grid's edges (j == Nw - 1, i == Nh - 1): block grids 1, 2 and 3 wide or tall, even against
    odd, nine spare pixels beside the grid (649 x 489), 49 blocks just above minimum support (70 x 70).  One plane 2.5 m away,
    turned 20 degrees about the vertical and -12 about the horizontal axis, +-1 count of noise; K is TUM3's with the principal
    point at the image's middle."""
    K4 = np.array([535.4, 539.2, w / 2 + 0.1, h / 2 - 0.4], np.float32)
    n = np.array([np.sin(np.deg2rad(20.0)), np.sin(np.deg2rad(-12.0)), 0.0])
    n[2] = np.sqrt(1.0 - n[0] ** 2 - n[1] ** 2)
    z = 2.5 / (_rays(K4, w, h) @ n)
    return AhcFrame(f"grid_edge_{w}x{h}_s{seed}", to_counts(z, 1, seed), K4, truth=([(n, 2.5)], np.zeros((h, w), int)),
                    info=dict(Nw=w // WIN, Nh=h // WIN))


def grid_edge_precondition(fr, o):
    """Every block is valid (the skip pattern then depends on the grid's size alone) and the grid has the claimed extent."""
    Nw, Nh = block_grid(*fr.size)
    assert (Nw, Nh) == (fr.info["Nw"], fr.info["Nh"]) and len(o["block_valid"]) == Nw * Nh
    assert o["block_valid"].all() and (o["block_N"] == WIN * WIN).all()
    return dict(blocks=Nw * Nh, planes=len(o["planes"]))


SWITCH_SIZES = [(800, 400), (810, 400), (1000, 600)]


def kernel_switch(w, h, seed=0):
    """The launcher's NB <= 3200 switch: 800 x 400 has exactly 3200 blocks (the small kernels at their limit), 810 x 400 has 3240
    (the big kernels at a small size), 1000 x 600 lies between that and the 1280 x 960 the big form otherwise runs at.  The room
    corner of plane_scenarios (floor, back wall, left wall) on TUM3's camera scaled to the size, +-2 counts of noise."""
    from plane_scenarios import room_corner
    K4 = scaled_k(w, h)
    planes, lab, _, d16 = room_corner(_Cam(w, h, K4), noise=2, seed=seed)
    return AhcFrame(f"switch_{w}x{h}_s{seed}", d16, K4, truth=(planes, lab), info=dict(blocks=(w // WIN) * (h // WIN)))


def kernel_switch_precondition(fr, o):
    nb = len(o["block_valid"])
    assert nb == fr.info["blocks"] and len(o["planes"]) == 3
    return dict(blocks=nb, small_form=nb <= 3200)


def _facet_field(w, h, K4, fw, fh, rows, cols, row0=0, col0=0, deg=50.0, z0=2.0, holes=()):
    """rows x cols facets of fw x fh blocks from block (row0, col0) on, no depth elsewhere: each a plane through its middle at
    z0, turned +-deg about the vertical axis in a checkerboard - horizontal neighbours form a continuous zigzag, vertical
    neighbours differ by steps below T_dz under the narrow field of view, and any two neighbours are 2 * deg apart."""
    Nw, Nh = block_grid(w, h)
    bl = -np.ones((Nh, Nw), int)
    normals, anchors = [], []
    for a in range(rows):
        for b in range(cols):
            r, c = row0 + a * fh, col0 + b * fw
            assert r + fh <= Nh and c + fw <= Nw
            bl[r:r + fh, c:c + fw] = len(normals)
            normals.append(tilt(deg if (a + b) % 2 == 0 else -deg, "y"))
            anchors.append((c * WIN + fw * WIN / 2 - 0.5, r * WIN + fh * WIN / 2 - 0.5))
    lab = block_labels_to_pixels(bl, w, h)
    lab[Nh * WIN:, :] = -1
    lab[:, Nw * WIN:] = -1
    d = to_counts(facet_depth(w, h, K4, lab, normals, anchors, z0))
    for (y, x) in holes:
        d[y, x] = 0
    return d, bl


def support_threshold():
    """`N >= AHC_MIN_SUPPORT` in the clustering and `dsSize * 100 >= AHC_MIN_SUPPORT` in the membership pass exactly at 3000
    points / 30 blocks: eight facets of 3 x 10 blocks along the bottom of a 640 x 480 frame (an even extent is linked completely
    only where it ends on the grid's last row: the i == Nh - 1 rule), neighbours 100 degrees apart.  Facets 2 and 5 have one pixel
    without depth, which costs them a whole block: 29 blocks, 2900 points, no plane.  The other six have N == 3000."""
    w, h = 640, 480
    K4 = tele_k(w, h)
    holes = [(h - 100 + 34, (20 + 2 * 3 + 1) * WIN + 5), (h - 100 + 95, (20 + 5 * 3 + 2) * WIN + 2)]
    d, bl = _facet_field(w, h, K4, 3, 10, 1, 8, row0=38, col0=20, holes=holes)
    return AhcFrame("support_threshold", d, K4, info=dict(bl=bl, holed=(2, 5), full=(0, 1, 3, 4, 6, 7)))


def support_threshold_precondition(fr, o):
    """The oracle reports six planes, each with N == 3000 exactly and rooted in a full facet; the holed facets have 29 valid
    blocks and no plane.  (A plane's N is the sum of its blocks' points: the flood fill adds labels, not points.)"""
    bl = fr.info["bl"].ravel()
    for k in fr.info["holed"]:
        assert o["block_valid"][bl == k].sum() == 29
    for k in fr.info["full"]:
        assert o["block_valid"][bl == k].sum() == 30
    assert len(o["planes"]) == 6 and (o["N"] == 3000).all()
    assert sorted(int(bl[r]) for r in o["rid"]) == list(fr.info["full"])
    Nw = fr.size[0] // WIN
    centres = o["seg"][WIN // 2::WIN, WIN // 2::WIN][:len(bl) // Nw, :Nw].ravel()
    for k in fr.info["holed"]:
        assert not centres[(bl == k) & (o["block_valid"] != 0)].any()
    return dict(planes=6, N=3000, holed_blocks=29)


def many_planes(w, h):
    """More planes than the device holds: facets of 3 x 11 blocks (odd extents: initGraph's stride of two then links every block
    of a facet), a checkerboard of +-50 degrees about the vertical axis, neighbours in both directions 100 degrees apart.
    640 x 480 holds 21 x 4 = 84 of them (`nFinal > planeCap` = 64 in k_ahc_refine), 1000 x 600 holds 33 x 5 = 165 (`nEx >= 128`
    in k_ahc_cluster), 1280 x 960 holds 42 x 8 = 336 (more than the 254 labels of a CV_8U image: every entry refuses the frame)."""
    K4 = tele_k(w, h)
    Nw, Nh = block_grid(w, h)
    d, bl = _facet_field(w, h, K4, 3, 11, Nh // 11, Nw // 3)
    return AhcFrame(f"many_planes_{w}x{h}", d, K4, to_host=1, info=dict(facets=(Nh // 11) * (Nw // 3)))


def many_planes_precondition(fr, o):
    """The oracle's plane count is the facet count, and lies in the range the size was chosen for."""
    n = len(o["N"])
    assert n == fr.info["facets"] and (o["N"] == 3300).all()
    lo, hi = {640: (65, 127), 1000: (129, 254), 1280: (255, 10 ** 6)}[fr.size[0]]
    assert lo <= n <= hi
    return dict(planes=n)


def comb(w=640, h=480, teeth_cols=None, deg=65.0, z0=2.0, K4=None):
    """Neighbour lists: block row 0 and every even block column are flat (z0 = 2 m, one node once merged); every other block below
    row 0 in the columns `teeth_cols` (default: all odd columns) is a planar block turned 65 degrees - about the vertical axis in
    even block rows, about the horizontal axis in odd ones, away from the optical axis - and centred on z0, so its borders stay
    continuous, it stays valid, and the 60-degree gate keeps it a single node beside the growing flat node.  All odd columns:
    47 x 32 = 1504 teeth, the flat node's list passes 376 (`Lp > listCap` / `Lc > listCap`, small form) - at 1280 x 960 95 x 64
    = 6080 teeth pass the big form's 1024.  Columns 1, 3, 5: 141 teeth, above the 64 entries of the short union and below
    the cap (`Lp + Lc > 64`: the union through binary-search ranks, no hand-back)."""
    K4 = K_TUM3 if K4 is None else K4
    Nw, Nh = block_grid(w, h)
    cols = list(range(1, Nw, 2)) if teeth_cols is None else list(teeth_cols)
    bl = np.zeros((Nh, Nw), int)
    normals, anchors = [np.array([0.0, 0.0, 1.0])], [(0.0, 0.0)]
    for i in range(1, Nh):
        for j in cols:
            bl[i, j] = len(normals)
            axis = "y" if i % 2 == 0 else "x"
            off = (j * WIN + 4.5 - float(K4[2])) if axis == "y" else (i * WIN + 4.5 - float(K4[3]))
            normals.append(tilt(deg if off >= 0 else -deg, axis))
            anchors.append((j * WIN + 4.5, i * WIN + 4.5))
    d = to_counts(facet_depth(w, h, K4, block_labels_to_pixels(bl, w, h), normals, anchors, z0))
    teeth = len(normals) - 1
    cap = 376 if Nw * Nh <= 3200 else 1024
    return AhcFrame(f"comb_{w}x{h}_{teeth}", d, K4, to_host=int(teeth > cap), info=dict(bl=bl, teeth=teeth, cap=cap))


def comb_precondition(fr, o):
    """Every block is valid; the oracle finds exactly one plane, whose N is 100 x the number of flat blocks (no tooth merged, no
    flat block left out); and the number of teeth 4-adjacent to a flat block - the flat node's neighbour list once it has
    swallowed the flat blocks, counted from the block layout alone - is on the claimed side of 64 and of the list cap."""
    bl = fr.info["bl"]
    flat = bl == 0
    assert o["block_valid"].all()
    assert len(o["planes"]) == 1 and o["N"][0] == 100 * int(flat.sum())
    adj = np.zeros_like(flat)
    adj[1:] |= flat[:-1]; adj[:-1] |= flat[1:]; adj[:, 1:] |= flat[:, :-1]; adj[:, :-1] |= flat[:, 1:]
    longest = int((adj & ~flat).sum())
    assert longest == fr.info["teeth"] > 64
    assert (longest > fr.info["cap"]) == bool(fr.to_host)
    normal = o["blocks"][:, 12:15]
    assert (np.abs(normal[~flat.ravel(), 2]) < 0.5).all() and (np.abs(normal[flat.ravel(), 2]) > 0.999).all()
    return dict(planes=1, N=int(o["N"][0]), list_length=longest, cap=fr.info["cap"])


def tie_wall():
    """Queue keys that tie (heap_less / heap_less_new / the `ties` loop of heap_sift_down): a flat wall at 10 000 counts under
    K = (525, 525, 319.5, 239.5).  Blocks mirrored about the principal point have the same sums, so many block MSEs (negative,
    about -2e-15) are equal as doubles - settled by node id - and far more are equal as floats only."""
    return AhcFrame("tie_wall", np.full((480, 640), 10000, np.uint16), K_CENTRED.copy(), info=dict(double_ties=True))


def tie_mirrored_noise(w=640, h=480, seed=5, double_ties=True):
    """The same ties with +-2 counts of noise mirrored about both axes ([[q, q[:, ::-1]], [q[::-1], q[::-1, ::-1]]]) under the
    centred K of the size: blocks opposite each other still tie as floats, a few as doubles.  The 400 x 300 frames (seeds 4 and
    3: one double tie and none) stay on the device and carry the tie branches.  The 640 x 480 frame is a finding, kept as one:
    the device hands it back, and to_host = 1 asserts that observation - unlike every other hand-back here it is NOT derived from
    the layout or from the oracle's outputs, and no precondition proves it.  The cause is inferred: a fronto-parallel wall with
    noise merges in a scattered order, so the growing node's frontier, its neighbour list, gets long; an instrumented build of
    the oracle (not part of this repository) counted a longest list of 991 entries for seed 5, far above the small form's 376.
    The counter does not say which capacity a frame hit, and the 2^19-word neighbour pool is the other candidate.  The ties
    before the hand-back still go through the device queue, and the frame's result is compared like any other."""
    q = np.random.default_rng(seed).integers(-2, 3, (h // 2, w // 2))
    n = np.block([[q, q[:, ::-1]], [q[::-1], q[::-1, ::-1]]])
    K4 = np.array([525.0, 525.0, w / 2 - 0.5, h / 2 - 0.5], np.float32)
    return AhcFrame(f"tie_mirrored_noise_{w}x{h}_s{seed}", (10000 + n).astype(np.uint16), K4, to_host=int((w, h) == (640, 480)),
                    info=dict(double_ties=double_ties))


def tie_raised_pixel():
    """One pixel raised by one count in every block of a flat wall under TUM3's K: block MSEs that differ as doubles and are equal
    as floats (the float key decides nothing, the double decides), and no double tie."""
    d = np.full((480, 640), 10000, np.uint16)
    d[3::WIN, 6::WIN] += 1
    return AhcFrame("tie_raised_pixel", d, K_TUM3.copy(), info=dict(double_ties=False))


def tie_counts(o):
    """(pairs' worth of valid blocks whose MSE equals another's as float32 but not as double, surplus blocks in groups of equal doubles)."""
    m = o["blocks"][o["block_valid"] != 0, 15]
    _, cd = np.unique(m, return_counts=True)
    f = m.astype(np.float32)
    _, cf = np.unique(f, return_counts=True)
    surplus_d, surplus_f = int((cd - 1).sum()), int((cf - 1).sum())
    return surplus_f - surplus_d, surplus_d


def tie_precondition(fr, o):
    """At least one pair of valid blocks with equal float32(mse) and different doubles; for the exact-tie frames at least one
    pair of equal doubles as well."""
    float_only, double = tie_counts(o)
    assert float_only >= 1
    if fr.info["double_ties"]:
        assert double >= 1
    return dict(float_only_ties=float_only, double_ties=double)


def crease(kind, seed=7):
    """The flood fill's same-pixel chains: two planes 130 degrees apart (+-65 degrees) meet at a crease through the middle of a
    line of blocks - vertical: the middle of block column 32; diagonal: the corner-to-corner diagonal of the blocks (i, i + 8).
    The crease blocks' normals lie between the two (65 degrees from each: they join neither), so both planes grow into them
    pixel by pixel, and the pixels next to the crease lie within the refine distance of both.  +-1 count of noise."""
    w, h = 640, 480
    K4 = K_TELE.copy()
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    a = np.deg2rad(65.0)
    if kind == "vertical":
        side = (u > 324.5).astype(int)
        normals = [np.array([-np.sin(a), 0.0, np.cos(a)]), np.array([np.sin(a), 0.0, np.cos(a)])]
        anchor = (324.5, 239.5)
    else:
        side = (u - v > 80).astype(int)                       # the line u - v = 80 runs corner to corner through blocks (i, i + 8)
        s = np.sin(a) / np.sqrt(2.0)
        normals = [np.array([-s, s, np.cos(a)]), np.array([s, -s, np.cos(a)])]
        anchor = (319.5, 239.5)
    z = facet_depth(w, h, K4, side, normals, [anchor, anchor], 2.0)
    ra = np.array([(anchor[0] - float(K4[2])) / float(K4[0]), (anchor[1] - float(K4[3])) / float(K4[1]), 1.0])
    planes = [(n, float(2.0 * (n @ ra))) for n in normals]
    return AhcFrame(f"crease_{kind}_s{seed}", to_counts(z, 1, seed), K4, truth=(planes, side), info=dict(kind=kind))


def crease_blocks(fr):
    Nw, Nh = block_grid(*fr.size)
    side = fr.truth[1]
    s = side[:Nh * WIN, :Nw * WIN].reshape(Nh, WIN, Nw, WIN)
    return (s.min((1, 3)) != s.max((1, 3)))


def crease_precondition(fr, o):
    """Two planes; no crease block is a block member of either (their pixels carry labels the flood fill gave them); and pixels of
    the crease blocks carry both labels."""
    assert len(o["planes"]) == 2
    cb = crease_blocks(fr)
    Nw, Nh = block_grid(*fr.size)
    seg = o["seg"][:Nh * WIN, :Nw * WIN].reshape(Nh, WIN, Nw, WIN).transpose(0, 2, 1, 3)[cb]
    both = sum(1 for b in seg if (b == 1).any() and (b == 2).any())
    assert both >= 0.9 * len(seg) and len(seg) >= 30
    return dict(crease_blocks=int(cb.sum()), blocks_with_both_labels=both)


# ---------------------------------------------------------------------------------------------------------------------------
# CAPE (float32 metres; the reference feeds metres into CAPE's millimetre thresholds too: only the 15-degree gate stops growth)

@dataclass
class CapeFrame:
    name: str
    depth: np.ndarray                      # [h, w] float32 metres
    K4: np.ndarray
    patch: int = 20
    capacity: int = 0                      # 1: designed to exceed CAPE_DEV_MAXP - 1 = 63 segments
    info: dict = field(default_factory=dict)
    pre: object = None


CAPE_BINS = 20


def cape_bins(c):
    """The histogram bin of every planar cell of oracle.cape_planes(...) (-1: not planar), with the kernel's formula
    (CAPE.cpp:81-104, Histogram.cpp: polar and azimuth angle of the normal on a 20 x 20 grid over [0, 3.14] x [-3.14, 3.14]), and
    whether any quotient lies within 1e-9 of an integer - there the device does not trust its own truncation and hands the
    frame back."""
    n = c["cells"][:, 12:15]
    planar = c["cell_planar"] != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        npn = np.sqrt(n[:, 0] ** 2 + n[:, 1] ** 2)
        vx = (CAPE_BINS - 1) * np.arccos(-n[:, 2]) / 3.14
        vy = (CAPE_BINS - 1) * (np.arctan2(n[:, 0] / npn, n[:, 1] / npn) + 3.14) / 6.28
    vx, vy = np.where(planar, vx, 0.5), np.where(planar, vy, 0.5)
    xq = vx.astype(np.int64)
    yq = np.where(xq > 0, np.where(np.isfinite(vy), vy, 0.0).astype(np.int64), 0)
    near = ~(np.abs(vx - np.rint(vx)) > 1e-9) | ((xq > 0) & ~(np.abs(vy - np.rint(vy)) > 1e-9)) | ((xq <= 0) & ~(vx < 1.0 - 1e-9))
    return np.where(planar, yq * CAPE_BINS + xq, -1), bool((near & planar).any())


def cape_first_seed(c):
    """(the seed of the first round by the reference's literal rule - `minMSE` refreshed from Grid[position in the candidate
    list], not from the candidate - , the arg-min of the MSE over the same candidates, the candidate count)."""
    bins, _ = cape_bins(c)
    hist = np.bincount(bins[bins >= 0], minlength=CAPE_BINS * CAPE_BINS)
    cand = np.flatnonzero(bins == int(hist.argmax()))                   # argmax: the first of equals
    mse = c["cell_mst"][:, 0]
    seed, m = int(cand[0]), np.float32(2 ** 31 - 1)
    for pos, i in enumerate(cand):
        if mse[i] < m:
            seed, m = int(i), mse[pos]
    return seed, int(cand[np.argmin(mse[cand])]), len(cand)


def _cape_walls(w, h, K4, label, normals, z0=2.0, noise=0.0, seed=0):
    z = facet_depth(w, h, K4, label, normals, [((w - 1) / 2.0, (h - 1) / 2.0)] * len(normals), z0)
    if noise:
        z = z + np.where(z > 0, np.random.default_rng(seed).uniform(-noise, noise, z.shape), 0.0)
    return z.astype(np.float32)


def cape_bin_tie():
    """"The fullest bin, the first of equals": the left half of the frame is a wall turned +32 degrees about the vertical axis,
    the right half one turned -32 degrees; the crease lies on a cell border, so each wall owns 16 x 24 cells and its own bin.
    3 mm of noise keep the float32 cell sums' smallest eigenvalue (hence the score) positive."""
    w, h = 640, 480
    u = np.arange(w)[None, :].repeat(h, 0)
    z = _cape_walls(w, h, K_TUM3, (u >= 320).astype(int), [tilt(32, "y"), tilt(-32, "y")], noise=0.003, seed=1)
    return CapeFrame("cape_bin_tie", z, K_TUM3.copy())


def cape_bin_tie_precondition(fr, c):
    bins, near = cape_bins(c)
    hist = np.sort(np.bincount(bins[bins >= 0], minlength=400))[::-1]
    assert hist[0] == hist[1] > 100 and not near and len(c["planes"]) == 2
    return dict(top_bins=(int(hist[0]), int(hist[1])), planes=len(c["planes"]))


def cape_seed_slip(seed=4):
    """The seed rule's index slip (`minMSE = cells[pos].MSE`): a wall turned 25 degrees with 2 mm of noise whose top-left cell has
    no depth.  The first candidate sets minMSE to cell 0's MSE - which is 0, the cell is not planar - so no later candidate
    replaces it: the literal rule seeds the first candidate, a plain arg-min another cell."""
    w, h = 640, 480
    z = _cape_walls(w, h, K_TUM3, np.zeros((h, w), int), [tilt(25, "y")], noise=0.002, seed=seed)
    z[:20, :20] = 0
    return CapeFrame("cape_seed_slip", z, K_TUM3.copy())


def cape_seed_slip_precondition(fr, c):
    literal, argmin, n = cape_first_seed(c)
    assert literal != argmin and n >= 5 and not cape_bins(c)[1]
    return dict(literal_seed=literal, argmin_seed=argmin, candidates=n, planes=len(c["planes"]))


def cape_four_cells():
    """`ncand < 5` ends the seeding: four planar cells (2 x 2) of a wall in an otherwise empty frame - no plane."""
    z = np.zeros((480, 640), np.float32)
    z[200:240, 300:340] = _cape_walls(640, 480, K_TUM3, np.zeros((480, 640), int), [tilt(25, "y")])[200:240, 300:340]
    return CapeFrame("cape_four_cells", z, K_TUM3.copy())


def cape_four_cells_precondition(fr, c):
    assert int((c["cell_planar"] != 0).sum()) == 4 and len(c["planes"]) == 0 and cape_first_seed(c)[2] == 4
    return dict(planar_cells=4, planes=0)


def cape_axis_wall(tilt_deg=0.0):
    """The `Xq == 0` branch: flat depth under K = (525, 525, 319.5, 239.5) - normals along the optical axis, the polar angle in
    the first bin, where the azimuth (0 / 0 when npn == 0) is not consulted.  With tilt_deg = 0 every cell normal is (0, 0, -1)
    exactly: the polar quotient is 0, an integer, so the device - which hands back any frame with a quotient within 1e-9 of an
    integer rather than trust its own truncation - is expected to hand this frame back (cape_bins reports it).  One degree of
    tilt (quotient 0.106) keeps the frame in the first polar bin and on the device."""
    w, h = 640, 480
    z = _cape_walls(w, h, K_CENTRED, np.zeros((h, w), int), [tilt(tilt_deg, "y")]) if tilt_deg else np.full((h, w), 2.0, np.float32)
    return CapeFrame(f"cape_axis_wall_{tilt_deg:g}", z, K_CENTRED.copy(), info=dict(near=not tilt_deg))


def cape_axis_wall_precondition(fr, c):
    bins, near = cape_bins(c)
    assert (c["cell_planar"] != 0).all() and (bins == 0).all() and near == fr.info["near"]
    n = c["cells"][:, 12:15]
    return dict(cells_in_bin_0=int((bins == 0).sum()), exact_axis_normals=int(((n[:, 0] == 0) & (n[:, 1] == 0)).sum()),
                near_integer=near, planes=len(c["planes"]))


def cape_capacity():
    """`S.np >= CAPE_DEV_MAXP - 1` (status CAPACITY): 10 x 8 = 80 facets of 6 x 6 cells at patch 10 on 640 x 480 (3072 cells, the
    device's limit), a checkerboard of +-25 degrees about the vertical axis - neighbours 50 degrees apart, every facet a segment
    of 36 cells with an eroded core: 80 planes where the device holds 63."""
    w, h = 640, 480
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    a, b = np.minimum(v // 60, 7), np.minimum(u // 60, 9)
    lab = a * 10 + b
    normals = [tilt(25 if (k // 10 + k % 10) % 2 == 0 else -25, "y") for k in range(80)]
    anchors = [((k % 10) * 60 + 29.5, (k // 10) * 60 + 29.5) for k in range(80)]
    z = facet_depth(w, h, K_TUM3, lab, normals, anchors, 2.0) + np.random.default_rng(2).uniform(-0.003, 0.003, (h, w))
    z[:, 600:] = 0
    return CapeFrame("cape_capacity", z.astype(np.float32), K_TUM3.copy(), patch=10, capacity=1)


def cape_capacity_precondition(fr, c):
    assert len(c["planes"]) >= 64 and not cape_bins(c)[1]
    return dict(planes=len(c["planes"]))


def cape_cell_limit(w):
    """Exactly CAPE_DEV_MAXCELLS = 3072 cells (640 x 480 at patch 10) on the device, against 3120 cells (650 x 480) and a width
    that is no multiple of the patch (645 x 480), neither of which qualifies for the device: the first goes to the host pool, the
    second is refused by planes_cape_core in either mode ("width/height must be multiples of PATCH_SIZE"; the oracle, like the
    reference, lets the spare pixels keep their row-major slot).  A wall turned 20 and -10 degrees, 1 mm of noise."""
    K4 = scaled_k(w, 480)
    n = np.array([np.sin(np.deg2rad(20.0)), np.sin(np.deg2rad(-10.0)), 0.0])
    n[2] = np.sqrt(1.0 - n[0] ** 2 - n[1] ** 2)
    z = _cape_walls(w, 480, K4, np.zeros((480, w), int), [n], noise=0.001, seed=w)
    return CapeFrame(f"cape_cells_{w}", z, K4, patch=10, info=dict(device=(w % 10 == 0 and (w // 10) * 48 <= 3072)))


def cape_cell_limit_precondition(fr, c):
    w = fr.depth.shape[1]
    assert len(c["cell_planar"]) == (w // 10) * 48 and len(c["planes"]) == 1
    return dict(cells=len(c["cell_planar"]), device=fr.info["device"])


def cape_degenerate(kind):
    """No depth at all (zeros), no number at all (NaN), and one planar cell alone."""
    z = np.zeros((480, 640), np.float32)
    if kind == "nan":
        z[:] = np.nan
    elif kind == "one_cell":
        z[100:120, 200:220] = 1.5
    return CapeFrame(f"cape_{kind}", z, K_TUM3.copy())


def cape_degenerate_precondition(fr, c):
    want = 1 if fr.name == "cape_one_cell" else 0
    assert int((c["cell_planar"] != 0).sum()) == want and len(c["planes"]) == 0
    return dict(planar_cells=want, planes=0)



# ---------------------------------------------------------------------------------------------------------------------------
# what the tests run: frames grouped into calls (one image size and one K4 per call), and the oracle's answers, computed once

def _with(pre, fr, **kw):
    fr.pre = pre
    for k, v in kw.items():
        setattr(fr, k, v)
    return fr


def no_depth():
    return AhcFrame("no_depth", np.zeros((480, 640), np.uint16), K_TELE.copy())


def no_depth_precondition(fr, o):
    assert not o["block_valid"].any() and len(o["planes"]) == 0
    return dict(planes=0)


def mixed_batch():
    """Hand-backs in the middle of a batch: [two-plane scene, full comb, no depth, 84 facets, two-plane scene, full comb, tie wall,
    two-plane scene] under one K (the narrow, centred one).  Frames 1, 3 and 5 exceed a capacity; their `jobs` words are zeroed,
    so k_voxel_grid gets no cloud for them, and the frames between them must come out untouched."""
    K4 = K_TELE
    return [_with(crease_precondition, crease("vertical", seed=11), name="mixed_0_scene"),
            _with(comb_precondition, comb(K4=K4), name="mixed_1_comb"),
            _with(no_depth_precondition, no_depth(), name="mixed_2_no_depth"),
            _with(many_planes_precondition, many_planes(640, 480), name="mixed_3_many_planes"),
            _with(crease_precondition, crease("diagonal", seed=12), name="mixed_4_scene"),
            _with(comb_precondition, comb(K4=K4), name="mixed_5_comb"),
            _with(tie_precondition, AhcFrame("mixed_6_tie_wall", tie_wall().depth, K4.copy(), info=dict(double_ties=True))),
            _with(crease_precondition, crease("vertical", seed=13), name="mixed_7_scene")]


@dataclass
class AhcCall:
    name: str
    frames: list
    cap: int = 64

    @property
    def K4(self):
        return self.frames[0].K4

    @property
    def depth(self):
        return np.stack([f.depth for f in self.frames])

    @property
    def to_host(self):
        return sum(f.to_host for f in self.frames)


@functools.lru_cache(maxsize=None)
def ahc_calls():
    """Every AHC scenario, grouped so that one image size and one K4 go through one call; a scenario alone at its size is sent
    twice (the batch entry takes the device path from two frames on)."""
    calls = []
    for w, h in GRID_EDGE_SIZES:
        calls.append(AhcCall(f"grid_edge_{w}x{h}", [_with(grid_edge_precondition, grid_edge(w, h, s)) for s in (3, 4)]))
    for w, h in SWITCH_SIZES:
        calls.append(AhcCall(f"switch_{w}x{h}", [_with(kernel_switch_precondition, kernel_switch(w, h, s)) for s in (0, 1)]))
    calls.append(AhcCall("tum3_640x480", [_with(comb_precondition, comb(teeth_cols=(1, 3, 5))), _with(comb_precondition, comb()),
                                          _with(tie_precondition, tie_raised_pixel())]))
    calls.append(AhcCall("centred_640x480", [_with(tie_precondition, tie_wall()), _with(tie_precondition, tie_mirrored_noise())]))
    calls.append(AhcCall("centred_400x300", [_with(tie_precondition, tie_mirrored_noise(400, 300, 4)),
                                             _with(tie_precondition, tie_mirrored_noise(400, 300, 3, double_ties=False))]))
    calls.append(AhcCall("tele_640x480", [_with(support_threshold_precondition, support_threshold()), _with(crease_precondition, crease("vertical")),
                                          _with(crease_precondition, crease("diagonal")), _with(many_planes_precondition, many_planes(640, 480))], cap=128))
    many = _with(many_planes_precondition, many_planes(1000, 600))
    calls.append(AhcCall("many_planes_1000x600", [many, many], cap=256))
    big = _with(comb_precondition, comb(1280, 960, K4=scaled_k(1280, 960)))
    calls.append(AhcCall("comb_1280x960", [big, big]))
    calls.append(AhcCall("mixed_640x480", mixed_batch(), cap=128))
    for c in calls:
        assert all(f.size == c.frames[0].size and np.array_equal(f.K4, c.K4) for f in c.frames), c.name
    return calls


def ahc_call(name):
    return next(c for c in ahc_calls() if c.name == name)


def refused_frame():
    """336 facets at 1280 x 960: more planes than the 254 labels of the CV_8U label image - every entry, host or device, refuses."""
    return _with(many_planes_precondition, many_planes(1280, 960))


_ORACLE = {}


def ahc_oracle(orc, fr):
    """oracle.ahc_planes of a frame, computed once per session and left unchanged."""
    key = (fr.name, fr.size, fr.K4.tobytes(), hash(fr.depth.tobytes()))
    if key not in _ORACLE:
        _ORACLE[key] = orc.ahc_planes(fr.depth, fr.K4, INV)
    return _ORACLE[key]


@dataclass
class CapeCall:
    name: str
    frames: list
    cap: int = 64
    refused: bool = False                  # the entry refuses the size (the oracle does not): host and device mode must refuse alike

    @property
    def patch(self):
        return self.frames[0].patch

    @property
    def K4(self):
        return self.frames[0].K4

    @property
    def depth(self):
        return np.stack([f.depth for f in self.frames])

    @property
    def device(self):
        w, h, p = self.frames[0].depth.shape[1], self.frames[0].depth.shape[0], self.patch
        return w % p == 0 and h % p == 0 and (w // p) * (h // p) <= 3072


@functools.lru_cache(maxsize=None)
def cape_calls():
    calls = [CapeCall("cape_tum3", [_with(cape_bin_tie_precondition, cape_bin_tie()), _with(cape_seed_slip_precondition, cape_seed_slip()),
                                    _with(cape_four_cells_precondition, cape_four_cells())] +
                                   [_with(cape_degenerate_precondition, cape_degenerate(k)) for k in ("zeros", "nan", "one_cell")]),
             CapeCall("cape_centred", [_with(cape_axis_wall_precondition, cape_axis_wall(0.0)), _with(cape_axis_wall_precondition, cape_axis_wall(1.0))]),
             CapeCall("cape_capacity", [_with(cape_capacity_precondition, cape_capacity()), _with(cape_cell_limit_precondition, cape_cell_limit(640)),
                                        _with(cape_capacity_precondition, cape_capacity())], cap=128)]
    for w in (650, 645):
        fr = _with(cape_cell_limit_precondition, cape_cell_limit(w))
        calls.append(CapeCall(f"cape_cells_{w}", [fr, fr], refused=w % 10 != 0))
    for c in calls:
        assert all(f.depth.shape == c.frames[0].depth.shape and f.patch == c.patch and np.array_equal(f.K4, c.K4) for f in c.frames), c.name
    return calls


def cape_oracle(orc, fr):
    key = (fr.name, fr.depth.shape, fr.K4.tobytes(), fr.patch, hash(fr.depth.tobytes()))
    if key not in _ORACLE:
        _ORACLE[key] = orc.cape_planes(fr.depth, fr.K4, patch=fr.patch)
    return _ORACLE[key]


def cape_expected_to_host(orc, fr):
    """1 where the frame is designed to exceed the device's 63 segments, or where the oracle-side recomputation of the histogram
    shows a quotient within 1e-9 of an integer (cape_axis_wall_0 - stated there); else 0."""
    return int(bool(fr.capacity) or cape_bins(cape_oracle(orc, fr))[1])
