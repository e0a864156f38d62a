"""Hand-built point clouds and planes that put the plane post-processing (Frame::ComputePlanes after the extractor) on its
thresholds: pcl::VoxelGrid's index sort and float centroid sums (k_voxel_grid / introsort_device.h on the device,
voxel_downsample on the host) and the gates + RANSAC refit of Frame::MaxPointDistanceFromPlane (k_plane_refit / refit_plane).

numpy only.  tests/test_post_edges_cpu.py holds the host entry points and the oracle to these scenarios,
tests/test_gpu_post_edges.py the device kernels through their test hooks (include/drfe_debug.h).

Voxel clouds.  A cloud is built from a sequence of leaf keys (one per point, the pattern under test); key k is the leaf
(k % 32, k // 32) of a lattice of 0.05 m leaves whose first leaf starts at 1 m, so every coordinate lies between 1 and 3 m and the
order of the keys is the order of VoxelGrid's leaf indices (index = x + y * divisions_x + z * divisions_x * divisions_y).  A
leaf's centroid is a float sum in the order std::sort leaves the leaf's points, so the coordinates are made to show that order:
up to SENSITIVE points of a leaf carry full random float32 mantissas, the others sit on multiples of 2^-8 m.  A sum of 20 000
coordinates below 3 m stays below 2^16, where a float's last bit is 2^-8: adding a lattice point never rounds, adding one of
the others rounds at the last bit of the running sum, and which bit that is depends on how many points came before it.  The
number of roundings per leaf is therefore bounded (the float64 definition stays within 2e-6 of the float sums at every size,
which 20 000 full-mantissa points in one leaf would not), yet the sum still changes with the order:
order_sensitive_leaves() counts the leaves in which the stable order and another order give different bits.
"""
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
LEAF = F32(0.05)
INV_LEAF = F32(1.0) / LEAF                     # 20.0f exactly: what VoxelGrid multiplies by
SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 20000)
PATTERNS = ("random", "few_leaves", "one_leaf", "ascending", "descending", "organ_pipe", "exponential", "scan_order")
ORD_HEAP_MAX = 1024                            # introsort_device.h: the longest range one lane heap-sorts
BASE_LEAF = 20                                 # leaf 20 starts at 1.0 m
SENSITIVE = 24                                 # points per leaf with full-mantissa coordinates
QUANTUM = 2.0 ** -8


# ----------------------------------------------------------------------------------------------------------------------
# voxel grid: key patterns

def pattern_keys(pattern, n, rng):
    """-> (keys [n] in [0, 1024), z leaf [n]) of the stated pattern; the leaf index is key + 1024 * z."""
    z = np.zeros(n, np.int64)
    if pattern == "random":
        k = rng.integers(0, 1024, n)
        z = rng.integers(0, 4, n)
    elif pattern == "few_leaves":
        k = rng.integers(0, 2 + n % 3, n)                                  # two to four leaves
    elif pattern == "one_leaf":
        k = np.full(n, 7)
    elif pattern == "ascending":
        k = np.sort(rng.integers(0, 1024, n))
    elif pattern == "descending":
        k = np.sort(rng.integers(0, 1024, n))[::-1]
    elif pattern == "organ_pipe":
        # over 4096 leaves: with 1024 the equal keys keep every partition balanced; this one drives libstdc++'s introsort out of
        # depth on a range of 962 records at n = 4097 (one lane's heap sort) and of 2771 at n = 8193 (handed back)
        k = np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]]) % 4096
        k, z = k % 1024, k // 1024
    elif pattern == "exponential":
        k = np.minimum(1023, rng.exponential(40, n).astype(np.int64))
    elif pattern == "scan_order":
        # a plane's pixels in raster order: 128 columns, a leaf covers 8 x 5 pixels, and the depth noise splits a leaf in two
        t = np.arange(n)
        k = (t // 128) // 5 * 32 + (t % 128) // 8
        z = rng.integers(0, 2, n)
    else:
        raise ValueError(pattern)
    return np.asarray(k, np.int64), z


def cloud_of_leaves(ix, iy, iz, rng, base=(BASE_LEAF, BASE_LEAF, BASE_LEAF)):
    """One point inside each given leaf (integer leaf coordinates relative to `base`): see the module text."""
    n = len(ix)
    leaf = np.stack([ix, iy, iz], 1).astype(np.float64) + np.asarray(base, np.float64)
    u = rng.uniform(0.12, 0.88, (n, 3))
    fine = ((leaf + u) * 0.05).astype(F32)
    coarse = (np.round((leaf + u) * 0.05 / QUANTUM) * QUANTUM).astype(F32)
    # SENSITIVE points of every leaf, chosen at random, keep their full mantissas
    key = (np.asarray(ix, np.int64) + 64 * np.asarray(iy, np.int64)) * 64 + np.asarray(iz, np.int64)
    shuffle = rng.permutation(n)
    order = shuffle[np.argsort(key[shuffle], kind="stable")]
    ks = key[order]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    rank = np.arange(n) - np.repeat(start, np.diff(np.r_[start, n]))
    sensitive = np.zeros(n, bool)
    sensitive[order[rank < SENSITIVE]] = True
    pts = np.where(sensitive[:, None], fine, coarse)
    assert np.array_equal(np.floor(pts * INV_LEAF).astype(np.int64), leaf.astype(np.int64))
    return np.ascontiguousarray(pts, F32)


@dataclass
class VoxelCase:
    name: str
    pts: np.ndarray
    pattern: str = ""
    keeps_input: bool = False         # the grid exceeds int32: PCL returns the input cloud, the device answers -1


def pattern_cloud(pattern, n, seed=0):
    rng = np.random.default_rng([PATTERNS.index(pattern), n, seed])
    k, z = pattern_keys(pattern, n, rng)
    return VoxelCase(f"{pattern}/{n}", cloud_of_leaves(k % 32, k // 32, z, rng), pattern)


_PATTERN_CACHE = {}


def pattern_clouds():
    """Every pattern at every size: 160 clouds, built once."""
    if "all" not in _PATTERN_CACHE:
        _PATTERN_CACHE["all"] = [pattern_cloud(p, n) for p in PATTERNS for n in SIZES]
    return _PATTERN_CACHE["all"]


def leaf_keys(pts, leaf=LEAF):
    """VoxelGrid's leaf index per point, in float32 as PCL computes it (filters/impl/voxel_grid.hpp:214-342); None where the
    grid exceeds int32 and PCL keeps the input."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    inv = F32(1.0) / F32(leaf)
    lo, hi = pts.min(0), pts.max(0)
    d = ((hi - lo) * inv).astype(np.int64) + 1
    if int(d[0]) * int(d[1]) * int(d[2]) > 2**31 - 1:
        return None
    ijk = np.floor(pts * inv).astype(np.int64)
    mn = np.floor(lo * inv).astype(np.int64)
    div = np.floor(hi * inv).astype(np.int64) - mn + 1
    ijk -= mn
    return ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]


def records_of(pts, leaf=LEAF):
    """The leaf << 32 | point records VoxelGrid sorts (drfe_debug_order_sort, kind 1)."""
    k = leaf_keys(pts, leaf)
    return (k.astype(np.uint64) << np.uint64(32)) | np.arange(len(k), dtype=np.uint64)


def centroids_in_order(pts, recs):
    """Float32 centroids of the leaves of sorted records, each leaf's points added one after the other in record order."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    key, idx = (recs >> np.uint64(32)).astype(np.int64), (recs & np.uint64(0xFFFFFFFF)).astype(np.int64)
    start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    count = np.diff(np.r_[start, len(key)])
    acc = np.zeros((len(start), 3), F32)
    for r in range(int(count.max())):                    # the r-th point of every leaf that has one
        live = np.flatnonzero(count > r)
        acc[live] = acc[live] + pts[idx[start[live] + r]]
    return acc / count.astype(F32)[:, None]


def float64_definition(pts, leaf=LEAF):
    """The definition tests/test_post_cpu.py holds the oracle to: float64 means of the leaves in ascending index order."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    inv = F32(1.0) / F32(leaf)
    ijk = np.floor(pts * inv).astype(np.int64)
    ijk -= ijk.min(0)
    dims = ijk.max(0) + 1
    key = ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * dims[0] * dims[1]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    sums = np.add.reduceat(pts[order].astype(np.float64), start, axis=0)
    return sums / np.diff(np.r_[start, len(ks)])[:, None]


def order_sensitive_leaves(pts, centroids):
    """Leaves whose centroid bits differ from the ones the stable order (points of a leaf in index order) gives."""
    recs = np.sort(records_of(pts))
    stable = centroids_in_order(pts, recs)
    assert stable.shape == centroids.shape
    return int((stable.view(np.uint32) != np.asarray(centroids, F32).view(np.uint32)).any(1).sum())


def forced_depths(n):
    """The depth limits that replace introsort's 2 lg n, as tests/test_gpu_lines.py forces them on the LSD sort."""
    lg = int(np.log2(max(1, n)))
    return sorted({0, 1, 2, 3, max(0, lg - 4), max(0, lg - 1), lg + 2})


# ----------------------------------------------------------------------------------------------------------------------
# voxel grid: geometric edges

def _patch(rng, n, origin, du, dv, noise=0.003):
    uv = rng.uniform(0, 1, (n, 2))
    p = np.asarray(origin, np.float64) + uv[:, :1] * np.asarray(du, np.float64) + uv[:, 1:] * np.asarray(dv, np.float64)
    return (p + rng.normal(0, noise, (n, 3))).astype(F32)


def geometric_cases():
    rng = np.random.default_rng(77)
    out = []
    out.append(VoxelCase("negative coordinates", _patch(rng, 3000, (-2.4, -1.9, -3.1), (1.1, 0.2, 0.1), (0.1, 0.9, -0.3))))
    # floor, not truncation: leaves -1 and 0 are different leaves on every axis
    p = _patch(rng, 3000, (-0.31, -0.27, -0.12), (0.62, 0.0, 0.1), (0.0, 0.55, 0.15))
    p[:40] = rng.uniform(-0.049, 0.049, (40, 3)).astype(F32)
    out.append(VoxelCase("straddling zero", p))
    # points exactly on leaf boundaries: k * 0.05f and its float neighbours, on every axis
    k = np.arange(-6, 7).astype(F32)
    edge = k * LEAF
    vals = np.concatenate([edge, np.nextafter(edge, F32(np.inf)), np.nextafter(edge, F32(-np.inf))]).astype(F32)
    g = np.stack(np.meshgrid(vals, vals[::3], vals[1::5], indexing="ij"), -1).reshape(-1, 3)
    out.append(VoxelCase("leaf boundaries", np.ascontiguousarray(g[rng.permutation(len(g))], F32)))
    # readDepthImage writes (0, 0, 0) for every pixel beyond 5 m: thousands of identical points beside a real plane
    p = _patch(rng, 2500, (-0.6, -0.5, 1.4), (1.2, 0.0, 0.3), (0.0, 1.0, 0.1))
    z = np.zeros((3000, 3), F32)
    mix = np.concatenate([p, z])[rng.permutation(5500)]
    out.append(VoxelCase("zeros beside a plane", np.ascontiguousarray(mix, F32)))
    # nx * ny * nz beyond int32: 1401^3.  PCL keeps the input
    p = _patch(rng, 600, (1.0, 1.0, 1.0), (0.5, 0.0, 0.0), (0.0, 0.5, 0.1))
    wide = np.concatenate([p, np.array([[0, 0, 0], [70.0, 70.0, 70.0]], F32)])[rng.permutation(602)]
    out.append(VoxelCase("box beyond int32", np.ascontiguousarray(wide, F32), keeps_input=True))
    # just below: 1290^3 = 2 146 689 000 leaves, keys of 31 bits (seven counting passes of five bits).  The far corner is one
    # point alone in its leaf: at 64 m a float centroid of several points could not meet the float64 definition's bound
    near = np.concatenate([p, np.array([[0, 0, 0], [64.49, 64.49, 64.49]], F32)])
    out.append(VoxelCase("box just below int32", np.ascontiguousarray(near[rng.permutation(len(near))], F32)))
    # no extent in one axis
    p = _patch(rng, 2000, (-0.5, -0.4, 1.5), (1.0, 0.0, 0.0), (0.0, 0.8, 0.0), noise=0.0)
    p[:, 2] = F32(1.5)
    out.append(VoxelCase("flat in z", p))
    p = p.copy()
    p[:, 0] = F32(-0.125)
    out.append(VoxelCase("flat in x and z", p))
    # +0.0 and -0.0 among the minima
    p = _patch(rng, 1500, (0.0, 0.0, 0.0), (0.7, 0.0, 0.0), (0.0, 0.6, 0.2), noise=0.0)
    p = np.abs(p)
    p[:30, 0] = F32(-0.0); p[30:60, 0] = F32(0.0); p[10:40, 1] = F32(-0.0); p[5:20, 2] = F32(0.0); p[20:35, 2] = F32(-0.0)
    out.append(VoxelCase("signed zeros at the minimum", np.ascontiguousarray(p[rng.permutation(len(p))], F32)))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# voxel grid: job lists

def job_list():
    """256 clouds for one call: sizes over every power-of-two class from 1 to 8192, each class met many times, empty clouds in
    between, and - ahead of ordinary clouds of their own size class - one cloud the device answers with -1 (grid beyond int32)
    and one it answers with -2 (organ pipe of 8193 leaf keys: libstdc++'s introsort runs out of depth on a range above 1024
    records; tests/test_post_edges_cpu.py asserts that from the host predicate).  -> (list of VoxelCase, index of the -1
    cloud, index of the -2 cloud)."""
    rng = np.random.default_rng(256)
    sizes = [1, 2, 3, 5, 9, 17, 40, 70, 130, 260, 520, 1030, 2050, 4100, 8200]
    cases = []
    wide = geometric_cases()[4]
    assert wide.keeps_input and 512 <= len(wide.pts) < 1024
    cases.append(VoxelCase("wide", wide.pts, keeps_input=True))                  # class 2^9, before the 520s and 600s
    pipe = pattern_cloud("organ_pipe", 8193)
    cases.append(pipe)                                                            # class 2^13, before the 8200s
    i = 0
    while len(cases) < 256:
        if i % 9 == 4:
            cases.append(VoxelCase("empty", np.zeros((0, 3), F32)))
        else:
            n = sizes[i % len(sizes)] + int(rng.integers(0, 3))
            pat = PATTERNS[i % len(PATTERNS)]
            if pat == "organ_pipe" and n > 1024:
                pat = "random"
            cases.append(pattern_cloud(pat, n, seed=1000 + i))
        i += 1
    return cases, 0, 1


# ----------------------------------------------------------------------------------------------------------------------
# planes and voxel clouds for the refit

PLANE_DTYPE = np.dtype([("normal", "<f8", (3,)), ("center", "<f8", (3,)), ("mse", "<f8"), ("curvature", "<f8"),
                        ("n_points", "<i4"), ("rid", "<i4")])      # drfe_plane


@dataclass
class RefitCase:
    name: str
    edge: str                       # the named edge this case is an instance of
    normal: tuple
    center: tuple
    cloud: np.ndarray
    max_point_dist: float = 9.0
    dist_threshold: float = 0.05
    accepted: object = None         # stated by hand where the construction decides it, else None
    design_k: float = 0.0           # the iteration bound the construction aims at (inlier fraction w: log 0.01 / log(1 - w^3))

    def plane(self):
        p = np.zeros((), PLANE_DTYPE)
        p["normal"], p["center"] = self.normal, self.center
        p["mse"], p["curvature"], p["n_points"], p["rid"] = 1e-5, 1e-4, 1000, 3
        return p

    def coef(self):
        n, c = np.asarray(self.normal, np.float64), np.asarray(self.center, np.float64)
        d = F32(-(n[0] * c[0] + n[1] * c[1] + n[2] * c[2]))
        return np.array([n[0], n[1], n[2], d], F32)


def gates(case):
    """The three gates of Frame::ComputePlanes / MaxPointDistanceFromPlane (src/Frame.cc:1003-1011, 1238-1242) in numpy:
    None if the plane reaches the RANSAC, else the number of the gate that rejects it."""
    c = case.coef()
    if c[3] > F32(case.max_point_dist):
        return 1
    if len(case.cloud) < 100:
        return 2
    p = case.cloud
    with np.errstate(invalid="ignore"):
        e = ((c[0] * p[:, 0] + c[1] * p[:, 1]) + c[2] * p[:, 2]) + c[3]
        if (np.abs(e.astype(np.float64)) > np.float64(case.dist_threshold)).any():
            return 3
    return None


def _sheet(rng, n, z=1.5, half=0.6, noise=0.002, offsets=None):
    xy = rng.uniform(-half, half, (n, 2))
    dz = rng.normal(0, noise, n) if offsets is None else offsets
    return np.column_stack([xy, z + dz]).astype(F32)


def _k_of(w):
    return float(np.log(0.01) / np.log(max(1e-16, 1.0 - w ** 3))) if w < 1 else 0.0


def refit_cases():
    rng = np.random.default_rng(4242)
    up, out = (0.0, 0.0, -1.0), []
    tilt = np.array([0.2, -0.5, -0.84]); tilt /= np.linalg.norm(tilt)

    def tilted(n, noise, d=1.7, half=0.6):
        a = np.cross(tilt, [1.0, 0, 0]); a /= np.linalg.norm(a)
        b = np.cross(tilt, a)
        uv = rng.uniform(-half, half, (n, 2))
        return (-d * tilt + uv[:, :1] * a + uv[:, 1:] * b + rng.normal(0, noise, (n, 1)) * tilt).astype(F32), tuple(-d * tilt)

    # gate 2: fewer than 100 voxels; and the sizes around a wavefront
    for n in (99, 100, 101):
        cloud, cen = tilted(n, 0.002)
        out.append(RefitCase(f"{n} voxels", "gate 2", tuple(tilt), cen, cloud, accepted=n >= 100))
    for n in (128, 129, 191, 192, 193, 255):
        cloud, cen = tilted(n, 0.003)
        out.append(RefitCase(f"n % 64 = {n % 64} ({n})", "wavefront tail", tuple(tilt), cen, cloud, accepted=True))
    # gate 1: d against Point.MaxDistance.  normal (0, 0, -1), centre (0, 0, z): d = z
    md = F32(2.5)
    for name, z, acc in (("d at max_point_dist", md, True), ("d one float above", np.nextafter(md, F32(9)), False),
                         ("d one float below", np.nextafter(md, F32(0)), True)):
        out.append(RefitCase(name, "gate 1", up, (0.0, 0.0, float(z)), _sheet(rng, 160, z=float(z)), max_point_dist=2.5, accepted=acc))
    # gate 3 and the tLess / tMost split.  Threshold 0.09375 (a float, with the same spacing on both sides), plane z = 0.1875:
    # a voxel at z = 0.09375 -/+ 2^-27 is one float above / below the threshold from the plane, and 0.1875 - z is exact
    th, d = 0.09375, 0.1875
    for name, e, acc in (("voxel at the threshold", F32(th), True), ("voxel one float above", np.nextafter(F32(th), F32(1)), False),
                         ("voxel one float below", np.nextafter(F32(th), F32(0)), True)):
        cloud = _sheet(rng, 150, z=d, half=0.4, noise=0.004)
        cloud[77] = (F32(0.05), F32(-0.11), F32(d) - e)
        assert F32(d) - cloud[77, 2] == e
        out.append(RefitCase(name, "gate 3", up, (0.0, 0.0, d), cloud, dist_threshold=th, accepted=acc))
    # exactly planar: every point an inlier of every hypothesis, one iteration
    g = np.stack(np.meshgrid(np.arange(-8, 8) / 16.0, np.arange(-6, 6) / 16.0, indexing="ij"), -1).reshape(-1, 2)
    cloud = np.column_stack([g, np.full(len(g), 1.5)]).astype(F32)[rng.permutation(len(g))]
    out.append(RefitCase("exactly planar", "planar", up, (0.0, 0.0, 1.5), cloud, accepted=True))
    cloud = np.column_stack([np.full(len(g), -0.75), g[:, 1] + 0.5, g[:, 0] + 2.0]).astype(F32)[rng.permutation(len(g))][:131]
    out.append(RefitCase("exactly planar, x = -0.75", "planar", (1.0, 0.0, 0.0), (-0.75, 0.5, 2.0), cloud, accepted=True))
    # collinear throughout: differences of the three coordinates are equal and exact, no sample is ever good
    t = (rng.permutation(256)[:150] / 128.0)
    line = np.column_stack([0.25 + t, -0.5 + t, 1.0 + t]).astype(F32)
    nl = np.array([1.0, 0.0, -1.0]) / np.sqrt(2.0)
    out.append(RefitCase("collinear throughout", "collinear", tuple(nl), (0.25, -0.5, 1.0), line, accepted=False))
    out.append(RefitCase("collinear throughout, 101", "collinear", tuple(nl), (0.25, -0.5, 1.0), line[:101].copy(), accepted=False))
    # a collinear majority: most samples are redrawn inside the 1000-attempt loop
    for k, nline in enumerate((120, 140)):
        t = (rng.permutation(256)[:nline] / 128.0)
        line = np.column_stack([0.25 + t, -0.5 + t, 1.0 + t])
        s = rng.uniform(0, 2, (40, 1)); v = rng.uniform(-0.4, 0.4, (40, 1))
        off = np.array([0.25, -0.5, 1.0]) + s * np.array([1.0, 1.0, 1.0]) + v * np.array([0.0, 1.0, 0.0]) + rng.normal(0, 0.002, (40, 1)) * nl
        cloud = np.concatenate([line, off]).astype(F32)[rng.permutation(nline + 40)]
        out.append(RefitCase(f"collinear majority {nline}/{nline + 40}", "collinear majority", tuple(nl), (0.25, -0.5, 1.0), cloud))
    # inlier fractions: two sheets 0.096 m apart inside the gate's slab; a sample from the larger sheet sees the fraction w of it
    for w, n in ((0.9967, 300), (0.9967, 330), (0.965, 300), (0.965, 343), (0.844, 300), (0.844, 415), (0.844, 3000), (0.7, 3008)):
        top = int(round(w * n))
        offs = np.where(np.arange(n) < top, 0.048, -0.048) + rng.normal(0, 0.0003, n)
        cloud = _sheet(rng, n, offsets=offs)[rng.permutation(n)]
        edge = "large cloud" if n >= 3000 else f"k near {round(_k_of(w))}"
        out.append(RefitCase(f"two sheets {top}/{n}", edge, up, (0.0, 0.0, 1.5), cloud, design_k=_k_of(top / n)))
    # k near 50 cannot pass gate 3 (a cloud inside the slab always has a plane that holds all of it): the extractor's plane
    # carries a NaN, whose distance never trips the gate's `>`; 45 % of the cloud on a plane, the rest anywhere in a cube
    for k, (n, frac) in enumerate(((300, 0.45), (320, 0.42))):
        on = int(n * frac)
        cloud = np.concatenate([_sheet(rng, on, noise=0.001), rng.uniform(-0.6, 0.6, (n - on, 3)) + [0, 0, 1.5]]).astype(F32)[rng.permutation(n)]
        out.append(RefitCase(f"plane in clutter {on}/{n}", "k near 50", (float("nan"), 0.0, -1.0), (0.0, 0.0, 1.5), cloud, dist_threshold=0.01,
                             design_k=_k_of(frac)))
    # a NaN coefficient over an ordinary plane
    for k, which in enumerate((0, 2)):
        cloud, cen = tilted(200, 0.003)
        nn = list(tilt); nn[which] = float("nan")
        out.append(RefitCase(f"NaN normal[{which}]", "NaN coefficient", tuple(nn), cen, cloud, accepted=True))
    # fewer than four inliers in the best model: scattered points, 1 mm threshold (again behind a NaN); the covariance fit is
    # skipped and the 50 iterations run out
    for k in range(2):
        cloud = (rng.uniform(-1, 1, (110 + 13 * k, 3)) + [0, 0, 2.0]).astype(F32)
        out.append(RefitCase(f"three inliers {k}", "fewer than four inliers", (0.0, float("nan"), -1.0), (0.0, 0.0, 2.0), cloud, dist_threshold=0.0005))
    # the sign of the fitted d against the extractor's: the same cloud under both signs of the extractor's plane, one of them flips
    cloud, cen = tilted(400, 0.003)
    out.append(RefitCase("extractor d > 0", "flip", tuple(tilt), cen, cloud, accepted=True))
    out.append(RefitCase("extractor d < 0", "flip", tuple(-tilt), cen, cloud, accepted=True))
    # near-isotropic inliers (close eigenvalues in pcl::computeRoots): a ball inside a 0.5 m threshold, and a cubic lattice whose
    # covariance is a multiple of the identity
    for k in range(2):
        v = rng.normal(0, 1, (260, 3)); v *= (0.24 * rng.uniform(0, 1, (260, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
        out.append(RefitCase(f"ball {k}", "near-isotropic", up, (0.0, 0.0, 1.5), (v + [0, 0, 1.5]).astype(F32), dist_threshold=0.5))
    g = np.stack(np.meshgrid(*[np.arange(-2, 3) / 16.0] * 3, indexing="ij"), -1).reshape(-1, 3)
    out.append(RefitCase("cubic lattice", "near-isotropic", up, (0.0, 0.0, 1.5), (g + [0, 0, 1.5]).astype(F32)[rng.permutation(125)], dist_threshold=0.5))
    # ordinary planes of several sizes, so that a call holds many
    for n, noise in ((640, 0.002), (1000, 0.006), (3000, 0.004)):
        cloud, cen = tilted(n, noise, half=1.2)
        out.append(RefitCase(f"plane {n}", "large cloud" if n >= 3000 else "ordinary", tuple(tilt), cen, cloud, dist_threshold=0.05, accepted=True))
    return out


REFIT_EDGES = ("gate 1", "gate 2", "gate 3", "planar", "collinear", "collinear majority", "k near 1", "k near 2", "k near 5", "k near 50",
               "flip", "fewer than four inliers", "near-isotropic", "NaN coefficient", "large cloud", "wavefront tail")


def refit_groups(cases):
    """Cases that share (max_point_dist, dist_threshold) go through one call: -> {(maxd, th): [indices]}."""
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c.max_point_dist, c.dist_threshold), []).append(i)
    return groups
