"""Hand-built maps and frames for the resident plane map (DESIGN.md sections 12 and 13): plane association's gate, work list,
min-reduction, decision and flag sweep (plane_match_kernels.hip) and the upkeep of the clouds (map_plane_kernels.hip), at their
thresholds, ties, chunk seams and stride trips.  Pure numpy: nothing here imports the project.

A scenario is dict(name, maps, steps).  maps is what plane_map_upload takes: dict(coefs [M, 4], bad [M], clouds (M arrays
[n, 3]), points [N, 3]).  steps run in order on the uploaded maps:
  match    frames = dict(map, Tcw, coefs, priors (3 index arrays or None)), params, flag_points, and the answer stated by hand:
           expect[f] = (map_idx, par_idx, ver_idx, nmatches, n_pairs) per frame, flags[s] = the flag bytes of map s;
  update   plane_map_update_batch's arguments (frame_map, Tcw, clouds, map_idx);
  rebuild  plane_map_rebuild_batch's jobs;
  edit     plane_map_edit's arguments.
update and rebuild state by hand `stats` (device_jobs, host_jobs, rounds, repacks since the upload) and `clouds_after`
({(map, plane): cloud}, the clouds the step was built to produce).  Every expected answer is written here from the construction;
no code of the project computes it.  tests/test_plane_map_edges_cpu.py proves on the host that the constructions do what they
say, tests/test_gpu_plane_map_edges.py holds the device to them.

Exactness.  Poses are the identity or PERM (an axis permutation with a translation that cancels the plane's offset), so the
world coefficients are the camera coefficients, or a permutation of them, with no rounding.  Frame planes are (0, 0, 1, d) or
(1, 0, 0, 0): an angle is then one coefficient of the map plane and a distance is |z + d| or |x|, one float operation that
is exact for the values used (powers of two, or z == -d).  Neighbours of a threshold are np.nextafter in float32.

Lattice clouds.  A cloud that goes through the voxel grid has one point per 0.05 m leaf: leaf key k is the leaf
(k % 256, k // 256 % 256, 20 + k // 65536), and its point sits at (leaf + u) * 0.05 with 0 < u < 1.  VoxelGrid orders its output
by leaf index (x fastest, then y, then z), which is the order of the keys (of (z leaf, key) where a case moves points to
another z leaf), a leaf with one point returns that point's bits, and a leaf with two returns (first + second) / 2 in float32.
The index of every point after an update is therefore known here.  The order of the points of an input cloud does not change
the output; it is shuffled with a fixed seed where the ascending order would send libstdc++'s introsort (which the device
reproduces) into its heap-sort branch on a range above 1024 records, which the device hands back to the host."""
import numpy as np

f32 = np.float32
I4 = np.eye(4, dtype=f32)
DEFAULTS = (f32(0.1), f32(0.86), f32(0.08716), f32(0.9962))      # dTh, aTh, verTh, parTh
WIDE = (f32(200.0),) + DEFAULTS[1:]                                # dTh above PointDistanceFromPlane's start value 100
TIGHT = (f32(0.01),) + DEFAULTS[1:]                                # dTh below the 0.05 m leaf, for the lattice clouds
PM_CHUNK = 2048                   # points per work item of k_pm_dist
PM_FLAG_POINTS = 2048             # points per workgroup of k_pm_flags
MP_TRIP = 256 * 256               # elements one trip of k_mp_gather / k_mp_commit / k_mp_move covers (MP_MAX_ROWS * 256)
ORD_HEAP_MAX = 1024               # the device hands a voxel job back when introsort heap-sorts a range above this

# PERM: camera axes (x, y, z) = world (y, z, x), translation (0, 0.5, 0).  transpose(Tcw) * (0, 1, 0, -0.5 + d) = (0, 0, 1, d):
# the products are 0 or the coefficient itself, and 0.5 - 0.5 + d = d.
PERM = np.array([[0, 1, 0, 0], [0, 0, 1, 0.5], [1, 0, 0, 0], [0, 0, 0, 1]], f32)

Z0 = np.array([0, 0, 1, 0], f32)          # the plane z = 0 seen from the identity pose: distance |z|, angle = pW[2]
X0 = np.array([1, 0, 0, 0], f32)          # the plane x = 0: distance |x|, angle = pW[0]


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def toward_zero(v):
    return np.nextafter(f32(v), f32(0))


def zplane(d):
    return np.array([0, 0, 1, d], f32)


def perm_zplane(d):
    """the camera coefficients that PERM turns into (0, 0, 1, d)"""
    return np.array([0, 1, 0, f32(-0.5) + f32(d)], f32)


def flat(z, n=8):
    """n points with the given z (x and y spread, never read by a (0, 0, 1, d) plane)"""
    return np.stack([np.linspace(-1, 1, n), np.linspace(1, -1, n), np.full(n, z)], 1).astype(f32)


def no_points():
    return np.zeros((0, 3), f32)


def mk_map(coefs, clouds, bad=None, points=None):
    coefs = np.asarray(coefs, f32).reshape(-1, 4)
    assert len(coefs) == len(clouds)
    return dict(coefs=coefs, bad=np.zeros(len(coefs), np.uint8) if bad is None else np.asarray(bad, np.uint8),
                clouds=[np.asarray(c, f32).reshape(-1, 3) for c in clouds],
                points=no_points() if points is None else np.asarray(points, f32).reshape(-1, 3))


def mk_frame(m, coefs, priors=None, Tcw=I4):
    return dict(map=m, Tcw=np.asarray(Tcw, f32), coefs=np.asarray(coefs, f32).reshape(-1, 4),
                priors=None if priors is None else tuple(np.asarray(p, np.int32) for p in priors))


def ex(mi, pi, vi, n, npairs=0):
    return (np.asarray(mi, np.int32).reshape(-1), np.asarray(pi, np.int32).reshape(-1), np.asarray(vi, np.int32).reshape(-1),
            int(n), int(npairs))


def match_step(maps, frames, expect, flags=None, params=DEFAULTS, flag_points=True):
    """flags: {map: bytes} for the maps that get a flag; every other map's flags are stated as zeros"""
    fl = {s: np.zeros(len(m["points"]), np.uint8) for s, m in enumerate(maps)}
    for s, v in (flags or {}).items():
        fl[s] = np.asarray(v, np.uint8)
        assert len(fl[s]) == len(maps[s]["points"])
    assert len(frames) == len(expect)
    return dict(kind="match", frames=frames, expect=expect, flags=fl, params=tuple(f32(v) for v in params), flag_points=flag_points)


def stats(device_jobs, host_jobs, rounds, repacks):
    return dict(device_jobs=device_jobs, host_jobs=host_jobs, rounds=rounds, repacks=repacks)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. gate and decision at exact thresholds
# ---------------------------------------------------------------------------------------------------------------------------

def case1_thresholds():
    """Eleven small maps in one upload, one frame each; every distance is |z| of an 8-point cloud, every angle is pW[2].
    gate      angles aTh, up(aTh), -aTh, -up(aTh): only the strict two pass the gate.  The two that do not pass carry the
              nearest clouds (1/64), so a gate of >= would match plane 0; the two that pass are at 1/16 and 1/32: plane 3.
    dist      one plane at exactly dTh: no match (parallel instead).  dist2 adds toward_zero(dTh): that one matches.
    tie2/3    two and three planes at 1/16: the first wins, the next equal one is parallel (|1| > parTh), the third is not
              (1 > 1 is false).  tie3b: 5/64, 1/16, 1/16: plane 1 replaces plane 0, the equal plane 2 is parallel.
    parver    angles parTh, up(parTh), up(parTh), verTh, below(verTh), -below(verTh), -1, 0.01, 0.02 with clouds 50 m away:
              parallel goes 1 -> 6, vertical 4 -> 7; the equal and the exactly-met ones assign nothing.  parver5 is the
              first five planes: parallel 1, vertical 4, so the later assignments of parver are the tightening.
    bad       a bad plane with the nearest cloud between two candidates, seen through PERM: the farther-but-good plane 2.
    nan       a NaN map coefficient (plane 0, nearest cloud) and a NaN frame coefficient (frame plane 1): neither passes a
              gate nor is parallel or vertical; frame plane 1 keeps its priors, whose index 5 is past the map's 2 planes.
              Its world coefficients are NaN, so it flags nothing; frame plane 0 flags the point at 0.25.
    priors    angle 0.8 writes nothing: priors (7, -1), (3, 4), (-1, 5) come back.  Index 7 is past the map's one plane,
              is not read, and as a non-negative mvpMapPlanes entry it flags the three points within 0.5 and counts them."""
    dTh, aTh, verTh, parTh = DEFAULTS
    a_up, p_up, v_dn = up(aTh), up(parTh), toward_zero(verTh)
    far = flat(50.0)
    maps = [
        mk_map([[0, 0, aTh, 0], [0, 0, a_up, 0], [0, 0, -aTh, 0], [0, 0, -a_up, 0]], [flat(1 / 64), flat(1 / 16), flat(1 / 64), flat(1 / 32)]),
        mk_map([Z0], [flat(dTh)]),
        mk_map([Z0, Z0], [flat(dTh), flat(toward_zero(dTh))]),
        mk_map([Z0, Z0], [flat(1 / 16)] * 2),
        mk_map([Z0] * 3, [flat(1 / 16)] * 3),
        mk_map([Z0] * 3, [flat(5 / 64), flat(1 / 16), flat(1 / 16)]),
        mk_map([[0, 0, a, 0] for a in (parTh, p_up, p_up, verTh, v_dn, -v_dn, -1.0, 0.01, 0.02)], [far] * 9),
        mk_map([[0, 0, a, 0] for a in (parTh, p_up, p_up, verTh, v_dn)], [far] * 5),
        mk_map([Z0] * 3, [flat(1 / 16), flat(1 / 64), flat(1 / 32)], bad=[0, 1, 0]),
        mk_map([[np.nan, 0, 1, 0], Z0], [flat(1 / 64), flat(1 / 16)], points=[[0, 0, 0.25], [0, 0, 2]]),
        mk_map([[0.6, 0, 0.8, 0]], [flat(1 / 64)], points=[[0, 0, 0.25], [0, 0, -0.25], [0, 0, 2], [5, 5, toward_zero(0.5)]]),
    ]
    frames = [mk_frame(s, [Z0]) for s in range(8)]
    frames.append(mk_frame(8, [perm_zplane(0)], Tcw=PERM))
    frames.append(mk_frame(9, [Z0, [0, 0, np.nan, 0]], priors=([-1, 5], [-1, -1], [-1, 3])))
    frames.append(mk_frame(10, [Z0, Z0], priors=([7, -1], [3, 4], [-1, 5])))
    expect = [ex([3], [-1], [-1], 1), ex([-1], [0], [-1], 0), ex([1], [0], [-1], 1), ex([0], [1], [-1], 1), ex([0], [1], [-1], 1),
              ex([1], [2], [-1], 1), ex([-1], [6], [7], 0), ex([-1], [1], [4], 0), ex([2], [-1], [-1], 1),
              ex([1, 5], [-1, -1], [-1, 3], 1, 1), ex([7, -1], [3, 4], [-1, 5], 0, 3)]
    return dict(name="thresholds", maps=maps, steps=[match_step(maps, frames, expect, flags={9: [1, 0], 10: [1, 1, 0, 1]})])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. more than 256 map planes
# ---------------------------------------------------------------------------------------------------------------------------

def _filler(M):
    """planes that no frame plane of case 2 gates, calls parallel or calls vertical (every angle 0.5), clouds of 1 to 4 points"""
    return [[0.5, 0, 0.5, 0]] * M, [flat(1 / 64, 1 + j % 4) for j in range(M)]


def case2_many_planes():
    """Maps of 257 and 600 planes (k_pm_gate's `j += 256` loop makes a second and a third trip); three frame planes each:
    Z0 (match), (0, 0, 1, -30) (30 m from every cloud: parallel only) and X0 (vertical only).  Plane 10 is the decoy for all
    three: (0.02, 0, 0.999, 0) with its cloud at 1/16 - an acceptable match, a parallel plane at 0.999 and a vertical one at
    0.02, each slightly worse than the plane that must win.
    M = 257: plane 256 = (0.01, 0, 1, 0), cloud at 1/32: match (1/32 < 1/16), parallel (1 > 0.999) and vertical (0.01 < 0.02).
    M = 600: plane 256 = (0.5, 0, 0.9999, 0), cloud 50 m away: gated but far, so parallel for Z0 as well;
             plane 512 = (0.01, 0.5, 0.5, 0): vertical for X0; plane 599 = (0.5, 0, 0.99, 0), cloud at 1/32: the match.
    A gate loop that made one trip would leave the decoy's index 10 everywhere."""
    decoy, decoy_cloud = [0.02, 0, 0.999, 0], flat(1 / 16, 3)
    c1, cl1 = _filler(257)
    c1[10], cl1[10] = decoy, decoy_cloud
    c1[256], cl1[256] = [0.01, 0, 1, 0], flat(1 / 32, 2)
    c2, cl2 = _filler(600)
    c2[10], cl2[10] = decoy, decoy_cloud
    c2[256], cl2[256] = [0.5, 0, 0.9999, 0], flat(50.0, 4)
    c2[512], cl2[512] = [0.01, 0.5, 0.5, 0], flat(1 / 64, 1)
    c2[599], cl2[599] = [0.5, 0, 0.99, 0], flat(1 / 32, 4)
    maps = [mk_map(c1, cl1), mk_map(c2, cl2)]
    fps = [Z0, zplane(-30), X0]
    frames = [mk_frame(0, fps), mk_frame(1, fps)]
    expect = [ex([256, -1, -1], [-1, 256, -1], [-1, -1, 256], 1), ex([599, -1, -1], [256, 256, -1], [-1, -1, 512], 1)]
    return dict(name="many_planes", maps=maps, steps=[match_step(maps, frames, expect)])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. where the minimum sits
# ---------------------------------------------------------------------------------------------------------------------------

MIN_SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2048 + 65, 4096, 4097)
MIN_SPOTS = (0, 63, 64, 255, 256, 2047, 2048)


def min_configs():
    """(cloud size, index of the near point, near value): every size with the near point at each of MIN_SPOTS it has and at
    n - 1, at 1/32 (within dTh); two controls with the near point at 1/4 (outside dTh)"""
    out = []
    for n in MIN_SIZES:
        for at in sorted({s for s in MIN_SPOTS if s < n} | {n - 1}):
            out.append((n, at, 1 / 32))
    return out + [(2049, 2048, 1 / 4), (4097, 63, 1 / 4)]


def case3_minimum():
    """One map, one frame, one call.  Configuration c (c = 1 .. 66) lives at height 8 c: map plane 2 c - 2 has a cloud of n
    points at 8 c + 1/2 (far) except index `at`, which is at 8 c + near; map plane 2 c - 1 has one point at 8 c + 1/16.
    Frame plane c - 1 is (0, 0, 1, -8 c): its distances are 1/2, near and 1/16 to its own two planes (exact: Sterbenz) and
    at least 7 to every other cloud.  With near = 1/32 the long cloud's plane wins only if the reduction finds that one
    point - in the first or last lane, in the second wavefront, in the first or second trip of a lane, as the first point
    of the second chunk, as a last chunk of one point; otherwise the one-point plane at 1/16 would be taken.  With near =
    1/4 the one-point plane must win.  Every plane is (0, 0, 1, .): the first plane a frame plane does not match is its
    parallel plane (index 0, or 1 for frame plane 0 when it matches plane 0)."""
    cfg = min_configs()
    coefs, clouds, fps, mi, pi = [], [], [], [], []
    for c, (n, at, near) in enumerate(cfg, 1):
        h = 8.0 * c
        cl = np.zeros((n, 3), f32)
        cl[:, 0] = np.arange(n) % 97
        cl[:, 2] = h + 0.5
        cl[at, 2] = h + near
        coefs += [zplane(-h), zplane(-h)]
        clouds += [cl, np.array([[0, 0, h + 1 / 16]], f32)]
        fps.append(zplane(-h))
        mi.append(2 * c - 2 if near < 0.1 else 2 * c - 1)
        pi.append(0 if mi[-1] != 0 else 1)
    maps = [mk_map(coefs, clouds)]
    expect = [ex(mi, pi, [-1] * len(cfg), len(cfg))]
    return dict(name="minimum", maps=maps, steps=[match_step(maps, [mk_frame(0, fps)], expect, flag_points=False)])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. values the key trick rests on
# ---------------------------------------------------------------------------------------------------------------------------

def case4_key_values():
    """Ten maps, one frame each, run under DEFAULTS and then under WIDE (dTh = 200 > 100, where the start value 100 itself is a
    match).  All map planes equal the frame plane's normal (angle 1: gated, and parallel when not matched - the first such
    plane only, since 1 > 1 is false).
    0 zero      X0 against the point (-0.0, -3, 2): 1 * -0.0 = -0.0, + 0 * -3 = -0.0, + 0 * 2 = +0.0, + 0: distance 0.0, key 0.
                The other point is at 1/2: a match only through the 0.0.
    1 hundred   one point at z = 100: the key equals the start value's bits.  No match / a match at 100 under WIDE.
    2 above     plane 0 at 150 and 200, plane 1 at 120: both give 100.  Under WIDE plane 0 matches at 100 and plane 1 (100 <
                100 false) is parallel; an uncapped 150 then 120 would end at plane 1.
    3 inf       one point at z = +inf: distance +inf, capped to 100.
    4 nan       (NaN, 0, 1/64): 0 * NaN is NaN, not below anything; (0, 0, NaN): z != 0 holds, the distance is NaN; the
                third point at 1/16 decides.
    5 zeros     plane 0 holds z == 0.0 and z == -0.0 points (distance 0 if they counted) and one at 1/16; plane 1 is at
                1/32 and must win.
    6 subnormal plane 0 at z = 2 * 2^-149, plane 1 at 2^-149 (keys 2 and 1): plane 1 replaces plane 0.  A comparison that
                flushed subnormals would skip both points as z == 0.
    7 chunk     2048 points with z == +-0.0 (the first work item's lanes all end at the start value and must not write),
                then one point at 1/16 as the second chunk.
    8 empty     no points: 100.   9 skipped   three z == +-0.0 points: 100."""
    sub1, sub2 = np.array([1, 2], np.uint32).view(f32)
    skipped = np.zeros((PM_CHUNK, 3), f32)
    skipped[:, 0] = np.arange(PM_CHUNK) % 31
    skipped[1::2, 2] = -0.0
    maps = [
        mk_map([X0], [[[-0.0, -3, 2], [0.5, 0, 1]]]),
        mk_map([Z0], [[[0, 0, 100]]]),
        mk_map([Z0, Z0], [[[0, 0, 150], [0, 0, 200]], [[0, 0, 120]]]),
        mk_map([Z0], [[[1, 2, np.inf]]]),
        mk_map([Z0], [[[np.nan, 0, 1 / 64], [0, 0, np.nan], [0, 0, 1 / 16]]]),
        mk_map([Z0, Z0], [[[1, 1, 0.0], [2, 2, -0.0], [0, 0, 1 / 16]], [[0, 0, 1 / 32]]]),
        mk_map([Z0, Z0], [[[0, 0, sub2]], [[0, 0, sub1]]]),
        mk_map([Z0], [np.vstack([skipped, [[0, 0, 1 / 16]]])]),
        mk_map([Z0], [no_points()]),
        mk_map([Z0], [[[1, 1, 0.0], [2, 2, -0.0], [3, 3, 0.0]]]),
    ]
    frames = [mk_frame(0, [X0])] + [mk_frame(s, [Z0]) for s in range(1, 10)]
    hit, hit1, miss = ex([0], [-1], [-1], 1), ex([1], [-1], [-1], 1), ex([-1], [0], [-1], 0)
    default = [hit, miss, miss, miss, hit, hit1, hit1, hit, miss, miss]
    wide = [hit, hit, ex([0], [1], [-1], 1), hit, hit, hit1, hit1, hit, hit, hit]
    return dict(name="key_values", maps=maps, steps=[match_step(maps, frames, default, flag_points=False),
                                                     match_step(maps, frames, wide, params=WIDE, flag_points=False)])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. flags
# ---------------------------------------------------------------------------------------------------------------------------

FLAG_SPOTS = (0, 63, 64, 2047, 2048)


def _flag_points(n, exact):
    """n map points 2 m above the plane z = 0 and 5 m from the plane x = 0, except: the spots (FLAG_SPOTS and n - 1) at
    +-below(1/2) (`exact` False: flagged) or +-1/2 (`exact` True: not flagged, and then the point after each spot is at
    below(1/2) instead), index 2 (NaN, 0, 0.1).  Returns (points, flags a matched Z0 sets)."""
    below = toward_zero(0.5)
    p = np.zeros((n, 3), f32)
    p[:, 0], p[:, 1], p[:, 2] = 5, np.arange(n) % 13, 2
    fl = np.zeros(n, np.uint8)
    spots = sorted({s for s in FLAG_SPOTS if s < n} | {n - 1}) if n else []
    for r, s in enumerate(spots):
        sign = -1 if r % 2 else 1
        p[s, 2] = sign * (0.5 if exact else below)
        fl[s] = 0 if exact else 1
    if exact:
        for s in spots:
            if s + 1 < n and s + 1 not in spots:
                p[s + 1, 2] = -below
                fl[s + 1] = 1
    if n > 5:
        p[2] = [np.nan, 0, 0.1]
        fl[2] = 0
    return p, fl


def case5_flags():
    """Ten maps in one upload, each with one plane Z0 whose cloud is at 1/16, so the frame plane Z0 matches it; their map
    points: 2047, 0, 1, 2048, 2049, 4097 (spots flagged) and 2047, 2048, 2049, 4097 (spots exactly at 1/2: not flagged, their
    successors are).  The map without points lies between two with points.
    frames 0-9   one matched Z0 each: the flags of _flag_points, n_pairs their number.
    map 5 twice  frame 10 is a second frame of map 5 whose plane X0 matches nothing (angle 0: vertical) but carries the prior
                 0, so it flags: the points 100 .. 139 and 4000 .. 4096 of map 5 are moved to x = 1/4 (and z = 2, so Z0 does
                 not flag them; none is a spot).  The map's flags are the OR of two disjoint sets.
    map 4 twice  frame 11 has Z0 twice: both match, n_pairs counts every point twice, the flags are set once.
    map 3 again  frame 12's only plane (0, 0, 1, -2) lies on the 2 m points and would flag nearly all of them, but its
                 distance to the cloud is above dTh: unmatched, it flags nothing, and map 3 keeps frame 3's flags only.
    Then the same frames with flag_points off: the same indices, n_pairs 0."""
    sizes = [(2047, False), (0, False), (1, False), (2048, False), (2049, False), (4097, False),
             (2047, True), (2048, True), (2049, True), (4097, True)]
    maps, flags, counts = [], {}, []
    for s, (n, exact) in enumerate(sizes):
        p, fl = _flag_points(n, exact)
        if s == 5:
            p[100:140, 0] = 0.25
            p[4000:4096, 0] = 0.25                 # 4096 = n - 1 is a spot and stays Z0's
        maps.append(mk_map([Z0], [flat(1 / 16)], points=p))
        flags[s] = fl
        counts.append(int(fl.sum()))
    x_set = np.zeros(4097, np.uint8)
    x_set[100:140] = 1
    x_set[4000:4096] = 1
    assert not (x_set & flags[5]).any()
    frames = [mk_frame(s, [Z0]) for s in range(10)]
    frames += [mk_frame(5, [X0], priors=([0], [-1], [-1])), mk_frame(4, [Z0, Z0]), mk_frame(3, [zplane(-2)])]
    hit = [ex([0], [-1], [-1], 1, counts[s]) for s in range(10)]
    extra = [ex([0], [-1], [0], 0, int(x_set.sum())), ex([0, 0], [-1, -1], [-1, -1], 2, 2 * counts[4]), ex([-1], [0], [-1], 0, 0)]
    flags[5] = flags[5] | x_set
    quiet = [e[:4] + (0,) for e in hit + extra]
    return dict(name="flags", maps=maps, steps=[match_step(maps, frames, hit + extra, flags=flags),
                                                match_step(maps, frames, quiet, flag_points=False)])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. degenerate batches
# ---------------------------------------------------------------------------------------------------------------------------

def case6_degenerate():
    """Map 0 has no planes and three points; map 1 has one plane, one cloud point (at 1/16) and one map point (at 1/4).
    call 1   one frame of 65 frame planes against map 1 (k_pm_decide's second block takes the 65th): the even ones are Z0 and
             match, the odd ones are 30 m away and call plane 0 parallel.  33 matches, 33 flagged pairs on the one point.
    call 2   a frame without planes, a frame with one plane seen through PERM, a frame without planes.
    call 3   map 0 (no planes) queried by two frame planes with priors: the priors come back, 0 matches; the prior 1 in
             mvpMapPlanes flags the one point of map 0 within 1/2, the -1 does not.
    call 4   one frame without planes, alone (no frame plane in the call at all)."""
    maps = [mk_map(np.zeros((0, 4), f32), [], points=[[0, 0, 2], [0, 0, 0.25], [0, 0, -2]]),
            mk_map([Z0], [[[0, 0, 1 / 16]]], points=[[3, 3, 0.25]])]
    many = [Z0 if i % 2 == 0 else zplane(-30) for i in range(65)]
    even = np.arange(65) % 2 == 0
    none = np.zeros((0, 4), f32)
    e_none = ex([], [], [], 0, 0)
    steps = [
        match_step(maps, [mk_frame(1, many)], [ex(np.where(even, 0, -1), np.where(even, -1, 0), [-1] * 65, 33, 33)], flags={1: [1]}),
        match_step(maps, [mk_frame(1, none), mk_frame(1, [perm_zplane(0)], Tcw=PERM), mk_frame(0, none)],
                   [e_none, ex([0], [-1], [-1], 1, 1), e_none], flags={1: [1]}),
        match_step(maps, [mk_frame(0, [Z0, Z0], priors=([1, -1], [2, -1], [-1, 0]))], [ex([1, -1], [2, -1], [-1, 0], 0, 1)],
                   flags={0: [0, 1, 0]}),
        match_step(maps, [mk_frame(1, none)], [e_none]),
    ]
    return dict(name="degenerate", maps=maps, steps=steps)


# ---------------------------------------------------------------------------------------------------------------------------
# lattice clouds
# ---------------------------------------------------------------------------------------------------------------------------

def lattice(keys, u=0.5, z=None):
    """One point in each leaf named by its key, at (leaf + u) * 0.05; z (a scalar or one value per point) replaces the
    z coordinate, and with it the z leaf."""
    k = np.asarray(keys, np.int64).reshape(-1)
    leaf = np.stack([k % 256, k // 256 % 256, 20 + k // 65536], 1).astype(np.float64)
    p = ((leaf + u) * 0.05).astype(f32)
    if z is not None:
        p[:, 2] = z
    return p


def shuffled(cloud, seed):
    return np.ascontiguousarray(cloud[np.random.default_rng(seed).permutation(len(cloud))])


# ---------------------------------------------------------------------------------------------------------------------------
# 7. match after the clouds changed, without another upload
# ---------------------------------------------------------------------------------------------------------------------------

Z_OLD, Z_MISS, Z_HIT = f32(1.025), f32(1.51), f32(1.54)       # z leaves 20, 30, 30


def case7_changed_clouds():
    """Five maps, one frame each, every frame plane (0, 0, 1, -1.54) under TIGHT (dTh = 0.01): a point at z = 1.54 is at
    distance 0.0, one at 1.51 at 0.03 and the old points at 1.025 at 0.515.  Points at 1.51 and 1.54 share z leaf 30 and so
    sort after every old point (z leaf 20), among themselves by x leaf.
    map 0 (a)  2040 old points (keys 0 .. 2039).  The update adds 20 leaves: keys 0 .. 7 at 1.51, keys 8 .. 19 at 1.54.  They
               become indices 2040 .. 2059: the 1.54 points are exactly the indices 2048 .. 2059, the second chunk of 12
               points.  No match before, a match after - but only if the work list now holds a second item for this plane.
    map 1 (b)  4099 old points and index 4099 at 1.54 (the fourth point of the third chunk): matched before.  The rebuild
               from one observation of 10 old-height points (identity Twc) leaves those 10: no match after.
    map 2 (c)  2000 old points; one frame names plane 0 with both of its frame planes: the first adds keys 0 .. 29 at 1.51
               (2030 points), the second keys 30 .. 47 at 1.51 and 48 .. 59 at 1.54 (2060 points; the 1.54 points are
               indices 2048 .. 2059) and a second point (u = 1/4) in every old leaf, whose centroid becomes the mean of the
               two, frame point first.  Two rounds; matched after.  (The old leaves are seen again because 30 points in
               front of 2030 sorted ones send introsort into its heap sort on 1400 records, which the device hands back;
               the uploaded clouds of maps 0 and 2 are shuffled for the same reason.)
    map 3 (e)  one plane at 1.545 (distance 0.005): matched before.  plane_map_edit appends plane 1, a rebuild fills it with
               10 points at 1.54: after, plane 1 (0.0 < 0.005) replaces plane 0 as the match.
    map 4 (d)  plane 0 at 1.54, plane 1 at 1.545: plane 0 before (plane 1 parallel).  plane_map_edit sets plane 0 bad: plane 1
               after.
    Stats since the upload: the update is 3 jobs in 2 rounds with one repack (uploaded slots have no room: round 1 grows
    maps 0 and 2 together; the new slots hold twice the cloud and 256 more, so round 2 fits); the rebuild of map 1 shrinks
    (no repack); the appended plane has a slot of 0 points, so its rebuild repacks.  No job returns to the host.
    Calls of one frame.  A call's work list holds as many items as the host's mirror of the cloud sizes gives the call's maps
    together, and an edit rewrites the whole mirror.  So the frames of maps 0 and 2 are matched alone right after the update,
    before anything else touches the mirror, and the frame of map 3 alone right after its rebuild: with a mirror from before
    the change their lists would be one item short, and a call over all five maps would hide that behind map 1, whose cloud
    shrank."""
    fp = zplane(-Z_HIT)
    old = lambda n: lattice(np.arange(n), z=Z_OLD)                                     # noqa: E731
    new = lambda lo, hi, z: lattice(np.arange(lo, hi), u=0.25, z=z)                     # noqa: E731
    a_add = np.vstack([new(0, 8, Z_MISS), new(8, 20, Z_HIT)])
    b0 = np.vstack([old(4099), lattice([5000], z=Z_HIT)])
    b_obs = old(10)
    c_add1, c_add2 = new(0, 30, Z_MISS), np.vstack([new(30, 48, Z_MISS), new(48, 60, Z_HIT)])
    c_again = lattice(np.arange(2000), u=0.25, z=Z_OLD)          # the second frame plane also sees every old leaf again
    e_new = lattice(np.arange(10), z=Z_HIT)
    near, nearer = lattice(np.arange(8), z=f32(1.545)), lattice(np.arange(8), z=Z_HIT)
    maps = [mk_map([Z0], [shuffled(old(2040), 6)]), mk_map([Z0], [b0]), mk_map([Z0], [shuffled(old(2000), 7)]), mk_map([Z0], [near]),
            mk_map([Z0, Z0], [nearer, near])]
    frames = [mk_frame(s, [fp]) for s in range(5)]
    miss, hit = ex([-1], [0], [-1], 0), ex([0], [-1], [-1], 1)
    before = [miss, hit, miss, hit, ex([0], [1], [-1], 1)]
    after = [hit, miss, hit, ex([1], [-1], [-1], 1), ex([1], [-1], [-1], 1)]
    steps = [
        match_step(maps, frames, before, params=TIGHT, flag_points=False),
        dict(kind="update", frame_map=[0, 2], Tcw=np.stack([I4, I4]), clouds=[[shuffled(a_add, 1)], [shuffled(c_add1, 2), shuffled(np.vstack([c_add2, c_again]), 3)]],
             map_idx=[[0], [0, 0]], stats=stats(3, 0, 2, 1),
             clouds_after={(0, 0): np.vstack([old(2040), a_add]), (2, 0): np.vstack([(c_again + old(2000)) / f32(2), c_add1, c_add2])}),
        match_step(maps, frames[0:1], after[0:1], params=TIGHT, flag_points=False),
        match_step(maps, frames[2:3], after[2:3], params=TIGHT, flag_points=False),
        dict(kind="rebuild", jobs=[(1, 0, [(I4, shuffled(b_obs, 4))])], stats=stats(4, 0, 3, 1), clouds_after={(1, 0): b_obs}),
        dict(kind="edit", map=4, index=[0], coefs=None, bad=[1]),
        dict(kind="edit", map=3, index=[1], coefs=[Z0], bad=None),
        dict(kind="rebuild", jobs=[(3, 1, [(I4, shuffled(e_new, 5))])], stats=stats(5, 0, 4, 2), clouds_after={(3, 1): e_new}),
        match_step(maps, frames[3:4], after[3:4], params=TIGHT, flag_points=False),
        match_step(maps, frames, after, params=TIGHT, flag_points=False),
    ]
    return dict(name="changed_clouds", maps=maps, steps=steps)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. long segments through upkeep
# ---------------------------------------------------------------------------------------------------------------------------

N_RESIDENT, N_FRAME, N_SHARED = 30000, 70000, 5000
N_AFTER = N_RESIDENT + N_FRAME - N_SHARED                      # 95 000 leaves
# repack() in map_plane.cpp: a plane whose round input `need` exceeds max(slot, 2 * cloud + 256) gets need + need / 2 + 256
SLOT = (N_RESIDENT + N_FRAME) + (N_RESIDENT + N_FRAME) // 2 + 256
N_FILL = SLOT - N_AFTER                                         # the frame cloud that fills the slot exactly: 55 256 points


def case8_long_segments():
    """One map, one plane, three updates through the identity pose, a match after the second and after the third.
    update 1  resident keys 0 .. 29 999 (u = 1/2), frame keys 25 000 .. 94 999 (u = 1/4): a 70 000-point segment (k_mp_gather's
              second trip starts at point 65 536), a 100 000-point input above the uploaded slot of 30 000, so the arena is
              repacked first (k_mp_move: 90 000 floats, a second trip) into a slot of 150 256, and 95 000 centroids are
              committed (285 000 floats: k_mp_commit's fifth trip).  Result: index == key; keys below 25 000 the resident
              point, keys from 30 000 the frame point, the 5 000 shared leaves (frame point + resident point) / 2.
    update 2  frame keys 0 .. 55 255 (u = 3/4): with the 95 000 resident points exactly the slot, so no repack; every frame point
              falls into an occupied leaf: 95 000 points again, the first 55 256 of them (frame point + current point) / 2.
    match     the frame plane through z leaf 21's points (keys from 65 536 on, all at (21 + 1/4) * 0.05): distance 0.0 to them,
              at least 0.025 to z leaf 20's.  Every near point has an index of 65 536 or more, the 33rd chunk onwards: a work
              list sized from the 30 000 points of the upload, or by the repack before update 1, ends before them.
    update 3  frame keys 0 .. 55 255 (u = 3/4) and the new key 131 072 (u = 1/8): one point more than the slot, so one more repack;
              95 001 points.
    match     the new leaf of update 3 is key 131 072 = (0, 0, z leaf 22): it sorts after every other point, index 95 000, and is
              the only point above z leaf 21.  The frame plane through its z is at distance 0.0 from it and more than 0.04
              from every other point, so under TIGHT it matches only through that last point of the last chunk: the end of
              the cloud the commit wrote and the work list sized from the count after update 3.
    No job returns to the host: the frame clouds are shuffled (the ascending order would reach the heap-sort branch)."""
    k_res, k_fr = np.arange(N_RESIDENT), np.arange(N_RESIDENT - N_SHARED, N_AFTER)
    resident, frame1 = lattice(k_res, 0.5), lattice(k_fr, 0.25)
    after1 = np.vstack([resident[:N_RESIDENT - N_SHARED], (frame1[:N_SHARED] + resident[N_RESIDENT - N_SHARED:]) / f32(2), frame1[N_SHARED:]])
    frame2 = lattice(np.arange(N_FILL), 0.75)
    after2 = after1.copy()
    after2[:N_FILL] = (frame2 + after1[:N_FILL]) / f32(2)
    frame3 = np.vstack([lattice(np.arange(N_FILL), 0.75), lattice([2 * 65536], 0.125)])
    after3 = np.vstack([after2, frame3[-1:]])
    after3[:N_FILL] = (frame3[:N_FILL] + after2[:N_FILL]) / f32(2)
    assert after1.dtype == f32 and after3.dtype == f32 and len(after3) == N_AFTER + 1
    assert N_FRAME > MP_TRIP and 3 * N_RESIDENT > MP_TRIP and SLOT == 150256 and N_FILL == 55256
    maps = [mk_map([Z0], [resident])]
    fp = zplane(-after3[-1, 2])
    upd = lambda cloud, seed, st, want: dict(kind="update", frame_map=[0], Tcw=I4[None], clouds=[[shuffled(cloud, seed)]],   # noqa: E731
                                             map_idx=[[0]], stats=st, clouds_after={(0, 0): want})
    steps = [
        upd(frame1, 11, stats(1, 0, 1, 1), after1),
        upd(frame2, 12, stats(2, 0, 2, 1), after2),
        match_step(maps, [mk_frame(0, [zplane(-after2[65536, 2])])], [ex([0], [-1], [-1], 1)], params=TIGHT, flag_points=False),
        upd(frame3, 13, stats(3, 0, 3, 2), after3),
        match_step(maps, [mk_frame(0, [fp])], [ex([0], [-1], [-1], 1)], params=TIGHT, flag_points=False),
    ]
    return dict(name="long_segments", maps=maps, steps=steps)


BUILDERS = (case8_long_segments, case3_minimum, case5_flags, case2_many_planes, case7_changed_clouds, case4_key_values,
            case1_thresholds, case6_degenerate)          # the larger uploads and calls first


def all_scenarios():
    return [b() for b in BUILDERS]


# ---------------------------------------------------------------------------------------------------------------------------
# replay on host-held maps
# ---------------------------------------------------------------------------------------------------------------------------

class HostMaps:
    """The maps held on the host and the steps replayed on them by an implementation `impl` with match(Tcw, coefs, map_coefs,
    bad, clouds, priors (3 or None), params) -> (mi, pi, vi, n), flag(Tcw, coefs, mi, points, flags) -> (flags, n_pairs),
    update(Tcw, frame_cloud, map_cloud) -> cloud and rebuild(Twcs, clouds) -> cloud: the per-frame loop of the reference
    (match, flag every frame of a map into the map's flags, update in (frame, frame plane) order)."""

    def __init__(self, maps, impl):
        self.impl = impl
        self.coefs = [m["coefs"].copy() for m in maps]
        self.bad = [m["bad"].copy() for m in maps]
        self.clouds = [[c.copy() for c in m["clouds"]] for m in maps]
        self.points = [m["points"] for m in maps]

    def match(self, step):
        """-> ([(mi, pi, vi, n, n_pairs) per frame], [flags per map])"""
        flags = [np.zeros(len(p), np.uint8) for p in self.points]
        out = []
        for fr in step["frames"]:
            s = fr["map"]
            mi, pi, vi, n = self.impl.match(fr["Tcw"], fr["coefs"], self.coefs[s], self.bad[s], self.clouds[s], fr["priors"], step["params"])
            npairs = 0
            if step["flag_points"]:
                flags[s], npairs = self.impl.flag(fr["Tcw"], fr["coefs"], mi, self.points[s], flags[s])
            out.append((mi, pi, vi, n, npairs))
        return out, flags

    def apply(self, step):
        if step["kind"] == "update":
            for f, s in enumerate(step["frame_map"]):
                for q, j in enumerate(step["map_idx"][f]):
                    if j >= 0:
                        self.clouds[s][j] = self.impl.update(step["Tcw"][f], step["clouds"][f][q], self.clouds[s][j])
        elif step["kind"] == "rebuild":
            for s, j, obs in step["jobs"]:
                self.clouds[s][j] = self.impl.rebuild([o[0] for o in obs], [o[1] for o in obs])
        elif step["kind"] == "edit":
            s = step["map"]
            for k, i in enumerate(step["index"]):
                if i == len(self.coefs[s]):
                    self.coefs[s] = np.vstack([self.coefs[s], np.asarray(step["coefs"][k], f32).reshape(1, 4)])
                    self.bad[s] = np.r_[self.bad[s], step["bad"][k] if step["bad"] is not None else 0].astype(np.uint8)
                    self.clouds[s].append(no_points())
                    continue
                if step["coefs"] is not None:
                    self.coefs[s][i] = step["coefs"][k]
                if step["bad"] is not None:
                    self.bad[s][i] = step["bad"][k]
        else:
            raise ValueError(step["kind"])

    def replay(self, steps):
        """-> per step: match -> (results, flags); update / rebuild -> {(map, plane): cloud} of the planes the step names;
        edit -> None"""
        out = []
        for st in steps:
            if st["kind"] == "match":
                out.append(self.match(st))
                continue
            self.apply(st)
            out.append({k: self.clouds[k[0]][k[1]].copy() for k in st.get("clouds_after", {})} or None)
        return out
