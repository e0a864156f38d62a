"""Hand-built frames that put the windowed ORB matchers on their decision points: equal-distance ties in and across grid
cells, distances on TH_HIGH, window and grid edges in float, the level rules, the rotation histogram's rounding and
ComputeThreeMaxima ties, long claim chains and the capacity limit.

Every scenario carries the expected outcome stated by hand from the reference source, with the line it exercises.
tests/test_match_edges_cpu.py holds the oracle to these outcomes; tests/test_gpu_match_edges.py holds the device to both.

Geometry: a 640 x 480 frame with fx = fy = 256, cx = 320, cy = 240, so that a last-frame keypoint at depth z = 1 under
identity poses projects back onto its own pixel coordinates exactly (x = (u - cx) / 256 and u = 256 x + cx are exact in
float for the coordinates used here).  Grid cells are 10 x 10 px (FRAME_GRID_COLS = 64, FRAME_GRID_ROWS = 48).  A window
at octave 0 has radius r = th exactly (mvScaleFactors[0] = 1).
"""
from dataclasses import dataclass, field

import numpy as np

W, H = 640, 480
FX = FY = 256.0
CX, CY = 320.0, 240.0
BF = 25.6                 # mb = bf / fx = 0.1 m: the motion-flag threshold (src/ORBmatcher.cc:1412-1413)
TH_HIGH, TH_LOW = 100, 50  # src/ORBmatcher.cc:38-39
F32 = np.float32

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])


def ulp_below(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def ulp_above(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def scale_factors(nlevels=8, scale=1.2):
    """ORBextractor's mvScaleFactor: the cumulative float product (src/ORBextractor.cc)."""
    s = np.ones(nlevels, np.float32)
    for k in range(1, nlevels):
        s[k] = F32(s[k - 1] * F32(scale))
    return s


def kps_array(rows):
    """rows: (x, y[, octave[, angle]])"""
    k = np.zeros(len(rows), KP_DTYPE)
    for i, r in enumerate(rows):
        k[i]["x"], k[i]["y"] = r[0], r[1]
        k[i]["octave"] = r[2] if len(r) > 2 else 0
        k[i]["angle"] = r[3] if len(r) > 3 else 0.0
        k[i]["size"], k[i]["response"], k[i]["class_id"] = 31.0, 1.0, -1
    return k


class Desc:
    """Descriptors at stated Hamming distances: every query gets its own random base; a candidate at distance d from a
    query is the base with d bits flipped, starting at bit `at` (two candidates with disjoint flip ranges are d1 + d2
    apart from each other, and unrelated bases are ~128 apart, far above TH_HIGH)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def base(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    @staticmethod
    def flip(d, n, at=0):
        assert 0 <= n and at + n <= 256
        bits = np.unpackbits(d.copy())
        bits[at:at + n] ^= 1
        return np.packbits(bits)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def translation(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (tx, ty, tz)
    return T


@dataclass
class LastScenario:
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1400-1531) on hand-built frames.
    Map points are the last frame's keypoints with depth, unprojected with Twc_last (Frame::UnprojectStereo), as the
    batch path builds them; host_only scenarios override map points / claims the batch path cannot carry."""
    name: str
    ref: str
    last_kps: np.ndarray
    last_desc: np.ndarray
    last_z: np.ndarray          # per last keypoint, 0 = no depth (no map point)
    cur_kps: np.ndarray
    cur_desc: np.ndarray
    expect: dict                # check_ori -> (nmatches, {cur index: last index}); every other entry -1 (or its pre-claim)
    th: float = 15.0
    Tcw_cur: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    Twc_last: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    cur_kps_un: np.ndarray = None
    mp_valid: np.ndarray = None
    mp_obs: np.ndarray = None
    pre: np.ndarray = None
    cur_obs: np.ndarray = None

    @property
    def host_only(self):
        return self.mp_valid is not None or self.mp_obs is not None or self.pre is not None or self.cur_obs is not None

    @property
    def Tcw_last(self):
        return np.linalg.inv(self.Twc_last.astype(np.float64)).astype(np.float32)

    def expected(self, check_ori):
        n, pairs = self.expect[check_ori]
        m = np.full(len(self.cur_kps), -1, np.int32) if self.pre is None else self.pre.astype(np.int32).copy()
        for c, l in pairs.items():
            m[c] = l
        return n, m


def depth_image(kps, z):
    """A depth image that hands every keypoint its z at the pixel ComputeStereoFromRGBD reads ((int)y, (int)x,
    src/Frame.cc:893-911)."""
    img = np.zeros((H, W), np.float32)
    for k, d in zip(kps, z):
        u, v = int(k["x"]), int(k["y"])
        if 0 <= u < W and 0 <= v < H:
            assert img[v, u] in (0.0, d), "two keypoints of one pixel with different depths"
            img[v, u] = d
    return img


def _one(pos, cur_pos, dist, d, last_oct=0, cur_oct=0, last_angle=0.0, cur_angle=0.0):
    b = d.base()
    return (pos[0], pos[1], last_oct, last_angle), b, (cur_pos[0], cur_pos[1], cur_oct, cur_angle), Desc.flip(b, dist)


def _lattice(name, ref, specs, expect, seed, th=4.0):
    """One query per lattice point, 40 px apart (windows of radius th never overlap), each with one candidate 1 px off
    its projection.  specs: (dist, last_angle, cur_angle)."""
    d = Desc(seed)
    L, LD, C, CD = [], [], [], []
    for i, (dist, la, ca) in enumerate(specs):
        x, y = 20.0 + 40.0 * (i % 15), 20.0 + 40.0 * (i // 15)
        l, ld, c, cd = _one((x, y), (x + 1.0, y + 1.0), dist, d, last_angle=la, cur_angle=ca)
        L.append(l); LD.append(ld); C.append(c); CD.append(cd)
    return LastScenario(name, ref, kps_array(L), np.array(LD), np.ones(len(L), np.float32), kps_array(C), np.array(CD),
                        expect, th=th)


def _all(n):
    return {i: i for i in range(n)}


# ---------------------------------------------------------------------------------------------------------------------
# SearchByProjection(Cur, Last)

def tie_cross_cell():
    """Equal distances: the reference keeps the FIRST candidate in GetFeaturesInArea order (cells ix-outer, iy-inner,
    insertion order in a cell; strict `dist<bestDist`, src/ORBmatcher.cc:1483-1487, src/Frame.cc:752-775).
    Query 0: cur 0 sits in cell (11, 9), cur 1 in cell (9, 11): column 9 is visited first, so the HIGHER index wins.
    Query 1: cur 2 and cur 3 share a cell: insertion order, cur 2.  Query 2: best and second tie one column apart, and a
    third candidate in the first column's cell row below holds the tie too: cur 6 (column 29, row 21) precedes cur 4
    (column 30) and cur 5 (column 31)."""
    d = Desc(11)
    b0, b1, b2 = d.base(), d.base(), d.base()
    last = kps_array([(100.0, 100.0), (300.0, 200.0), (300.0, 300.0)])
    cur = kps_array([(106.0, 94.0), (94.0, 106.0), (300.5, 200.5), (301.0, 201.0), (302.0, 300.0), (308.0, 300.0),
                     (292.0, 306.0)])
    cd = np.array([Desc.flip(b0, 20, 0), Desc.flip(b0, 20, 40), Desc.flip(b1, 30, 0), Desc.flip(b1, 30, 100),
                   Desc.flip(b2, 12, 0), Desc.flip(b2, 12, 20), Desc.flip(b2, 12, 40)])
    exp = {1: 0, 2: 1, 6: 2}
    return LastScenario("tie_cross_cell", "src/ORBmatcher.cc:1483-1487, src/Frame.cc:752-775", last, np.array([b0, b1, b2]),
                        np.ones(3, np.float32), cur, cd, {False: (3, exp), True: (3, exp)})


def tie_wide_window():
    """The same rule on the whole-wavefront path of the window gather: one cell holds 70 records (more than the 64 visit
    positions of the quarter-wave routine) at distances above TH_HIGH, and the tie sits in the columns on either side:
    cur 71 (column 39, visited first) ties with cur 70 (column 41) and with cur 0 / cur 1 inside the dense cell.
    A second query over the same window is near only cur 5 and cur 66, tied at 15 in the dense cell: insertion order,
    cur 5 (visit position 6) before cur 66 (visit position 67, the same lane one trip later)."""
    d = Desc(12)
    b0, b1 = d.base(), d.base()
    rows = [(400.0 + 0.05 * (i % 60), 300.0 + 0.05 * (i // 60) + 0.1 * (i % 7)) for i in range(70)]
    rows += [(412.0, 300.0), (388.0, 301.0)]
    cur = kps_array(rows)
    far = Desc.flip(b0, 128, 0)
    cd = np.array([far] * 72)
    cd[0] = cd[1] = Desc.flip(b0, 15, 60)
    cd[70] = Desc.flip(b0, 15, 0)
    cd[71] = Desc.flip(b0, 15, 20)
    # the second query is the same dense cell seen through another descriptor: far from everything except cur 5 / cur 66
    cd[5] = Desc.flip(b1, 15, 0)
    cd[66] = Desc.flip(b1, 15, 30)
    last = kps_array([(400.0, 300.0), (401.0, 302.0)])
    exp = {71: 0, 5: 1}
    s = LastScenario("tie_wide_window", "src/ORBmatcher.cc:1483-1487, src/Frame.cc:752-775", last, np.array([b0, b1]),
                     np.ones(2, np.float32), cur, cd, {False: (2, exp), True: (2, exp)}, th=15.0)
    return s


def dist_thresholds():
    """bestDist<=TH_HIGH accepts 99 and 100 and rejects 101 (src/ORBmatcher.cc:1496); one candidate per window."""
    specs = [(99, 0.0, 0.0), (100, 0.0, 0.0), (101, 0.0, 0.0), (0, 0.0, 0.0), (256, 0.0, 0.0)]
    exp = {0: 0, 1: 1, 3: 3}
    return _lattice("dist_thresholds", "src/ORBmatcher.cc:1496", specs, {False: (3, exp), True: (3, exp)}, 21)


def window_edges():
    """GetFeaturesInArea's strict `fabs(distx)<r && fabs(disty)<r` (src/Frame.cc:771): with r = 15 a candidate at
    |dx| == 15 or |dy| == 15 is out, one ulp inside is in, one ulp outside is out.  One candidate per window; the query
    sits at (bx, by) exactly, so dx = x - bx is exact."""
    d = Desc(31)
    cases = [(lambda b: b + 15.0, lambda b: b, False), (lambda b: b - 15.0, lambda b: b, False),
             (lambda b: b, lambda b: b + 15.0, False), (lambda b: b, lambda b: b - 15.0, False),
             (lambda b: ulp_below(b + 15.0), lambda b: b, True), (lambda b: b, lambda b: ulp_above(b - 15.0), True),
             (lambda b: ulp_above(b - 15.0), lambda b: ulp_below(b + 15.0), True), (lambda b: ulp_above(b + 15.0), lambda b: b, False),
             (lambda b: b + 14.0, lambda b: b - 14.0, True)]
    L, LD, C, CD, exp = [], [], [], [], {}
    for i, (fx, fy, ok) in enumerate(cases):
        bx, by = 100.0 + 100.0 * (i % 5), 100.0 + 100.0 * (i // 5)
        l, ld, c, cd = _one((bx, by), (fx(bx), fy(by)), 10, d)
        L.append(l); LD.append(ld); C.append(c); CD.append(cd)
        if ok:
            exp[i] = i
    n = len(exp)
    return LastScenario("window_edges", "src/Frame.cc:771", kps_array(L), np.array(LD), np.ones(len(L), np.float32),
                        kps_array(C), np.array(CD), {False: (n, exp), True: (n, exp)}, th=15.0)


def grid_rounding():
    """PosInGrid's round((x-mnMinX)*mfGridElementWidthInv) in float (src/Frame.cc:817-818): 45 * (64/640.f) is exactly
    4.5 in float and rounds AWAY from zero to cell 5; one ulp below 45 is cell 4.  Query 0 ties cur 0 (x = 45, cell 5)
    with cur 1 (x = 45 - ulp, cell 4): cell 4 is visited first, so cur 1 wins.  Query 1 is the same on y (45 -> row 5)."""
    inv = F32(64) / F32(640)
    assert F32(F32(45.0) * inv) == F32(4.5) and F32(F32(ulp_below(45.0)) * inv) < F32(4.5)
    d = Desc(41)
    b0, b1 = d.base(), d.base()
    last = kps_array([(45.0, 100.0), (200.0, 45.0)])
    cur = kps_array([(45.0, 100.0), (ulp_below(45.0), 100.0), (200.0, 45.0), (200.0, ulp_below(45.0))])
    cd = np.array([Desc.flip(b0, 9, 0), Desc.flip(b0, 9, 50), Desc.flip(b1, 9, 0), Desc.flip(b1, 9, 50)])
    exp = {1: 0, 3: 1}
    return LastScenario("grid_rounding", "src/Frame.cc:817-818", last, np.array([b0, b1]), np.ones(2, np.float32), cur, cd,
                        {False: (2, exp), True: (2, exp)})


def undistorted_cell():
    """The matchers read mvKeysUn (src/Frame.cc:762, src/ORBmatcher.cc:1476): cur 1's raw x (52) is in cell 5 but its
    undistorted x (38) is in cell 4, ahead of cur 0 (cell 5) in the scan; the tie goes to cur 1."""
    d = Desc(42)
    b0 = d.base()
    last = kps_array([(45.0, 100.0)])
    cur = kps_array([(48.0, 100.0), (52.0, 100.0)])
    cur_un = kps_array([(48.0, 100.0), (38.0, 100.0)])
    cd = np.array([Desc.flip(b0, 9, 0), Desc.flip(b0, 9, 50)])
    exp = {1: 0}
    return LastScenario("undistorted_cell", "src/Frame.cc:762, src/ORBmatcher.cc:1476", last, np.array([b0]),
                        np.ones(1, np.float32), cur, cd, {False: (1, exp), True: (1, exp)}, cur_kps_un=cur_un)


def image_borders(side):
    """Projections outside [mnMinX, mnMaxX] x [mnMinY, mnMaxY] are skipped (strict `u<mnMinX || u>mnMaxX`,
    src/ORBmatcher.cc:1436-1439); on the border itself the window is clamped to the grid (src/Frame.cc:735-749).
    A translation of 2^-16 (low) or 2^-15 (high) moves every projection by 1/256 or 1/128 px exactly."""
    d = Desc(43 if side == "low" else 44)
    if side == "low":
        T = translation(-2.0 ** -16, -2.0 ** -16)          # u = x - 1/256
        e = 1.0 / 256
        # last: on the border after the shift (in), just outside (out), a corner (in)
        lp = [(e, 100.0 + e), (0.0, 200.0 + e), (100.0 + e, e), (200.0 + e, 0.0), (e, e)]
        cp = [(0.25, 100.0), (0.25, 200.0), (100.0, 0.25), (200.0, 0.25), (3.0, 3.0)]
        ok = [True, False, True, False, True]
    else:
        T = translation(2.0 ** -15, 2.0 ** -15)            # u = x + 1/128
        e = 1.0 / 128
        # PosInGrid puts x >= 635 / y >= 475 in column 64 / row 48, off the grid (src/Frame.cc:817-821): cur 5 and cur 6
        # are inside the window but in no cell, so nothing finds them
        lp = [(640.0 - e, 100.0 - e), (640.0 - 1.0 / 256, 200.0 - e), (100.0 - e, 480.0 - e), (200.0 - e, 480.0 - 1.0 / 256),
              (640.0 - e, 480.0 - e), (640.0 - e, 300.0 - e), (300.0 - e, 480.0 - e)]
        cp = [(634.0, 100.0), (634.0, 200.0), (100.0, 474.0), (200.0, 474.0), (633.0, 473.0), (635.0, 300.0), (300.0, 475.0)]
        ok = [True, False, True, False, True, False, False]
    L, LD, C, CD, exp = [], [], [], [], {}
    for i, (l, c, o) in enumerate(zip(lp, cp, ok)):
        a, ad, b, bd = _one(l, c, 10, d)
        L.append(a); LD.append(ad); C.append(b); CD.append(bd)
        if o:
            exp[i] = i
    n = len(exp)
    return LastScenario(f"image_border_{side}", "src/ORBmatcher.cc:1436-1439, src/Frame.cc:735-749, :817-821", kps_array(L), np.array(LD),
                        np.ones(len(L), np.float32), kps_array(C), np.array(CD), {False: (n, exp), True: (n, exp)},
                        th=15.0, Tcw_cur=T)


def level_rules(motion):
    """The window's level range (src/ORBmatcher.cc:1448-1453) with GetFeaturesInArea's quirk bCheckLevels =
    (minLevel>0) || (maxLevel>=0) (src/Frame.cc:750): forward motion at octave 0 gives (0, -1), no level check at all.
    Query 0 is at octave 0, query 1 at octave 7; each window holds candidates at octaves 0, 1, 2, 6, 7 with distances
    30, 28, 25, 40, 45.  motion: 'none' (identity), 'forward' (tlc.z = 0.5 > mb), 'backward' (tlc.z = -0.5)."""
    z = {"none": 1.0, "forward": 1.5, "backward": 0.5}[motion]
    T = translation(tz={"none": 0.0, "forward": -0.5, "backward": 0.5}[motion])
    d = Desc(50)
    b0, b1 = d.base(), d.base()
    # u - 320 = z * (x - 320) after the move: last x chosen so that the projections are (170, 240) and (440, 240)
    proj = [(170.0, 240.0), (440.0, 240.0)]
    last = kps_array([(320.0 + (u - 320.0) / z, 240.0, oct_) for (u, _), oct_ in zip(proj, (0, 7))])
    octs, dists = (0, 1, 2, 6, 7), (30, 28, 25, 40, 45)
    rows, cd = [], []
    for q, (u, v) in enumerate(proj):
        for j, (o, dist) in enumerate(zip(octs, dists)):
            rows.append((u - 4.0 + 2.0 * j, v + 1.0, o))
            cd.append(Desc.flip((b0, b1)[q], dist, 0))
    best = {  # (query 0 at octave 0, query 1 at octave 7) -> winning octave
        "none": (1, 6),          # [-1, 1] and [6, 8]
        "forward": (2, 7),       # (0, -1): no check; [7, inf)
        "backward": (0, 2),      # [0, 0]; [0, 7]
    }[motion]
    exp = {octs.index(best[0]): 0, 5 + octs.index(best[1]): 1}
    return LastScenario(f"levels_{motion}", "src/ORBmatcher.cc:1448-1453, src/Frame.cc:750-758", last, np.array([b0, b1]),
                        np.full(2, z, np.float32), kps_array(rows), np.array(cd), {False: (2, exp), True: (2, exp)},
                        th=15.0, Tcw_cur=T)


def _half_rot(k):
    """A float rot with rot * (1.0f/30) exactly k + 0.5 in float (round() and rint() differ there for even k)."""
    f = F32(1.0) / F32(30.0)
    r = F32(30.0 * (k + 0.5))
    for _ in range(3000):
        r = np.nextafter(r, F32(-np.inf))
    for _ in range(6000):
        if F32(r * f) == F32(k + 0.5):
            return float(r)
        r = np.nextafter(r, F32(np.inf))
    raise AssertionError("no half-integer rot")


def rotation_wrap():
    """rot<0 -> rot+=360 (src/ORBmatcher.cc:1503-1504): 11 matches at rot 0 (bin 0), one at rot = -2^-10 (-> 359.999,
    bin round(12.0) = 12 with the reference's factor 1/HISTO_LENGTH); ComputeThreeMaxima keeps bin 12 only if
    1 >= 0.1f*11: it does not, so the wrapped match is dropped (src/ORBmatcher.cc:1516-1528, :1698-1702)."""
    specs = [(10, 20.0, 20.0)] * 11 + [(10, 20.0, 20.0 + 2.0 ** -10)]
    exp = _all(12)
    exp_o = _all(11)
    return _lattice("rotation_wrap", "src/ORBmatcher.cc:1503-1504, :1698-1702", specs, {False: (12, exp), True: (11, exp_o)}, 61)


def rotation_half_bin():
    """bin = round(rot*factor) (src/ORBmatcher.cc:1505): rot = 135 gives rot*factor == 4.5 exactly in float, which rounds
    half away from zero to bin 5, not 4.  Bins: 0 x10, 4 x2, 7 x2 -> ind1 = 0, ind2 = 4, ind3 = 7 (ComputeThreeMaxima,
    :1666-1696); the half-way match lands alone in bin 5 and is dropped."""
    r45 = _half_rot(4)
    specs = [(10, 0.0, 0.0)] * 10 + [(10, 120.0, 0.0)] * 2 + [(10, 210.0, 0.0)] * 2 + [(10, r45, 0.0)]
    return _lattice("rotation_half_bin", "src/ORBmatcher.cc:1505, :1666-1696", specs,
                    {False: (15, _all(15)), True: (14, _all(14))}, 62)


def rotation_equal_bins():
    """Equal bin counts: strict `s>max1` / `s>max2` / `s>max3` keep the FIRST bins (src/ORBmatcher.cc:1675-1695): bins 1,
    4, 7, 9 hold three matches each; bin 9's are dropped."""
    specs = []
    for b in (1, 4, 7, 9):
        specs += [(10, 30.0 * b, 0.0)] * 3
    return _lattice("rotation_equal_bins", "src/ORBmatcher.cc:1675-1695", specs,
                    {False: (12, _all(12)), True: (9, _all(9))}, 63)


def rotation_tenth():
    """max2<0.1f*(float)max1 in float (src/ORBmatcher.cc:1698-1705): 0.1f*10 rounds to exactly 1.0f, so with max1 = 10
    a second and third bin of ONE match each are kept (in double, 1 < 1.0000000149 would drop them).  Bins 0 x10,
    4 x1, 8 x1."""
    specs = [(10, 0.0, 0.0)] * 10 + [(10, 120.0, 0.0), (10, 240.0, 0.0)]
    return _lattice("rotation_tenth", "src/ORBmatcher.cc:1698-1705", specs, {False: (12, _all(12)), True: (12, _all(12))}, 64)


def rotation_tenth_20():
    """max1 = 20: 0.1f*20 is exactly 2.0f in float; max2 = 2 is kept, max3 = 1 < 2 is not (src/ORBmatcher.cc:1698-1705).
    Bins 0 x20, 3 x2, 6 x1."""
    specs = [(10, 0.0, 0.0)] * 20 + [(10, 90.0, 0.0)] * 2 + [(10, 180.0, 0.0)]
    return _lattice("rotation_tenth_20", "src/ORBmatcher.cc:1698-1705", specs, {False: (23, _all(23)), True: (22, _all(22))},
                    65)


def claim_chain(n=1200):
    """A displacement chain: map point i's window holds cur i-1 (distance 10) and cur i (distance 20).  In the
    reference's sequential loop point 0 takes cur 0, and every later point finds its best already claimed by an
    observed map point (src/ORBmatcher.cc:1469-1471) and takes its second: point i -> cur i for all i.  Resolving that
    needs about n sweeps of the device's fixed point.  The chain snakes over the image in rows 8 px apart; r = 3."""
    pos = []
    y, x, step = 8.0, 8.0, 4.0
    while len(pos) < n:
        pos.append((x, y))
        nx = x + step
        if 8.0 <= nx <= 632.0:
            x = nx
        else:                                             # turn: two vertical steps of 4 px, then the other way
            pos.append((x, y + 4.0))
            y += 8.0
            step = -step
    pos = pos[:n]
    rng = np.random.default_rng(71)
    cur_desc = [rng.integers(0, 256, 32, dtype=np.uint8)]
    for i in range(1, n):                                 # a random walk: consecutive keypoints 30 bits apart
        bits = np.unpackbits(cur_desc[-1])
        bits[rng.choice(256, 30, replace=False)] ^= 1
        cur_desc.append(np.packbits(bits))
    last_desc = [Desc.flip(cur_desc[0], 0)]
    for i in range(1, n):                                 # 10 of the 30 differing bits from cur i-1 towards cur i
        a, b = np.unpackbits(cur_desc[i - 1]), np.unpackbits(cur_desc[i])
        diff = np.flatnonzero(a != b)
        q = a.copy()
        q[diff[:10]] = b[diff[:10]]
        last_desc.append(np.packbits(q))
    last_pos = [pos[0]] + [((pos[i - 1][0] + pos[i][0]) / 2, (pos[i - 1][1] + pos[i][1]) / 2) for i in range(1, n)]
    last = kps_array(last_pos)
    cur = kps_array(pos)
    ld, cd = np.array(last_desc), np.array(cur_desc)
    assert hamming(ld[1], cd[0]) == 10 and hamming(ld[1], cd[1]) == 20
    return LastScenario(f"claim_chain_{n}", "src/ORBmatcher.cc:1469-1471, :1496-1499", last, ld, np.ones(n, np.float32), cur, cd,
                        {False: (n, _all(n)), True: (n, _all(n))}, th=3.0)


def claim_at_th_high():
    """A claim at exactly TH_HIGH blocks: point 0's best is cur 0 at distance 100, accepted (`bestDist<=TH_HIGH`,
    src/ORBmatcher.cc:1496) and claimed by an observed map point; point 1's best is cur 0 too (distance 50), which is now
    skipped (:1469-1471), so point 1 takes cur 1 at distance 60."""
    d = Desc(82)
    kd = d.base()
    a = Desc.flip(kd, 100, 0)
    b = Desc.flip(kd, 50, 100)
    c1 = Desc.flip(b, 60, 150)
    assert hamming(a, kd) == 100 and hamming(b, kd) == 50 and hamming(b, c1) == 60 and hamming(a, c1) > TH_HIGH
    last = kps_array([(100.0, 100.0), (103.0, 100.0)])
    cur = kps_array([(101.0, 100.0), (106.0, 100.0)])
    exp = {0: 0, 1: 1}
    return LastScenario("claim_at_th_high", "src/ORBmatcher.cc:1469-1471, :1496", last, np.array([a, b]), np.ones(2, np.float32),
                        cur, np.array([kd, c1]), {False: (2, exp), True: (2, exp)})


def claims_observations():
    """Claims and observations (src/ORBmatcher.cc:1469-1471, :1496-1499):
      cur 0 is claimed on entry by an observed point: skipped, point 0 takes cur 1 (distance 20 against 10);
      cur 2 is claimed on entry by a point WITHOUT observations: point 1 overwrites it;
      point 2 (obsPositive == 0) takes cur 3; point 3 (observed) then takes cur 3 as well and overwrites it: both count;
      point 4 is not a map point (no depth -> mp_valid false) and matches nothing although cur 4 is at distance 0."""
    d = Desc(81)
    bs = [d.base() for _ in range(5)]
    last = kps_array([(100.0, 100.0), (200.0, 100.0), (300.0, 100.0), (301.0, 101.0), (400.0, 100.0)])
    cur = kps_array([(101.0, 100.0), (99.0, 101.0), (201.0, 100.0), (300.5, 100.5), (400.0, 100.0)])
    cd = np.array([Desc.flip(bs[0], 10), Desc.flip(bs[0], 20, 50), Desc.flip(bs[1], 10), Desc.flip(bs[2], 10), bs[4]])
    ld = np.array(bs)
    ld[3] = Desc.flip(bs[2], 4, 200)                      # point 3's best is cur 3 as well (distance 14)
    pre = np.array([7, -1, 9, -1, -1], np.int32)
    cur_obs = np.array([1, 0, 0, 0, 0], np.uint8)
    mp_obs = np.array([1, 1, 0, 1, 1], np.uint8)
    mp_valid = np.array([1, 1, 1, 1, 0], np.uint8)
    exp = {1: 0, 2: 1, 3: 3}
    return LastScenario("claims_observations", "src/ORBmatcher.cc:1469-1471, :1496-1499", last, ld, np.ones(5, np.float32), cur, cd,
                        {False: (4, exp), True: (4, exp)}, pre=pre, cur_obs=cur_obs, mp_obs=mp_obs, mp_valid=mp_valid)


def empty(which):
    """A frame with no keypoints on one side: nothing to match (src/ORBmatcher.cc:1415, GetFeaturesInArea empty)."""
    d = Desc(90)
    b = d.base()
    one = kps_array([(100.0, 100.0)])
    none = kps_array([])
    if which == "cur":
        return LastScenario("empty_cur", "src/ORBmatcher.cc:1415, :1455-1456", one, np.array([b]), np.ones(1, np.float32),
                            none, np.zeros((0, 32), np.uint8), {False: (0, {}), True: (0, {})})
    return LastScenario("empty_last", "src/ORBmatcher.cc:1415", none, np.zeros((0, 32), np.uint8), np.zeros(0, np.float32),
                        one, np.array([b]), {False: (0, {}), True: (0, {})})


def capacity(n_last, n_cur):
    """n_last map points on a 64-column lattice (10 x 7.375 px), each with its own keypoint in the current frame at distance 5
    (src/ORBmatcher.cc:1415-1499 with r = 3: every window holds one lattice keypoint); the current frame holds n_cur
    keypoints, the ones beyond n_last at random positions with unrelated descriptors."""
    rng = np.random.default_rng(n_last * 7 + n_cur)
    pos = [(4.0 + 10.0 * (i % 64), 2.0 + 7.375 * (i // 64)) for i in range(n_last)]
    ld = rng.integers(0, 256, (n_last, 32), dtype=np.uint8)
    cd = np.concatenate([np.array([Desc.flip(x, 5, 100) for x in ld]).reshape(-1, 32),
                         rng.integers(0, 256, (n_cur - n_last, 32), dtype=np.uint8)])
    extra = [(float(F32(rng.uniform(1, 639))), float(F32(rng.uniform(1, 479)))) for _ in range(n_cur - n_last)]
    s = LastScenario(f"capacity_{n_last}_{n_cur}", "src/ORBmatcher.cc:1415-1499", kps_array(pos), ld, np.ones(n_last, np.float32),
                     kps_array(pos + extra), cd, {False: (n_last, _all(n_last)), True: (n_last, _all(n_last))}, th=3.0)
    return s


def last_scenarios():
    """Every SearchByProjection(Cur, Last) scenario that fits a default context (1000 features)."""
    out = [tie_cross_cell(), tie_wide_window(), dist_thresholds(), window_edges(), grid_rounding(), undistorted_cell(),
           image_borders("low"), image_borders("high"), level_rules("none"), level_rules("forward"), level_rules("backward"),
           rotation_wrap(), rotation_half_bin(), rotation_equal_bins(), rotation_tenth(), rotation_tenth_20(),
           claim_at_th_high(), claims_observations(), empty("cur"), empty("last")]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# SearchByProjection(Frame, vector<MapPoint*>) (src/ORBmatcher.cc:41-130)

TRACKED_DTYPE = np.dtype([("track_in_view", "u1"), ("bad", "u1"), ("obs_positive", "u1"), ("pad", "u1"),
                          ("level", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"),
                          ("view_cos", "<f4"), ("desc", "u1", (32,))])


@dataclass
class MapScenario:
    name: str
    ref: str
    kps: np.ndarray
    desc: np.ndarray
    tracked: np.ndarray          # TRACKED_DTYPE
    nnratio: float
    th: float
    expect: tuple                # (nmatches, {frame index: map point index})

    def expected(self):
        n, pairs = self.expect
        m = np.full(len(self.kps), -1, np.int32)
        for c, l in pairs.items():
            m[c] = l
        return n, m


def ratio_accepts(nnratio, d1, d2):
    """`bestDist>mfNNratio*bestDist2` with float mfNNratio and int distances (src/ORBmatcher.cc:121): the product is a
    float product, the comparison a float comparison."""
    return not (F32(d1) > F32(F32(nnratio) * F32(d2)))


def ratio_boundary_pairs(nnratio):
    """(bestDist, bestDist2) pairs on the float boundary of nnratio*bestDist2: where the float product is an integer,
    that integer (accepted: `>` is false) and one above (rejected).  For 0.6 / 0.8 / 0.9 the float product is the
    integer while the exact product of the float ratio lies one ulp off it (0.9f * 10 = 8.99999976 rounds to 9.0f):
    the pair is accepted in float and, for 0.9, rejected in double."""
    out = []
    for d2 in range(2, 101):
        p = F32(F32(nnratio) * F32(d2))
        if p == np.floor(p) and 1 <= p < d2:
            out.append((int(p), d2))
            out.append((int(p) + 1, d2))
        if len(out) >= 10:
            break
    return out


def map_ratio(nnratio):
    """Best and second on the same level: the ratio test at the float boundary (src/ORBmatcher.cc:121).  Plus a pair on
    different levels (no ratio test, :121 `bestLevel==bestLevel2`), a best == second tie on one level (rejected) and on
    two levels (accepted: the first visited, the higher index), and bestDist on TH_HIGH (:119)."""
    d = Desc(int(nnratio * 100))
    pairs = ratio_boundary_pairs(nnratio)
    kps, desc, tr, exp = [], [], [], {}
    cases = [(d1, d2, 0, 0) for d1, d2 in pairs] + [(60, 61, 0, 1), (40, 40, 0, 0), (100, 200, 0, 0), (101, 200, 0, 0)]
    for i, (d1, d2, l1, l2) in enumerate(cases):
        x, y = 30.0 + 60.0 * (i % 10), 30.0 + 60.0 * (i // 10)
        b = d.base()
        t = np.zeros((), TRACKED_DTYPE)
        t["track_in_view"], t["obs_positive"], t["level"] = 1, 1, 1
        t["proj_x"], t["proj_y"], t["proj_xr"], t["view_cos"], t["desc"] = x, y, -1.0, 0.9, b
        tr.append(t)
        # second candidate first in the scan (column before), best second: the best is not simply the first visited
        kps.append((x - 2.0, y, l2)); desc.append(Desc.flip(b, d2, 0))
        kps.append((x + 2.0, y, l1)); desc.append(Desc.flip(b, d1, 100))
        best = 2 * i + 1 if d1 < d2 else 2 * i    # on a tie the first visited holds
        accept = d1 <= TH_HIGH and (l1 != l2 or ratio_accepts(nnratio, min(d1, d2), max(d1, d2)))
        if accept:
            exp[best] = i
    # a tie on two levels, the projection 4.75 px left of the block's x0 (a multiple of 10): cur 2i at x0 - 4 is in cell column
    # x0/10 (round(x0/10 - 0.4)), cur 2i+1 at x0 - 5.5 in column x0/10 - 1 (round(x0/10 - 0.55)), which the scan visits
    # first, so the HIGHER index wins (for the 0.6 case, x0 = 270: columns 27 and 26)
    b = d.base()
    i = len(tr)
    x, y = 30.0 + 60.0 * (i % 10), 30.0 + 60.0 * (i // 10)
    t = np.zeros((), TRACKED_DTYPE)
    t["track_in_view"], t["obs_positive"], t["level"] = 1, 1, 1
    t["proj_x"], t["proj_y"], t["proj_xr"], t["view_cos"], t["desc"] = x - 4.75, y, -1.0, 0.9, b
    tr.append(t)
    kps.append((x - 4.0, y, 0)); desc.append(Desc.flip(b, 30, 0))
    kps.append((x - 5.5, y, 1)); desc.append(Desc.flip(b, 30, 100))
    exp[2 * i + 1] = i
    tracked = np.array(tr, TRACKED_DTYPE)
    return MapScenario(f"map_ratio_{nnratio}", "src/ORBmatcher.cc:99-125", kps_array(kps), np.array(desc), tracked, nnratio, 1.0,
                       (len(exp), exp))


def map_scenarios():
    return [map_ratio(r) for r in (0.6, 0.75, 0.8, 0.9)]


# ---------------------------------------------------------------------------------------------------------------------
# the same frames on the oracle's side

K4 = np.array([FX, FY, CX, CY], np.float32)


def oracle_last(orc, s: LastScenario):
    """(cur FrameOracle, last FrameOracle, map points as MAPPOINT_DTYPE of the oracle).  The oracle reads mvKeysUn, so
    the current frame is built from cur_kps_un where the scenario has one."""
    sc = scale_factors()
    cur_k = s.cur_kps if s.cur_kps_un is None else s.cur_kps_un
    cur = orc.FrameOracle(cur_k, s.cur_desc.reshape(-1, 32), np.zeros((H, W), np.float32), K4, BF, W, H, sc)
    last = orc.FrameOracle(s.last_kps, s.last_desc.reshape(-1, 32), depth_image(s.last_kps, s.last_z), K4, BF, W, H, sc)
    world, valid = last.unproject(s.Twc_last)
    mp = np.zeros(last.N, orc.MAPPOINT_DTYPE)
    mp["valid"] = valid if s.mp_valid is None else valid & s.mp_valid
    mp["obsPositive"] = 1 if s.mp_obs is None else s.mp_obs
    mp["world"] = world
    mp["desc"] = last.desc
    return cur, last, mp


def oracle_search_last(orc, s: LastScenario, check_ori):
    cur, last, mp = oracle_last(orc, s)
    return orc.search_by_projection_last(cur, last, s.Tcw_cur, s.Tcw_last, mp, s.th, False, check_ori, s.pre, s.cur_obs)


def oracle_tracked(orc, t):
    o = np.zeros(len(t), orc.TRACKED_DTYPE)
    for a, b in (("track_in_view", "trackInView"), ("bad", "bad"), ("obs_positive", "obsPositive"), ("level", "level"),
                 ("proj_x", "projX"), ("proj_y", "projY"), ("proj_xr", "projXR"), ("view_cos", "viewCos"), ("desc", "desc")):
        o[b] = t[a]
    return o


def oracle_search_map(orc, s: MapScenario):
    fo = orc.FrameOracle(s.kps, s.desc, np.zeros((H, W), np.float32), K4, BF, W, H, scale_factors())
    return orc.search_by_projection_map(fo, oracle_tracked(orc, s.tracked), s.th, s.nnratio)


# ---------------------------------------------------------------------------------------------------------------------
# The keyframe matchers: Fuse (src/ORBmatcher.cc:829-979, :981-1104), SearchByProjection(pKF, Scw, ...) (:294-407) and
# the relocalisation SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1537-1660) on one keyframe.

FRUSTUM_POINT_DTYPE = np.dtype([("world", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                                ("max_distance", "<f4")])
KF_DISTS = (30, 49, 50, 51, 64, 65, 100, 101)      # point 0 is the tie; the others one candidate each


@dataclass
class KeyFrameScenario:
    name: str
    ref: str
    kps: np.ndarray
    desc: np.ndarray
    pts: np.ndarray
    pdesc: np.ndarray
    winner: list           # per point: the keypoint the scan keeps (first minimum in GetFeaturesInArea order)
    dist: list             # per point: its distance


def keyframe_points():
    """Eight map points, each projecting (identity pose, z = 1) to (x0 + 5, y0 + 5) with x0, y0 multiples of 10: the cell
    boundary of PosInGrid.  Point 0 has two candidates at distance 30: kp 0 at (+1, -1) in cell column x0/10 + 1, kp 1 at
    (-1, +1) in column x0/10, visited first: the higher index wins (strict `dist<bestDist`, :391, :948, :1078, :1613).
    Points 1-7 have one candidate at (+1, +1) with distances 49, 50, 51, 64, 65, 100, 101: TH_LOW (:398, :956, :1086) and
    ORBdist 64 / 100 (:1620) with their neighbours.  Both candidates are within 1.5 px, inside Fuse's chi-square gate
    (e2 * invSigma2 <= 5.99, :940) and every window (th = 3 at the predicted level 1).  The normal points along the
    viewing ray and the distance bounds bracket the depth: maxDistance = 1.05 dist predicts level 1."""
    d = Desc(91)
    kps, kdesc, pts, pdesc, winner, dist = [], [], [], [], [], []
    for i, dd in enumerate(KF_DISTS):
        x0, y0 = 100.0 + 60.0 * (i % 8), 100.0 + 60.0 * (i // 8)
        u, v = x0 + 5.0, y0 + 5.0
        b = d.base()
        if i == 0:
            kps += [(u + 1.0, v - 1.0), (u - 1.0, v + 1.0)]
            kdesc += [Desc.flip(b, dd, 0), Desc.flip(b, dd, 100)]
            winner.append(1)
        else:
            winner.append(len(kps))
            kps.append((u + 1.0, v + 1.0))
            kdesc.append(Desc.flip(b, dd, 0))
        dist.append(dd)
        w = np.array([(u - CX) / FX, (v - CY) / FY, 1.0], np.float32)
        r = float(np.linalg.norm(w.astype(np.float64)))
        t = np.zeros((), FRUSTUM_POINT_DTYPE)
        t["world"], t["normal"] = w, (w / F32(r)).astype(np.float32)
        t["max_distance"], t["min_distance"] = F32(1.05 * r), F32(0.5 * r)
        pts.append(t)
        pdesc.append(b)
    return KeyFrameScenario("keyframe_points", "src/ORBmatcher.cc:294-407, :829-1104, :1537-1660", kps_array(kps), np.array(kdesc),
                            np.array(pts, FRUSTUM_POINT_DTYPE), np.array(pdesc), winner, dist)


def kf_expected_new(s: KeyFrameScenario, limit):
    """new[keypoint] = point for every point whose best distance is <= limit (each window holds only its own point)."""
    out = np.full(len(s.kps), -1, np.int32)
    for i, (w, dd) in enumerate(zip(s.winner, s.dist)):
        if dd <= limit:
            out[w] = i
    return int((out >= 0).sum()), out


# ---------------------------------------------------------------------------------------------------------------------
# SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:409-524)

@dataclass
class InitScenario:
    name: str
    ref: str
    kps1: np.ndarray
    desc1: np.ndarray
    kps2: np.ndarray
    desc2: np.ndarray
    prev: np.ndarray
    nnratio: float
    expect: tuple          # (nmatches, matches12)


def init_accepts(nnratio, d1, d2):
    """`bestDist<=TH_LOW` then `bestDist<(float)bestDist2*mfNNratio` (src/ORBmatcher.cc:463-465), in float."""
    return d1 <= TH_LOW and F32(d1) < F32(F32(d2) * F32(nnratio))


def init_ratio(nnratio):
    """One F1 keypoint per window (windowSize 10, level 0): its F2 window holds a best and a second at (d1, d2).  The pairs
    are the float boundary of the ratio (ratio_boundary_pairs; `<` rejects the product itself) and one below it, a
    best == second tie, TH_LOW 50 / 51 with no second
    (bestDist2 = INT_MAX), and for 0.9 the pair (44, 49): 44 < 44.1.  The best sits in the later cell column but has the
    lower distance."""
    d = Desc(200 + int(nnratio * 100))
    pairs = [(a, b) for a, b in ratio_boundary_pairs(nnratio) if a <= TH_LOW]
    cases = pairs + [(a - 1, b) for a, b in pairs[::2]] + [(30, 30), (50, None), (51, None), (44, 49)]
    k1, d1s, k2, d2s, m12 = [], [], [], [], []
    for i, (a, b) in enumerate(cases):
        x, y = 30.0 + 50.0 * (i % 12), 30.0 + 50.0 * (i // 12)
        base = d.base()
        k1.append((x, y)); d1s.append(base)
        if b is not None:
            k2.append((x - 3.0, y)); d2s.append(Desc.flip(base, b, 0))
        k2.append((x + 3.0, y)); d2s.append(Desc.flip(base, a, 100))
        ok = init_accepts(nnratio, a, 2 ** 31 - 1 if b is None else b)
        m12.append(len(k2) - 1 if ok else -1)
    m12 = np.array(m12, np.int32)
    kp1 = kps_array(k1)
    prev = np.stack([kp1["x"], kp1["y"]], 1).astype(np.float32)
    return InitScenario(f"init_ratio_{nnratio}", "src/ORBmatcher.cc:409-524", kp1, np.array(d1s), kps_array(k2), np.array(d2s), prev,
                        nnratio, (int((m12 >= 0).sum()), m12))


def init_scenarios():
    return [init_ratio(r) for r in (0.6, 0.75, 0.8, 0.9)]


# ---------------------------------------------------------------------------------------------------------------------
# MatchORBPoints (src/ORBmatcher.cc:1332-1394) and cv::BFMatcher(NORM_HAMMING) k-NN

def orb_points():
    """BFMatcher 1-NN of the current descriptors against the last ones; `distance<max(2*min_dist, 15)` (:1366) with
    min_dist = 5, so the threshold is 15: distances 5, 14, 14 and 7 pass, 15 and 20 do not.  cur 5 is 7 from last 2 and
    from last 4: the lower train index, last 2, wins.  The quirk `!LastFrame.mvbOutlier[i]` (:1384) indexes the outlier
    flags by the good-match COUNTER: the flag at 1 drops the second good match (cur 1), not last 1.
    Returns (cur_desc, last_desc, last_mp, last_outlier, expected NPair, expected out)."""
    d = Desc(300)
    last = [d.base() for _ in range(6)]
    last[4] = Desc.flip(last[2], 14, 0)
    cur = [Desc.flip(last[0], 5, 50), Desc.flip(last[1], 14, 50), Desc.flip(last[3], 15, 50), Desc.flip(last[5], 20, 50),
           Desc.flip(last[5], 14, 100), Desc.flip(last[2], 7, 0)]
    assert hamming(cur[5], last[2]) == 7 and hamming(cur[5], last[4]) == 7
    last_mp = np.arange(6, dtype=np.int32) + 100
    outlier = np.array([0, 1, 0, 0, 0, 0], np.uint8)
    out = np.array([100, -1, -1, -1, 105, 102], np.int32)
    return np.array(cur), np.array(last), last_mp, outlier, 4, out


def bf_ties():
    """cv::BFMatcher k-NN with exact ties: equal distances keep ascending train order.  q0: t1 and t3 at 10, t0 at 12 ->
    2-NN (t1, t3); q1: t2 at 0 twice (t2 == t4) -> (t2, t4); q2: one train row only -> the second neighbour is -1."""
    d = Desc(301)
    q = [d.base(), d.base(), d.base()]
    t = [Desc.flip(q[0], 12, 0), Desc.flip(q[0], 10, 20), q[1].copy(), Desc.flip(q[0], 10, 40), q[1].copy()]
    exp_idx = np.array([[1, 3], [2, 4]], np.int32)
    exp_dist = np.array([[10, 10], [0, 0]], np.int32)
    return np.array(q), np.array(t), exp_idx, exp_dist
