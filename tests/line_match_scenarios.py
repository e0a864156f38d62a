"""Hand-built key lines that put the line matchers (LSDmatcher) on their decision points: equal Hamming distances in
and across the lanes of the strided scans, midpoints on the radius, slopes on r * 0.01, distances on TH_HIGH / TH_LOW,
the ratio test on its float boundary, projections on the image border, degenerate slopes, claims with and without
observations, the level quirk of GetLinesInArea, the distance bands / cones on exact values and the MAD gap rule.

Every scenario carries the outcome stated by hand from the reference source (src/LSDmatcher.cpp, src/Frame.cc:781-813,
src/KeyFrame.cc:749-786, src/Frame.cc:560-584, include/auxiliar.h:22-41); nothing here calls the oracle or the library.
tests/test_line_match_edges_cpu.py holds the oracle to these outcomes and checks that every input sits where it is
claimed to sit; tests/test_gpu_line_match_edges.py holds the device to both.

Geometry: a 640 x 480 frame with fx = fy = 512, cx = 320, cy = 240, bounds 0 .. 640 x 0 .. 480.  Under identity poses an
end point (X, Y, 1) projects to (512 X + 320, 512 Y + 240) exactly in float for the coordinates used here, so X = +-0.625
lands on u = 0 / 640.  The windows have radius r = 5 * mvScaleFactors[level] in every entry: SearchByProjection(F,
vpMapLines, th = 1) takes RadiusByViewingCos = 5 for viewCos > 0.998, the other entries are called with th = 5.
The wavefront stride of the device scans is 64: indices i, i + 64, i + 128 share a lane."""
from dataclasses import dataclass, field

import numpy as np

from match_scenarios import Desc, F32, ratio_boundary_pairs, scale_factors, ulp_above, ulp_below

W, H = 640, 480
FX = FY = 512.0
CX, CY = 320.0, 240.0
BF = 51.2
MB = F32(F32(BF) / F32(FX))            # mb = bf / fx, the motion-flag threshold (src/LSDmatcher.cpp:33-34)
TH_HIGH, TH_LOW = 100, 50              # include/LSDmatcher.h
WAVE = 64
CAM = dict(fx=FX, fy=FY, cx=CX, cy=CY, bf=BF, min_x=0.0, max_x=float(W), min_y=0.0, max_y=float(H))

LINE_DTYPE = np.dtype([("pt_x", "<f4"), ("pt_y", "<f4"), ("angle", "<f4"), ("octave", "<i4")])
MAPLINE_DTYPE = np.dtype([("valid", "<i4"), ("octave", "<i4"), ("obs_positive", "<i4"), ("pad", "<i4"),
                          ("world", "<f8", (6,)), ("desc", "u1", (32,))])
TRACKED_LINE_DTYPE = np.dtype([("in_view", "<i4"), ("level", "<i4"), ("obs_positive", "<i4"), ("x1", "<f4"),
                               ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("view_cos", "<f4"), ("desc", "u1", (32,))])
FRUSTUM_LINE_DTYPE = np.dtype([("world", "<f8", (6,)), ("normal", "<f8", (3,)), ("min_distance", "<f4"),
                               ("max_distance", "<f4")])


def cam9():
    return np.array([FX, FY, CX, CY, MB, 0.0, W, 0.0, H], np.float32)


def translation_z(tz):
    T = np.eye(4, dtype=np.float32)
    T[2, 3] = tz
    return T


# ---------------------------------------------------------------------------------------------------------------------
# The reference expressions in numpy, in the types the C++ has (for the conditions, never for an expectation)

def area_gates(x1, y1, x2, y2, r, px, py, angle):
    """Radius and slope test of Frame::GetLinesInArea / KeyFrame::GetLinesInArea (src/Frame.cc:793-800): `0.5 * (x1 + x2)`
    is a float sum widened to double, the difference and the squares are double, the sum is stored to a float and compared
    with the float product r * r; slope is float and compared with the double r * 0.01.  -> (passes radius, passes slope)"""
    x1, y1, x2, y2, r, px, py, angle = (F32(v) for v in (x1, y1, x2, y2, r, px, py, angle))
    with np.errstate(all="ignore"):
        mx = 0.5 * float(F32(x1 + x2)) - float(px)
        my = 0.5 * float(F32(y1 + y2)) - float(py)
        distance = F32(mx * mx + my * my)
        radius_ok = not (distance > F32(r * r))
        slope = F32(F32(F32(y1 - y2) / F32(x1 - x2)) - angle)
        slope_ok = not (float(slope) > float(r) * 0.01)
    return radius_ok, slope_ok


def level_gate(octave, min_level, max_level):
    """the level test, src/Frame.cc:787 / :802-807: on with minLevel > 0 || maxLevel > 0"""
    if not (min_level > 0 or max_level > 0):
        return True
    if octave < min_level:
        return False
    return not (max_level >= 0 and octave > max_level)


def radius_edge(c, r):
    """(last float coordinate still inside, first one outside) for a key line straight below a midpoint at c"""
    y = F32(c + float(r)) - F32(2.0 ** -10)
    while area_gates(0, c, 0, c, r, 0, np.nextafter(y, F32(np.inf)), 0)[0]:
        y = np.nextafter(y, F32(np.inf))
    assert area_gates(0, c, 0, c, r, 0, y, 0)[0]
    return float(y), float(np.nextafter(y, F32(np.inf)))


def slope_edge(r):
    """(largest float slope that passes `slope > r * 0.01`, the next float, which fails)"""
    s = F32(float(F32(r)) * 0.01)
    while float(s) > float(F32(r)) * 0.01:
        s = np.nextafter(s, F32(-np.inf))
    while not float(np.nextafter(s, F32(np.inf))) > float(F32(r)) * 0.01:
        s = np.nextafter(s, F32(np.inf))
    return float(s), float(np.nextafter(s, F32(np.inf)))


def project(X, Y, Z):
    """u, v as src/LSDmatcher.cpp:61-63 computes them under an identity pose"""
    with np.errstate(all="ignore"):
        invz = F32(1.0) / F32(Z)
        return F32(F32(F32(FX) * F32(X)) * invz) + F32(CX), F32(F32(F32(FY) * F32(Y)) * invz) + F32(CY)


def reference_scan(cands, nnratio, tie_last=False, second_other=False):
    """src/LSDmatcher.cpp:97-136 over cands = [(index, dist, octave)] in index order -> accepted index or None.
    The two wrong readings the scan scenarios must tell apart from the reference: tie_last turns both strict `<` into
    `<=` (the last index wins a tie); second_other hands bestLevel2 to the LAST candidate at bestDist2 instead of the
    one the sequential scan leaves there."""
    best_dist, best_level, best_dist2, best_level2, best_idx = 256, -1, 256, -1, -1
    lt = (lambda a, b: a <= b) if tie_last else (lambda a, b: a < b)
    for idx, dist, octave in cands:
        if lt(dist, best_dist):
            best_dist2, best_dist, best_level2, best_level, best_idx = best_dist, dist, best_level, octave, idx
        elif lt(dist, best_dist2):
            best_level2, best_dist2 = octave, dist
    if second_other:
        rest = [c for c in cands if c[0] != best_idx and c[1] == best_dist2]
        if rest:
            best_level2 = rest[-1][2]
    if best_dist <= TH_HIGH and not (best_level == best_level2 and F32(best_dist) > F32(F32(nnratio) * F32(best_dist2))):
        return best_idx
    return None


# ---------------------------------------------------------------------------------------------------------------------
# One call of a windowed search: key lines, queries, and the three ways the entries receive a query

@dataclass
class Named:
    """a candidate a scenario talks about: its query, its index, the stated Hamming distance, whether it passes the radius
    and slope tests of its query's window, and (scan scenarios) its lane"""
    q: int
    idx: int
    dist: int
    radius: bool = True
    slope: bool = True
    lane: int = None


class Scene:
    """n key lines parked far outside every window (x >= 5000, random descriptors) that the scenarios overwrite."""

    def __init__(self, seed, n):
        self.d = Desc(seed)
        self.cur = np.zeros(n, LINE_DTYPE)
        self.cur["pt_x"] = 5000.0 + 10.0 * np.arange(n)
        self.cur["pt_y"] = 5000.0
        self.desc = self.d.rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.q = []
        self.named = []
        self.free = 0

    def put(self, idx, x, y, angle=0.0, octave=0, desc=None):
        self.cur[idx] = (x, y, angle, octave)
        if desc is not None:
            self.desc[idx] = desc
        return idx

    def add(self, x, y, angle=0.0, octave=0, desc=None):
        self.free += 1
        return self.put(self.free - 1, x, y, angle, octave, desc)

    def query(self, x1, y1, x2, y2, level=0, desc=None, obs=1, valid=1, z=(1.0, 1.0)):
        self.q.append(dict(x1=x1, y1=y1, x2=x2, y2=y2, level=level, desc=self.d.base() if desc is None else desc, obs=obs,
                           valid=valid, z=z))
        return len(self.q) - 1

    def cand(self, q, idx, dist, at=0, **kw):
        """key line idx gets query q's descriptor with `dist` bits flipped from bit `at`"""
        self.desc[idx] = Desc.flip(self.q[q]["desc"], dist, at)
        self.named.append(Named(q, idx, dist, **kw))
        return idx

    # the three presentations of the queries
    def tracked(self):
        t = np.zeros(len(self.q), TRACKED_LINE_DTYPE)
        for i, q in enumerate(self.q):
            t[i] = (q["valid"], q["level"], q["obs"], q["x1"], q["y1"], q["x2"], q["y2"], 1.0, q["desc"])
        return t

    def world(self, q):
        (z1, z2) = q["z"]
        return [(float(F32(q["x1"])) - CX) / FX * z1, (float(F32(q["y1"])) - CY) / FY * z1, z1,
                (float(F32(q["x2"])) - CX) / FX * z2, (float(F32(q["y2"])) - CY) / FY * z2, z2]

    def map_lines(self):
        m = np.zeros(len(self.q), MAPLINE_DTYPE)
        for i, q in enumerate(self.q):
            m[i] = (q["valid"], q["level"], q["obs"], 0, self.world(q), q["desc"])
        return m

    def frustum_lines(self):
        """normal (0, 0, 1) (inside the 60-degree cone everywhere in this image), a wide distance band, and a distance ratio
        of 1.2^(level - 0.5): PredictScale = ceil(level - 0.5) = level, far from both neighbours"""
        f = np.zeros(len(self.q), FRUSTUM_LINE_DTYPE)
        for i, q in enumerate(self.q):
            w = np.array(self.world(q))
            dist = np.linalg.norm(0.5 * (w[:3] + w[3:]))
            f[i] = (w, (0.0, 0.0, 1.0), 0.01, q.get("dmax", F32(dist * 1.2 ** (q["level"] - 0.5))))
        return f

    def descs(self):
        return np.array([q["desc"] for q in self.q], np.uint8).reshape(-1, 32)

    def skip(self):
        return np.array([0 if q["valid"] else 1 for q in self.q], np.uint8)


@dataclass
class WindowScenario:
    name: str
    ref: str
    scene: Scene
    expect: dict                 # "map" / "last": (nmatches, {key line: query}); "fuse": {query: (key line, distance)}
    r0: float = 5.0              # window radius at level 0
    nnratio: float = 0.9
    pre: np.ndarray = None       # claims on entry (cur_ml) and their observation flags
    cur_obs: np.ndarray = None
    Tcw_last: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    mono: bool = False

    def cur_ml(self):
        return np.full(len(self.scene.cur), -1, np.int32) if self.pre is None else self.pre.astype(np.int32).copy()

    def expected(self, entry):
        n, pairs = self.expect[entry]
        m = self.cur_ml()
        for k, q in pairs.items():
            m[k] = q
        return n, m

    def expected_fuse(self):
        nq = len(self.scene.q)
        bi, bd = np.full(nq, -1, np.int32), np.full(nq, np.iinfo(np.int32).max, np.int32)
        for q, (k, d) in self.expect["fuse"].items():
            bi[q] = k
            if k >= 0:
                bd[q] = d
        return bi, bd


def oracle_map(orc, s):
    return orc.lsd_search_by_projection_map(scale_factors(), s.scene.tracked(), s.scene.cur, s.scene.desc, s.r0 / 5.0, s.nnratio,
                                            s.cur_ml(), s.cur_obs)


def oracle_last(orc, s):
    return orc.lsd_search_by_projection_last(cam9(), np.eye(4, dtype=np.float32), s.Tcw_last, scale_factors(), s.scene.map_lines(),
                                             s.scene.cur, s.scene.desc, s.r0, s.mono, s.nnratio, s.cur_ml(), s.cur_obs)


def oracle_fuse(orc, s, sim3=False):
    T = np.eye(4, dtype=np.float32)
    if sim3:
        T[:3, :] *= F32(2.0)                  # Scw = 2 [I | 0]: the decomposition (:759-763) is exact
    fn = orc.lsd_fuse_search_sim3 if sim3 else orc.lsd_fuse_search
    return fn(cam9(), T, 1.2, scale_factors(), s.scene.frustum_lines(), s.scene.descs(), s.scene.skip(), s.scene.cur,
              s.scene.desc, s.r0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. Window gates: one query and one candidate (Hamming distance 10) per lattice point

def _centre(i):
    return 40.0 + 60.0 * (i % 10), 40.0 + 60.0 * (i // 10)


H_SEG, UP_SEG, DOWN_SEG, POINT_SEG = (-10.0, 0.0, 10.0, 0.0), (0.0, 10.0, 0.0, -10.0), (0.0, -10.0, 0.0, 10.0), (0.0, 0.0, 0.0, 0.0)


def window_gates():
    """Frame::GetLinesInArea, src/Frame.cc:781-813 (KeyFrame::GetLinesInArea, src/KeyFrame.cc:749-781, is the same text).
    Every case is one query with one candidate; `keep` says by hand whether the candidate is in the window of
    SearchByProjection(F, vpMapLines) (levels l-1 .. l, src/LSDmatcher.cpp:159-161), of SearchByProjection(Cur, Last)
    without motion (levels o-1 .. o+1, :90) and of Fuse (no level test in GetLinesInArea, octave window l-1 .. l, :975).

    radius: `distance > r * r` (:795) keeps the offset (3, 4) at r = 5 and drops the next float; at level 1 r = 5 * 1.2f
    rounds to 6.0f, at level 2 r = 5 * (1.2f * 1.2f) = 7.2000003 and r * r is rounded in float - the last float inside and
    the first outside come from radius_edge().
    slope: `slope > r * 0.01` (:799) compares a float with a double: float(0.05) lies above the double 0.05 and fails, the
    float below passes; the test is one-sided, slope -3 passes.  The query is horizontal ((y1 - y2) / (x1 - x2) = -0), so
    slope = -angle exactly.
    degenerate: x1 == x2 with y1 > y2 gives +inf (nothing passes), y1 < y2 gives -inf (everything passes); a query whose
    end points coincide gives 0 / 0 = NaN, which fails no comparison (everything passes).
    levels: bCheckLevels = minLevel > 0 || maxLevel > 0 (:787): the window (-1, 0) of a level-0 map line checks nothing."""
    T, F_ = True, False
    s5 = scale_factors()
    r1, r2 = F32(F32(5.0) * s5[1]), F32(F32(5.0) * s5[2])
    s0_in, s0_out = slope_edge(5.0)
    s1_in, s1_out = slope_edge(r1)
    # name, segment, level, candidate offset, angle, octave, keep (map, last, fuse)
    cases = [
        ("radius_on", H_SEG, 0, (3.0, 4.0), 0.0, 0, (T, T, T)),
        ("radius_ulp_out", H_SEG, 0, (3.0, "ulp"), 0.0, 0, (F_, F_, F_)),
        ("radius_l1_last_in", H_SEG, 1, (0.0, "r1_in"), 0.0, 1, (T, T, T)),
        ("radius_l1_first_out", H_SEG, 1, (0.0, "r1_out"), 0.0, 1, (F_, F_, F_)),
        ("radius_l2_last_in", H_SEG, 2, (0.0, "r2_in"), 0.0, 2, (T, T, T)),
        ("radius_l2_first_out", H_SEG, 2, (0.0, "r2_out"), 0.0, 2, (F_, F_, F_)),
        ("slope_below_bound", H_SEG, 0, (0.0, 0.0), -s0_in, 0, (T, T, T)),
        ("slope_float_0.05", H_SEG, 0, (0.0, 0.0), -s0_out, 0, (F_, F_, F_)),
        ("slope_l1_last_in", H_SEG, 1, (0.0, 0.0), -s1_in, 1, (T, T, T)),
        ("slope_l1_first_out", H_SEG, 1, (0.0, 0.0), -s1_out, 1, (F_, F_, F_)),
        ("slope_negative", H_SEG, 0, (0.0, 0.0), 3.0, 0, (T, T, T)),
        ("slope_plus_inf", UP_SEG, 0, (0.0, 0.0), 1e30, 0, (F_, F_, F_)),
        ("slope_minus_inf", DOWN_SEG, 0, (0.0, 0.0), -1e30, 0, (T, T, T)),
        ("slope_nan", POINT_SEG, 0, (0.0, 0.0), 0.0, 0, (T, T, T)),
        ("slope_nan_steep", POINT_SEG, 0, (1.0, 1.0), -1e30, 0, (T, T, T)),
        # level quirk: level-0 map line, window (-1, 0): no level test at all
        ("l0_oct0", H_SEG, 0, (0.0, 0.0), 0.0, 0, (T, T, T)),
        ("l0_oct1", H_SEG, 0, (0.0, 0.0), 0.0, 1, (T, T, F_)),
        ("l0_oct2", H_SEG, 0, (0.0, 0.0), 0.0, 2, (T, F_, F_)),
        ("l0_oct5", H_SEG, 0, (0.0, 0.0), 0.0, 5, (T, F_, F_)),
        # level 1: map (0, 1), last (0, 2), fuse 0 .. 1
        ("l1_oct0", H_SEG, 1, (0.0, 0.0), 0.0, 0, (T, T, T)),
        ("l1_oct1", H_SEG, 1, (0.0, 0.0), 0.0, 1, (T, T, T)),
        ("l1_oct2", H_SEG, 1, (0.0, 0.0), 0.0, 2, (F_, T, F_)),
        ("l1_oct3", H_SEG, 1, (0.0, 0.0), 0.0, 3, (F_, F_, F_)),
        # level 2: map (1, 2), last (1, 3), fuse 1 .. 2
        ("l2_oct0", H_SEG, 2, (0.0, 0.0), 0.0, 0, (F_, F_, F_)),
        ("l2_oct1", H_SEG, 2, (0.0, 0.0), 0.0, 1, (T, T, T)),
        ("l2_oct2", H_SEG, 2, (0.0, 0.0), 0.0, 2, (T, T, T)),
        ("l2_oct3", H_SEG, 2, (0.0, 0.0), 0.0, 3, (F_, T, F_)),
        ("l2_oct4", H_SEG, 2, (0.0, 0.0), 0.0, 4, (F_, F_, F_)),
    ]
    sc = Scene(101, 140)
    exp = {"map": {}, "last": {}, "fuse": {}}
    names = []
    for i, (name, seg, level, off, angle, octave, keep) in enumerate(cases):
        cx, cy = _centre(i)
        q = sc.query(cx + seg[0], cy + seg[1], cx + seg[2], cy + seg[3], level=level)
        py = cy + off[1] if not isinstance(off[1], str) else {"ulp": ulp_above(cy + 4.0), "r1_in": radius_edge(cy, r1)[0],
                                                              "r1_out": radius_edge(cy, r1)[1], "r2_in": radius_edge(cy, r2)[0],
                                                              "r2_out": radius_edge(cy, r2)[1]}[off[1]]
        k = sc.add(cx + off[0], py, angle, octave)
        sc.cand(q, k, 10, radius=name not in ("radius_ulp_out", "radius_l1_first_out", "radius_l2_first_out"),
                slope=name not in ("slope_float_0.05", "slope_l1_first_out", "slope_plus_inf"))
        names.append(name)
        for e, kp in zip(("map", "last"), keep):
            if kp:
                exp[e][k] = q
        exp["fuse"][q] = (k, 10) if keep[2] else (-1, 0)
    s = WindowScenario("window_gates", "src/Frame.cc:781-813, src/KeyFrame.cc:749-781, src/LSDmatcher.cpp:85-90, :159-161, :975",
                       sc, {"map": (len(exp["map"]), exp["map"]), "last": (len(exp["last"]), exp["last"]), "fuse": exp["fuse"]})
    s.case_names = names
    s.edges = dict(r1=float(r1), r2=float(r2), s0=(s0_in, s0_out), s1=(s1_in, s1_out))
    return s


# the motion modes of SearchByProjection(Cur, Last): (name, z translation of Tcw_last, bMono, mode stated by hand).
# tlc = Rlw * twc + tlw = tlw under an identity current pose; bForward = tlc.z > mb && !bMono, bBackward = -tlc.z > mb && !bMono
# (src/LSDmatcher.cpp:33-34): both comparisons are strict.
MOTIONS = [("still", 0.0, False, "none"), ("on_mb", float(MB), False, "none"), ("ulp_above_mb", ulp_above(MB), False, "fwd"),
           ("on_minus_mb", -float(MB), False, "none"), ("ulp_below_minus_mb", -ulp_above(MB), False, "bwd"),
           ("forward", 1.0, False, "fwd"), ("backward", -1.0, False, "bwd"), ("forward_mono", 1.0, True, "none"),
           ("backward_mono", -1.0, True, "none")]

# candidate octave -> kept, per last-frame octave and mode (src/LSDmatcher.cpp:85-90 with src/Frame.cc:787, :802-807):
# octave 0: forward (0, -1) and backward (0, 0) switch the level test off, no motion (-1, 1) keeps octaves <= 1;
# octave 2: forward (2, -1) has no upper bound, backward (0, 2), no motion (1, 3)
MOTION_KEEP = {(0, "fwd"): (1, 1, 1, 1, 1), (0, "bwd"): (1, 1, 1, 1, 1), (0, "none"): (1, 1, 0, 0, 0),
               (2, "fwd"): (0, 0, 1, 1, 1), (2, "bwd"): (1, 1, 1, 0, 0), (2, "none"): (0, 1, 1, 1, 0)}


def motion_levels(name, tz, mono, mode):
    sc = Scene(102, 140)
    exp = {}
    i = 0
    for oct_last in (0, 2):
        for oct_cand in range(5):
            cx, cy = _centre(i)
            q = sc.query(cx - 10.0, cy, cx + 10.0, cy, level=oct_last)
            k = sc.cand(q, sc.add(cx, cy, 0.0, oct_cand), 10)
            if MOTION_KEEP[(oct_last, mode)][oct_cand]:
                exp[k] = q
            i += 1
    return WindowScenario(f"motion_{name}", "src/LSDmatcher.cpp:33-34, :85-90, src/Frame.cc:787, :802-807", sc,
                          {"last": (len(exp), exp)}, Tcw_last=translation_z(tz), mono=mono)


# ---------------------------------------------------------------------------------------------------------------------
# 2. The best / second scan

# The orderings.  Candidates (distance, octave) and, per index order, (accepted candidate or None, best, second) stated by hand from
# src/LSDmatcher.cpp:113-125 (strict <: the first of equals holds; a new best hands its level to bestLevel2) and :128-131
# (bestLevel == bestLevel2 && bestDist > 0.9f * bestDist2 rejects: 19 > 18.0, 20 > 18.0, 10 > 9.0).  Every one of them has a tie,
# and its outcome changes under "the last index wins a tie" or "second = the other candidate of equal distance" (checked by
# reference_scan() in the CPU test); scan_thresholds() below has no ties to misread.
SCAN_SETS = {
    # A is always best; second is the first of B (A's octave: rejected) and C (another octave: accepted) in index order
    "19_20_20": (dict(A=(19, 0), B=(20, 0), C=(20, 1)),
                 dict(ABC=(None, "A", "B"), ACB=("A", "A", "C"), BAC=(None, "A", "B"), BCA=(None, "A", "B"),
                      CAB=("A", "A", "C"), CBA=("A", "A", "C"))),
    # best is the first of A and B, second the other one, in another octave: accepted; C never enters
    "20_20_21": (dict(A=(20, 0), B=(20, 1), C=(21, 0)),
                 dict(ABC=("A", "A", "B"), ACB=("A", "A", "B"), BAC=("B", "B", "A"), BCA=("B", "B", "A"),
                      CAB=("A", "A", "B"), CBA=("B", "B", "A"))),
    "10_10_30": (dict(A=(10, 0), B=(10, 1), C=(30, 1)),
                 dict(ABC=("A", "A", "B"), ACB=("A", "A", "B"), BAC=("B", "B", "A"), BCA=("B", "B", "A"),
                      CAB=("A", "A", "B"), CBA=("B", "B", "A"))),
}
# index triples by the positions (in index order) of best and second for "best and second in one lane"
PAIR_LANE = {(0, 1): (5, 69, 100), (0, 2): (5, 40, 133), (1, 2): (3, 5, 69)}
PLACEMENTS = ("three_lanes", "pair_one_lane", "all_one_lane", "across_stride")
# the lane each index is meant to fall into (the CPU test compares them with idx % 64)
LANES = {(5, 70, 135): (5, 6, 7), (5, 69, 133): (5, 5, 5), (63, 64, 65): (63, 0, 1), (5, 69, 100): (5, 5, 36), (5, 40, 133): (5, 40, 5),
         (3, 5, 69): (3, 5, 5)}


def scan_scenario(set_name, order, placement):
    cands, table = SCAN_SETS[set_name]
    winner, best, second = table[order]
    if placement == "three_lanes":
        idx = (5, 70, 135)
    elif placement == "all_one_lane":
        idx = (5, 69, 133)
    elif placement == "across_stride":
        idx = (63, 64, 65)
    else:
        idx = PAIR_LANE[tuple(sorted((order.index(best), order.index(second))))]
    sc = Scene(200 + sum(map(ord, set_name + order)), 140)
    q = sc.query(90.0, 100.0, 110.0, 100.0, level=1)
    at = 0
    for c, k, lane in zip(order, idx, LANES[idx]):
        dist, octave = cands[c]
        sc.put(k, 100.0, 100.0, 0.0, octave)
        sc.cand(q, k, dist, at, lane=lane)
        at += 40
    exp = (1, {idx[order.index(winner)]: q}) if winner else (0, {})
    s = WindowScenario(f"scan_{set_name}_{order}_{placement}", "src/LSDmatcher.cpp:97-136, :168-209", sc, {"map": exp, "last": exp})
    s.set_name, s.order, s.idx, s.table = set_name, order, idx, (winner, best, second)
    return s


def scan_scenarios():
    return [scan_scenario(n, o, p) for n in SCAN_SETS for o in SCAN_SETS[n][1] for p in PLACEMENTS]


def scan_thresholds(nnratio):
    """One candidate (bestDist2 = 256, bestLevel2 = -1: no ratio test, src/LSDmatcher.cpp:97-100), bestDist on TH_HIGH (:128
    `bestDist <= TH_HIGH`: 100 accepted, 101 rejected) and the ratio test on the float boundary of mfNNratio * bestDist2 (:130,
    float product, float comparison): for every pair (p, d2) with a float product equal to the integer p, bestDist = p - 1
    and p are accepted and p + 1 is rejected (pairs with p + 1 == d2 are left out: they would be a tie, not a ratio case).  Best and
    second share octave 1; the second comes first in index order.  No two candidates of a query are equally far here, so these
    scenarios - unlike the orderings above - have no tie for a wrong tie rule to misread; they hold the thresholds."""
    sc = Scene(300 + int(nnratio * 100), 140)
    exp = {}
    i = 0

    def one(d1, d2, keep):
        nonlocal i
        cx, cy = _centre(i)
        q = sc.query(cx - 10.0, cy, cx + 10.0, cy, level=1)
        if d2 is not None:
            sc.cand(q, sc.add(cx + 1.0, cy, 0.0, 1), d2, 128)
        k = sc.cand(q, sc.add(cx, cy, 0.0, 1), d1, 0)
        if keep:
            exp[k] = q
        i += 1

    one(60, None, True)
    one(TH_HIGH, None, True)
    one(TH_HIGH + 1, None, False)
    pairs = [p for p in ratio_boundary_pairs(nnratio)[0::2] if p[0] >= 2 and p[0] + 1 < p[1]]
    for p, d2 in pairs:
        one(p - 1, d2, True)
        one(p, d2, True)
        one(p + 1, d2, False)
    s = WindowScenario(f"scan_thresholds_{nnratio}", "src/LSDmatcher.cpp:97-100, :128-131", sc,
                       {"map": (len(exp), exp), "last": (len(exp), exp)}, nnratio=nnratio)
    s.pairs = pairs
    return s


# ---------------------------------------------------------------------------------------------------------------------
# 3. Claims

def claims():
    """src/LSDmatcher.cpp:105-107 / :176-178: a key line whose map line has observations is no candidate; any other claim is
    overwritten (:133 / :206) and nmatches counts every assignment.
    q0: key line 0 (distance 5) holds map line 77 with observations -> skipped, key line 1 (distance 40) is taken.
    q1 (no observations) takes key line 2 at 10; q2 sees the same line at 5 and overwrites it: nmatches counts both.
    q3: key line 3 holds map line 78 without observations on entry -> overwritten.
    q4: both its candidates (4, 5) are held with observations -> nothing.
    q5 (observations) takes key line 6 at 10; q6 prefers it too (5) but must take key line 7 at 30.
    q7 (observations) takes key line 8; q8 sees only that line -> nothing."""
    sc = Scene(400, 140)
    pre = np.full(140, -1, np.int32)
    obs = np.zeros(140, np.uint8)
    c = [_centre(i) for i in range(9)]

    def q_at(p, **kw):
        return sc.query(p[0] - 10.0, p[1], p[0] + 10.0, p[1], level=1, **kw)

    def k_at(p, octave):
        return sc.add(p[0], p[1], 0.0, octave)

    q0 = q_at(c[0]); sc.cand(q0, k_at(c[0], 0), 5, 0); sc.cand(q0, k_at(c[0], 1), 40, 100)
    pre[0], obs[0] = 77, 1
    q1 = q_at(c[1], obs=0); sc.cand(q1, k_at(c[1], 1), 10, 0)
    q2 = q_at(c[1], desc=Desc.flip(sc.q[q1]["desc"], 5, 0)); sc.named.append(Named(q2, 2, 5))
    q3 = q_at(c[3]); sc.cand(q3, k_at(c[3], 1), 10, 0)
    pre[3], obs[3] = 78, 0
    q4 = q_at(c[4]); sc.cand(q4, k_at(c[4], 0), 10, 0); sc.cand(q4, k_at(c[4], 1), 20, 100)
    pre[4], obs[4], pre[5], obs[5] = 80, 1, 81, 1
    q5 = q_at(c[5]); sc.cand(q5, k_at(c[5], 0), 10, 0)
    q6 = q_at(c[5], desc=Desc.flip(sc.q[q5]["desc"], 5, 0)); sc.named.append(Named(q6, 6, 5))
    sc.desc[sc.add(c[5][0], c[5][1], 0.0, 1)] = Desc.flip(sc.q[q6]["desc"], 30, 100); sc.named.append(Named(q6, 7, 30))
    q7 = q_at(c[7]); sc.cand(q7, k_at(c[7], 1), 10, 0)
    q8 = q_at(c[7], desc=Desc.flip(sc.q[q7]["desc"], 3, 200)); sc.named.append(Named(q8, 8, 13))
    exp = (7, {1: q0, 2: q2, 3: q3, 6: q5, 7: q6, 8: q7})
    return WindowScenario("claims", "src/LSDmatcher.cpp:105-107, :133-134, :176-178, :206-207", sc, {"map": exp, "last": exp},
                          pre=pre, cur_obs=obs)


CHAIN_N = 200


def claim_chain():
    """200 map lines on a row of 200 key lines 3 px apart, windows of radius 2.5 * 1.2 = 3: map line i sees key line i - 1
    at distance 10 and key line i at distance 20, in alternating octaves (no ratio test).  Every third map line (i % 3 == 2)
    has no observations, and key lines 19, 39, ... sit in octave 3, outside every window, so the chain restarts there.
    The sequential rule (src/LSDmatcher.cpp:105-107, :133): map line i takes key line i - 1 unless it is held by a line with
    observations (then its own key line i), and what it takes is held with its own observation flag.  An order-free
    "every map line takes its nearest" gives another answer wherever a line with observations holds its own key line."""
    n = CHAIN_N
    sc = Scene(500, n)
    m = sc.d.base()
    for i in range(n):
        x = 10.0 + 3.0 * i
        q = sc.query(x - 1.5 - 0.25, 100.0, x - 1.5 + 0.25, 100.0, level=1, desc=m, obs=0 if i % 3 == 2 else 1)
        own = Desc.flip(m, 20, (37 * i) % 200)
        sc.put(i, x, 100.0, 0.0, 3 if i % 20 == 19 else i % 2, own)
        sc.named.append(Named(q, i, 20))
        if i:
            sc.named.append(Named(q, i - 1, 10))
        m = Desc.flip(own, 10, (37 * i + 100) % 200 + 20)        # the next map line: 10 from this key line
    # the construction rule, spelled out
    holder = [-1] * n           # key line -> map line
    held_obs = [0] * n
    nm = 0
    for i in range(n):
        cand = []
        if i and sc.cur["octave"][i - 1] <= 2 and not (holder[i - 1] >= 0 and held_obs[i - 1]):
            cand.append(i - 1)                                   # distance 10: preferred
        if sc.cur["octave"][i] <= 2:
            cand.append(i)                                       # distance 20, never claimed before map line i
        if cand:
            holder[cand[0]], held_obs[cand[0]] = i, 0 if i % 3 == 2 else 1
            nm += 1
    exp = (nm, {k: h for k, h in enumerate(holder) if h >= 0})
    return WindowScenario("claim_chain", "src/LSDmatcher.cpp:105-107, :133-134", sc, {"map": exp, "last": exp}, r0=2.5)


# ---------------------------------------------------------------------------------------------------------------------
# 4. Projection gates, distance bands, cones and PredictScale

NEGATIVE_LEVEL_MAX = (1.0015, 1.75)        # mnMaxDistance values with PredictScale(1.2f * max) == -1


def on_max_band(mx):
    """dist == 1.2f * max, the far edge of the distance band (src/MapLine.cpp GetMaxDistanceInvariance)"""
    return float(F32(F32(1.2) * F32(mx)))


N_CENTRE = 8           # key lines 0 .. 7 at the principal point, octave = index, distance 30 - 2 * octave from the common descriptor


@dataclass
class FrustumScenario:
    """Map lines for Frame::isInFrustum(MapLine*, 0.5) (src/Frame.cc:660-727), LSDmatcher::Fuse (src/LSDmatcher.cpp:884-993, th = 5)
    and, for the subset `last`, SearchByProjection(Cur, Last) (:36-136, octave 0, th = 5).  in_view / level / fuse are stated by
    hand; level None = a distance ratio on an exact product of the scale table, compared with the oracle alone."""
    names: list
    lines: np.ndarray
    descs: np.ndarray
    in_view: list
    level: list
    fuse: list                   # key line, -1 (dropped), -2 (level outside the pyramid) or None (oracle alone)
    cur: np.ndarray
    cur_desc: np.ndarray
    last: list                   # indices into lines
    last_expect: tuple           # (nmatches, {key line: position in `last`})
    named: list
    uv: dict                     # name -> the projection the bound cases claim


def frustum():
    """Symmetric lines SP = (-a, 0, z), EP = (a, 0, z): OM = 0.5 (SP + EP) - Ow = (0, 0, z) and dist = z exactly.
    bands (src/Frame.cc:703-704, `dist < minDistance || dist > maxDistance` with 0.8f * min and 1.2f * max): 0.8f * 2.5f rounds
    to 2.0f and 1.2f * 2.5f to 3.0f, so z = 2 / z = 3 are on the bands and accepted; the next float outside is dropped.
    cone: viewCos = 1 / 2 equals the limit 0.5 (`viewCos < limit`, :716: accepted); Fuse's `OM.dot(pn) < 0.5 * dist` (:956) with
    normal (0, s, 0.5) is 1.0 < 1.0 (accepted); the float below 0.5 in the normal drops both.
    PredictScale (src/MapLine.cpp:381-390) does not clamp: ratios 1.2^(L - 0.5) give level L for L = 0, 1, 2, 7, 8, 9;
    isInFrustum hands the raw level back, the Fuse entry reports -2 for levels outside 0 .. 7.
    depth (:58): z < 0 at either end drops the line; z == 0 with X = Y = 0 does not: 1 / 0 = inf, fx * 0 * inf = NaN, and a NaN
    fails no bound (:65-77) and no window test (src/Frame.cc:795, :799), so every key line of the octave window is a candidate.
    bounds (:65-77, strict rejects): u == 0, u == 640, v == 0, v == 480 are accepted, the next float outside is dropped.
    level -1: ceil(log(ratio) / log(1.2f)) is negative only for ratio <= 1 / 1.2, and the band keeps dist <= 1.2f * max, so it
    comes out on the band alone: dist == 1.2f * max at the maxima of NEGATIVE_LEVEL_MAX, where the float quotient max / dist falls
    at or below 1 / 1.2f (at max = 2.5 it does not: band_max_on stays at level 0).  These are exact-ratio cases: the CPU test asserts
    that the oracle says -1 there; given that, the Fuse entries report -2 (mvScaleFactors[-1] is out of bounds, :963)."""
    d = Desc(600)
    D = d.base()
    s8 = scale_factors()
    names, recs, descs, in_view, level, fuse = [], [], [], [], [], []
    kl, kd, named, uv = [], [], [], {}
    for o in range(N_CENTRE):
        kl.append((CX, CY, 0.0, o)); kd.append(Desc.flip(D, 30 - 2 * o, 32 * o))

    def add(name, w, normal, dmin, dmax, iv, lv, fu, desc=D):
        names.append(name); recs.append((w, normal, dmin, dmax)); descs.append(desc)
        in_view.append(iv); level.append(lv); fuse.append(fu)

    def sym(z, a=0.125):
        return (-a, 0.0, z, a, 0.0, z)

    up = (0.0, 0.0, 1.0)
    l1 = F32(2.0 * 1.2 ** 0.5)
    add("band_min_on", sym(2.0), up, 2.5, l1, 1, 1, 1)
    add("band_min_below", sym(ulp_below(2.0)), up, 2.5, l1, 0, 0, -1)
    add("band_max_on", sym(3.0), up, 0.01, 2.5, 1, None, None)
    add("band_max_above", sym(ulp_above(3.0)), up, 0.01, 2.5, 0, 0, -1)
    for mx in NEGATIVE_LEVEL_MAX:
        add(f"level_neg_{mx}", sym(on_max_band(mx)), up, 0.01, mx, 1, None, -2)
    add("cone_on", sym(2.0), (0.0, 0.7, 0.5), 0.01, l1, 1, 1, 1)
    add("cone_below", sym(2.0), (0.0, 0.7, ulp_below(0.5)), 0.01, l1, 0, 0, -1)
    for L in (0, 1, 2, 7, 8, 9):
        add(f"level_{L}", sym(2.0), up, 0.01, F32(2.0 * 1.2 ** (L - 0.5)), 1, L, L if L < 8 else -2)
    for k in range(8):
        add(f"ratio_scale_{k}", sym(2.0), up, 0.01, F32(F32(2.0) * s8[k]), 1, None, None)
    add("depth_sp", (-0.125, 0.0, -1.0, 0.125, 0.0, 2.0), up, 0.01, 10.0, 0, 0, -1)
    add("depth_ep", (-0.125, 0.0, 2.0, 0.125, 0.0, -1.0), up, 0.01, 10.0, 0, 0, -1)
    last = [len(names) - 2, len(names) - 1]
    last_exp = {}

    # image bounds: z = 1, each case with its own key line (octave 0, angle 5: the slope test passes) at its midpoint
    def beyond(x, bound, sign, fxy, c):
        """the float nearest to x whose projection is the next float outside `bound`; below 0 the neighbours are subnormal and
        no projection reaches them: there it is the nearest projection the end point can produce, one ulp of the coordinate out"""
        want = np.nextafter(F32(bound), F32(sign * np.inf))
        while True:
            x = np.nextafter(F32(x), F32(sign * np.inf))
            p = F32(F32(F32(fxy) * x) * F32(1.0)) + F32(c)
            if p == want or (bound == 0.0 and p < 0):
                return float(x)
            assert sign * (float(p) - float(want)) < 0, "stepped over the neighbour of the bound"

    XL, XR, YT, YB = -0.625, 0.625, -0.46875, 0.46875
    bounds = [("u1_min_on", (XL, 0.125, -0.5, 0.125), True), ("u1_min_out", (beyond(XL, 0.0, -1, FX, CX), 0.125, -0.5, 0.125), False),
              ("u2_max_on", (0.5, 0.125, XR, 0.125), True), ("u2_max_out", (0.5, 0.125, beyond(XR, W, 1, FX, CX), 0.125), False),
              ("u1_max_on", (XR, -0.125, 0.5, -0.125), True), ("u1_max_out", (beyond(XR, W, 1, FX, CX), -0.125, 0.5, -0.125), False),
              ("v1_min_on", (0.125, YT, 0.25, -0.375), True), ("v1_min_out", (0.125, beyond(YT, 0.0, -1, FY, CY), 0.25, -0.375), False),
              ("v2_max_on", (-0.125, 0.375, -0.25, YB), True), ("v2_max_out", (-0.125, 0.375, -0.25, beyond(YB, H, 1, FY, CY)), False),
              ("v2_min_on", (-0.375, -0.375, -0.25, YT), True), ("v2_min_out", (-0.375, -0.375, -0.25, beyond(YT, 0.0, -1, FY, CY)), False)]
    for name, (xa, ya, xb, yb), keep in bounds:
        b = d.base()
        w = (xa, ya, 1.0, xb, yb, 1.0)
        dist = float(np.linalg.norm([0.5 * (xa + xb), 0.5 * (ya + yb), 1.0]))
        k = len(kl)
        kl.append((FX * 0.5 * (xa + xb) + CX, FY * 0.5 * (ya + yb) + CY, 5.0, 0)); kd.append(Desc.flip(b, 10))
        add(name, w, up, 0.01, F32(dist * 1.2 ** -0.5), 1 if keep else 0, 0, k if keep else -1, desc=b)
        named.append(Named(len(names) - 1, k, 10))
        uv[name] = (project(xa, ya, 1.0), project(xb, yb, 1.0))
        if keep:
            last_exp[k] = len(last)
        last.append(len(names) - 1)
    # zero depth comes last: it scans every key line, and the best of octaves 0 .. 1 is key line 1 (28 against 30)
    add("depth_zero", (0.0, 0.0, 0.0, 0.0, 0.0, 2.0), up, 0.01, F32(1.2 ** 0.5), 1, 1, 1)
    last_exp[1] = len(last)
    last.append(len(names) - 1)
    lines = np.zeros(len(recs), FRUSTUM_LINE_DTYPE)
    for i, r in enumerate(recs):
        lines[i] = r
    cur = np.zeros(len(kl), LINE_DTYPE)
    for i, r in enumerate(kl):
        cur[i] = r
    return FrustumScenario(names, lines, np.array(descs, np.uint8), in_view, level, fuse, cur, np.array(kd, np.uint8), last,
                           (len(last_exp), last_exp), named, uv)


def frustum_map_lines(f):
    m = np.zeros(len(f.last), MAPLINE_DTYPE)
    for i, k in enumerate(f.last):
        m[i] = (1, 0, 1, 0, f.lines["world"][k], f.descs[k])
    return m


# ---------------------------------------------------------------------------------------------------------------------
# 5. Fuse: first strict minimum in index order, skipped lines

FUSE_TIES = [((5, 69), (5, 5), 5), ((69, 70), (5, 6), 69), ((5, 69, 133), (5, 5, 5), 5)]       # indices, their lanes, the winner


def fuse_ties():
    """src/LSDmatcher.cpp:985-989 (`dist<bestDist` in vIndices order): of equal distances the lowest index wins - in one lane
    (5, 69, 133), in neighbouring indices of different lanes (69, 70) - also against key line 137, which ties with them.  The third
    line is one bit away from the first: the tied key lines are at 21 and key line 137 at 19 wins at the highest index.
    A skipped line (!pML || isBad(), :906) returns -1."""
    out = []
    for idxs, lanes, win in FUSE_TIES:
        sc = Scene(700 + sum(idxs), 140)
        q = sc.query(90.0, 100.0, 110.0, 100.0, level=0)
        q2 = sc.query(90.0, 100.0, 110.0, 100.0, level=0, valid=0, desc=sc.q[q]["desc"])
        q3 = sc.query(90.0, 100.0, 110.0, 100.0, level=0, desc=Desc.flip(sc.q[q]["desc"], 1, 250))
        for j, (k, lane) in enumerate(zip(idxs, lanes)):
            sc.put(k, 100.0, 100.0, 0.0, 0)
            sc.cand(q, k, 20, 40 * j, lane=lane)
            sc.named.append(Named(q3, k, 21))
        sc.put(137, 100.0, 100.0, 0.0, 0)
        sc.cand(q3, 137, 19, 200)
        sc.named.append(Named(q, 137, 20))
        s = WindowScenario("fuse_tie_" + "_".join(map(str, idxs)), "src/LSDmatcher.cpp:906, :985-989", sc,
                           {"fuse": {q: (win, 20), q2: (-1, 0), q3: (137, 19)}})
        out.append(s)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 6. SearchByProjection(pKF, Scw, vpLines, vpMatched, th)

@dataclass
class KfScenario:
    scene: Scene
    matched: np.ndarray
    expect: tuple                # (nmatches, {key line: map line})
    ref: str = "src/LSDmatcher.cpp:399-499"

    def expected(self):
        new = np.full(len(self.scene.cur), -1, np.int32)
        for k, q in self.expect[1].items():
            new[k] = q
        return self.expect[0], new


def kf_first_come():
    """`bestDist<=TH_LOW` (:494): 50 accepted, 51 rejected.  First come, first served (:475-476, :496): q2 takes key line 2
    (10); q3 prefers it (12) and takes key line 3 (32) instead; q4 takes key line 4, q5 prefers it and its second best sits in
    octave 2, outside 0 .. 1 (:480): nothing; q6 / q7 the same with the second best outside the radius.  Key line 8 is matched on
    entry (vpMatched[idx], :475): q8 takes key line 9 at 40 although key line 8 is at 5.  q9 is offered twice (q10): the first takes
    key line 10, the second key line 11.  q11 lies on the far edge of its distance band, where PredictScale gives -1 (see
    frustum()): the reference would read mvScaleFactors[-1] (:461); the line is dropped although key line 12 is at 5 in octave 0."""
    sc = Scene(800, 70)
    matched = np.zeros(70, np.uint8)
    c = [_centre(i) for i in range(8)]

    def q_at(p, **kw):
        return sc.query(p[0] - 10.0, p[1], p[0] + 10.0, p[1], level=1, **kw)

    q0 = q_at(c[0]); sc.cand(q0, sc.add(*c[0], 0.0, 1), TH_LOW)
    q1 = q_at(c[1]); sc.cand(q1, sc.add(*c[1], 0.0, 1), TH_LOW + 1)
    for j, (octave, dx) in enumerate(((1, 0.0), (2, 0.0), (1, 7.0))):
        p = c[2 + j]
        qa = q_at(p)
        sc.cand(qa, sc.add(*p, 0.0, 0), 10, 0)
        k2 = sc.cand(qa, sc.add(p[0] + dx, p[1], 0.0, octave), 30, 100, radius=dx == 0.0)
        qb = q_at(p, desc=Desc.flip(sc.q[qa]["desc"], 2, 200))
        sc.named += [Named(qb, k2 - 1, 12), Named(qb, k2, 32, radius=dx == 0.0)]
    q8 = q_at(c[5]); sc.cand(q8, sc.add(*c[5], 0.0, 1), 5, 0); sc.cand(q8, sc.add(*c[5], 0.0, 1), 40, 100)
    matched[8] = 1
    q9 = q_at(c[6]); sc.cand(q9, sc.add(*c[6], 0.0, 1), 10, 0); sc.cand(q9, sc.add(*c[6], 0.0, 0), 20, 100)
    q10 = q_at(c[6], desc=sc.q[q9]["desc"]); sc.named += [Named(q10, 10, 10), Named(q10, 11, 20)]
    z = on_max_band(NEGATIVE_LEVEL_MAX[0])
    q11 = sc.query(CX - 10.0, CY, CX + 10.0, CY, level=0, z=(z, z))
    sc.q[q11]["dmax"] = F32(NEGATIVE_LEVEL_MAX[0])
    sc.cand(q11, sc.add(CX, CY, 0.0, 0), 5)
    exp = (8, {0: q0, 2: 2, 3: 3, 4: 4, 6: 6, 9: q8, 10: q9, 11: q10})
    return KfScenario(sc, matched, exp)


# ---------------------------------------------------------------------------------------------------------------------
# 7. SearchBySim3

@dataclass
class Sim3Scenario:
    """Both keyframes at the identity pose, s12 = 1, R12 = I, t12 = 0: a map line of either projects into the other where it
    projects in its own.  Key line i of a keyframe carries map line i (lines / descs / skip)."""
    kl1: np.ndarray
    kd1: np.ndarray
    lines1: np.ndarray
    descs1: np.ndarray
    skip1: np.ndarray
    kl2: np.ndarray
    kd2: np.ndarray
    lines2: np.ndarray
    descs2: np.ndarray
    skip2: np.ndarray
    expect: tuple                # (nFound, {i1: i2})
    named: list                  # (direction, map line, key line of the other keyframe, distance)
    names: list
    ref: str = "src/LSDmatcher.cpp:504-748, src/KeyFrame.cc:783-786"

    def expected(self):
        m = np.full(len(self.kl1), -1, np.int32)
        for a, b in self.expect[1].items():
            m[a] = b
        return self.expect[0], m


def sim3_pairs():
    """Pair p is key line p of KF1 and key line p of KF2 (KF1 has one extra key line, 'rival', next to pair 1).
    agree: 1 -> 2 finds it at 10, 2 -> 1 at 12: kept (:712-727).
    rival: 2 -> 1 sees KF1's line 1 at 21 and the rival (which carries no map line) at 20: the pair is dropped.
    skip1 / skip2: the line is skipped on one side (:553, :644): dropped.
    th_high / th_high_1: `bestDist<=TH_HIGH` (:633): 100 kept, 101 dropped.
    u_max: an end point projects to u == 640 = mnMaxX exactly; KeyFrame::IsInImage is x >= min && x < max (src/KeyFrame.cc:785): outside,
    dropped (the 2 -> 1 line is a shorter segment that is inside and does find its partner).  u_min: u == 0 is inside: kept.
    band_on / band_below: the midpoint in the other camera is (0, 0, z) with z = 2 = 0.8f * 2.5f (`dist3D < minDistance`, :595: kept)
    and the float below (dropped).
    level_neg: the midpoint is on the far edge of the band, where PredictScale gives -1 (see frustum()): mvScaleFactors[-1] (:603), dropped."""
    d = Desc(900)
    cases = ["agree", "rival", "skip1", "skip2", "th_high", "th_high_1", "u_max", "u_min", "band_on", "band_below", "level_neg"]
    n = len(cases)
    kl1, kl2 = np.zeros(n + 1, LINE_DTYPE), np.zeros(n, LINE_DTYPE)
    kd1, kd2 = np.zeros((n + 1, 32), np.uint8), np.zeros((n, 32), np.uint8)
    l1, l2 = np.zeros(n + 1, FRUSTUM_LINE_DTYPE), np.zeros(n, FRUSTUM_LINE_DTYPE)
    ds1, ds2 = np.zeros((n + 1, 32), np.uint8), np.zeros((n, 32), np.uint8)
    skip1, skip2 = np.zeros(n + 1, np.uint8), np.zeros(n, np.uint8)
    named, exp = [], {}

    def line(w, dmin=0.01, dmax=None):
        w = np.array(w, np.float64)
        dist = np.linalg.norm(0.5 * (w[:3] + w[3:]))
        return (w, (0.0, 0.0, 1.0), dmin, F32(dist * 1.2 ** -0.5) if dmax is None else dmax)     # level 0: octave 0 key lines only

    for p, name in enumerate(cases):
        cx, cy = _centre(p + 11)                                             # second lattice row, away from the borders
        w = ((cx - 10.0 - CX) / FX, (cy - CY) / FY, 1.0, (cx + 10.0 - CX) / FX, (cy - CY) / FY, 1.0)
        wa = wb = w
        mid = (cx, cy)
        dmin, dmax = 0.01, None
        if name == "u_max":
            wa = (0.5, -0.25, 1.0, 0.625, -0.25, 1.0)                        # 576 .. 640
            wb = (0.5, -0.25, 1.0, 0.6171875, -0.25, 1.0)                    # 576 .. 636: inside
            mid = (607.0, 112.0)
        elif name == "u_min":
            wa = wb = (-0.625, -0.25, 1.0, -0.5, -0.25, 1.0)                 # 0 .. 64
            mid = (32.0, 112.0)
        elif name in ("band_on", "band_below"):
            z = 2.0 if name == "band_on" else ulp_below(2.0)
            a = 0.125 if name == "band_on" else 0.0625                       # two windows around the principal point: the key
            wa = wb = (-a, 0.0, z, a, 0.0, z)                                # lines are told apart by their descriptors
            mid, dmin = (CX, CY), 2.5
        elif name == "level_neg":
            z = on_max_band(NEGATIVE_LEVEL_MAX[1])
            wa = wb = (-0.09375, 0.0, z, 0.09375, 0.0, z)
            mid, dmax = (CX, CY), F32(NEGATIVE_LEVEL_MAX[1])
        b1, b2 = d.base(), d.base()                                          # descriptors of the two map lines
        d12, d21 = (TH_HIGH, 12) if name == "th_high" else (TH_HIGH + 1, 12) if name == "th_high_1" else (10, 21 if name == "rival" else 12)
        kl1[p], kl2[p] = (mid[0], mid[1], 0.0, 0), (mid[0], mid[1], 0.0, 0)
        kd2[p] = Desc.flip(b1, d12)                                          # what map line p of KF1 finds in KF2
        kd1[p] = Desc.flip(b2, d21)                                          # what map line p of KF2 finds in KF1
        l1[p], l2[p], ds1[p], ds2[p] = line(wa, dmin, dmax), line(wb, dmin, dmax), b1, b2
        named += [("12", p, p, d12), ("21", p, p, d21)]
        if name == "rival":
            kl1[n] = (mid[0] + 1.0, mid[1], 0.0, 0)
            kd1[n] = Desc.flip(b2, 20, 100)
            l1[n], skip1[n] = line(w), 1
            named.append(("21", p, n, 20))
        skip1[p], skip2[p] = name == "skip1", name == "skip2"
        if name in ("agree", "th_high", "u_min", "band_on"):
            exp[p] = p
    return Sim3Scenario(kl1, kd1, l1, ds1, skip1, kl2, kd2, l2, ds2, skip2, (len(exp), exp), named, cases)


def sim3_args(s):
    """(T1w, T2w, s12, R12, t12), (the ten per-keyframe arrays) in the order both SearchBySim3 entries take them"""
    I = np.eye(4, dtype=np.float32)
    return (I, I, 1.0, np.eye(3, dtype=np.float32), np.zeros(3, np.float32)), \
           (s.lines1, s.descs1, s.skip1, s.kl1, s.kd1, s.lines2, s.descs2, s.skip2, s.kl2, s.kd2)


# ---------------------------------------------------------------------------------------------------------------------
# 8. Descriptor matchers on the 2-NN lists of cv::BFMatcher

def _knn_sets(seed, rows):
    """rows: per query (d0, d1) -> queries, train rows (2 per query: 2q at d0, 2q + 1 at d1, disjoint flips)"""
    d = Desc(seed)
    Q, T = [], []
    for d0, d1 in rows:
        b = d.base()
        Q.append(b); T.append(Desc.flip(b, d0, 0)); T.append(Desc.flip(b, d1, 128))
    return np.array(Q, np.uint8), np.array(T, np.uint8)


def ratio_rule():
    """SearchByDescriptor(KeyFrame*, Frame&), src/LSDmatcher.cpp:257-276: `distance[0] / distance[1] < 1.0f / 1.5f` in float.
    2/3, 20/30 and 40/60 round to the bound itself (rejected), 19/30 is below it, 0/0 (two identical train rows) is NaN
    (rejected), 0/7 accepted.  Query 6 passes the ratio but its key line has no map line (:270).  Queries 7 and 8 both have
    train row 14 as their nearest: the later query holds the row (:272) and nmatches counts both.
    -> (queries, train rows, has_line, nmatches, out[train row])"""
    rows = [(2, 3), (20, 30), (40, 60), (19, 30), (0, 0), (0, 7), (5, 40), (2, 42)]
    Q, T = _knn_sets(1000, rows)
    Q = np.concatenate([Q, Desc.flip(T[14], 3, 60)[None]])          # query 8: 3 from train row 14, 3 + 2 + 42 from row 15
    has = np.ones(9, np.uint8)
    has[6] = 0
    out = np.full(16, -1, np.int32)
    out[6], out[10], out[14] = 3, 5, 8
    return Q, T, has, 4, out, rows + [(3, 47)]


def gap_rule(n):
    """SearchByDescriptor(KeyFrame*, KeyFrame*) / SerachForInitialize (src/LSDmatcher.cpp:224-238, :295-311) and
    SearchForTriangulation (:346-364) with Frame::lineDescriptorMAD (src/Frame.cc:575-583): the gap median is element n / 2 of
    the DESCENDING order (conpare_descriptor_by_NN12_dist), the deviations are sorted ascending, MAD = 1.4826 * element n / 2;
    a gap is accepted when it exceeds 0.5 * MAD (0.1 * MAD for triangulation), strictly.
    n = 1: MAD 0, gap 7 accepted.  n = 2: gaps (10, 2): median 2, deviations (0, 8), MAD 11.86: 10 > 5.93 accepted, 2 not;
    triangulation 1.19: both.  n = 4: gaps (1, 10, 22, 60): descending median 10, deviations (0, 9, 12, 50), element 2 = 12,
    MAD 17.79: 0.5 * MAD = 8.90 accepts 10, 22, 60 (an ascending median, 22, gives 15.57 and rejects the 10); 0.1 * MAD = 1.78
    accepts the same.  n = 5: gaps (1, 10, 22, 60, 3): median 10, deviations (0, 7, 9, 12, 50), MAD 13.34: 6.67 accepts 10, 22, 60;
    1.33 accepts the 3 as well.
    -> (queries, train rows, gaps, accepted by 0.5, accepted by 0.1)"""
    gaps, half, tenth = {1: ((7,), (1,), (1,)), 2: ((10, 2), (1, 0), (1, 1)), 4: ((1, 10, 22, 60), (0, 1, 1, 1), (0, 1, 1, 1)),
                         5: ((1, 10, 22, 60, 3), (0, 1, 1, 1, 0), (0, 1, 1, 1, 1))}[n]
    Q, T = _knn_sets(1100 + n, [(5, 5 + g) for g in gaps])
    return Q, T, gaps, half, tenth


def gap_expected(n, accepted, has_train=None):
    """(nmatches, out[query] = train row) of the gap matchers: query q's nearest train row is 2q; it is taken when the hand-stated
    flag says so and (has_train given) that row carries a map line"""
    out = np.full(n, -1, np.int32)
    for q, a in enumerate(accepted):
        if a and (has_train is None or has_train[2 * q]):
            out[q] = 2 * q
    return int((out >= 0).sum()), out


def gap_rule_equal(gap):
    """All gaps equal: MAD = 0, the threshold is 0 and the test is a strict `>`: gap 0 (a 2-NN tie, which BFMatcher lists in
    ascending train order) is rejected, any positive gap accepted.  -> (queries, train rows)"""
    return _knn_sets(1200 + gap, [(5, 5 + gap)] * 3)


# ---------------------------------------------------------------------------------------------------------------------
# 9. Sizes

def sized(n_cur):
    """n_cur key lines, one query whose only candidate is the last one (distance 10)."""
    sc = Scene(1300 + n_cur, n_cur)
    q = sc.query(90.0, 100.0, 110.0, 100.0, level=0)
    sc.put(n_cur - 1, 100.0, 100.0, 0.0, 0)
    sc.cand(q, n_cur - 1, 10)
    exp = (1, {n_cur - 1: q})
    return WindowScenario(f"size_{n_cur}", "src/LSDmatcher.cpp:103, :174", sc, {"map": exp, "last": exp, "fuse": {q: (n_cur - 1, 10)}})


SIZES = (1, 64, 65, 4096)
