"""Hand-built scenes that put map-point and map-line triangulation on its decision points: each
threshold one float step either side of where its decision flips (5.991 / 7.8 sigma^2, 0.9998, cosParallaxRays > 0, the two
ratio tests), equal stereo cosines, z == 0, w == 0, dist == 0, a rank-deficient A, KF2's residual with KF1's mbf,
UnprojectStereo on the distorted keys, the line idx2 quirk in and out of range, the baseline skip at equality.

The builders make one-pair scenes (two keyframes, one match); find_flip() locates a gate's flip by bisection on the float's bit
pattern with the numpy restatement (tests/triangulate_numpy.py) alone; ladder() returns the scenes around it; cases() lists every
hand-built case with the outcome stated by hand from the reference source; merge() concatenates one-pair scenes into one call
with one pair per scene, so that KF1 is rarely keyframe 0 and every offset is non-zero.  Nothing here calls the library's
triangulation entries: tests/test_triangulate_cpu.py holds the host to these cases, tests/test_gpu_triangulate_edges.py the
device."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulate_numpy as TN  # noqa: E402

f32, F = np.float32, np.float32
P, L = TN.P_CODES, TN.L_CODES
POINT_FEATS = ("un", "raw", "octave", "u_right", "depth")
LINE_FEATS = ("ends", "octave", "depth", "lines3d")


# --- builders ----------------------------------------------------------------------------------------------------------------

def pt_scene(kfs, feats1, feats2, matches=((0, 0),), n_levels=8):
    """two keyframes (records), their keypoint lists (dicts of un, raw, octave, u_right, depth), one pair"""
    sc, sg = TN.scale_tables(n_levels)
    f = [dict(un=np.array([k["un"] for k in fs], f32), raw=np.array([k.get("raw", k["un"]) for k in fs], f32),
              octave=np.array([k.get("octave", 0) for k in fs], np.int32), u_right=np.array([k.get("u_right", -1.0) for k in fs], f32),
              depth=np.array([k.get("depth", -1.0) for k in fs], f32)) for fs in (feats1, feats2)]
    s = dict(kf=np.array(kfs), scale_factors=np.tile(sc, (2, 1)), level_sigma2=np.tile(sg, (2, 1)),
             offsets=np.int32([0, len(feats1), len(feats1) + len(feats2)]), kf1=np.int32([0]), kf2=np.int32([1]),
             match_offsets=np.int32([0, len(matches)]), matches=np.int32(matches).reshape(-1, 2))
    for key in f[0]:
        s[key] = np.concatenate([f[0][key], f[1][key]])
    return s


def proj(kf, X):
    T = kf["Tcw"].reshape(3, 4).astype(np.float64)
    x = T[:, :3] @ np.asarray(X, np.float64) + T[:, 3]
    return [kf["fx"] * x[0] / x[2] + kf["cx"], kf["fy"] * x[1] / x[2] + kf["cy"]], x[2]


def two(X=(0.2, 0.1, 2.0), t2=(-0.3, 0.0, 0.0), st1=False, st2=False, R2=None, Ow2=None):
    """KF1 at the origin, KF2 at pose (R2, t2) (its centre input Ow2 if given: the baseline test reads it), a point X seen by
    both; the keypoints are its projections"""
    k1 = TN.keyframe(np.eye(3), np.zeros(3))
    k2 = TN.keyframe(np.eye(3) if R2 is None else R2, np.array(t2), Ow=Ow2)
    u1, z1 = proj(k1, X)
    u2, z2 = proj(k2, X)
    p1 = dict(un=u1, u_right=u1[0] - 40.0 / z1 if st1 else -1.0, depth=z1 if st1 else -1.0)
    p2 = dict(un=u2, u_right=u2[0] - 40.0 / z2 if st2 else -1.0, depth=z2 if st2 else -1.0)
    return k1, k2, p1, p2


def line_scene(d1, d2, n1=2, n2=3, idx2=1):
    """KF1 with n1 key lines, KF2 with n2; one match (0, idx2); depth lines d1 (KF1's, per line), d2 (KF2's)"""
    k1 = TN.keyframe(np.eye(3), np.zeros(3))
    k2 = TN.keyframe(np.eye(3), np.array([-0.3, 0.0, 0.0]))
    A, B = np.array([0.1, 0.0, 2.0]), np.array([0.3, 0.2, 2.2])
    ends, l3 = [], []
    for kf in (k1, k2):
        T = kf["Tcw"].reshape(3, 4).astype(np.float64)
        a, b = T[:, :3] @ A + T[:, 3], T[:, :3] @ B + T[:, 3]
        ends.append([kf["fx"] * a[0] / a[2] + kf["cx"], kf["fy"] * a[1] / a[2] + kf["cy"], kf["fx"] * b[0] / b[2] + kf["cx"],
                     kf["fy"] * b[1] / b[2] + kf["cy"]])
        l3.append(np.concatenate([a, b]))
    sc, sg = TN.scale_tables()
    s = dict(kf=np.array([k1, k2]), scale_factors=np.tile(sc, (2, 1)), level_sigma2=np.tile(sg, (2, 1)),
             offsets=np.int32([0, n1, n1 + n2]), ends=np.array([ends[0]] * n1 + [ends[1]] * n2, f32),
             octave=np.zeros(n1 + n2, np.int32), depth=np.array(list(d1) + list(d2), f32),
             lines3d=np.array([l3[0]] * n1 + [l3[1]] * n2, np.float64), kf1=np.int32([0]), kf2=np.int32([1]),
             match_offsets=np.int32([0, 1]), matches=np.int32([[0, idx2]]))
    return s


def bits_of(v):
    return int(np.float32(v).view(np.int32))


def float_of(bits):
    return np.int32(bits).view(np.float32)


def find_flip(make, lo, hi, decide):
    """the bit pattern of the least float32 v in [lo, hi] (positive, by bit pattern) with decide(status of make(v)) !=
    decide(at lo), by the numpy restatement alone; also returns decide(at lo)"""
    a, b = bits_of(lo), bits_of(hi)
    d0 = decide(TN.triangulate(make(F(lo)))["status"][0])
    assert decide(TN.triangulate(make(F(hi)))["status"][0]) != d0
    while b - a > 1:
        m = (a + b) // 2
        if decide(TN.triangulate(make(float_of(m)))["status"][0]) == d0:
            a = m
        else:
            b = m
    return b, d0


# --- the gates found by bisection: name -> (make, lo, hi, decide) --------------------------------------------------------------

def _reproj_gate(stereo):
    """5.991 sigma^2 (mono) / 7.8 sigma^2 (stereo), compared in double: KF1's level sigma^2"""
    k1, k2, p1, p2 = two(st1=stereo)
    p1["un"] = [p1["un"][0] + 0.8, p1["un"][1] - 0.5]
    if stereo:
        p1["u_right"] += 0.6

    def make(s2):
        s = pt_scene([k1, k2], [p1], [p2])
        s["level_sigma2"] = s["level_sigma2"].copy()
        s["level_sigma2"][0, 0] = s2
        return s
    return make, 1e-4, 4.0, lambda st: st == P["reproj1"]


def _parallax_gate():
    """cosParallaxRays < 0.9998 (a double) for two monocular keypoints: KF2 moved along x"""
    X = (0.0, 0.0, 3.0)

    def make(tx):
        k1, k2, p1, p2 = two(X=X, t2=(-float(tx), 0.0, 0.0))
        k2["Ow"] = np.float32([1.0, 0.0, 0.0])        # keep the pair (the baseline test reads Ow)
        return pt_scene([k1, k2], [p1], [p2])
    return make, 0.01, 0.2, lambda st: st == P["no_parallax"]


R_ALONG_X = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], np.float64)       # camera z = world x


def _equal_cos_gate():
    """cosParallaxStereo1 == cosParallaxStereo2 (= cosParallaxRays + 1, rays just past perpendicular): KF1's depth"""
    k1, k2, _, _ = two(R2=R_ALONG_X, t2=(0.0, 0.0, 1.0))
    p2 = dict(un=[float(k2["cx"]) + 0.05, float(k2["cy"])])

    def make(d):
        p1 = dict(un=[float(k1["cx"]), 260.0], u_right=100.0, depth=d)
        return pt_scene([k1, k2], [p1], [p2])
    return make, 0.5, 2000.0, lambda st: st == P["no_parallax"]


def ratio_make():
    """the ratio tests: KF1's keypoint at octave 1, KF2's at 0, KF1's scale factor of level 1 the variable; returns
    (make, k1, k2)"""
    k1, k2, p1, p2 = two()
    p1["octave"], p2["octave"] = 1, 0

    def make(sc):
        s = pt_scene([k1, k2], [p1], [p2])
        s["scale_factors"] = s["scale_factors"].copy()
        s["scale_factors"][0, 1] = sc
        return s
    return make, k1, k2


def _ratio_gate(above):
    """ratioDist * ratioFactor < ratioOctave flips as KF1's scale grows; ratioDist > ratioOctave * ratioFactor as it shrinks
    (the variable is then the reciprocal of the scale)"""
    make = ratio_make()[0]
    if above:
        return make, 1.2, 50.0, lambda st: st == P["scale"]
    return (lambda v: make(F(1.0) / v)), F(1.0) / F(1.2), 50.0, lambda st: st == P["scale"]


def _baseline_make():
    k1, k2, p1, p2 = two()

    def make(mb):
        k = k2.copy()
        k["mb"] = mb
        return pt_scene([k1, k], [p1], [p2])
    return make, TN._dist(k2["Ow"], k1["Ow"])


GATES = dict(reproj_mono=lambda: _reproj_gate(False), reproj_stereo=lambda: _reproj_gate(True), parallax_09998=_parallax_gate,
             equal_stereo_cosines=_equal_cos_gate, ratio_above=lambda: _ratio_gate(True), ratio_below=lambda: _ratio_gate(False))
LADDERS = tuple(GATES) + ("baseline_mb",)


@functools.lru_cache(maxsize=None)
def flip_of(name):
    """(make, bit pattern of the flip, the decision below it) of a gate; the baseline's flip is one step above the distance
    between the centres (a pair is skipped if the baseline is < mb)"""
    if name == "baseline_mb":
        make, base = _baseline_make()
        return make, bits_of(base) + 1, False
    make, lo, hi, decide = GATES[name]()
    b, d0 = find_flip(make, lo, hi, decide)
    return make, b, d0


def ladder(name, steps=8):
    """the 2 * steps + 1 one-pair scenes from `steps` ulp below a gate's flip to `steps` ulp above it"""
    make, b, _ = flip_of(name)
    return [make(float_of(b + k)) for k in range(-steps, steps + 1)]


# --- the fixed cases ------------------------------------------------------------------------------------------------------------

def cos_rays_scenes():
    """cosParallaxRays > 0: KF2 looks along world x, so KF1's keypoint at cx gives perpendicular rays (cos == 0 exactly); one
    scene each for du = -0.25, 0, 0.25"""
    k1, k2, _, _ = two(R2=R_ALONG_X, t2=(0.0, 0.0, 1.0))
    p2 = dict(un=[float(k2["cx"]), float(k2["cy"])])
    return [pt_scene([k1, k2], [dict(un=[float(k1["cx"]) + du, 260.0])], [p2]) for du in (-0.25, 0.0, 0.25)]


def ratio_equality_scene():
    """equality of the first test: ratioOctave == ratioDist * ratioFactor exactly is kept (strict <); returns (scene, X)"""
    make, k1, k2 = ratio_make()
    X = np.float32([0.2, 0.1, 2.0])
    d1 = TN._dist(X, k1["Ow"])
    d2 = TN._dist(X, k2["Ow"])
    rd = F(d2 / d1)
    prod = F(rd * F(F(1.5) * F(1.2)))
    return make(prod), X


def _low_parallax_stereo1():
    return two(X=(0.2, 0.1, 30.0), t2=(-0.01, 0.0, 0.0), st1=True, Ow2=(1.0, 0.0, 0.0))


def z_zero_scene():
    """z1 == 0: the stereo point lands on KF1's plane (Twc and Tcw are independent inputs); low parallax: stereo 1"""
    k1, k2, p1, p2 = _low_parallax_stereo1()
    k1["Tcw"] = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -p1["depth"]])
    return pt_scene([k1, k2], [p1], [p2])


def w_zero_scene():
    """w == 0: keypoints at the principal point, A's third column zero and its fourth orthogonal to the rest"""
    k1 = TN.keyframe(np.eye(3), np.array([0.5, 0.25, 0.0]))
    k2 = TN.keyframe(np.eye(3), np.array([-0.5, -0.25, 0.0]))
    k2["Tcw"] = np.float32([1, 0, 0, -0.5, 0, 1, 0, -0.25, 0.1, 0, 1, 0])
    pc = dict(un=[float(k1["cx"]), float(k1["cy"])])
    return pt_scene([k1, k2], [pc], [pc])


def rank_deficient_scene():
    """rank-deficient A with w != 0: KF2's first two rows equal KF1's (rows 2, 3 of A repeat rows 0, 1)"""
    k1 = TN.keyframe(np.eye(3), np.array([0.1, 0.0, 0.5]))
    k2 = TN.keyframe(np.eye(3), np.array([-0.2, 0.0, 0.5]))
    k2["Tcw"] = np.concatenate([k1["Tcw"][:8], np.float32([0.3, 0, 1, 0.5])])
    pa = dict(un=[300.0, 200.0])
    return pt_scene([k1, k2], [pa], [pa])


def dist_zero_scene():
    """dist == 0: KF1's centre (GetCameraCenter, an input of its own) on the unprojected point"""
    k1, k2, p1, p2 = _low_parallax_stereo1()
    s = pt_scene([k1, k2], [p1], [p2])
    X = TN._twc(k1["Twc"], [F(F((F(p1["un"][0]) - k1["cx"]) * F(p1["depth"])) * k1["invfx"]),
                            F(F((F(p1["un"][1]) - k1["cy"]) * F(p1["depth"])) * k1["invfy"]), F(p1["depth"])])
    s["kf"] = s["kf"].copy()
    s["kf"][0]["Ow"] = np.float32(X)
    s["kf"][1]["Ow"] = np.float32([5.0, 0.0, 0.0])
    return s


def kf2_residual_scenes():
    """KF2's stereo residual is computed with KF1's mbf: the scene with equal mbf (accepted) and with KF1's doubled (KF2's own
    stays 40: its residual is now off by 40 / z)"""
    k1, k2, p1, p2 = two(st2=True)
    ok = pt_scene([k1, k2], [p1], [p2])
    k1["mbf"] = F(80.0)
    return ok, pt_scene([k1, k2], [p1], [p2])


def distorted_keys_scenes():
    """UnprojectStereo reads the distorted keys: returns (k1, p1, the scene with raw != un, the scene with raw = un)"""
    k1, k2, p1, p2 = _low_parallax_stereo1()
    p1["raw"] = [p1["un"][0] + 0.5, p1["un"][1] - 0.25]
    return k1, p1, pt_scene([k1, k2], [p1], [p2]), pt_scene([k1, k2], [dict(p1, raw=p1["un"])], [p2])


def line_idx2_scenes():
    """bStereo2 is read from KF1's line idx2: in range with and without depth, and past KF1's lines"""
    return [line_scene([-1.0, 2.0], [2.0, -1.0, -1.0], idx2=1),      # KF1's line idx2 has depth, KF2's has none: stereo 2
            line_scene([-1.0, -1.0], [2.0, 2.0, 2.0], idx2=1),       # KF1's line idx2 without depth, KF2's with: no line
            line_scene([-1.0, 2.0], [2.0, 2.0, 2.0], idx2=2),        # idx2 past KF1's lines: bStereo2 false, flagged
            line_scene([2.0, -1.0], [2.0, 2.0, 2.0], idx2=2)]


def line_gate_scenes():
    """sp behind KF2, ep behind KF2, KF1's centre on the line's end"""
    out = []
    for tz in (2.0, 2.1):
        s = line_scene([2.0, 2.0], [2.0, 2.0, 2.0], idx2=0)
        s["kf"] = s["kf"].copy()
        s["kf"][1]["Tcw"] = np.float32([1, 0, 0, 0.3, 0, 1, 0, 0, 0, 0, -1, tz])     # KF2 looks back
        out.append(s)
    s = line_scene([2.0, 2.0], [2.0, 2.0, 2.0], idx2=0)
    s["kf"] = s["kf"].copy()
    s["kf"][0]["Ow"] = np.float32(TN._twc(s["kf"][0]["Twc"], [F(v) for v in s["lines3d"][0, 3:]]))
    out.append(s)
    return out


def baseline_scenes():
    """mb equal to the distance between the centres (kept) and one step above it (skipped)"""
    make, base = _baseline_make()
    return make(base), make(np.nextafter(base, F(1)))


def cases():
    """every hand-built case as (name, scene, line, expectation); an expectation is a dict over the one match / pair of the
    scene: status, status_not, status_in, branch, pair_skipped, accepted (see holds())"""
    out = []

    def add(name, scene, line=False, **expect):
        out.append((name, scene, line, expect))
    for name in GATES:
        make, b, _ = flip_of(name)
        lo, at, hi = (make(float_of(b + k)) for k in (-1, 0, 1))
        if name.startswith("reproj"):
            e = (dict(status=P["reproj1"]), dict(status_not=P["reproj1"]))
        elif name == "parallax_09998":
            e = (dict(status=P["no_parallax"], branch=0), dict(status_not=P["no_parallax"], branch=1))
        elif name == "equal_stereo_cosines":
            e = (dict(status_not=P["no_parallax"], branch=2), dict(status=P["no_parallax"]))
        else:
            e = (dict(status_not=P["scale"]), dict(status=P["scale"]))
        add(name + "_below", lo, **e[0])
        add(name + "_at", at, **e[1])
        add(name + "_above", hi)
    for du, s in zip(("minus", "zero", "plus"), cos_rays_scenes()):
        add("cos_rays_" + du, s, **(dict(branch=0) if du == "zero" else {}))
    add("ratio_plain", ratio_make()[0](F(1.2)), status=0)
    add("ratio_equality", ratio_equality_scene()[0], status_in=(0, P["scale"]))
    add("z1_zero", z_zero_scene(), status=P["z1"], branch=2)
    add("w_zero", w_zero_scene(), status=P["w_zero"], branch=1)
    add("rank_deficient", rank_deficient_scene(), status_not=P["w_zero"], branch=1)
    add("dist_zero", dist_zero_scene(), status=P["dist"], branch=2)
    ok, off = kf2_residual_scenes()
    add("kf2_residual_own_mbf", ok, status=0)
    add("kf2_residual_kf1_mbf", off, status=P["reproj2"])
    _, _, s, s2 = distorted_keys_scenes()
    add("distorted_keys", s, branch=2)
    add("distorted_keys_raw_is_un", s2, branch=2)
    q = line_idx2_scenes()
    add("line_idx2_kf1_has_depth", q[0], True, status=0, branch=3)
    add("line_idx2_kf1_no_depth", q[1], True, status=L["no_stereo"])
    add("line_idx2_past_no_stereo", q[2], True, status=L["no_stereo"] | TN.PAST_KF1)
    add("line_idx2_past_stereo1", q[3], True, status=TN.PAST_KF1, branch=2, accepted=1)
    g = line_gate_scenes()
    add("line_sp_behind_kf2", g[0], True, status=L["z_sp2"])
    add("line_ep_behind_kf2", g[1], True, status=L["z_ep2"])
    add("line_dist_zero", g[2], True, status=L["dist"])
    eq, above = baseline_scenes()
    add("baseline_equal", eq, pair_skipped=0)
    add("baseline_one_step_above", above, pair_skipped=1, status=1)
    return out


def holds(expect, r, i=0):
    """asserts a case's expectation on match / pair i of a result"""
    for key, want in expect.items():
        if key == "status_not":
            assert r["status"][i] != want, (key, r["status"][i])
        elif key == "status_in":
            assert r["status"][i] in want, (key, r["status"][i])
        else:
            assert r[key][i] == want, (key, r[key][i])


def merge(scenes, line=False):
    """one call of len(scenes) pairs from one-pair scenes (all points or all lines, one number of levels): keyframes, their
    scale and sigma^2 tables and their features appended, keyframe indices and feature offsets shifted"""
    feats = LINE_FEATS if line else POINT_FEATS
    out = {k: [] for k in ("kf", "scale_factors", "level_sigma2", "kf1", "kf2", "matches") + feats}
    offsets, mo = [0], [0]
    nk = 0
    for s in scenes:
        assert len(s["kf1"]) == 1
        for k in ("kf", "scale_factors", "level_sigma2", "matches") + feats:
            out[k].append(np.asarray(s[k]))
        offsets += [offsets[-1] + int(o) for o in s["offsets"][1:]]
        out["kf1"].append(np.asarray(s["kf1"], np.int32) + nk)
        out["kf2"].append(np.asarray(s["kf2"], np.int32) + nk)
        mo.append(mo[-1] + int(s["match_offsets"][-1]))
        nk += len(s["kf"])
    r = {k: np.concatenate(v) for k, v in out.items()}
    r["matches"] = r["matches"].astype(np.int32).reshape(-1, 2)
    r["offsets"], r["match_offsets"] = np.int32(offsets), np.int32(mo)
    return r
