"""Independent numpy restatement of the reference's plane association, written from the reference text
in explicit float32 steps, for the bit-exact tests of drfe_plane_match_host / drfe_plane_flag_points_host /
drfe_plane_match_status_host and the device batch:

- PlaneMatcher::SearchMapByCoefficients        src/PlaneMatcher.cpp:11-91
- PlaneMatcher::PointDistanceFromPlane         src/PlaneMatcher.cpp:206-226
- PlaneMatcher::bMatchStatus                   src/PlaneMatcher.cpp:94-201
- Map::FlagMatchedPlanePoints                  src/Map.cc:406-431
- Frame::ComputePlaneWorldCoeff(_MF)           src/Frame.cc:1311-1328

Map planes are indexed in vpMapPlanes order; -1 stands for a null MapPlane*."""
import numpy as np

f32 = np.float32
DEFAULTS = (f32(0.1), f32(0.86), f32(0.08716), f32(0.9962))    # PlaneMatcher(float dTh, aTh, verTh, parTh) defaults


def world_coef(Tcw, coef, Rwc_MF=None):
    """cv::transpose(mTcw, temp) (top-left 3x3 replaced by Rwc_MF for the _MF form), then temp * coef: gemm's small-matrix
    path, float products summed left to right, then + 0"""
    T = np.asarray(Tcw, f32).reshape(4, 4).T.copy()
    if Rwc_MF is not None:
        T[:3, :3] = np.asarray(Rwc_MF, f32).reshape(3, 3)
    c = np.asarray(coef, f32).reshape(4)
    out = np.zeros(4, f32)
    for r in range(4):
        acc = T[r, 0] * c[0]
        for k in range(1, 4):
            acc = f32(acc + T[r, k] * c[k])
        out[r] = f32(acc + f32(0.0))
    return out


def angle_of(pM, pW):
    pW = np.asarray(pW, f32)
    return f32(f32(pM[0] * pW[0] + pM[1] * pW[1]) + pM[2] * pW[2])


def point_distance_from_plane(pM, cloud):
    """res = 100 (double); for every point with z != 0: dis = abs(float expr) widened, res = dis if dis < res"""
    cloud = np.asarray(cloud, f32).reshape(-1, 3)
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        dis = np.abs(((pM[0] * x + pM[1] * y) + pM[2] * z) + pM[3]).astype(np.float64)
        keep = (z != 0) & (dis < 100.0)
    return float(dis[keep].min()) if keep.any() else 100.0


def search_map_by_coefficients(Tcw, coefs, map_coefs, map_bad, clouds, map_idx=None, par_idx=None, ver_idx=None,
                               params=DEFAULTS):
    """-> (mvpMapPlanes, mvpParallelPlanes, mvpVerticalPlanes as index arrays, nmatches); the priors are kept where nothing
    new is written (the reference does not reset the vectors)"""
    dTh, aTh, verTh, parTh = (f32(v) for v in params)
    coefs = np.asarray(coefs, f32).reshape(-1, 4)
    P = len(coefs)
    mi = np.full(P, -1, np.int32) if map_idx is None else np.array(map_idx, np.int32)
    pi = np.full(P, -1, np.int32) if par_idx is None else np.array(par_idx, np.int32)
    vi = np.full(P, -1, np.int32) if ver_idx is None else np.array(ver_idx, np.int32)
    nmatches = 0
    for i in range(P):
        pM = world_coef(Tcw, coefs[i])
        ldTh, lverTh, lparTh = dTh, verTh, parTh
        found = False
        for j in range(len(map_coefs)):
            if map_bad[j]:
                continue
            angle = angle_of(pM, map_coefs[j])
            if angle > aTh or angle < -aTh:
                dis = point_distance_from_plane(pM, clouds[j])
                if dis < float(ldTh):
                    ldTh = f32(dis)
                    mi[i] = j
                    found = True
                    continue
            if angle > lparTh or angle < -lparTh:
                lparTh = f32(abs(angle))
                pi[i] = j
                continue
            if angle < lverTh and angle > -lverTh:
                lverTh = f32(abs(angle))
                vi[i] = j
                continue
        if found:
            nmatches += 1
    return mi, pi, vi, nmatches


def flag_matched_plane_points(Tcw, coefs, map_idx, points, flags=None):
    """-> (flags OR-ed, nMatches); the hard-coded 0.5, dTh unused; isBad() of the matched plane not read"""
    points = np.asarray(points, f32).reshape(-1, 3)
    fl = np.zeros(len(points), np.uint8) if flags is None else np.array(flags, np.uint8)
    n = 0
    coefs = np.asarray(coefs, f32).reshape(-1, 4)
    for i in range(len(coefs)):
        if map_idx[i] < 0:
            continue
        pM = world_coef(Tcw, coefs[i])
        x, y, z = points[:, 0], points[:, 1], points[:, 2]
        with np.errstate(invalid="ignore", over="ignore"):
            dis = np.abs(((pM[0] * x + pM[1] * y) + pM[2] * z) + pM[3]).astype(np.float64)
            hit = dis < 0.5
        fl[hit] = 1
        n += int(hit.sum())
    return fl, n


def match_status(Tcw, coefs, matched_coefs, matched, mf_contrast, Rwc_MF=None):
    """bMatchStatus; angle_MF (uninitialised in the reference without MF_contrast) canonicalised to 0"""
    coefs = np.asarray(coefs, f32).reshape(-1, 4)
    if len(coefs) < 2:
        return True
    for i in range(len(coefs)):
        if not matched[i]:
            continue
        angle = angle_of(world_coef(Tcw, coefs[i]), matched_coefs[i])
        angle_mf = angle_of(world_coef(Tcw, coefs[i], Rwc_MF), matched_coefs[i]) if mf_contrast else f32(0.0)
        a, m = float(abs(angle)), float(abs(angle_mf))
        if a < m - 0.0005 and a > m - 0.05:
            return False
    return True


def random_scene(seed, n_map=24, n_planes=6, cloud=300, n_points=2000, special=True):
    """A test scene, not part of the restatement: a Manhattan-ish map (world planes of three axes, noisy normals, clouds on
    and near them, a few bad planes) and a frame observing some of them from a random pose; clouds carry z == 0, -0.0 and
    NaN points when `special`."""
    rng = np.random.default_rng(seed)
    axes = np.eye(3)
    map_coefs, clouds = [], []
    for j in range(n_map):
        n = axes[rng.integers(3)] + rng.normal(0, 0.03 if j % 3 else 0.2, 3)
        n /= np.linalg.norm(n)
        if rng.random() < 0.3:
            n = -n
        d = rng.uniform(-3, 3)
        map_coefs.append(np.r_[n, d])
        m = int(rng.integers(0, cloud)) if j % 7 else 0
        u = np.cross(n, [0.3, 0.5, 0.8]); u /= np.linalg.norm(u)
        v = np.cross(n, u)
        pts = (-d * n)[None] + rng.uniform(-2, 2, (m, 1)) * u + rng.uniform(-2, 2, (m, 1)) * v
        pts += n[None] * rng.normal(0, 0.04, (m, 1)) + n[None] * rng.choice([0.0, 0.0, 0.07, 0.15, 0.5], size=(m, 1))
        pts = pts.astype(f32)
        if special and m > 4:
            pts[0, 2] = 0.0
            pts[1, 2] = -0.0
            pts[2, 2] = np.nan
            pts[3, 0] = np.nan
        clouds.append(pts)
    map_coefs = np.asarray(map_coefs, f32)
    bad = (rng.random(n_map) < 0.15).astype(np.uint8)
    a = rng.normal(0, 0.2, 3)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    Tcw = np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = R, rng.normal(0, 1, 3)
    Tcw = Tcw.astype(f32)
    coefs = []
    for i in range(n_planes):
        w = map_coefs[rng.integers(n_map)].astype(np.float64).copy()
        w[:3] += rng.normal(0, 0.02, 3)
        w[3] += rng.normal(0, 0.08)
        c = np.linalg.inv(Tcw.astype(np.float64)).T @ w      # pM = Tcw^T c
        coefs.append(c)
    coefs = np.asarray(coefs, f32)
    pts = rng.uniform(-4, 4, (n_points, 3)).astype(f32)
    return Tcw, coefs, map_coefs, bad, clouds, pts
