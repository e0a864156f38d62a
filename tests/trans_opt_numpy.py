"""An independent restatement of Optimizer::TranslationOptimization (reference src/Optimizer.cc:3211-3980) in float64 Python /
numpy, written from the reference text in the order DESIGN.md section 21 reads it.  What g2o runs under it (chi2, Huber,
constructQuadraticForm, the 6x6 LDLT, the Levenberg step control, SE3Quat::exp) is tests/pose_opt_numpy.py's; stated here are the
up-front float rotation of the map geometry, the *OnlyTranslation edges (errors and Jacobians) and the outer loop with its own
counting.  Plus the scene lists.  Used by tests/test_trans_opt_cpu.py and tests/test_gpu_trans_opt.py."""
import math

import numpy as np

import pose_opt_numpy as pon
from pose_opt_numpy import D, F, MATCHED, PARALLEL, VERTICAL, frame, pack, tables_equal  # noqa: F401


# ------------------------------------------------------------------------------------------------------------------------------
# the rotation, once, in float
def gemm_rotate(R, x):
    """cv::Mat Xc = R_cw * Xw through gemm's small-matrix path: a float dot left to right, then (float)(t * 1 + 0 * 0) in double.
    R [3, 3] float32, x [n, 3] float32 -> [n, 3] float64 (`e->Xc[k] = Xc.at<float>(k)`)"""
    R, x = np.asarray(R, F), np.asarray(x, F).reshape(-1, 3)
    out = np.zeros((len(x), 3), D)
    with np.errstate(all="ignore"):
        for r in range(3):
            t = (R[r, 0] * x[:, 0] + R[r, 1] * x[:, 1]) + R[r, 2] * x[:, 2]
            assert t.dtype == F
            out[:, r] = (t.astype(D) * 1.0 + 0.0 * 0.0).astype(F).astype(D)
    return out


def rotate_normal(R, plane):
    """Plane3D::rotateNormal(Converter::toMatrix3d(R_cw)): the floats widened, a double product on the normal; d untouched"""
    Rd = [[float(R[r, c]) for c in range(3)] for r in range(3)]
    n = [Rd[r][0] * plane[0] + Rd[r][1] * plane[1] + Rd[r][2] * plane[2] for r in range(3)]
    return n + [plane[3]]


def plane_error(kind, meas, Xc, t):
    """computeError of EdgePlaneOnlyTranslation (3), EdgeParallelPlaneOnlyTranslation (4), EdgeVerticalPlaneOnlyTranslation (5):
    localPlane = w2n + Xc (Plane3D.h:204-212), then ominus / ominus_par / ominus_ver of the measurement"""
    l = list(Xc[:3])
    l.append(Xc[3] - (t[0] * l[0] + t[1] * l[1] + t[2] * l[2]))
    if l[3] < 0.0:
        l = [-v for v in l]
    l = pon.plane_normalize(l)
    if kind == 3:
        return pon.angles_in_frame(l[:3], meas[:3]) + [(-l[3]) - (-meas[3])]
    if kind == 4:
        nor = l[:3]
        if meas[0] * nor[0] + meas[1] * nor[1] + meas[2] * nor[2] < 0:
            nor = [-v for v in nor]
        return pon.angles_in_frame(nor, meas[:3]) + [0.0]
    a, m = l[:3], meas[:3]
    v = [a[1] * m[2] - a[2] * m[1], a[2] * m[0] - a[0] * m[2], a[0] * m[1] - a[1] * m[0]]
    nv = pon._sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    ax = [pon._div(c, nv) for c in v]
    sn, c = pon.cr_sincos(math.pi / 2)              # AngleAxisd(M_PI / 2, v / |v|).toRotationMatrix()
    sa = [sn * k for k in ax]
    ca = [(1.0 - c) * k for k in ax]
    A = [[0.0] * 3 for _ in range(3)]
    tmp = ca[0] * ax[1]
    A[0][1], A[1][0] = tmp - sa[2], tmp + sa[2]
    tmp = ca[0] * ax[2]
    A[0][2], A[2][0] = tmp + sa[1], tmp - sa[1]
    tmp = ca[1] * ax[2]
    A[1][2], A[2][1] = tmp - sa[0], tmp + sa[0]
    for k in range(3):
        A[k][k] = ca[k] * ax[k] + c
    b = [A[i][0] * a[0] + A[i][1] * a[1] + A[i][2] * a[2] for i in range(3)]
    return pon.angles_in_frame(b, m) + [0.0]


def plane_jacobian(kind, meas, Xc, q, t):
    """BaseUnaryEdge::linearizeOplus() over all six dimensions, then columns 0..2 overwritten with 0: only the perturbations of
    dimensions 3..5 reach the result"""
    delta = 1e-9
    scalar = 1.0 / (2 * delta)
    J = np.zeros((3, 6))
    for d in range(3, 6):
        u = [0.0] * 6
        u[d] = delta
        _, pt, _ = pon.oplus(q, t, u)
        e1 = plane_error(kind, meas, Xc, pt)
        u[d] = -delta
        _, pt, _ = pon.oplus(q, t, u)
        e2 = plane_error(kind, meas, Xc, pt)
        for r in range(3):
            J[r, d] = scalar * (e1[r] - e2[r])
    return J


class TransGraph(pon.Graph):
    """The edges of one frame: measurements, information, deltas and thresholds as PoseOptimization's graph sets them (they are
    the same text, :3248-3249, :3449-3461, :3687-3688), the geometry rotated up front, the translation-only errors and Jacobians"""

    def __init__(self, fr):
        super().__init__(fr)
        R = np.asarray(fr["Tcw"], F).reshape(4, 4)[:3, :3]
        n_pts, n_lines = self.n_pts, self.n_lines
        if n_pts:
            self.X[:n_pts, :3] = gemm_rotate(R, np.asarray(fr["Xw"], F).reshape(-1, 3))
        if n_lines:
            le = np.asarray(fr["line_ends"], D).reshape(-1, 3)      # start, end, start, end ..: the edge order
            with np.errstate(all="ignore"):
                self.X[n_pts:n_pts + 2 * n_lines, :3] = gemm_rotate(R, le.astype(F))    # Converter::toCvVec
        for j in range(n_pts + 2 * n_lines, self.n):
            self.X[j] = rotate_normal(R, list(self.X[j]))

    def errors(self, idx, q, t):
        with np.errstate(all="ignore"):
            e = np.zeros((len(idx), 3))
            k = self.kind[idx]
            cam = k < 3
            if cam.any():
                ii = idx[cam]
                p = [self.X[ii, c] + t[c] for c in range(3)]            # estimate().mapTrans(Xc)
                kk = k[cam]
                m = self.meas[ii]
                r0 = (p[0] / p[2]) * self.fx + self.cx
                r1 = (p[1] / p[2]) * self.fy + self.cy
                invz = (1.0 / p[2]).astype(F).astype(D)                 # const float invz = 1.0f / trans_xyz[2]
                s0 = (p[0] * invz) * self.fx + self.cx
                s1 = (p[1] * invz) * self.fy + self.cy
                s2 = s0 - self.bf * invz
                ec = np.zeros((len(ii), 3))
                mono, st, ln = kk == 0, kk == 1, kk == 2
                ec[mono, 0] = (m[:, 0] - r0)[mono]
                ec[mono, 1] = (m[:, 1] - r1)[mono]
                ec[st, 0] = (m[:, 0] - s0)[st]
                ec[st, 1] = (m[:, 1] - s1)[st]
                ec[st, 2] = (m[:, 2] - s2)[st]
                ec[ln, 0] = ((m[:, 0] * r0 + m[:, 1] * r1) + m[:, 2])[ln]
                e[cam] = ec
            for j in np.nonzero(~cam)[0]:
                i = idx[j]
                e[j] = plane_error(int(self.kind[i]), list(self.meas[i]), list(self.X[i]), t)
            return e

    def jacobians(self, idx, q, t):
        with np.errstate(all="ignore"):
            J = np.zeros((len(idx), 3, 6))
            k = self.kind[idx]
            cam = k < 3
            if cam.any():
                ii = idx[cam]
                x, y, z = (self.X[ii, c] + t[c] for c in range(3))
                invz = 1.0 / z
                invz_2 = invz * invz
                fx, fy, bf = self.fx, self.fy, self.bf
                Jc = np.zeros((len(ii), 3, 6))
                Jc[:, 0, 3] = -invz * fx
                Jc[:, 0, 5] = x * invz_2 * fx
                Jc[:, 1, 4] = -invz * fy
                Jc[:, 1, 5] = y * invz_2 * fy
                st = k[cam] == 1
                Jc[st, 2, 3] = Jc[st, 0, 3]
                Jc[st, 2, 5] = (Jc[:, 0, 5] - bf * invz_2)[st]
                ln = k[cam] == 2
                if ln.any():
                    lx, ly = self.meas[ii, 0], self.meas[ii, 1]
                    L = np.zeros((len(ii), 3, 6))
                    L[:, 0, 3] = fx * lx * invz
                    L[:, 0, 4] = fy * ly * invz
                    L[:, 0, 5] = -(fx * lx * x + fy * ly * y) * invz_2
                    Jc[ln] = L[ln]
                J[cam] = Jc
            for j in np.nonzero(~cam)[0]:
                i = idx[j]
                J[j] = plane_jacobian(int(self.kind[i]), list(self.meas[i]), list(self.X[i]), q, t)
            return J


class TransOptimizer(pon.Optimizer):
    """optimize() is SparseOptimizer::optimize with Levenberg as pose_opt_numpy states it; run() is this function's outer loop"""

    def __init__(self, fr):
        self.fr = fr
        self.g = TransGraph(fr)
        self.x = [0.0] * 6
        self.iterations = self.trials = self.rejected = self.nbad_stops = self.small = self.big = 0
        self.last_rejected = False
        self.robust = True

    def run(self):
        fr, g = self.fr, self.g
        n_slots = g.n_slots
        out = dict(Tcw=np.asarray(fr["Tcw"], F).reshape(16).copy(), returns=0, rounds=0, iterations=0, trials=0,
                   diag=np.zeros(8, np.int32), point_outlier=np.zeros(g.n_pts, np.uint8),
                   line_outlier=np.zeros(g.n_lines, np.uint8), plane_outlier=np.zeros(n_slots, np.uint8),
                   par_plane_outlier=np.zeros(n_slots, np.uint8), ver_plane_outlier=np.zeros(n_slots, np.uint8))
        n_initial = g.n_pts                        # nInitialCorrespondences counts points only
        if n_initial < 3:                          # after the point and line loops, before the plane loop
            return out
        n_bad = 0
        last_rejected_rounds = empty_rounds = 0
        points = np.arange(g.n_pts, dtype=np.int64)
        lines = np.arange(g.n_pts, g.n_pts + 2 * g.n_lines, dtype=np.int64)
        planes = np.arange(g.n_pts + 2 * g.n_lines, g.n, dtype=np.int64)
        for it in range(4):
            q, t = pon.to_se3quat(fr["Tcw"])
            self.last_rejected = False
            if g.level.all():
                empty_rounds += 1
            q, t = self.optimize(q, t)
            out["rounds"] += 1
            last_rejected_rounds += self.last_rejected
            n_bad = 0
            with np.errstate(all="ignore"):
                # mono and stereo points, then the planes: an outlier's error is computed again, an inlier's is what the last
                # computeActiveErrors left
                for idx in (points, planes):
                    redo = idx[g.level[idx]]
                    if len(redo):
                        g.err[redo] = g.errors(redo, q, t)
                    chi2 = g.chi2(idx, g.err[idx]).astype(F)
                    g.level[idx] = chi2.astype(D) > g.th[idx]
                    n_bad += int(g.level[idx].sum())
                # the lines: both ends again only when the line is an outlier; nLineBad is not returned
                redo = lines[g.level[lines]]
                if len(redo):
                    g.err[redo] = g.errors(redo, q, t)
                if len(lines):
                    c = (g.err[lines, 0] * g.err[lines, 0]).astype(F).astype(D) > g.th[lines]
                    g.level[lines] = np.repeat(c[0::2] | c[1::2], 2)
            if it == 2:
                self.robust = False
            if g.n < 10:                           # optimizer.edges().size(): a line is two, par / ver edges only with bStruct
                break
        R = pon.quat_matrix(q)
        T = np.zeros((4, 4), F)
        with np.errstate(all="ignore"):
            for r in range(3):
                for c in range(3):
                    T[r, c] = F(R[r][c])
                T[r, 3] = F(t[r])
        T[3, 3] = 1
        out["Tcw"] = T.reshape(16)
        out["returns"] = n_initial - n_bad
        out["iterations"], out["trials"] = self.iterations, self.trials
        out["diag"][:6] = (self.rejected, last_rejected_rounds, self.nbad_stops, self.small, self.big, empty_rounds)
        out["point_outlier"][:] = g.level[:g.n_pts]
        out["line_outlier"][:] = g.level[g.n_pts:g.n_pts + 2 * g.n_lines:2]
        keys = ("plane_outlier", "par_plane_outlier", "ver_plane_outlier")
        for j, (ps, slot) in enumerate(g.plane_slot):
            out[keys[ps]][slot] = g.level[g.n_pts + 2 * g.n_lines + j]
        return out


def translation_optimization(fr):
    """Optimizer::TranslationOptimization of one frame (a dict as frame() makes it): the outputs of drfe_pose_opt_out for it"""
    return TransOptimizer(fr).run()


def table(frames):
    """the outputs of a call over these frames, concatenated as lib.trans_opt_host lays them out"""
    outs = [translation_optimization(fr) for fr in frames]
    r = {}
    for k in ("Tcw", "diag"):
        r[k] = np.stack([o[k] for o in outs]) if outs else np.zeros((0, 16 if k == "Tcw" else 8), F if k == "Tcw" else np.int32)
    for k in ("returns", "rounds", "iterations", "trials"):
        r[k] = np.array([o[k] for o in outs], np.int32)
    for k in ("point_outlier", "line_outlier", "plane_outlier", "par_plane_outlier", "ver_plane_outlier"):
        r[k] = np.concatenate([o[k] for o in outs]) if outs else np.zeros(0, np.uint8)
    return r


_TABLES = {}


def numpy_table(name, frames):
    """table(frames), computed once per process under `name`"""
    if name not in _TABLES:
        _TABLES[name] = table(frames)
    return _TABLES[name]


# ------------------------------------------------------------------------------------------------------------------------------
# scenes: pose_opt_numpy.frame with start_rot = 0, so that the start rotation is the planted one
# the kernel's boundaries (dr_slam_amd/csrc/trans_opt_internal.h)
TO_THREADS, TO_PLANE_GROUP, TO_WAVE = 256, 32, 64


def tframe(rng, *a, **kw):
    kw.setdefault("start_rot", 0.0)
    return frame(rng, *a, **kw)


def behaviour_frames():
    """Named finite frames that take the paths DESIGN.md section 21 lists; tests assert through the diagnostics that they do"""
    rng = np.random.default_rng(3024)
    fr = {}
    # every point an outlier after round one: rounds two to four have no active edge
    fr["all_outliers"] = tframe(np.random.default_rng(1), 12, outlier_frac=1.0, mode="stereo", outlier_px=(150, 300))
    # plain frames: rejected trials, a round whose last trial is rejected, the _nBad >= 3 stop
    fr["points"] = tframe(rng, 60, outlier_frac=0.2)
    fr["stereo_lines"] = tframe(rng, 40, 5, mode="stereo")
    fr["struct"] = tframe(rng, 30, 3, planes=(MATCHED, MATCHED | PARALLEL | VERTICAL, MATCHED | PARALLEL), b_struct=1)
    fr["far_start"] = tframe(rng, 50, 4, start_trans=0.4, outlier_frac=0.3)
    f = tframe(rng, 20, identity=True)
    f["Xw"][1] = (0.1, -0.2, -2.0)                  # Zc + t_z < 0: finite everywhere
    fr["zc_negative"] = f
    # a wrong start rotation: the function leaves the rotation alone
    fr["wrong_rotation"] = frame(rng, 60, 4, planes=(MATCHED,), start_rot=0.02)
    return fr


def nonfinite_frames():
    """Zc + t_z == 0 exactly on a mono and on a stereo edge under the start pose (the identity): inf and NaN flow through, the
    rotation rows of H and b are no longer zero, and the device hands the frame back"""
    rng = np.random.default_rng(3025)
    fr = {}
    for name, ur in (("zc_zero_mono", -1.0), ("zc_zero_stereo", 300.0)):
        f = tframe(rng, 20, identity=True)
        f["Xw"][0] = (0.3, 0.2, 0.0)
        f["u_right"][0] = ur
        fr[name] = f
    return fr


def counting_frames():
    """The counting rules of :3420 and :3969-3979"""
    rng = np.random.default_rng(3026)
    fr = {"0": tframe(rng, 0), "2": tframe(rng, 2), "3": tframe(rng, 3),
          "2_points_5_lines_3_planes": tframe(rng, 2, 5, planes=(MATCHED,) * 3),
          "3_points_3_lines": tframe(rng, 3, 3), "4_points_3_lines": tframe(rng, 4, 3)}
    # three inlier points, four plane edges planted as outliers: the return value is negative
    f = tframe(rng, 3, 0, planes=(MATCHED | PARALLEL, MATCHED | VERTICAL), b_struct=1, noise=0.1, start_trans=0.0)
    f["plane_meas"][:, :3] = f["plane_meas"][:, [1, 2, 0]] * np.array([1, -1, 1], F)
    f["plane_meas"][:, 3] += 3.0
    fr["negative_return"] = f
    # lines that are all outliers: the same number as without them
    f = tframe(rng, 30, 4, noise=0.3)
    g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f.items()}
    f["line_fn"][:, 2] += 400.0
    g["line_fn"], g["line_ends"] = np.zeros((0, 3)), np.zeros((0, 6))
    fr["lines_all_outliers"], fr["lines_removed"] = f, g
    return fr


def size_frames():
    """Edge counts one below, at and one above the kernel's boundaries: the point / line edges of a pass (TO_THREADS), the plane
    edges of a pass (TO_PLANE_GROUP) and a wavefront (TO_WAVE)"""
    rng = np.random.default_rng(3077)
    fr = {"9": tframe(rng, 9), "10": tframe(rng, 10)}
    for n in (TO_WAVE - 1, TO_WAVE, TO_WAVE + 1, TO_THREADS - 1, TO_THREADS, TO_THREADS + 1):
        fr[str(n)] = tframe(rng, n, outlier_frac=0.1)
    fr["250+2x4"] = tframe(rng, TO_THREADS - 6, 4)
    for n in (TO_PLANE_GROUP - 1, TO_PLANE_GROUP, TO_PLANE_GROUP + 1):
        fr[f"{n}_planes"] = tframe(rng, 20, 0, planes=(MATCHED,) * (n - 2) + (MATCHED | PARALLEL,), b_struct=1)
    return fr


def mix_frames():
    """pose_opt_numpy.mix_frames' mixes: mono / stereo / alternating, 0 / 1 / 33 lines, 0 / 1 / 3 plane slots with each map plane
    alone and together, bStruct on and off (off ignores the parallel and vertical inputs)"""
    rng = np.random.default_rng(3078)
    fr = {}
    for mode in ("mono", "stereo", "alternate"):
        fr[mode] = tframe(rng, 40, mode=mode, outlier_frac=0.1)
    for nl in (1, 33):
        fr[f"{nl}_lines"] = tframe(rng, 30, nl)
    for bs in (0, 1):
        for name, planes in (("m", (MATCHED,)), ("p", (PARALLEL,)), ("v", (VERTICAL,)), ("mpv", (MATCHED | PARALLEL | VERTICAL,)),
                             ("3slots", (MATCHED, PARALLEL | VERTICAL, MATCHED | VERTICAL))):
            fr[f"planes_{name}_struct{bs}"] = tframe(rng, 12, 2, planes=planes, b_struct=bs)
    return fr


def random_frames(n=20, seed=3099):
    """n random frames of at most 200 edges"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nl = int(rng.integers(0, 12))
        planes = tuple(int(v) for v in rng.integers(1, 8, int(rng.integers(0, 4))))
        npts = int(rng.integers(3, 200 - 2 * nl - 3 * len(planes)))
        out.append(tframe(rng, npts, nl, planes=planes, b_struct=int(rng.integers(0, 2)),
                          mode=("mono", "stereo", "alternate")[int(rng.integers(0, 3))], outlier_frac=float(rng.uniform(0, 0.3))))
    return out


def planted_frame():
    """150 points, 6 lines, 20 % gross outliers, the start translation 0.05 off"""
    return tframe(np.random.default_rng(3150), 150, 6, outlier_frac=0.2, start_trans=0.05)


def caller_frames():
    rng = np.random.default_rng(3041)
    return [tframe(rng, 40, 3, planes=(MATCHED | PARALLEL, MATCHED | VERTICAL), b_struct=1, outlier_frac=0.2), tframe(rng, 25, 0, mode="mono"),
            tframe(rng, 2, 4, planes=(MATCHED,)), tframe(rng, 30, 4, planes=(7,), b_struct=0, mode="stereo")]
