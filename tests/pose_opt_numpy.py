"""An independent restatement of Optimizer::PoseOptimization (reference src/Optimizer.cc:601-1338) and of what g2o and Eigen run
under it, in float64 Python / numpy, written from the reference text in the order DESIGN.md section 20 reads it: the point and line
edges element-wise over arrays of edges, every ordered sum a cumulative sum from +0.0 in active-edge order, the plane edges, the
6x6 LDLT, the Levenberg step control and SE3Quat::exp in Python scalars; sin / cos / atan2 / x^3 through mpmath rounded once.  Plus
a scene generator (a planted pose, noisy points with planted gross outliers, lines and planes consistent with the pose), pack()
and tables_equal().  Used by tests/test_pose_opt_cpu.py and tests/test_gpu_pose_opt.py."""
import math

import numpy as np

F = np.float32
D = np.float64
DBL_MAX = 1.7976931348623157e308
TABLE_KEYS = ("Tcw", "returns", "rounds", "iterations", "trials", "diag", "point_outlier", "line_outlier", "plane_outlier",
              "par_plane_outlier", "ver_plane_outlier")
SETTINGS = (0.5, 50.0, 0.1, 0.1, 100.0, 50.0, 0.0)     # Plane.AngleInfo DistanceInfo ParallelInfo VerticalInfo Chi VPChi (TUM3.yaml)
MATCHED, PARALLEL, VERTICAL = 1, 2, 4


# ------------------------------------------------------------------------------------------------------------------------------
# libm, correctly rounded
def _mp():
    import mpmath
    mpmath.mp.prec = 400
    return mpmath


def cr_sincos(t):
    t = float(t)
    if t != t or math.isinf(t):
        return math.nan, math.nan
    mp = _mp()
    return float(mp.sin(mp.mpf(t))), float(mp.cos(mp.mpf(t)))


def cr_atan2(y, x):
    y, x = float(y), float(x)
    if y != y or x != x:
        return math.nan
    if y == 0 or x == 0 or math.isinf(y) or math.isinf(x):
        return math.atan2(y, x)              # exact cases: 0, pi/4, pi/2, 3pi/4, pi as the nearest doubles, signed as y
    mp = _mp()
    return float(mp.atan2(mp.mpf(y), mp.mpf(x)))


def cr_cube(x):
    x = float(x)
    if x != x or math.isinf(x) or x == 0:
        return x * x * x
    mp = _mp()
    try:
        return float(mp.mpf(x) ** 3)
    except OverflowError:
        return math.copysign(math.inf, x)


def _sqrt(x):
    """IEEE sqrt: NaN below zero, no exception"""
    with np.errstate(all="ignore"):
        return float(np.sqrt(D(x)))


def _div(a, b):
    """IEEE division: no exception at zero"""
    with np.errstate(all="ignore"):
        return float(D(a) / D(b))


# ------------------------------------------------------------------------------------------------------------------------------
# Eigen's quaternion and g2o's SE3Quat, Python scalars; q = [x, y, z, w]
def quat_from_matrix(m):
    """Quaterniond(Matrix3d)"""
    q = [0.0] * 4
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0.0:
        t = _sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = _div(0.5, t)
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = _sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = _div(0.5, t)
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def normalize_rotation(q):
    """SE3Quat::normalizeRotation"""
    if q[3] < 0:
        q = [-c for c in q]
    z = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if z > 0:
        s = _sqrt(z)
        q = [_div(c, s) for c in q]
    return q


def quat_matrix(q):
    """Quaternion::toRotationMatrix"""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def quat_mul(a, b):
    """Eigen's generic quat_product"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def quat_rotate(q, v):
    """Quaternion::_transformVector; works on scalars and on arrays of vectors (v a list of three arrays)"""
    x, y, z, w = q
    uv = [y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]]
    uv = [c + c for c in uv]
    cr = [y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]]
    return [v[k] + w * uv[k] + cr[k] for k in range(3)]


def to_se3quat(Tcw):
    """Converter::toSE3Quat"""
    T = np.asarray(Tcw, F).reshape(4, 4).astype(D)
    q = normalize_rotation(quat_from_matrix([[float(T[r, c]) for c in range(3)] for r in range(3)]))
    return q, [float(T[0, 3]), float(T[1, 3]), float(T[2, 3])]


def se3_exp(u):
    """SE3Quat::exp: (q, t, theta < 1e-5)"""
    om, up = u[:3], u[3:]
    theta = _sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    Om2 = [[Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c] + Om[r][2] * Om[2][c] for c in range(3)] for r in range(3)]
    eye = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    small = theta < 0.00001
    if small:
        R = [[eye[r][c] + Om[r][c] + Om2[r][c] for c in range(3)] for r in range(3)]
        V = R
    else:
        sn, cs = cr_sincos(theta)
        a = _div(sn, theta)
        b = _div(1 - cs, theta * theta)
        c3 = _div(theta - sn, cr_cube(theta))
        R = [[eye[r][c] + a * Om[r][c] + b * Om2[r][c] for c in range(3)] for r in range(3)]
        V = [[eye[r][c] + b * Om[r][c] + c3 * Om2[r][c] for c in range(3)] for r in range(3)]
    t = [V[r][0] * up[0] + V[r][1] * up[1] + V[r][2] * up[2] for r in range(3)]
    return normalize_rotation(quat_from_matrix(R)), t, small


def oplus(q, t, u):
    """VertexSE3Expmap::oplusImpl: exp(u) * estimate"""
    eq, et, small = se3_exp(u)
    r = quat_rotate(eq, t)
    nt = [et[k] + r[k] for k in range(3)]
    return normalize_rotation(quat_mul(eq, q)), nt, small


# ------------------------------------------------------------------------------------------------------------------------------
# Plane3D and the three plane edges, Python scalars
def plane_normalize(c):
    n = _sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    inv = _div(1.0, n)
    c = [v * inv for v in c]
    if c[3] < 0.0:
        c = [-v for v in c]
    return c


def to_plane3d(coe):
    coe = np.asarray(coe, F)
    c = [float(v) for v in coe]
    if coe[3] < 0:
        c = [-v for v in c]
    return plane_normalize(c)


def plane_rotation(v):
    az = cr_atan2(v[1], v[0])
    el = cr_atan2(v[2], _sqrt(v[0] * v[0] + v[1] * v[1]))
    s1, c1 = cr_sincos(abs(0.5 * az))
    if 0.5 * az < 0:
        s1 = -s1
    s2, c2 = cr_sincos(abs(0.5 * -el))
    if 0.5 * -el < 0:
        s2 = -s2
    qa = [s1 * 0.0, s1 * 0.0, s1 * 1.0, c1]
    qb = [s2 * 0.0, s2 * 1.0, s2 * 0.0, c2]
    return quat_matrix(quat_mul(qa, qb))


def angles_in_frame(nor, m):
    R = plane_rotation(nor)
    n = [R[0][i] * m[0] + R[1][i] * m[1] + R[2][i] * m[2] for i in range(3)]
    return [cr_atan2(n[1], n[0]), cr_atan2(n[2], _sqrt(n[0] * n[0] + n[1] * n[1]))]


def plane_error(kind, meas, Xw, q, t):
    R = quat_matrix(q)
    l = [R[i][0] * Xw[0] + R[i][1] * Xw[1] + R[i][2] * Xw[2] for i in range(3)]
    l.append(Xw[3] - (t[0] * l[0] + t[1] * l[1] + t[2] * l[2]))
    if l[3] < 0.0:
        l = [-v for v in l]
    l = plane_normalize(l)
    if kind == 3:
        return angles_in_frame(l[:3], meas[:3]) + [(-l[3]) - (-meas[3])]
    if kind == 4:
        nor = l[:3]
        if meas[0] * nor[0] + meas[1] * nor[1] + meas[2] * nor[2] < 0:
            nor = [-v for v in nor]
        return angles_in_frame(nor, meas[:3]) + [0.0]
    a, m = l[:3], meas[:3]
    v = [a[1] * m[2] - a[2] * m[1], a[2] * m[0] - a[0] * m[2], a[0] * m[1] - a[1] * m[0]]
    nv = _sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    ax = [_div(c, nv) for c in v]
    sn, c = cr_sincos(math.pi / 2)
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
    return angles_in_frame(b, m) + [0.0]


def plane_jacobian(kind, meas, Xw, q, t):
    """BaseUnaryEdge::linearizeOplus"""
    delta = 1e-9
    scalar = 1.0 / (2 * delta)
    J = np.zeros((3, 6))
    for d in range(6):
        u = [0.0] * 6
        u[d] = delta
        pq, pt, _ = oplus(q, t, u)
        e1 = plane_error(kind, meas, Xw, pq, pt)
        u[d] = -delta
        pq, pt, _ = oplus(q, t, u)
        e2 = plane_error(kind, meas, Xw, pq, pt)
        for r in range(3):
            J[r, d] = scalar * (e1[r] - e2[r])
    return J


# ------------------------------------------------------------------------------------------------------------------------------
# Eigen::LDLT<MatrixXd>, lower, unblocked
def ldlt_solve(H, b):
    """-> (isPositive, x or None)"""
    n = 6
    A = [[float(H[i][j]) for j in range(n)] for i in range(n)]
    tr = list(range(n))
    sign = 0                                  # 0 zero, 1 positive semi-definite, -1 negative, 2 indefinite
    for k in range(n):
        big = k
        best = abs(A[k][k])
        for i in range(k + 1, n):
            if abs(A[i][i]) > best:
                best, big = abs(A[i][i]), i
        tr[k] = big
        if k != big:
            for j in range(k):
                A[k][j], A[big][j] = A[big][j], A[k][j]
            for i in range(big + 1, n):
                A[i][k], A[i][big] = A[i][big], A[i][k]
            A[k][k], A[big][big] = A[big][big], A[k][k]
            for i in range(k + 1, big):
                A[i][k], A[big][i] = A[big][i], A[i][k]
        if k > 0:
            temp = [A[j][j] * A[k][j] for j in range(k)]
            s = A[k][0] * temp[0]
            for j in range(1, k):
                s = s + A[k][j] * temp[j]
            A[k][k] -= s
            for i in range(k + 1, n):
                s = A[i][0] * temp[0]
                for j in range(1, k):
                    s = s + A[i][j] * temp[j]
                A[i][k] -= s
        akk = A[k][k]
        valid = abs(akk) > 0
        if k == 0 and not valid:
            sign = 0
            tr = list(range(n))
            break
        if valid:
            for i in range(k + 1, n):
                A[i][k] /= akk
        if sign == 1:
            if akk < 0:
                sign = 2
        elif sign == -1:
            if akk > 0:
                sign = 2
        elif sign == 0:
            if akk > 0:
                sign = 1
            elif akk < 0:
                sign = -1
    if sign not in (0, 1):
        return False, None
    x = [float(v) for v in b]
    for k in range(n):
        x[k], x[tr[k]] = x[tr[k]], x[k]
    for i in range(n):
        if x[i] != 0:
            for j in range(i + 1, n):
                x[j] -= x[i] * A[j][i]
    tol = 1.0 / DBL_MAX
    for i in range(n):
        x[i] = x[i] / A[i][i] if abs(A[i][i]) > tol else 0.0
    for i in range(n - 2, -1, -1):
        s = A[i + 1][i] * x[i + 1]
        for j in range(i + 2, n):
            s = s + A[j][i] * x[j]
        x[i] -= s
    for k in range(n - 1, -1, -1):
        x[k], x[tr[k]] = x[tr[k]], x[k]
    return True, x


# ------------------------------------------------------------------------------------------------------------------------------
# the graph of one frame
class Graph:
    """The edges of one frame in the order the reference inserts them, and the passes over the active ones"""

    def __init__(self, fr):
        K = np.asarray(fr["K"], F).astype(D)
        self.fx, self.fy, self.cx, self.cy = (float(v) for v in K)
        self.bf = float(np.asarray(fr["bf"], F).astype(D))
        obs = np.asarray(fr.get("obs", np.zeros((0, 2))), F).reshape(-1, 2)
        ur = np.asarray(fr.get("u_right", np.zeros(0)), F).reshape(-1)
        n_pts = len(ur)
        lf = np.asarray(fr.get("line_fn", np.zeros((0, 3))), D).reshape(-1, 3)
        le = np.asarray(fr.get("line_ends", np.zeros((0, 6))), D).reshape(-1, 6)
        n_lines = len(lf)
        kind, meas, X, info, delta, th = [], [], [], [], [], []
        d_mono, d_stereo = float(D(F(math.sqrt(5.991)))), float(D(F(math.sqrt(7.815))))
        for i in range(n_pts):
            mono = ur[i] < 0
            kind.append(0 if mono else 1)
            meas.append([float(obs[i, 0]), float(obs[i, 1]), 0.0 if mono else float(ur[i]), 0.0])
            X.append([float(v) for v in np.asarray(fr["Xw"], F).reshape(-1, 3)[i]] + [0.0])
            w = float(np.asarray(fr["inv_sigma2"], F).reshape(-1)[i])
            info.append([w, w, w])
            delta.append(d_mono if mono else d_stereo)
            th.append(float(F(5.991)) if mono else float(F(7.815)))
        for i in range(n_lines):
            for end in range(2):
                kind.append(2)
                meas.append(list(lf[i]) + [0.0])
                X.append(list(le[i, 3 * end:3 * end + 3]) + [0.0])
                info.append([1.0, 1.0, 1.0])
                delta.append(d_stereo)
                th.append(float(F(2) * F(5.991)))
        pm = np.asarray(fr.get("plane_meas", np.zeros((0, 4))), F).reshape(-1, 4)
        pw = np.asarray(fr.get("plane_world", np.zeros((0, 12))), F).reshape(-1, 12)
        mask = np.asarray(fr.get("plane_mask", np.zeros(0)), np.uint8).reshape(-1)
        st = [float(v) for v in fr.get("plane_settings", SETTINGS)]
        angle_info, dis_info = 3282.8 / (st[0] * st[0]), st[1] * st[1]
        par_info, ver_info = 3282.8 / (st[2] * st[2]), 3282.8 / (st[3] * st[3])
        self.plane_slot = []                       # (pass, slot) of every plane edge
        for ps in range(3 if fr.get("b_struct", 0) else 1):
            for i in range(len(mask)):
                if not mask[i] & (1 << ps):
                    continue
                kind.append(3 + ps)
                meas.append(to_plane3d(pm[i]))
                X.append(to_plane3d(pw[i, 4 * ps:4 * ps + 4]))
                w = (angle_info, par_info, ver_info)[ps]
                info.append([w, w, dis_info if ps == 0 else 0.0])
                chi = st[4] if ps == 0 else st[5]
                delta.append(float(D(F(math.sqrt(chi)))))
                th.append(chi)
                self.plane_slot.append((ps, i))
        self.n_pts, self.n_lines, self.n_slots = n_pts, n_lines, len(mask)
        self.kind = np.array(kind, np.int64)
        self.meas = np.array(meas, D).reshape(-1, 4)
        self.X = np.array(X, D).reshape(-1, 4)
        self.info = np.array(info, D).reshape(-1, 3)
        self.delta = np.array(delta, D)
        self.th = np.array(th, D)
        self.n = len(kind)
        self.dim = np.where(np.isin(self.kind, (0, 4, 5)), 2, 3)
        self.err = np.zeros((self.n, 3))
        self.level = np.zeros(self.n, bool)        # True: level 1, the outlier flag of the edge's feature
        self.dsqr = (self.delta * self.delta).astype(F).astype(D)      # float dsqr = delta * delta

    # -- computeError over a set of edges ---------------------------------------------------------------------------------
    def errors(self, idx, q, t):
        with np.errstate(all="ignore"):
            e = np.zeros((len(idx), 3))
            k = self.kind[idx]
            cam = k < 3
            if cam.any():
                ii = idx[cam]
                p = quat_rotate(q, [self.X[ii, 0], self.X[ii, 1], self.X[ii, 2]])
                p = [p[c] + t[c] for c in range(3)]
                kk = k[cam]
                m = self.meas[ii]
                r0 = (p[0] / p[2]) * self.fx + self.cx
                r1 = (p[1] / p[2]) * self.fy + self.cy
                invz = (1.0 / p[2]).astype(F).astype(D)
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
                e[j] = plane_error(int(self.kind[i]), list(self.meas[i]), list(self.X[i]), q, t)
            return e

    def chi2(self, idx, e):
        """BaseEdge::chi2 = e . (Omega e), Omega the D x D diagonal with its zeros multiplied through"""
        with np.errstate(all="ignore"):
            out = np.zeros(len(idx))
            for dim in (2, 3):
                sel = self.dim[idx] == dim
                if not sel.any():
                    continue
                ee, w = e[sel], self.info[idx[sel]]
                s = None
                for i in range(dim):
                    we = None
                    for j in range(dim):
                        term = (w[:, i] if i == j else 0.0) * ee[:, j]
                        we = term if we is None else we + term
                    term = ee[:, i] * we
                    s = term if s is None else s + term
                out[sel] = s
            return out

    def huber(self, idx, chi2):
        """RobustKernelHuber::robustify: rho[0], rho[1]"""
        with np.errstate(all="ignore"):
            d, dsqr = self.delta[idx], self.dsqr[idx]
            sq = np.sqrt(chi2)
            inl = chi2 <= dsqr
            return np.where(inl, chi2, 2 * sq * d - dsqr), np.where(inl, 1.0, d / sq)

    def jacobians(self, idx, q, t):
        with np.errstate(all="ignore"):
            J = np.zeros((len(idx), 3, 6))
            k = self.kind[idx]
            cam = k < 3
            if cam.any():
                ii = idx[cam]
                p = quat_rotate(q, [self.X[ii, 0], self.X[ii, 1], self.X[ii, 2]])
                x, y, z = (p[c] + t[c] for c in range(3))
                invz = 1.0 / z
                invz_2 = invz * invz
                fx, fy, bf = self.fx, self.fy, self.bf
                Jc = np.zeros((len(ii), 3, 6))
                Jc[:, 0, 0] = x * y * invz_2 * fx
                Jc[:, 0, 1] = -(1 + (x * x * invz_2)) * fx
                Jc[:, 0, 2] = y * invz * fx
                Jc[:, 0, 3] = -invz * fx
                Jc[:, 0, 5] = x * invz_2 * fx
                Jc[:, 1, 0] = (1 + y * y * invz_2) * fy
                Jc[:, 1, 1] = -x * y * invz_2 * fy
                Jc[:, 1, 2] = -x * invz * fy
                Jc[:, 1, 4] = -invz * fy
                Jc[:, 1, 5] = y * invz_2 * fy
                st = k[cam] == 1
                Jc[st, 2, 0] = (Jc[:, 0, 0] - bf * y * invz_2)[st]
                Jc[st, 2, 1] = (Jc[:, 0, 1] + bf * x * invz_2)[st]
                Jc[st, 2, 2] = Jc[st, 0, 2]
                Jc[st, 2, 3] = Jc[st, 0, 3]
                Jc[st, 2, 5] = (Jc[:, 0, 5] - bf * invz_2)[st]
                ln = k[cam] == 2
                if ln.any():
                    lx, ly = self.meas[ii, 0], self.meas[ii, 1]
                    L = np.zeros((len(ii), 3, 6))
                    L[:, 0, 0] = -fy * ly - fx * lx * x * y * invz_2 - fy * ly * y * y * invz_2
                    L[:, 0, 1] = fx * lx + fx * lx * x * x * invz_2 + fy * ly * x * y * invz_2
                    L[:, 0, 2] = -fx * lx * y * invz + fy * ly * x * invz
                    L[:, 0, 3] = fx * lx * invz
                    L[:, 0, 4] = fy * ly * invz
                    L[:, 0, 5] = -(fx * lx * x + fy * ly * y) * invz_2
                    Jc[ln] = L[ln]
                J[cam] = Jc
            for j in np.nonzero(~cam)[0]:
                i = idx[j]
                J[j] = plane_jacobian(int(self.kind[i]), list(self.meas[i]), list(self.X[i]), q, t)
            return J

    def quadratic_terms(self, idx, J, e, robust):
        """BaseUnaryEdge::constructQuadraticForm per edge: what it adds to H [n, 6, 6] and takes from b [n, 6]"""
        with np.errstate(all="ignore"):
            n = len(idx)
            Ht, bt = np.zeros((n, 6, 6)), np.zeros((n, 6))
            rho1 = self.huber(idx, self.chi2(idx, e))[1] if robust else None
            for dim in (2, 3):
                sel = self.dim[idx] == dim
                if not sel.any():
                    continue
                A, ee, om = J[sel], e[sel], self.info[idx[sel]]
                Om = np.zeros((A.shape[0], dim, dim))
                for m in range(dim):
                    Om[:, m, m] = om[:, m]
                r1 = rho1[sel] if robust else None
                W = r1[:, None, None] * Om if robust else Om
                T = np.zeros((A.shape[0], 6, dim))
                Tb = np.zeros((A.shape[0], 6, dim))
                for i in range(6):
                    for k in range(dim):
                        s = sb = None
                        for m in range(dim):
                            a = A[:, m, i] * W[:, m, k]
                            ab = (r1 * A[:, m, i]) * Om[:, m, k] if robust else A[:, m, i] * Om[:, m, k]
                            s = a if s is None else s + a
                            sb = ab if sb is None else sb + ab
                        T[:, i, k], Tb[:, i, k] = s, sb
                Hs, bs = np.zeros((A.shape[0], 6, 6)), np.zeros((A.shape[0], 6))
                for i in range(6):
                    for j in range(6):
                        s = None
                        for k in range(dim):
                            a = T[:, i, k] * A[:, k, j]
                            s = a if s is None else s + a
                        Hs[:, i, j] = s
                    s = None
                    for k in range(dim):
                        a = Tb[:, i, k] * ee[:, k]
                        s = a if s is None else s + a
                    bs[:, i] = s
                Ht[sel], bt[sel] = Hs, bs
            return Ht, bt


def ordered_sum(terms):
    """+0.0 + t0 + t1 + .. along axis 0, strictly in order"""
    with np.errstate(all="ignore"):
        z = np.zeros((1,) + terms.shape[1:])
        return np.cumsum(np.concatenate([z, terms], axis=0), axis=0)[-1]


# ------------------------------------------------------------------------------------------------------------------------------
# SparseOptimizer::optimize with OptimizationAlgorithmLevenberg, and the outer loop
class Optimizer:
    def __init__(self, fr):
        self.fr = fr
        self.g = Graph(fr)
        self.x = [0.0] * 6                         # the solver's x: what a failed solve leaves in place
        self.iterations = self.trials = self.rejected = self.nbad_stops = self.small = self.big = 0
        self.last_rejected = False
        self.robust = True

    def active_chi2(self, act, q, t):
        """computeActiveErrors, activeRobustChi2"""
        g = self.g
        e = g.errors(act, q, t)
        g.err[act] = e
        c = g.chi2(act, e)
        if self.robust:
            c = g.huber(act, c)[0]
        return float(ordered_sum(c))

    def optimize(self, q, t, its=10):
        g = self.g
        act = np.nonzero(~g.level)[0]
        if len(act) == 0:
            return q, t                            # no active vertex: optimize() returns at once
        lam = ni = 0.0
        n_bad = 0
        for it in range(its):
            current = self.active_chi2(act, q, t)
            ini = current
            J = g.jacobians(act, q, t)
            Ht, bt = g.quadratic_terms(act, J, g.err[act], self.robust)
            H = ordered_sum(Ht)
            b = ordered_sum(-bt)
            self.iterations += 1
            if it == 0:
                mx = 0.0
                for j in range(6):
                    a = abs(float(H[j, j]))
                    mx = mx if a < mx else a       # std::max(fabs(h), maxDiagonal)
                lam = 1e-5 * mx
                ni = 2.0
                n_bad = 0
            rho = 0.0
            qmax = 0
            while True:
                q_save, t_save = list(q), list(t)
                Hl = [[float(H[i, j]) + (lam if i == j else 0.0) for j in range(6)] for i in range(6)]
                ok, x = ldlt_solve(Hl, [float(v) for v in b])
                if ok:
                    self.x = x
                q, t, small = oplus(q, t, self.x)
                self.trials += 1
                self.small += small
                self.big += not small
                temp = self.active_chi2(act, q, t)
                if not ok:
                    temp = DBL_MAX
                with np.errstate(all="ignore"):
                    rho = D(current) - D(temp)
                    scale = D(0.0)
                    for j in range(6):
                        scale = scale + D(self.x[j]) * (D(lam) * D(self.x[j]) + D(b[j]))
                    scale = scale + 1e-3
                    rho = float(rho / scale)
                if rho > 0 and math.isfinite(temp):
                    alpha = 1.0 - cr_cube(2 * rho - 1)
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                    self.last_rejected = False
                else:
                    with np.errstate(all="ignore"):
                        lam = float(D(lam) * D(ni))
                        ni = float(D(ni) * 2)
                    q, t = q_save, t_save
                    self.rejected += 1
                    self.last_rejected = True
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                break
            with np.errstate(all="ignore"):
                if float((D(ini) - D(current)) * 1e3) < ini:
                    n_bad += 1
                else:
                    n_bad = 0
            if n_bad >= 3:
                self.nbad_stops += 1
                break
        return q, t

    def run(self):
        fr, g = self.fr, self.g
        n_slots = g.n_slots
        out = dict(Tcw=np.asarray(fr["Tcw"], F).reshape(16).copy(), returns=0, rounds=0, iterations=0, trials=0,
                   diag=np.zeros(8, np.int32), point_outlier=np.zeros(g.n_pts, np.uint8),
                   line_outlier=np.zeros(g.n_lines, np.uint8), plane_outlier=np.zeros(n_slots, np.uint8),
                   par_plane_outlier=np.zeros(n_slots, np.uint8), ver_plane_outlier=np.zeros(n_slots, np.uint8))
        n_initial = g.n_pts + g.n_lines + len(g.plane_slot)
        if n_initial < 3:
            return out
        n_bad = 0
        last_rejected_rounds = empty_rounds = 0
        q, t = to_se3quat(fr["Tcw"])
        single = np.concatenate([np.arange(g.n_pts), np.arange(g.n_pts + 2 * g.n_lines, g.n)]).astype(np.int64)
        for it in range(4):
            q, t = to_se3quat(fr["Tcw"])
            self.last_rejected = False
            if g.level.all():
                empty_rounds += 1
            q, t = self.optimize(q, t)
            out["rounds"] += 1
            last_rejected_rounds += self.last_rejected
            # points and planes: an outlier's error is recomputed, an inlier's is what the last computeActiveErrors left
            redo = single[g.level[single]]
            if len(redo):
                g.err[redo] = g.errors(redo, q, t)
            with np.errstate(all="ignore"):
                chi2 = g.chi2(single, g.err[single]).astype(F)
                g.level[single] = chi2.astype(D) > g.th[single]
                lines = np.arange(g.n_pts, g.n_pts + 2 * g.n_lines)
                if len(lines):
                    g.err[lines] = g.errors(lines, q, t)
                    c = (g.err[lines, 0] * g.err[lines, 0]).astype(F).astype(D) > g.th[lines]
                    both = c[0::2] | c[1::2]
                    g.level[lines] = np.repeat(both, 2)
            n_bad = int(g.level[single].sum()) + int(g.level[g.n_pts:g.n_pts + 2 * g.n_lines:2].sum())
            if it == 2:
                self.robust = False
            if g.n < 10:
                break
        R = quat_matrix(q)
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


def pose_optimization(fr):
    """Optimizer::PoseOptimization of one frame (a dict as frame() makes it): the outputs of drfe_pose_opt_out for it"""
    return Optimizer(fr).run()


def table(frames):
    """the outputs of a call over these frames, concatenated as lib.pose_opt_host lays them out"""
    outs = [pose_optimization(fr) for fr in frames]
    r = {}
    for k in ("Tcw", "diag"):
        r[k] = np.stack([o[k] for o in outs]) if outs else np.zeros((0, 16 if k == "Tcw" else 8), F if k == "Tcw" else np.int32)
    for k in ("returns", "rounds", "iterations", "trials"):
        r[k] = np.array([o[k] for o in outs], np.int32)
    for k in ("point_outlier", "line_outlier", "plane_outlier", "par_plane_outlier", "ver_plane_outlier"):
        r[k] = np.concatenate([o[k] for o in outs]) if outs else np.zeros(0, np.uint8)
    return r


def tables_equal(a, b, keys=TABLE_KEYS):
    """the names of the arrays that differ: a NaN equals a NaN whatever its payload, everything else is compared by bytes"""
    bad = []
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            bad.append(k)
            continue
        if x.dtype.kind == "f":
            nx, ny = np.isnan(x), np.isnan(y)
            it = x.dtype.itemsize
            same = (nx & ny) | (x.view(f"u{it}") == y.view(f"u{it}"))
            if not same.all():
                bad.append(k)
        elif x.tobytes() != y.tobytes():
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------------------------------------
# scenes
CAM = (517.3, 516.5, 318.6, 255.3)                  # TUM3
BF = 40.0


def rot(axis, ang):
    a = np.asarray(axis, D)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * (Kx @ Kx)


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(F)


def project(Xc, K=CAM):
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)


def frame(rng, n_points=100, n_lines=0, planes=(), b_struct=0, mode="alternate", outlier_frac=0.0, noise=0.7, start_rot=0.02,
          start_trans=0.05, K=CAM, bf=BF, settings=SETTINGS, identity=False, outlier_px=(25, 80)):
    """One frame around a planted pose: dict with the inputs of drfe_pose_opt_problems for it plus what was planted (`true_Tcw`,
    `planted_outlier` per point).  mode: "mono", "stereo" or "alternate".  planes: per slot a mask of MATCHED | PARALLEL | VERTICAL."""
    Rt = rot(rng.normal(size=3), rng.uniform(0, 0.5))
    tt = rng.uniform(-1, 1, 3)
    if identity:                                    # the planted and the start pose are the identity, exactly
        Rt, tt, start_rot, start_trans = np.eye(3), np.zeros(3), 0.0, 0.0
    Xc = np.stack([rng.uniform(-1.2, 1.2, n_points), rng.uniform(-0.9, 0.9, n_points), rng.uniform(1.0, 6.0, n_points)], axis=1)
    Xw = ((Xc - tt) @ Rt).astype(F)                 # R^T (Xc - t)
    Xc = Xw.astype(D) @ Rt.T + tt
    octave = rng.integers(0, 8, n_points)
    sigma = 1.2 ** octave
    uv = project(Xc, K) + rng.normal(size=(n_points, 2)) * noise * sigma[:, None]
    ur = uv[:, 0] - bf / Xc[:, 2] + rng.normal(size=n_points) * noise * sigma
    planted = rng.random(n_points) < outlier_frac
    uv[planted] += rng.choice([-1, 1], (int(planted.sum()), 2)) * rng.uniform(outlier_px[0], outlier_px[1], (int(planted.sum()), 2))
    if mode == "mono":
        ur[:] = -1
    elif mode == "alternate":
        ur[0::2] = -1
    fr = dict(K=np.array(K, F), bf=F(bf), b_struct=int(b_struct), obs=uv.astype(F), u_right=ur.astype(F),
              inv_sigma2=(1 / sigma ** 2).astype(F), octave=octave.astype(np.int32), Xw=Xw, plane_settings=tuple(settings), planted_outlier=planted,
              true_Tcw=pose(Rt, tt))
    # lines: a 3-D segment in front of the camera, the line function through its two projections
    P = np.stack([rng.uniform(-1, 1, (n_lines, 2)), rng.uniform(-0.8, 0.8, (n_lines, 2)), rng.uniform(1.5, 5, (n_lines, 2))], axis=2)
    ends_w = (P.reshape(-1, 3) - tt) @ Rt
    pc = project(ends_w @ Rt.T + tt, K).reshape(n_lines, 2, 2)
    h1 = np.concatenate([pc[:, 0], np.ones((n_lines, 1))], axis=1)
    h2 = np.concatenate([pc[:, 1], np.ones((n_lines, 1))], axis=1)
    fn = np.cross(h1, h2)
    fn = fn / np.maximum(np.linalg.norm(fn[:, :2], axis=1, keepdims=True), 1e-12)
    fn[:, 2] += rng.normal(size=n_lines) * 0.5 if n_lines else 0
    fr["line_fn"] = fn.reshape(-1, 3)
    fr["line_ends"] = ends_w.reshape(-1, 6)
    # planes: a world plane, what the camera measures of it, and a parallel and a vertical world plane
    S = len(planes)
    meas, world = np.zeros((S, 4), F), np.zeros((S, 12), F)
    for i in range(S):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        d = rng.uniform(1, 4)
        nc = Rt @ n
        dc = d - tt @ nc
        meas[i] = np.concatenate([nc, [dc]]) + rng.normal(size=4) * 0.002
        if rng.random() < 0.5:
            meas[i] = -meas[i]
        v = np.cross(n, rng.normal(size=3))
        v /= np.linalg.norm(v)
        world[i] = np.concatenate([n, [d], (n if i % 2 == 0 else -n), [d + 1.0], v, [rng.uniform(1, 3)]])
    fr["plane_meas"], fr["plane_world"], fr["plane_mask"] = meas, world, np.array(planes, np.uint8).reshape(-1)
    dR = rot(rng.normal(size=3), start_rot)
    fr["Tcw"] = pose(dR @ Rt, tt + rng.normal(size=3) * start_trans).reshape(16)
    return fr


def behaviour_frames():
    """Named frames that take the paths DESIGN.md section 20 lists; tests assert through the diagnostics that they do"""
    rng = np.random.default_rng(2024)
    fr = {}
    # every edge an outlier after round one: rounds two to four have no active edge
    fr["all_outliers"] = frame(np.random.default_rng(1), 12, outlier_frac=1.0, mode="stereo", outlier_px=(150, 300))
    # plain frames: rejected trials, a round whose last trial is rejected, the _nBad >= 3 stop, theta on both sides of 1e-5
    fr["points"] = frame(rng, 60, outlier_frac=0.2)
    fr["stereo_lines"] = frame(rng, 40, 5, mode="stereo")
    fr["struct"] = frame(rng, 30, 3, planes=(MATCHED, MATCHED | PARALLEL | VERTICAL, MATCHED | PARALLEL), b_struct=1)
    # a point with Zc == 0 exactly and one behind the camera under the start pose (the identity): inf and NaN flow through
    f = frame(rng, 20, identity=True)
    f["Xw"][0] = (0.3, 0.2, 0.0)
    f["Xw"][1] = (0.1, -0.2, -2.0)
    f["Xw"][2] = (0.2, 0.1, 0.0)
    f["u_right"][0], f["u_right"][2] = -1, 300.0    # Zc == 0 on a mono and on a stereo edge
    fr["zc_zero"] = f
    f = frame(rng, 20, identity=True, start_rot=0.0)
    f["Xw"][1] = (0.1, -0.2, -2.0)                  # Zc < 0 only: finite everywhere
    fr["zc_negative"] = f
    return fr


def size_frames():
    """Frames at the edge counts where a path changes: fewer than 3 correspondences, the `edges().size() < 10` break, the chunk of
    the device's workgroup (256 point / line edges, 16 plane edges) and its wavefront (64)"""
    rng = np.random.default_rng(77)
    fr = {"0": frame(rng, 0), "2": frame(rng, 2), "3": frame(rng, 3), "9": frame(rng, 9), "10": frame(rng, 10),
          "9_lines": frame(rng, 5, 2), "10_lines": frame(rng, 4, 3), "2_lines_as_4_edges": frame(rng, 0, 2)}
    for n in (63, 64, 65, 255, 256, 257):
        fr[str(n)] = frame(rng, n, outlier_frac=0.1)
    fr["250+2x4"] = frame(rng, 250, 4)
    fr["16_planes"] = frame(rng, 20, 0, planes=(MATCHED,) * 16, b_struct=1)
    fr["17_planes"] = frame(rng, 20, 0, planes=(MATCHED,) * 15 + (MATCHED | PARALLEL,), b_struct=1)
    return fr


def mix_frames():
    """Mixes of edge kinds: mono / stereo / alternating, 0 / 1 / 33 lines, 0 / 1 / 3 plane slots with each map plane alone and
    together, bStruct on and off"""
    rng = np.random.default_rng(78)
    fr = {}
    for mode in ("mono", "stereo", "alternate"):
        fr[mode] = frame(rng, 40, mode=mode, outlier_frac=0.1)
    for nl in (1, 33):
        fr[f"{nl}_lines"] = frame(rng, 30, nl)
    for bs in (0, 1):
        for name, planes in (("m", (MATCHED,)), ("p", (PARALLEL,)), ("v", (VERTICAL,)), ("mpv", (MATCHED | PARALLEL | VERTICAL,)),
                             ("3slots", (MATCHED, PARALLEL | VERTICAL, MATCHED | VERTICAL))):
            fr[f"planes_{name}_struct{bs}"] = frame(rng, 12, 2, planes=planes, b_struct=bs)
    fr["planes_only"] = frame(rng, 0, 0, planes=(MATCHED | PARALLEL | VERTICAL,) * 3, b_struct=1)
    return fr


def random_frames(n=20, seed=99):
    """n random frames of at most 200 edges"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nl = int(rng.integers(0, 12))
        planes = tuple(int(v) for v in rng.integers(1, 8, int(rng.integers(0, 4))))
        npts = int(rng.integers(3, 200 - 2 * nl - 3 * len(planes)))
        out.append(frame(rng, npts, nl, planes=planes, b_struct=int(rng.integers(0, 2)), mode=("mono", "stereo", "alternate")[int(rng.integers(0, 3))],
                         outlier_frac=float(rng.uniform(0, 0.3))))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the native caller (tests/native/pose_opt_caller.cpp)
def caller_blob(frames):
    """pose_opt_caller's input for these frames.  Every frame gets one key point and one key line without a map point / map line in
    front of its matched ones, which the caller must skip and leave unflagged."""
    import struct
    inv = (1 / (1.2 ** np.arange(8)) ** 2).astype(F)
    b = [struct.pack("<i", len(frames)), inv.tobytes()]
    for fr in frames:
        N, NL, M = len(fr["u_right"]), len(fr["line_fn"]), len(fr["plane_mask"])
        b.append(np.asarray(fr["Tcw"], F).tobytes() + np.asarray(fr["K"], F).tobytes() + F(fr["bf"]).tobytes())
        b.append(struct.pack("<4i", int(fr["b_struct"]), N + 1, NL + 1, M))
        b.append(struct.pack("<B3fi3f", 0, 10.0, 20.0, -1.0, 0, 0.0, 0.0, 1.0))
        for i in range(N):
            assert fr["inv_sigma2"][i] == inv[fr["octave"][i]]
            b.append(struct.pack("<B3fi3f", 1, *fr["obs"][i], fr["u_right"][i], int(fr["octave"][i]), *fr["Xw"][i]))
        b.append(struct.pack("<B9d", 0, *([0.0] * 9)))
        for i in range(NL):
            b.append(struct.pack("<B9d", 1, *fr["line_fn"][i], *fr["line_ends"][i]))
        for i in range(M):
            b.append(struct.pack("<B16f", int(fr["plane_mask"][i]), *fr["plane_meas"][i], *fr["plane_world"][i]))
    return b"".join(b)


def caller_expected(result, frames):
    """what pose_opt_caller writes, from a pose_opt_host / pose_opt_batch result over the same frames: both passes"""
    import struct
    P = pack(frames)
    one = []
    for f, fr in enumerate(frames):
        po, lo, so = P["point_offsets"], P["line_offsets"], P["plane_offsets"]
        one.append(struct.pack("<i", int(result["returns"][f])) + np.asarray(result["Tcw"][f], F).tobytes() + b"\0" +
                   result["point_outlier"][po[f]:po[f + 1]].tobytes() + b"\0" + result["line_outlier"][lo[f]:lo[f + 1]].tobytes() +
                   b"".join(result[k][so[f]:so[f + 1]].tobytes() for k in ("plane_outlier", "par_plane_outlier", "ver_plane_outlier")))
    return b"".join(one) * 2


def caller_frames():
    rng = np.random.default_rng(41)
    return [frame(rng, 40, 3, planes=(MATCHED | PARALLEL, MATCHED | VERTICAL), b_struct=1, outlier_frac=0.2), frame(rng, 25, 0, mode="mono"),
            frame(rng, 2, 0), frame(rng, 30, 4, planes=(7,), b_struct=0, mode="stereo")]


_TABLES = {}


def numpy_table(name, frames):
    """table(frames), computed once per process under `name`"""
    if name not in _TABLES:
        _TABLES[name] = table(frames)
    return _TABLES[name]


def pack(frames):
    """the frames of a call as the dict lib.pose_opt_host / Context.pose_opt_batch take"""
    n = len(frames)

    def part(f, key, shape, dt):
        v = np.asarray(f.get(key, ()), dt)
        return v.reshape(shape) if v.size else np.zeros((0,) + shape[1:], dt)

    def cat(key, shape, dt):
        return np.concatenate([part(f, key, shape, dt) for f in frames]) if n else np.zeros((0,) + shape[1:], dt)

    def offsets(key, shape):
        return np.concatenate([[0], np.cumsum([len(part(f, key, shape, D)) for f in frames])]).astype(np.int32)
    settings = frames[0].get("plane_settings", SETTINGS) if frames else SETTINGS
    assert all(tuple(f.get("plane_settings", SETTINGS)) == tuple(settings) for f in frames)
    return dict(Tcw=cat("Tcw", (-1, 16), F), K=cat("K", (-1, 4), F),
                bf=np.array([f["bf"] for f in frames], F), b_struct=np.array([f.get("b_struct", 0) for f in frames], np.uint8),
                point_offsets=offsets("u_right", (-1,)), obs=cat("obs", (-1, 2), F), u_right=cat("u_right", (-1,), F),
                inv_sigma2=cat("inv_sigma2", (-1,), F), Xw=cat("Xw", (-1, 3), F),
                line_offsets=offsets("line_fn", (-1, 3)), line_fn=cat("line_fn", (-1, 3), D), line_ends=cat("line_ends", (-1, 6), D),
                plane_offsets=offsets("plane_mask", (-1,)), plane_meas=cat("plane_meas", (-1, 4), F),
                plane_world=cat("plane_world", (-1, 12), F), plane_mask=cat("plane_mask", (-1,), np.uint8),
                plane_settings=np.array(settings, D))
