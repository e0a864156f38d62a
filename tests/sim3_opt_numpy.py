"""An independent restatement of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:3982-4177) in float64 Python / numpy, written
from the reference text in the order DESIGN.md section 22 reads it: g2o::Sim3 (the exponential's four branches, map, inverse,
operator*), the two projection edges, BaseBinaryEdge's numeric Jacobian and quadratic form for the one free vertex, the Levenberg
loop over seven dimensions, the two optimize() calls and the two classifications.  Eigen's quaternion, Huber's kernel's float
constant, the LDLT's statements and the correctly rounded sin / cos / cube are tests/pose_opt_numpy.py's; exp goes through mpmath,
rounded once.  Ordered sums are cumulative sums from +0.0.  Plus the scene lists.  Used by tests/test_sim3_opt_cpu.py and
tests/test_gpu_sim3_opt.py."""
import math

import numpy as np

import pose_opt_numpy as pon
from pose_opt_numpy import D, DBL_MAX, F, ordered_sum, tables_equal as _tables_equal

TABLE_KEYS = ("S12", "T12", "Scw", "returns", "n_bad", "iterations", "trials", "diag", "outlier")
IN_KEYS = ("S12", "K1", "K2", "R1w", "t1w", "R2w", "t2w", "th2", "fix_scale")
MATCH_KEYS = ("index", "P3D1w", "P3D2w", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")


def tables_equal(a, b, keys=TABLE_KEYS):
    return _tables_equal(a, b, keys)


def cr_exp(x):
    x = float(x)
    if x == 0:
        return 1.0
    mp = pon._mp()
    return float(mp.exp(mp.mpf(x)))


# ------------------------------------------------------------------------------------------------------------------------------
# g2o::Sim3 as (q [x, y, z, w], t, s), Python scalars
def sim3_map(S, v):
    """s * (r * xyz) + t; v three scalars or three arrays"""
    q, t, s = S
    r = pon.quat_rotate(q, v)
    return [s * r[k] + t[k] for k in range(3)]


def sim3_inverse(S):
    q, t, s = S
    m = pon._div(-1.0, s)
    qc = [-q[0], -q[1], -q[2], q[3]]
    return qc, pon.quat_rotate(qc, [m * t[0], m * t[1], m * t[2]]), pon._div(1.0, s)


def sim3_mul(A, B):
    return pon.quat_mul(A[0], B[0]), sim3_map(A, B[1]), A[2] * B[2]


def sim3_exp(u):
    """Sim3(const Vector7d&): ((q, t, s), theta < eps)"""
    om, up, sigma = u[:3], u[3:6], u[6]
    theta = pon._sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    s = cr_exp(sigma)
    Om2 = [[Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c] + Om[r][2] * Om[2][c] for c in range(3)] for r in range(3)]
    eye = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    eps = 0.00001
    small = theta < eps
    if not small:
        sn, cs = pon.cr_sincos(theta)
    if small:
        R = [[eye[r][c] + Om[r][c] + Om2[r][c] for c in range(3)] for r in range(3)]
    else:
        a = sn / theta
        b = (1 - cs) / (theta * theta)
        R = [[eye[r][c] + a * Om[r][c] + b * Om2[r][c] for c in range(3)] for r in range(3)]
    if abs(sigma) < eps:
        C = 1.0
        if small:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = (1 - cs) / theta2
            B = (theta - sn) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        else:
            a = s * sn
            b = s * cs
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    W = [[A * Om[r][c] + B * Om2[r][c] + C * eye[r][c] for c in range(3)] for r in range(3)]
    t = [W[r][0] * up[0] + W[r][1] * up[1] + W[r][2] * up[2] for r in range(3)]
    return (pon.quat_from_matrix(R), t, s), small


def oplus(S, x, fix_scale):
    """VertexSim3Expmap::oplusImpl: x[6] = 0 through the caller's list when the scale is fixed; Sim3(x) * estimate"""
    if fix_scale:
        x[6] = 0.0
    E, small = sim3_exp(x)
    return sim3_mul(E, S), small


def compute_scale(x, b, lam):
    with np.errstate(all="ignore"):
        scale = D(0.0)
        for j in range(7):
            scale = scale + D(x[j]) * (D(lam) * D(x[j]) + D(b[j]))
        return float(scale + 1e-3)


def to_cvmat(S):
    """Converter::toCvMat(g2o::Sim3)"""
    q, t, s = S
    R = pon.quat_matrix(q)
    T = np.zeros((4, 4), F)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                T[r, c] = F(s * R[r][c])
            T[r, 3] = F(t[r])
    T[3, 3] = 1
    return T.reshape(16)


def from_pose(R, t):
    """g2o::Sim3(toMatrix3d(R), toVector3d(t), 1.0)"""
    R = np.asarray(R, F).reshape(3, 3).astype(D)
    t = np.asarray(t, F).reshape(3).astype(D)
    return pon.quat_from_matrix([[float(R[r, c]) for c in range(3)] for r in range(3)]), [float(v) for v in t], 1.0


def s12_tuple(S12):
    v = [float(x) for x in np.asarray(S12, D).reshape(8)]
    return v[:4], v[4:7], v[7]


def scw(pr, S):
    return to_cvmat(sim3_mul(S, from_pose(pr["R2w"], pr["t2w"])))


def camera_points(R, t, X):
    """cv::Mat P3Dc = Rcw * P3Dw + tcw: one gemm with a C term on floats, then widened.  X [n, 3] -> [n, 3] float64"""
    R, t, X = np.asarray(R, F).reshape(3, 3), np.asarray(t, F).reshape(3), np.asarray(X, F).reshape(-1, 3)
    out = np.zeros((len(X), 3), D)
    with np.errstate(all="ignore"):
        for r in range(3):
            d = (R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]
            assert d.dtype == F
            out[:, r] = (d.astype(D) * 1.0 + D(t[r]) * 1.0).astype(F).astype(D)
    return out


def ldlt_solve7(H, b):
    """Eigen::LDLT<MatrixXd> (lower, unblocked, pivoted) of the 7x7 H and its solve of H x = b -> (isPositive, x or None): the
    statements of tests/pose_opt_numpy.py's 6x6 form written out at n = 7"""
    n = 7
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
class Graph:
    """The edges of one problem in insertion order (e12(i), e21(i), ...), arrays over matches"""

    def __init__(self, pr):
        self.K1 = [float(v) for v in np.asarray(pr["K1"], F).astype(D)]
        self.K2 = [float(v) for v in np.asarray(pr["K2"], F).astype(D)]
        self.P1c = camera_points(pr["R1w"], pr["t1w"], pr["P3D1w"])
        self.P2c = camera_points(pr["R2w"], pr["t2w"], pr["P3D2w"])
        self.n = len(self.P1c)
        self.obs1 = np.asarray(pr["obs1"], F).reshape(-1, 2).astype(D)
        self.obs2 = np.asarray(pr["obs2"], F).reshape(-1, 2).astype(D)
        self.info = np.stack([np.asarray(pr["inv_sigma2_1"], F).reshape(-1).astype(D),
                              np.asarray(pr["inv_sigma2_2"], F).reshape(-1).astype(D)], axis=1)     # [n, 2]
        th2 = F(pr["th2"])
        self.th2 = float(D(th2))
        self.delta = float(D(np.sqrt(th2)))        # const float deltaHuber = sqrt(th2)
        assert np.sqrt(th2).dtype == F
        self.err = np.zeros((self.n, 4), D)
        self.gone = np.zeros(self.n, bool)

    def errors(self, act, S):
        """computeError of both edges of the matches `act` under S: [len(act), 4]"""
        with np.errstate(all="ignore"):
            p = sim3_map(S, [self.P2c[act, k] for k in range(3)])
            e = np.zeros((len(act), 4), D)
            e[:, 0] = self.obs1[act, 0] - ((p[0] / p[2]) * self.K1[0] + self.K1[2])
            e[:, 1] = self.obs1[act, 1] - ((p[1] / p[2]) * self.K1[1] + self.K1[3])
            p = sim3_map(sim3_inverse(S), [self.P1c[act, k] for k in range(3)])
            e[:, 2] = self.obs2[act, 0] - ((p[0] / p[2]) * self.K2[0] + self.K2[2])
            e[:, 3] = self.obs2[act, 1] - ((p[1] / p[2]) * self.K2[1] + self.K2[3])
        return e

    def chi2(self, act, e):
        """[len(act), 2]: chi2 of e12 and e21"""
        with np.errstate(all="ignore"):
            out = np.zeros((len(act), 2), D)
            for k in range(2):
                i, e0, e1 = self.info[act, k], e[:, 2 * k], e[:, 2 * k + 1]
                out[:, k] = e0 * (i * e0 + 0.0 * e1) + e1 * (0.0 * e0 + i * e1)
        return out

    def huber(self, c):
        """RobustKernelHuber::robustify on an array of chi2: (rho0, rho1)"""
        with np.errstate(all="ignore"):
            dsqr = float(D(F(self.delta * self.delta)))
            sq = np.sqrt(c)
            inl = c <= dsqr
            return np.where(inl, c, (2.0 * sq) * self.delta - dsqr), np.where(inl, 1.0, self.delta / sq)

    def terms(self, act, S, fix_scale):
        """linearizeOplus and constructQuadraticForm: [2 len(act), 35] in active-edge order"""
        scalar = 1.0 / (2 * 1e-9)
        n = len(act)
        J = np.zeros((n, 4, 7), D)
        with np.errstate(all="ignore"):
            for d in range(7):
                es = []
                for sign in (1e-9, -1e-9):
                    u = [0.0] * 7
                    u[d] = sign
                    Sp, _ = oplus(S, u, fix_scale)
                    es.append(self.errors(act, Sp))
                J[:, :, d] = scalar * (es[0] - es[1])
            e = self.err[act]
            _, rho1 = self.huber(self.chi2(act, e))
            out = np.zeros((n, 2, 35), D)
            for k in range(2):
                info, r1 = self.info[act, k], rho1[:, k]
                e0, e1 = e[:, 2 * k], e[:, 2 * k + 1]
                J0, J1 = J[:, 2 * k, :], J[:, 2 * k + 1, :]
                omr0 = (-(info * e0 + 0.0 * e1)) * r1
                omr1 = (-(0.0 * e0 + info * e1)) * r1
                W00, W01, W10, W11 = r1 * info, r1 * 0.0, r1 * 0.0, r1 * info
                for i in range(7):
                    T0 = J0[:, i] * W00 + J1[:, i] * W10
                    T1 = J0[:, i] * W01 + J1[:, i] * W11
                    for j in range(i + 1):
                        out[:, k, i * (i + 1) // 2 + j] = T0 * J0[:, j] + T1 * J1[:, j]
                    out[:, k, 28 + i] = J0[:, i] * omr0 + J1[:, i] * omr1
        return out.reshape(2 * n, 35)


class Optimizer:
    def __init__(self, pr):
        self.pr = pr
        self.g = Graph(pr)
        self.fix = bool(pr["fix_scale"])
        self.x = [0.0] * 7
        self.iterations = self.trials = self.rejected = self.nbad_stops = self.small = self.big = 0
        self.last_rejected = False

    def active_chi2(self, act, S):
        g = self.g
        e = g.errors(act, S)
        g.err[act] = e
        rho0, _ = g.huber(g.chi2(act, e))
        return float(ordered_sum(rho0.reshape(-1)))

    def optimize(self, S, its):
        g = self.g
        act = np.nonzero(~g.gone)[0]
        if len(act) == 0:
            return S
        lam = ni = 0.0
        n_bad = 0
        for it in range(its):
            current = self.active_chi2(act, S)
            ini = current
            terms = g.terms(act, S, self.fix)
            sums = ordered_sum(terms)
            H = np.zeros((7, 7), D)
            for i in range(7):
                for j in range(i + 1):
                    H[i, j] = H[j, i] = sums[i * (i + 1) // 2 + j]
            b = sums[28:]
            self.iterations += 1
            if it == 0:
                mx = 0.0
                for j in range(7):
                    a = abs(float(H[j, j]))
                    mx = mx if a < mx else a
                lam = 1e-5 * mx
                ni = 2.0
                n_bad = 0
            rho = 0.0
            qmax = 0
            while True:
                S_save = S
                Hl = [[float(H[i, j]) + (lam if i == j else 0.0) for j in range(7)] for i in range(7)]
                with np.errstate(all="ignore"):
                    ok, x = ldlt_solve7(Hl, [float(v) for v in b])
                if ok:
                    self.x = x
                S, small = oplus(S, self.x, self.fix)
                self.trials += 1
                self.small += small
                self.big += not small
                temp = self.active_chi2(act, S)
                if not ok:
                    temp = DBL_MAX
                with np.errstate(all="ignore"):
                    rho = float((D(current) - D(temp)) / D(compute_scale(self.x, b, lam)))
                if rho > 0 and math.isfinite(temp):
                    alpha = 1.0 - pon.cr_cube(2 * rho - 1)
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                    self.last_rejected = False
                else:
                    with np.errstate(all="ignore"):
                        lam = float(D(lam) * D(ni))
                        ni = float(D(ni) * 2)
                    S = S_save
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
        return S

    def classify(self, S):
        """(the active matches, their outlier verdict on _error as it stands, the same on errors recomputed at S)"""
        g = self.g
        act = np.nonzero(~g.gone)[0]
        with np.errstate(all="ignore"):
            c = g.chi2(act, g.err[act])
            stale = (c[:, 0] > g.th2) | (c[:, 1] > g.th2)
            c = g.chi2(act, g.errors(act, S))
            fresh = (c[:, 0] > g.th2) | (c[:, 1] > g.th2)
        return act, stale, fresh

    def run(self):
        pr, g = self.pr, self.g
        out = dict(returns=0, n_bad=0, iterations=np.zeros(2, np.int32), trials=np.zeros(2, np.int32), diag=np.zeros(8, np.int32),
                   outlier=np.zeros(g.n, np.uint8))
        S0 = s12_tuple(pr["S12"])
        S = S0
        n_bad = early = last_rejected_phases = stale_decided = 0
        for phase in range(2):
            its = 5 if phase == 0 else (10 if n_bad > 0 else 5)
            it0, tr0 = self.iterations, self.trials
            self.last_rejected = False
            S = self.optimize(S, its)
            out["iterations"][phase] = self.iterations - it0
            out["trials"][phase] = self.trials - tr0
            last_rejected_phases += self.last_rejected
            act, stale, fresh = self.classify(S)
            if self.last_rejected:
                stale_decided += int((stale != fresh).sum())
            g.gone[act[stale]] = True
            if phase == 0:
                n_bad = int(stale.sum())
                if g.n - n_bad < 10:
                    early = 1
                    break
            else:
                out["returns"] = int((~stale).sum())
        if early:
            S = S0
        out["n_bad"] = n_bad
        out["diag"][:7] = (self.rejected, last_rejected_phases, self.nbad_stops, self.small, self.big, early, stale_decided)
        out["outlier"][:] = g.gone
        out["S12"] = np.array(list(S[0]) + list(S[1]) + [S[2]], D)
        out["T12"] = to_cvmat(S)
        out["Scw"] = scw(pr, S)
        return out


def optimize_sim3(pr):
    """Optimizer::OptimizeSim3 of one problem (a dict as problem() makes it): the outputs of drfe_sim3_opt_out for it"""
    return Optimizer(pr).run()


def table(problems):
    """the outputs of a call over these problems, concatenated as lib.sim3_opt_host lays them out"""
    outs = [optimize_sim3(pr) for pr in problems]
    shapes = dict(S12=((0, 8), D), T12=((0, 16), F), Scw=((0, 16), F), iterations=((0, 2), np.int32), trials=((0, 2), np.int32),
                  diag=((0, 8), np.int32))
    r = {}
    for k, (shape, dt) in shapes.items():
        r[k] = np.stack([o[k] for o in outs]).astype(dt) if outs else np.zeros(shape, dt)
    for k in ("returns", "n_bad"):
        r[k] = np.array([o[k] for o in outs], np.int32)
    r["outlier"] = np.concatenate([o["outlier"] for o in outs]) if outs else np.zeros(0, np.uint8)
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# scenes
CAM1 = (517.3, 516.5, 318.6, 255.3)                 # TUM3
CAM2 = (535.4, 539.2, 320.1, 247.6)                 # TUM2


def rot(axis, ang):
    axis = np.asarray(axis, D) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * (Kx @ Kx)


def quat_of(R):
    return pon.normalize_rotation(pon.quat_from_matrix([[float(R[r, c]) for c in range(3)] for r in range(3)]))


def problem(rng, n=60, outlier_frac=0.0, noise=0.7, fix_scale=1, K2=CAM1, start=(0.01, 0.03, 0.0), th2=10.0, scale=1.0,
            identity=False, far=1.0):
    """A loop candidate: key frame 2's camera points P2c in front of it, key frame 1 sees them through the planted S12 (P1c = s R
    P2c + t); each key frame has its own map point of every match (its camera point taken back through its pose).  The start
    estimate is the planted one moved by `start` (rotation angle, translation, log scale).  `identity` puts both key frames at the
    origin with the identity as planted and start estimate, so that the float products leave the camera points as they are.
    `far` scales the scene about key frame 2: at a large one the translation is weakly observable."""
    if identity:
        R1w = R2w = np.eye(3)
        t1w = t2w = np.zeros(3)
        R12, t12, s12 = np.eye(3), np.zeros(3), 1.0
    else:
        R1w, R2w = rot(rng.normal(size=3), rng.uniform(0, 0.8)), rot(rng.normal(size=3), rng.uniform(0, 0.8))
        t1w, t2w = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
        R12, t12 = rot(rng.normal(size=3), rng.uniform(0.02, 0.2)), rng.uniform(-0.3, 0.3, 3)
        s12 = 1.0 if fix_scale and scale == 1.0 else scale
    P2c = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.2, 1.2, n), rng.uniform(1.5, 6.0, n)], axis=1) * far
    P1c = s12 * (P2c @ R12.T) + t12
    P3D2w = (P2c - t2w) @ R2w
    P3D1w = (P1c - t1w) @ R1w

    def proj(P, K):
        return np.stack([P[:, 0] / P[:, 2] * K[0] + K[2], P[:, 1] / P[:, 2] * K[1] + K[3]], axis=1)
    obs1 = proj(P1c, CAM1) + rng.normal(size=(n, 2)) * noise
    obs2 = proj(P2c, K2) + rng.normal(size=(n, 2)) * noise
    bad = rng.permutation(n)[:int(round(outlier_frac * n))]
    obs1[bad] += rng.uniform(15, 60, (len(bad), 2)) * rng.choice([-1, 1], (len(bad), 2))
    octave = rng.integers(0, 8, (n, 2))
    inv = (F(1.0) / (F(1.2) ** octave.astype(F)) ** 2).astype(F)
    if identity:
        Rs, ts, ss = R12, t12, s12
    else:
        Rs = rot(rng.normal(size=3), start[0]) @ R12
        ts = t12 + rng.normal(size=3) * start[1]
        ss = s12 * math.exp(start[2])
    S12 = np.array(quat_of(Rs) + [float(v) for v in ts] + [ss], D)
    return dict(S12=S12, K1=np.array(CAM1, F), K2=np.array(K2, F), R1w=R1w.astype(F).reshape(9), t1w=t1w.astype(F),
                R2w=R2w.astype(F).reshape(9), t2w=t2w.astype(F), th2=F(th2), fix_scale=np.uint8(fix_scale),
                index=np.sort(rng.permutation(4 * n + 4)[:n]).astype(np.int32), P3D1w=P3D1w.astype(F), P3D2w=P3D2w.astype(F),
                obs1=obs1.astype(F), obs2=obs2.astype(F), inv_sigma2_1=inv[:, 0].copy(), inv_sigma2_2=inv[:, 1].copy(),
                planted=(R12, t12, s12))


def depth_problem(seed, kind, z):
    """A problem at the identity whose match 3 has, after the map, depth z on edge `kind` (0: e12 maps P2c, 1: e21 maps P1c), and
    three planted outliers"""
    rng = np.random.default_rng(seed)
    pr = problem(rng, n=40, outlier_frac=0.075, identity=True)
    key = "P3D2w" if kind == 0 else "P3D1w"
    pr[key] = pr[key].copy()
    pr[key][3, 2] = z
    return pr


def behaviour_problems():
    """name -> problem; what each shows is asserted through the diagnostics in test_sim3_opt_cpu.py"""
    rs = np.random.default_rng
    return dict(
        clean=problem(rs(1), n=60, noise=0.5),
        outliers=problem(rs(2), n=80, outlier_frac=0.2),
        # far scenes, found by a search over seeds: the weakly observable translation converges slowly, so that the second
        # optimize() runs into its limit: 5 iterations after no outlier, 10 after some
        five_more=problem(rs(5002), n=46, start=(0.015070262173496132, 11.686579637947009, 0.0), noise=0.0, far=100.0),
        ten_more=problem(rs(5013), n=35, outlier_frac=0.2, start=(0.0038264785211440055, 10.403841337629688, 0.0), noise=0.001,
                         far=300.0),
        too_few=problem(rs(3), n=14, outlier_frac=0.5),
        unequal_k=problem(rs(4), n=50, outlier_frac=0.1, K2=CAM2),
        far_start=problem(rs(5), n=70, outlier_frac=0.1, start=(0.08, 0.25, 0.0)),
        tight=problem(rs(6), n=30, noise=0.05, start=(1e-7, 1e-7, 0.0)),
        nbad_stop=problem(rs(7), n=40, noise=2.5, outlier_frac=0.3, start=(0.0, 0.0, 0.0)),
        z0_e12=depth_problem(11, 0, 0.0),
        z0_e21=depth_problem(12, 1, 0.0),
        zneg_e12=depth_problem(13, 0, -2.0),
        zneg_e21=depth_problem(14, 1, -2.0),
        free_small=problem(rs(8), n=60, outlier_frac=0.1, fix_scale=0, scale=1.0, start=(0.01, 0.03, 1e-7)),
        free_big=problem(rs(9), n=60, outlier_frac=0.1, fix_scale=0, scale=1.3, start=(0.02, 0.05, 0.05)),
    )


SIZES = (0, 9, 10, 11, 63, 64, 65, 255, 256, 257)


def size_problems():
    return [problem(np.random.default_rng(100 + n), n=n, outlier_frac=0.1 if n >= 20 else 0.0) for n in SIZES]


def random_problems(count=20, seed=100):
    """every fourth with a free scale.  Seed 100: under seed 99 one free-scale step's sigma is an argument at which the host's
    libm exp is one ulp from the correctly rounded value the restatement uses (no certified exp exists yet)"""
    rng = np.random.default_rng(seed)
    return [problem(rng, n=int(rng.integers(40, 120)), outlier_frac=0.15, fix_scale=int(i % 4 != 0),
                    scale=1.0 if i % 4 else float(rng.uniform(0.8, 1.25)), start=(0.02, 0.05, 0.02 if i % 4 == 0 else 0.0))
            for i in range(count)]


def mix_problems(count, seed=7, n=24):
    """`count` small problems, every third with a free scale"""
    rng = np.random.default_rng(seed)
    return [problem(rng, n=n + i % 5, outlier_frac=0.1, fix_scale=int(i % 3 != 1), start=(0.01, 0.03, 0.01 if i % 3 == 1 else 0.0))
            for i in range(count)]


def pack(problems):
    """a list of problems as the dict lib._sim3_opt_pack takes"""
    r = {}
    for k in IN_KEYS:
        r[k] = np.stack([np.asarray(pr[k]) for pr in problems]) if problems else np.zeros(0)
    counts = [len(np.asarray(pr["P3D1w"]).reshape(-1, 3)) for pr in problems]
    r["match_offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    for k in MATCH_KEYS:
        parts = [np.asarray(pr[k]) for pr in problems if len(np.asarray(pr[k]))]
        r[k] = np.concatenate(parts) if parts else np.zeros(0)
    return r


_TABLES = {}


def numpy_table(name, problems):
    """table(problems), computed once per name and shared by the tests; never modified"""
    if name not in _TABLES:
        _TABLES[name] = table(problems)
    return _TABLES[name]


# ------------------------------------------------------------------------------------------------------------------------------
# tests/native/sim3_opt_caller.cpp: one current key frame, its loop candidates, and the same problems for the ctypes path
INV_SIGMA2 = (F(1.0) / (F(1.2) ** np.arange(8, dtype=F)) ** 2).astype(F)


def caller_scene(n_cand=4, n_keys=90, seed=21, fix_scale=1):
    """(blob, problems): the current key frame has n_keys key points, of which some have no map point (state 2) or a bad one (1);
    candidate c sees a subset of them through its planted S12 and lists some map points that are bad (1), or do not list it (3):
    the adaptor leaves those out as the reference's `continue`s do.  Candidate 0 has too few matches to be accepted and candidate
    1 too many outliers, so that the loop goes on to candidate 2."""
    import struct
    rng = np.random.default_rng(seed)

    def proj(P, K):
        return np.stack([P[:, 0] / P[:, 2] * K[0] + K[2], P[:, 1] / P[:, 2] * K[1] + K[3]], axis=1)
    R1w, t1w = rot(rng.normal(size=3), 0.4), rng.uniform(-2, 2, 3)
    P1c = np.stack([rng.uniform(-1.5, 1.5, n_keys), rng.uniform(-1.2, 1.2, n_keys), rng.uniform(1.5, 6.0, n_keys)], axis=1)
    P3D1w = ((P1c - t1w) @ R1w).astype(F)
    obs1 = (proj(P1c, CAM1) + rng.normal(size=(n_keys, 2)) * 0.6).astype(F)
    oct1 = rng.integers(0, 8, n_keys).astype(np.int32)
    state1 = rng.choice([0, 0, 0, 0, 0, 0, 1, 2], n_keys).astype(np.uint8)

    def kf_blob(K, R, t, pts, octs, world, states):
        b = np.asarray(K, F).tobytes() + np.asarray(R, F).tobytes() + np.asarray(t, F).tobytes() + struct.pack("<i", len(pts))
        for i in range(len(pts)):
            b += np.asarray(pts[i], F).tobytes() + struct.pack("<i", int(octs[i])) + np.asarray(world[i], F).tobytes()
            b += struct.pack("<B", int(states[i]))
        return b
    th2 = F(10.0)
    blob = struct.pack("<ii", n_cand, fix_scale) + th2.tobytes() + INV_SIGMA2.tobytes()
    blob += kf_blob(CAM1, R1w, t1w, obs1, oct1, P3D1w, state1)
    problems = []
    for c in range(n_cand):
        R2w, t2w = rot(rng.normal(size=3), 0.5), rng.uniform(-2, 2, 3)
        R12, t12 = rot(rng.normal(size=3), rng.uniform(0.02, 0.2)), rng.uniform(-0.3, 0.3, 3)
        seen = np.sort(rng.permutation(n_keys)[:18 if c == 0 else 70])
        order = rng.permutation(len(seen))                       # the candidate's key point j shows the current one's seen[order[j]]
        P2c = (P1c[seen[order]] - t12) @ R12
        P3D2w = ((P2c - t2w) @ R2w).astype(F)
        obs2 = proj(P2c, CAM2) + rng.normal(size=(len(seen), 2)) * 0.6
        if c == 1:
            obs2 += rng.uniform(20, 60, obs2.shape)
        obs2 = obs2.astype(F)
        oct2 = rng.integers(0, 8, len(seen)).astype(np.int32)
        state2 = rng.choice([0, 0, 0, 0, 0, 0, 0, 1, 3], len(seen)).astype(np.uint8)
        match = np.full(n_keys, -1, np.int32)
        match[seen[order]] = np.arange(len(seen))
        match[rng.permutation(n_keys)[:5]] = -1                  # what RANSAC and SearchBySim3 left unmatched
        S12 = np.array(quat_of(rot(rng.normal(size=3), 0.01) @ R12) + [float(v) for v in t12 + rng.normal(size=3) * 0.03] + [1.0], D)
        blob += kf_blob(CAM2, R2w, t2w, obs2, oct2, P3D2w, state2) + S12.tobytes() + match.tobytes()
        keep = [i for i in range(n_keys) if match[i] >= 0 and state1[i] == 0 and state2[match[i]] == 0]
        j = match[keep]
        problems.append(dict(S12=S12, K1=np.array(CAM1, F), K2=np.array(CAM2, F), R1w=R1w.astype(F).reshape(9), t1w=t1w.astype(F),
                             R2w=R2w.astype(F).reshape(9), t2w=t2w.astype(F), th2=th2, fix_scale=np.uint8(fix_scale),
                             index=np.array(keep, np.int32), P3D1w=P3D1w[keep], P3D2w=P3D2w[j], obs1=obs1[keep], obs2=obs2[j],
                             inv_sigma2_1=INV_SIGMA2[oct1[keep]], inv_sigma2_2=INV_SIGMA2[oct2[j]], n_keys=n_keys,
                             unmatched=match < 0))
    return blob, problems


def caller_expected(result, problems):
    """what sim3_opt_caller writes, from the ctypes path's result over caller_scene's problems"""
    import struct
    off = pack(problems)["match_offsets"]

    def record(c):
        pr = problems[c]
        null = pr["unmatched"].astype(np.uint8).copy()
        null[pr["index"][result["outlier"][off[c]:off[c + 1]] != 0]] = 1
        return (struct.pack("<ii", c, int(result["returns"][c])) + result["S12"][c].tobytes() + result["Scw"][c].tobytes()
                + null.tobytes())
    ok = [c for c in range(len(problems)) if result["returns"][c] >= 20]
    first = ok[0] if ok else -1
    loop = b"".join(record(c) for c in range(len(problems) if first < 0 else first + 1))
    batch = b"".join(record(c) for c in range(len(problems)))
    return loop + struct.pack("<i", -1) + batch + struct.pack("<i", -1) + struct.pack("<ii", first, first)
