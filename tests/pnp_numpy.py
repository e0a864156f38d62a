"""An independent restatement of PnPsolver for the tests: the reference's control flow with its per-point
arrays (pws, us, alphas, pcs) kept as the reference keeps them, IEEE double as Python floats (the same format and roundings as
numpy.float64 scalars, math.sqrt correctly rounded), float32 steps as numpy.float32; its own Jacobi SVD, back-substitution,
Householder QR, MulTransposed order and cv::RNG; glibc's rand() and the sampling from ransac_numpy; and a TableWalker with
iterate's `||` loop."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ransac_numpy import GlibcRand, iteration_count, sample_sets, trunc32 as _trunc32  # noqa: E402

F = np.float32
DBL_EPS = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
MAX_CORR, MAX_ITERATIONS, MAX_TAIL, LDS_CORR = 4096, 300, 300, 2048
QNAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), np.float64)[0]


def _div(a, b):
    """IEEE double division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    return math.sqrt(a) if a >= 0 else (math.nan if a == a else a)


def _sqrtn(a):
    """sqrt with the sign of zero and NaN as IEEE"""
    if a != a:
        return a
    if a == 0:
        return a
    if a < 0:
        return math.nan
    return math.inf if a == math.inf else math.sqrt(a)


# ------------------------------------------------------------------------------------------------------------------------------
# SetRansacParameters, sampling
def ransac_parameters(N, probability, min_inliers, max_iterations, epsilon):
    """(mRansacMinInliers, mRansacMaxIts) after SetRansacParameters with minSet = 4"""
    eps = F(epsilon)
    with np.errstate(all="ignore"):
        n_min = _trunc32(F(N) * eps)
        n_min = max(n_min, int(min_inliers), 4)
        q = F(n_min) / F(N)
        if eps < q:
            eps = q
    return n_min, iteration_count(n_min == N, eps, probability, max_iterations)


def sample_quads(seed, N, rows):
    return sample_sets(seed, N, rows, 4)


# ------------------------------------------------------------------------------------------------------------------------------
# OpenCV pieces
class CvRNG:
    def __init__(self, state=0x12345678):
        self.state = state

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF


def jacobi_svd(A, want_v=True):
    """JacobiSVDImpl_<double> of the m x n matrix A (list of rows), m >= n: (w, u_rows, vt).  u_rows[i] is the i-th left singular
    vector (the rotated row i of A^T, normalised), vt[i] the i-th row of the accumulated rotations."""
    m, n = len(A), len(A[0])
    At = [[float(A[k][i]) for k in range(m)] for i in range(n)]
    Vt = [[1.0 if i == k else 0.0 for k in range(n)] for i in range(n)]
    eps, minval = DBL_EPS * 10, DBL_MIN
    W = [0.0] * n
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd += At[i][k] * At[i][k]
        W[i] = sd
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, b, p = W[i], W[j], 0.0
                for k in range(m):
                    p += Ai[k] * Aj[k]
                if abs(p) <= eps * _sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = _sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = _sqrt(_div(delta, gamma))
                    c = _div(p, gamma * s * 2)
                else:
                    c = _sqrt(_div(gamma + beta, gamma * 2))
                    s = _div(p, gamma * c * 2)
                a = b = 0.0
                for k in range(m):
                    t0 = c * Ai[k] + s * Aj[k]
                    t1 = -s * Ai[k] + c * Aj[k]
                    Ai[k], Aj[k] = t0, t1
                    a += t0 * t0
                    b += t1 * t1
                W[i], W[j] = a, b
                changed = True
                Vi, Vj = Vt[i], Vt[j]
                for k in range(n):
                    t0 = c * Vi[k] + s * Vj[k]
                    t1 = -s * Vi[k] + c * Vj[k]
                    Vi[k], Vj[k] = t0, t1
        if not changed:
            break
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd += At[i][k] * At[i][k]
        W[i] = _sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    rng = CvRNG()
    for i in range(n):
        sd = W[i]
        ii = 0
        while ii < 100 and sd <= minval:
            val0 = 1.0 / m
            for k in range(m):
                At[i][k] = val0 if (rng.next() & 256) != 0 else -val0
            for _it in range(2):
                for j in range(i):
                    sd = 0.0
                    for k in range(m):
                        sd += At[i][k] * At[j][k]
                    asum = 0.0
                    for k in range(m):
                        t = At[i][k] - sd * At[j][k]
                        At[i][k] = t
                        asum += abs(t)
                    asum = _div(1, asum) if asum > eps * 100 else 0.0
                    for k in range(m):
                        At[i][k] *= asum
            sd = 0.0
            for k in range(m):
                sd += At[i][k] * At[i][k]
            sd = _sqrt(sd)
            ii += 1
        s = _div(1, sd) if sd > minval else 0.0
        for k in range(m):
            At[i][k] *= s
    return W, At, Vt


def _threshold(w):
    th = 0.0
    for v in w:
        th += v
    return th * (DBL_EPS * 2)


def svd_solve(A, b):
    """cvSolve(A, b, x, CV_SVD), one right-hand side"""
    m, n = len(A), len(A[0])
    w, u, vt = jacobi_svd(A)
    x = [0.0] * n
    th = _threshold(w)
    for i in range(n):
        wi = w[i]
        if abs(wi) <= th:
            continue
        wi = _div(1, wi)
        s = 0.0
        for j in range(m):
            s += u[i][j] * b[j]
        s *= wi
        for j in range(n):
            x[j] = x[j] + s * vt[i][j]
    return x, w, th


def svd_invert3(A):
    """cvInvert(A, Ainv, CV_SVD): (inverse as 9 values, w, threshold)"""
    w, u, vt = jacobi_svd(A)
    x = [0.0] * 9
    th = _threshold(w)
    for i in range(3):
        wi = w[i]
        if abs(wi) <= th:
            continue
        wi = _div(1, wi)
        buf = [u[i][j] * wi for j in range(3)]
        for r in range(3):
            s = vt[i][r]
            for j in range(3):
                x[r * 3 + j] = x[r * 3 + j] + s * buf[j]
    return x, w, th


def mul_transposed(M):
    """cvMulTransposed(M, dst, 1) below gemm's gate: the upper triangle, each element a sum over the rows in order, mirrored"""
    rows, n = len(M), len(M[0])
    out = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):
            s = 0.0
            for k in range(rows):
                s += M[k][i] * M[k][j]
            out[i][j] = s
            out[j][i] = s
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# EPnP
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _dist2(p1, p2):
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2])


class Trace:
    """what a test wants to know about a compute_pose: the matrices handed to the SVD, the early returns of qr_solve, ..."""

    def __init__(self):
        self.svd_inputs = []       # (matrix as list of rows)
        self.qr_early = 0
        self.invert_dropped = 0    # singular values of cvInvert under the SVBkSb threshold
        self.solve_dropped = 0


def qr_solve(a, b, x, trace=None):
    """a: 24 values (6x4), b: 6, x: 4; all modified in place"""
    nr, nc = 6, 4
    A1, A2 = [0.0] * nr, [0.0] * nr
    for k in range(nc):
        kk = k * nc + k
        p = kk
        eta = abs(a[p])
        for _i in range(k + 1, nr):
            elt = abs(a[p])
            if eta < elt:
                eta = elt
            p += nc
        if eta == 0:
            if trace is not None:
                trace.qr_early += 1
            return
        inv_eta = _div(1.0, eta)
        s = 0.0
        p = kk
        for _i in range(k, nr):
            a[p] *= inv_eta
            s += a[p] * a[p]
            p += nc
        sigma = _sqrt(s)
        if a[kk] < 0:
            sigma = -sigma
        a[kk] += sigma
        A1[k] = sigma * a[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            p = kk
            for _i in range(k, nr):
                s += a[p] * a[p + j - k]
                p += nc
            tau = _div(s, A1[k])
            p = kk
            for _i in range(k, nr):
                a[p + j - k] -= tau * a[p]
                p += nc
    for j in range(nc):
        jj = j * nc + j
        tau = 0.0
        p = jj
        for i in range(j, nr):
            tau += a[p] * b[i]
            p += nc
        tau = _div(tau, A1[j])
        p = jj
        for i in range(j, nr):
            b[i] -= tau * a[p]
            p += nc
    x[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        p = i * nc + i + 1
        for j in range(i + 1, nc):
            s += a[p] * x[j]
            p += 1
        x[i] = _div(b[i] - s, A2[i])


def gauss_newton(L, rho, betas, trace=None):
    x = [0.0] * 4
    for _ in range(5):
        a, b = [0.0] * 24, [0.0] * 6
        for i in range(6):
            r = L[i]
            a[4 * i + 0] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3]
            a[4 * i + 1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3]
            a[4 * i + 2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3]
            a[4 * i + 3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3]
            b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] +
                             r[3] * betas[0] * betas[2] + r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] +
                             r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] + r[8] * betas[2] * betas[3] +
                             r[9] * betas[3] * betas[3])
        qr_solve(a, b, x, trace)
        for i in range(4):
            betas[i] += x[i]


def find_betas(which, L, rho, trace=None):
    cols = {1: (0, 1, 3, 6), 2: (0, 1, 2), 3: (0, 1, 2, 3, 4)}[which]
    A = [[L[i][c] for c in cols] for i in range(6)]
    if trace is not None:
        trace.svd_inputs.append(A)
    b, w, th = svd_solve(A, rho)
    if trace is not None:
        trace.solve_dropped += sum(1 for v in w if abs(v) <= th)
    betas = [0.0] * 4
    if which == 1:
        if b[0] < 0:
            betas[0] = _sqrtn(-b[0])
            betas[1] = _div(-b[1], betas[0])
            betas[2] = _div(-b[2], betas[0])
            betas[3] = _div(-b[3], betas[0])
        else:
            betas[0] = _sqrtn(b[0])
            betas[1] = _div(b[1], betas[0])
            betas[2] = _div(b[2], betas[0])
            betas[3] = _div(b[3], betas[0])
        return betas
    if b[0] < 0:
        betas[0] = _sqrtn(-b[0])
        betas[1] = _sqrtn(-b[2]) if b[2] < 0 else 0.0
    else:
        betas[0] = _sqrtn(b[0])
        betas[1] = _sqrtn(b[2]) if b[2] > 0 else 0.0
    if b[1] < 0:
        betas[0] = -betas[0]
    betas[2] = 0.0 if which == 2 else _div(b[3], betas[0])
    return betas


def compute_pose(pws, us, K, trace=None):
    """EPnP over the correspondences pws [n][3], us [n][2] (Python floats); K = (fu, fv, uc, vc).  Returns (R [9], t [3])."""
    n = len(pws)
    fu, fv, uc, vc = K
    cws = [[0.0] * 3 for _ in range(4)]
    for i in range(n):
        for j in range(3):
            cws[0][j] += pws[i][j]
    for j in range(3):
        cws[0][j] = _div(cws[0][j], float(n))
    PW0 = [[pws[i][j] - cws[0][j] for j in range(3)] for i in range(n)]
    G = mul_transposed(PW0)
    if trace is not None:
        trace.svd_inputs.append(G)
    dc, uct, _ = jacobi_svd(G)
    for i in range(1, 4):
        k = _sqrtn(_div(dc[i - 1], float(n)))
        for j in range(3):
            cws[i][j] = cws[0][j] + k * uct[i - 1][j]
    cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
    if trace is not None:
        trace.svd_inputs.append(cc)
    ci, w, th = svd_invert3(cc)
    if trace is not None:
        trace.invert_dropped += sum(1 for v in w if abs(v) <= th)
    alphas = []
    for i in range(n):
        p = pws[i]
        a = [0.0] * 4
        for j in range(3):
            a[1 + j] = ci[3 * j] * (p[0] - cws[0][0]) + ci[3 * j + 1] * (p[1] - cws[0][1]) + ci[3 * j + 2] * (p[2] - cws[0][2])
        a[0] = 1.0 - a[1] - a[2] - a[3]
        alphas.append(a)
    M = []
    for i in range(n):
        a, u, v = alphas[i], us[i][0], us[i][1]
        m1, m2 = [0.0] * 12, [0.0] * 12
        for q in range(4):
            m1[3 * q] = a[q] * fu
            m1[3 * q + 2] = a[q] * (uc - u)
            m2[3 * q + 1] = a[q] * fv
            m2[3 * q + 2] = a[q] * (vc - v)
        M.append(m1)
        M.append(m2)
    MtM = mul_transposed(M)
    if trace is not None:
        trace.svd_inputs.append(MtM)
    _, ut, _ = jacobi_svd(MtM)
    v = [ut[11], ut[10], ut[9], ut[8]]
    dv = [[None] * 6 for _ in range(4)]
    for i in range(4):
        a, b = 0, 1
        for j in range(6):
            dv[i][j] = [v[i][3 * a] - v[i][3 * b], v[i][3 * a + 1] - v[i][3 * b + 1], v[i][3 * a + 2] - v[i][3 * b + 2]]
            b += 1
            if b > 3:
                a += 1
                b = a + 1
    L = []
    for i in range(6):
        L.append([_dot(dv[0][i], dv[0][i]), 2.0 * _dot(dv[0][i], dv[1][i]), _dot(dv[1][i], dv[1][i]),
                  2.0 * _dot(dv[0][i], dv[2][i]), 2.0 * _dot(dv[1][i], dv[2][i]), _dot(dv[2][i], dv[2][i]),
                  2.0 * _dot(dv[0][i], dv[3][i]), 2.0 * _dot(dv[1][i], dv[3][i]), 2.0 * _dot(dv[2][i], dv[3][i]),
                  _dot(dv[3][i], dv[3][i])])
    rho = [_dist2(cws[0], cws[1]), _dist2(cws[0], cws[2]), _dist2(cws[0], cws[3]), _dist2(cws[1], cws[2]),
           _dist2(cws[1], cws[3]), _dist2(cws[2], cws[3])]
    sols = {}
    for which in (1, 2, 3):
        betas = find_betas(which, L, rho, trace)
        gauss_newton(L, rho, betas, trace)
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            for j in range(4):
                for k in range(3):
                    ccs[j][k] += betas[i] * v[i][3 * j + k]
        pcs = [[a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j] for j in range(3)] for a in alphas]
        if pcs[0][2] < 0.0:
            pcs = [[-c for c in p] for p in pcs]
        pc0, pw0 = [0.0] * 3, [0.0] * 3
        for i in range(n):
            for j in range(3):
                pc0[j] += pcs[i][j]
                pw0[j] += pws[i][j]
        for j in range(3):
            pc0[j] = _div(pc0[j], float(n))
            pw0[j] = _div(pw0[j], float(n))
        abt = [[0.0] * 3 for _ in range(3)]
        for i in range(n):
            for j in range(3):
                for k in range(3):
                    abt[j][k] += (pcs[i][j] - pc0[j]) * (pws[i][k] - pw0[k])
        if trace is not None:
            trace.svd_inputs.append([r[:] for r in abt])
        _, u_rows, vt = jacobi_svd(abt)
        # U[i][j] = u_rows[j][i], V[i][j] = vt[j][i]
        R = [[u_rows[0][i] * vt[0][j] + u_rows[1][i] * vt[1][j] + u_rows[2][i] * vt[2][j] for j in range(3)] for i in range(3)]
        det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
               R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
        if det < 0:
            R[2] = [-R[2][0], -R[2][1], -R[2][2]]
        t = [pc0[0] - _dot(R[0], pw0), pc0[1] - _dot(R[1], pw0), pc0[2] - _dot(R[2], pw0)]
        sum2 = 0.0
        for i in range(n):
            pw = pws[i]
            Xc = _dot(R[0], pw) + t[0]
            Yc = _dot(R[1], pw) + t[1]
            inv = _div(1.0, _dot(R[2], pw) + t[2])
            ue = uc + fu * Xc * inv
            ve = vc + fv * Yc * inv
            u, vv = us[i]
            sum2 += _sqrtn((u - ue) * (u - ue) + (vv - ve) * (vv - ve))
        sols[which] = (_div(sum2, float(n)), R, t)
    N = 1
    if sols[2][0] < sols[1][0]:
        N = 2
    if sols[3][0] < sols[N][0]:
        N = 3
    _, R, t = sols[N]
    return [R[i][j] for i in range(3) for j in range(3)], t


def check_inliers(R, t, K, p2d, Xw, max_err):
    """CheckInliers over float32 arrays p2d [N, 2], Xw [N, 3], max_err [N]: bool [N]"""
    N = len(p2d)
    out = np.zeros(N, bool)
    fu, fv, uc, vc = K
    with np.errstate(all="ignore"):
        for i in range(N):
            x, y, z = float(Xw[i, 0]), float(Xw[i, 1]), float(Xw[i, 2])
            Xc = F(R[0] * x + R[1] * y + R[2] * z + t[0])
            Yc = F(R[3] * x + R[4] * y + R[5] * z + t[1])
            invZ = F(_div(1.0, R[6] * x + R[7] * y + R[8] * z + t[2]))
            ue = uc + fu * float(Xc) * float(invZ)
            ve = vc + fv * float(Yc) * float(invZ)
            dx = F(float(p2d[i, 0]) - ue)
            dy = F(float(p2d[i, 1]) - ve)
            e2 = F(F(dx * dx) + F(dy * dy))
            out[i] = bool(e2 < max_err[i])
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the table
def canon(a):
    a = np.array(a, np.float64)
    a[np.isnan(a)] = QNAN
    return a


def pack_mask(inl, words):
    b = np.zeros(words * 64, np.uint8)
    b[:len(inl)] = inl
    return np.packbits(b, bitorder="little").view(np.uint64)


def unpack_mask(row, N):
    return np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder="little")[:N].astype(bool)


def solver_of(problems, s):
    a, b = int(problems["offsets"][s]), int(problems["offsets"][s + 1])
    g = {k: np.asarray(problems[k])[s] for k in ("probability", "min_inliers", "max_iterations", "epsilon", "th2", "tail", "seed")}
    g["K"] = np.asarray(problems["K"], F).reshape(-1, 4)[s]
    g["p2d"] = np.asarray(problems["p2d"], F).reshape(-1, 2)[a:b]
    g["Xw"] = np.asarray(problems["Xw"], F).reshape(-1, 3)[a:b]
    g["sigma2"] = np.asarray(problems["sigma2"], F)[a:b]
    return g


def table(problems, traces=None):
    """The table drfe_pnp_ransac_host fills, in lib._pnp_pack's layout.  traces: a list that receives (s, h or ('refine', h), Trace)."""
    off = np.asarray(problems["offsets"], np.int64)
    n = len(off) - 1
    maxit = np.asarray(problems["max_iterations"], np.int64).reshape(-1)
    tail = np.asarray(problems["tail"], np.int64).reshape(-1)
    cap = np.maximum(maxit, 1) + tail
    words = (np.diff(off) + 63) // 64
    row0 = np.concatenate([[0], np.cumsum(cap)])
    mask0 = np.concatenate([[0], np.cumsum(cap * words)])
    rows, W = int(row0[-1]), int(mask0[-1])
    r = dict(iterations=np.zeros(n, np.int32), min_inliers=np.zeros(n, np.int32), hypotheses=np.zeros(n, np.int32),
             refines=np.zeros(n, np.int32), row0=row0[:-1], words=words, mask0=mask0[:-1],
             sample=np.zeros((rows, 4), np.int32), R=np.zeros((rows, 9)), t=np.zeros((rows, 3)),
             inliers=np.zeros(rows, np.int32), mask=np.zeros(W, np.uint64), best=np.zeros(rows, np.int32),
             returns=np.zeros(rows, np.uint8), refined_R=np.zeros((rows, 9)), refined_t=np.zeros((rows, 3)),
             refined_inliers=np.zeros(rows, np.int32), refined_mask=np.zeros(W, np.uint64))
    for s in range(n):
        g = solver_of(problems, s)
        N = len(g["p2d"])
        mi, it = ransac_parameters(N, g["probability"], g["min_inliers"], g["max_iterations"], g["epsilon"])
        r["iterations"][s], r["min_inliers"][s] = it, mi
        if N < mi:
            continue
        hyp = it + int(g["tail"])
        r["hypotheses"][s] = hyp
        K = tuple(float(v) for v in g["K"])
        max_err = (g["sigma2"] * F(g["th2"])).astype(F)
        pws = [[float(v) for v in p] for p in g["Xw"]]
        us = [[float(v) for v in p] for p in g["p2d"]]
        a, w, m0 = int(row0[s]), int(words[s]), int(mask0[s])
        smp = sample_quads(int(g["seed"]), N, hyp)
        r["sample"][a:a + hyp] = smp
        masks = []
        for h in range(hyp):
            tr = Trace() if traces is not None else None
            R, t = compute_pose([pws[i] for i in smp[h]], [us[i] for i in smp[h]], K, tr)
            if traces is not None:
                traces.append((s, h, tr))
            inl = check_inliers(R, t, K, g["p2d"], g["Xw"], max_err)
            masks.append(inl)
            r["R"][a + h], r["t"][a + h] = canon(R), canon(t)
            r["inliers"][a + h] = int(inl.sum())
            r["mask"][m0 + h * w:m0 + (h + 1) * w] = pack_mask(inl, w)
        best_count, best = 0, -1
        refined = {}
        for h in range(hyp):
            c = int(r["inliers"][a + h])
            if c >= mi:
                if c > best_count:
                    best_count, best = c, h
                if best not in refined:
                    idx = np.flatnonzero(masks[best])
                    tr = Trace() if traces is not None else None
                    R, t = compute_pose([pws[i] for i in idx], [us[i] for i in idx], K, tr)
                    if traces is not None:
                        traces.append((s, ("refine", best), tr))
                    inl = check_inliers(R, t, K, g["p2d"], g["Xw"], max_err)
                    refined[best] = int(inl.sum())
                    r["refined_R"][a + best], r["refined_t"][a + best] = canon(R), canon(t)
                    r["refined_inliers"][a + best] = refined[best]
                    r["refined_mask"][m0 + best * w:m0 + (best + 1) * w] = pack_mask(inl, w)
                r["returns"][a + h] = 1 if refined[best] > mi else 0
            r["best"][a + h] = best
        r["refines"][s] = len(refined)
    return r


TABLE_KEYS = ("iterations", "min_inliers", "hypotheses", "refines", "sample", "R", "t", "inliers", "mask", "best", "returns",
              "refined_R", "refined_t", "refined_inliers", "refined_mask")


def tables_equal(a, b):
    """the keys whose bytes differ"""
    return [k for k in TABLE_KEYS
            if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).astype(a[k].dtype).tobytes()]


# ------------------------------------------------------------------------------------------------------------------------------
# iterate() over a table, and the reference's loop run literally
class OffTheTail(Exception):
    """a schedule needs a row past iterations + tail"""


class TableWalker:
    """PnPsolver::iterate as a cursor over one solver's table t (lib.pnp_table's dict), N its correspondences"""

    def __init__(self, t, N):
        self.t, self.N, self.done = t, N, 0

    def iterate(self, n_iterations):
        """(kind, row, no_more): kind 'refined' (the refined pose of row), 'best' (mBestTcw of row) or None"""
        t = self.t
        if self.N < t["min_inliers"]:
            return None, -1, True
        cur = 0
        while self.done < t["iterations"] or cur < n_iterations:
            if self.done >= len(t["inliers"]):
                raise OffTheTail()
            h = self.done
            cur += 1
            self.done += 1
            if t["returns"][h]:
                return "refined", int(t["best"][h]), False
        if self.done >= t["iterations"]:
            b = int(t["best"][self.done - 1]) if self.done > 0 else -1
            if b >= 0:
                return "best", b, True
            return None, -1, True
        return None, -1, False

    def find(self):
        return self.iterate(self.t["iterations"])


class LiteralSolver:
    """the reference's iterate() (:165-258) statement for statement over member variables, computing every row itself: what
    TableWalker is held to"""

    def __init__(self, g):
        self.g = g
        self.N = len(g["p2d"])
        self.mi, self.max_its = ransac_parameters(self.N, g["probability"], g["min_inliers"], g["max_iterations"], g["epsilon"])
        self.K = tuple(float(v) for v in g["K"])
        self.max_err = (g["sigma2"] * F(g["th2"])).astype(F)
        self.pws = [[float(v) for v in p] for p in g["Xw"]]
        self.us = [[float(v) for v in p] for p in g["p2d"]]
        self.rng = GlibcRand(int(g["seed"]))
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best_row = -1
        self.best_mask = None
        self.refine_cache = {}

    def iterate(self, nIterations):
        if self.N < self.mi:
            return None, -1, True
        nCurrentIterations = 0
        while self.mnIterations < self.max_its or nCurrentIterations < nIterations:
            nCurrentIterations += 1
            self.mnIterations += 1
            avail = list(range(self.N))
            idx = []
            for _ in range(4):
                r = self.rng.random_int(0, len(avail) - 1)
                idx.append(avail[r])
                avail[r] = avail[-1]
                avail.pop()
            R, t = compute_pose([self.pws[i] for i in idx], [self.us[i] for i in idx], self.K)
            inl = check_inliers(R, t, self.K, self.g["p2d"], self.g["Xw"], self.max_err)
            if inl.sum() >= self.mi:
                if inl.sum() > self.mnBestInliers:
                    self.best_mask = inl
                    self.mnBestInliers = int(inl.sum())
                    self.best_row = self.mnIterations - 1
                if self.best_row not in self.refine_cache:     # Refine() is a function of mvbBestInliers alone
                    sel = np.flatnonzero(self.best_mask)
                    R, t = compute_pose([self.pws[i] for i in sel], [self.us[i] for i in sel], self.K)
                    self.refine_cache[self.best_row] = int(check_inliers(R, t, self.K, self.g["p2d"], self.g["Xw"], self.max_err).sum())
                if self.refine_cache[self.best_row] > self.mi:
                    return "refined", self.best_row, False
        if self.mnIterations >= self.max_its:
            if self.mnBestInliers >= self.mi:
                return "best", self.best_row, True
            return None, -1, True
        return None, -1, False

    def find(self):
        return self.iterate(self.max_its)


# ------------------------------------------------------------------------------------------------------------------------------
# scenes
K_DEFAULT = np.array([517.3, 516.5, 318.6, 255.3], F)


def rot(axis, ang):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * Kx @ Kx


def random_solver(rng, N, min_inliers=10, max_iterations=300, probability=0.99, epsilon=0.5, th2=5.991, tail=5, seed=1,
                  outlier_frac=0.3, noise=0.0, K=K_DEFAULT):
    """A camera in front of N world points; a fraction of the image points is moved far away.  Returns (solver dict, truth)."""
    R = rot(rng.normal(size=3), rng.uniform(0.1, 0.6))
    t = rng.uniform(-0.3, 0.3, 3) + np.array([0, 0, 0.5])
    Xc = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.0, 1.0, N), rng.uniform(2.0, 6.0, N)], 1)
    Xw = ((Xc - t) @ R).astype(F)                       # Xc = R Xw + t
    Xc32 = Xw.astype(float) @ R.T + t
    p = np.stack([K[0] * Xc32[:, 0] / Xc32[:, 2] + K[2], K[1] * Xc32[:, 1] / Xc32[:, 2] + K[3]], 1) if N else np.zeros((0, 2))
    p = p + rng.normal(size=p.shape) * noise
    out = rng.random(N) < outlier_frac
    p[out] += rng.uniform(40, 120, (int(out.sum()), 2)) * rng.choice([-1, 1], (int(out.sum()), 2))
    sig = (1.2 ** (2 * rng.integers(0, 4, N))).astype(F)
    f = dict(K=K, probability=probability, min_inliers=min_inliers, max_iterations=max_iterations, epsilon=epsilon, th2=th2,
             tail=tail, seed=seed, p2d=p.astype(F), Xw=Xw, sigma2=sig)
    return f, dict(R=R, t=t, inliers=~out)


def pack(solvers):
    n = len(solvers)
    g = {k: np.array([s[k] for s in solvers], dt) for k, dt in (
        ("probability", np.float64), ("min_inliers", np.int32), ("max_iterations", np.int32), ("epsilon", F), ("th2", F),
        ("tail", np.int32), ("seed", np.uint32))}
    g["K"] = np.array([s["K"] for s in solvers], F).reshape(n, 4)
    g["offsets"] = np.concatenate([[0], np.cumsum([len(s["p2d"]) for s in solvers])]).astype(np.int32)
    g["p2d"] = np.concatenate([np.asarray(s["p2d"], F).reshape(-1, 2) for s in solvers] + [np.zeros((0, 2), F)])
    g["Xw"] = np.concatenate([np.asarray(s["Xw"], F).reshape(-1, 3) for s in solvers] + [np.zeros((0, 3), F)])
    g["sigma2"] = np.concatenate([np.asarray(s["sigma2"], F).reshape(-1) for s in solvers] + [np.zeros(0, F)])
    return g


def degenerate_solvers(rng):
    """dict name -> solver: coplanar world points; four coincident ones (N = 4, every sample is them); a generic scene to tell
    them from; a scene whose hypotheses are NaN.  (A point at Zc == 0 needs a pose that is exact in binary, which no EPnP row
    is: zc_zero_case holds CheckInliers to it under a supplied pose, on the host and through the device's sweep.)"""
    out = {}
    f, _ = random_solver(rng, 12, min_inliers=6, max_iterations=4, tail=1, seed=3, outlier_frac=0.0)
    Xw = f["Xw"].copy()
    Xw[:, 2] = F(1.0)                                   # the plane z = 1
    K = K_DEFAULT
    p = np.stack([K[0] * Xw[:, 0] / F(4) + K[2], K[1] * Xw[:, 1] / F(4) + K[3]], 1)   # camera at z = -3, identity rotation
    out["coplanar"] = dict(f, Xw=Xw, p2d=p.astype(F))
    f, _ = random_solver(rng, 4, min_inliers=4, max_iterations=3, tail=1, seed=5, outlier_frac=0.0)
    out["coincident"] = dict(f, Xw=np.tile(np.array([[0.5, -0.25, 3.0]], F), (4, 1)))
    f, tr = random_solver(rng, 16, min_inliers=6, max_iterations=6, tail=0, seed=7, outlier_frac=0.0)
    out["generic"] = f
    f, _ = random_solver(rng, 9, min_inliers=4, max_iterations=4, tail=1, seed=11, outlier_frac=0.0)
    Xw = f["Xw"].copy()
    Xw[:4] = np.nan                                     # a sample that draws one of them is a NaN hypothesis
    out["nan"] = dict(f, Xw=Xw)
    return out


def zc_zero_case():
    """A pose and points with Zc == 0 exactly, 132 correspondences (three wavefront rounds of the device's sweep):
    (R, t, K, p2d, Xw, max_err, kind) for check_inliers.  kind[i]: 0 a point in front of the camera on its own projection (an
    inlier), 1 Zc == 0 with Xc != 0 (invZc = +inf, an infinite projection), 2 Zc == 0 with Xc == Yc == 0 (fu * 0 * inf: a NaN
    projection, which must fail `error2 < max`)."""
    R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    t = [0.0, 0.0, -2.0]
    base_X = np.array([[0.5, 0.25, 4.0], [0.5, 0.25, 2.0], [0.0, 0.0, 2.0]], F)
    base_p = np.array([[K_DEFAULT[0] * 0.25 + K_DEFAULT[2], K_DEFAULT[1] * 0.125 + K_DEFAULT[3]], [100.0, 100.0],
                       [K_DEFAULT[2], K_DEFAULT[3]]], F)
    kind = np.tile(np.arange(3), 44)
    return (R, t, tuple(float(v) for v in K_DEFAULT), base_p[kind], base_X[kind], np.full(132, 5.991, F), kind)


def searched_solver(seed):
    """one of a family of small noisy scenes with 35 % outliers; the tests name the members they found a property in"""
    rng = np.random.default_rng(1000 + seed)
    N = int(rng.integers(12, 40))
    return random_solver(rng, N, min_inliers=6, max_iterations=10, tail=3, seed=seed, outlier_frac=0.35,
                         noise=float(rng.choice([0.0, 0.5, 1.5])))[0]


# ------------------------------------------------------------------------------------------------------------------------------
# the native caller (tests/native/pnp_caller.cpp)
def caller_scene(rng, verdicts=(0, 0, 1)):
    """Three candidates over one frame of 90 keypoints: (input file bytes, problems of the ctypes path, per candidate the frame
    keypoints its correspondences belong to, the number of keypoints).  Candidate 0 has too few map points (bNoMore at once), 1 and
    2 are planted scenes that see the frame under the same pose."""
    n_keys = 90
    f, _ = random_solver(rng, n_keys, outlier_frac=0.3, noise=0.3)
    octave = rng.integers(0, 8, n_keys).astype(np.int32)
    sig = (1.2 ** (2 * np.arange(8))).astype(F)
    blob = [np.array([3, len(verdicts)], np.int32).tobytes(), np.array(verdicts, np.uint8).tobytes(), K_DEFAULT.tobytes(),
            sig.tobytes(), np.array([n_keys], np.int32).tobytes(), f["p2d"].tobytes(), octave.tobytes()]
    solvers, indices = [], []
    for i in range(3):
        state = rng.choice([0, 1, 2], n_keys, p=[0.7, 0.1, 0.2]).astype(np.uint8)
        if i == 0:
            state[7:] = 2
        world = f["Xw"].copy()
        moved = rng.random(n_keys) < 0.1 * i
        world[moved] += rng.normal(size=(int(moved.sum()), 3)).astype(F)
        blob += [state.tobytes(), world.tobytes()]
        sel = np.flatnonzero(state == 0)
        indices.append(sel)
        solvers.append(dict(K=K_DEFAULT, probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991, tail=5,
                            seed=i + 1, p2d=f["p2d"][sel], Xw=world[sel], sigma2=sig[octave[sel]]))
    return b"".join(blob), pack(solvers), indices, n_keys


def _caller_record(cand, no_more, t, kind, b, index, n_keys):
    T = np.zeros(16, F)
    flags = np.zeros(0, np.uint8)
    n_in = 0
    if kind is not None:
        R, tr, cnt, m = (("refined_R", "refined_t", "refined_inliers", "refined_mask") if kind == "refined" else
                         ("R", "t", "inliers", "mask"))
        T = np.eye(4, dtype=F)
        T[:3, :3] = t[R][b].reshape(3, 3).astype(F)
        T[:3, 3] = t[tr][b].astype(F)
        T = T.reshape(16)
        n_in = int(t[cnt][b])
        flags = np.zeros(n_keys, np.uint8)
        flags[index[unpack_mask(t[m][b], len(index))]] = 1
    return np.array([cand, no_more, int(kind is not None), n_in, len(flags)], np.int32).tobytes() + T.tobytes() + flags.tobytes()


def caller_expected(tables, indices, n_keys, verdicts=(0, 0, 1)):
    """what pnp_caller writes, from the tables (lib.pnp_table dicts, with a tail no walk runs off): (bytes, poses handed back,
    whether a walk read rows past `iterations`)"""
    walkers = [TableWalker(t, len(ix)) for t, ix in zip(tables, indices)]
    out, handed, past = [], 0, False
    alive = [True] * len(walkers)
    match = False
    while any(alive) and not match:
        for i, w in enumerate(walkers):
            if not alive[i]:
                continue
            kind, b, no_more = w.iterate(5)
            past |= w.done > w.t["iterations"]
            if no_more:
                alive[i] = False
            out.append(_caller_record(i, int(no_more), w.t, kind, b, indices[i], n_keys))
            if kind is not None:
                good = handed < len(verdicts) and verdicts[handed] != 0
                handed += 1
                if good:
                    match = True
                    break
    # find() of a fresh solver over the last candidate
    i = len(tables) - 1
    kind, b, _ = TableWalker(tables[i], len(indices[i])).find()
    out.append(_caller_record(-1, 0, tables[i], kind, b, indices[i], n_keys))
    return b"".join(out), handed, past
