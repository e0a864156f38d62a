"""An independent restatement of Sim3Solver (reference src/Sim3Solver.cc) in numpy: every step in float32 / float64 scalars or
element-wise arrays in the order DESIGN.md section 16 reads the reference's OpenCV calls, its own Jacobi and Rodrigues, sin / cos /
atan2 through mpmath rounded once, glibc's rand() and the sampling from ransac_numpy.  Plus a scene generator, the reference's
iterate() run literally (Solver), and a walk over a finished table (TableWalker).  Used by tests/test_sim3_cpu.py and
tests/test_gpu_sim3.py."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ransac_numpy import GlibcRand, iteration_count, sample_sets  # noqa: E402

F = np.float32
D = np.float64
DBL_EPS = 2.220446049250313e-16
FLT_EPS = F(1.1920929e-07)
QNAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]
MAX_CORR, MAX_ITERATIONS = 4096, 300


# ------------------------------------------------------------------------------------------------------------------------------
# SetRansacParameters, sampling
def sample_triples(seed, N, iterations):
    return sample_sets(seed, N, iterations, 3)


def ransac_iterations(N, probability, min_inliers, max_iterations):
    """SetRansacParameters: the clamped mRansacMaxIts"""
    with np.errstate(all="ignore"):
        eps = F(min_inliers) / F(N)
    return iteration_count(min_inliers == N, eps, probability, max_iterations)


# ------------------------------------------------------------------------------------------------------------------------------
# libm
def _mp():
    import mpmath
    mpmath.mp.prec = 400
    return mpmath


def cr_atan2(y, x):
    """atan2 of two doubles, y >= 0, correctly rounded"""
    y, x = float(y), float(x)
    if y != y or x != x:
        return math.nan
    if y == 0 or x == 0 or math.isinf(y) or math.isinf(x):
        return math.atan2(y, x)              # exact cases: 0, pi/4, pi/2, 3pi/4, pi as the nearest doubles
    mp = _mp()
    return float(mp.atan2(mp.mpf(y), mp.mpf(x)))


def cr_sincos(t):
    t = float(t)
    if t != t or math.isinf(t):
        return math.nan, math.nan
    mp = _mp()
    return float(mp.sin(mp.mpf(t))), float(mp.cos(mp.mpf(t)))


# ------------------------------------------------------------------------------------------------------------------------------
# OpenCV readings
def scale32(v, alpha):
    """convertTo(CV_32F, alpha) of float32 data: a copy when alpha is 1 within DBL_EPSILON, else v * (float)alpha + 0.f"""
    if abs(float(alpha) - 1.0) < DBL_EPS:
        return v
    return v * F(alpha) + F(0)


def gemm_rows(A, X, alpha, c, beta):
    """(float)(t * alpha + c * beta) with t the float dot of A's row r (3 floats) and X's columns; X [..., 3]"""
    out = []
    for r in range(3):
        t = A[r][0] * X[..., 0] + A[r][1] * X[..., 1] + A[r][2] * X[..., 2]
        out.append((np.asarray(t, D) * D(alpha) + D(c[r]) * D(beta)).astype(F))
    return np.stack(out, -1)


def apply34(T, X):
    T = np.asarray(T, F).reshape(3, 4)
    return gemm_rows(T[:, :3], X, 1.0, T[:, 3], 1.0)


def to_image(P, K):
    invz = F(1) / P[..., 2]
    x, y = P[..., 0] * invz, P[..., 1] * invz
    return np.stack([K[0] * x + K[2], K[1] * y + K[3]], -1)


def bound32(sigma2):
    """vector<size_t>::push_back(9.210 * sigma2) read back in a float comparison"""
    return (D(9.210) * np.asarray(sigma2, D)).astype(np.uint64).astype(F)


def hyp32(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(F(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(F(1) + a * a)
    return F(0)


def jacobi4(A):
    """cv::eigen of a symmetric 4x4 float32 matrix (JacobiImpl_<float>): eigenvalues descending, eigenvectors as rows"""
    n = 4
    A = [[F(A[i][j]) for j in range(n)] for i in range(n)]
    V = [[F(1) if i == j else F(0) for j in range(n)] for i in range(n)]
    W = [A[i][i] for i in range(n)]
    indR, indC = [0] * n, [0] * n

    def row_max(k):
        m, mv = k + 1, abs(A[k][k + 1])
        for i in range(k + 2, n):
            if mv < abs(A[k][i]):
                mv, m = abs(A[k][i]), i
        return m

    def col_max(k):
        m, mv = 0, abs(A[0][k])
        for i in range(1, k):
            if mv < abs(A[i][k]):
                mv, m = abs(A[i][k]), i
        return m
    for k in range(n):
        if k < n - 1:
            indR[k] = row_max(k)
        if k > 0:
            indC[k] = col_max(k)
    for _ in range(n * n * 30):
        k, mv = 0, abs(A[0][indR[0]])
        for i in range(1, n - 1):
            if mv < abs(A[i][indR[i]]):
                mv, k = abs(A[i][indR[i]]), i
        l = indR[k]
        for i in range(1, n):
            if mv < abs(A[indC[i]][i]):
                mv, k, l = abs(A[indC[i]][i]), indC[i], i
        p = A[k][l]
        if abs(p) <= FLT_EPS:
            break
        y = F(D(W[l] - W[k]) * D(0.5))
        t = abs(y) + hyp32(p, y)
        s = hyp32(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        A[k][l] = F(0)
        W[k] = W[k] - t
        W[l] = W[l] + t

        def rot(a0, b0):
            return a0 * c - b0 * s, a0 * s + b0 * c
        for i in range(k):
            A[i][k], A[i][l] = rot(A[i][k], A[i][l])
        for i in range(k + 1, l):
            A[k][i], A[i][l] = rot(A[k][i], A[i][l])
        for i in range(l + 1, n):
            A[k][i], A[l][i] = rot(A[k][i], A[l][i])
        for i in range(n):
            V[k][i], V[l][i] = rot(V[k][i], V[l][i])
        for idx in (k, l):
            if idx < n - 1:
                indR[idx] = row_max(idx)
            if idx > 0:
                indC[idx] = col_max(idx)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return W, V


def rodrigues(vec):
    """cv::Rodrigues of a float32 rotation vector into a float32 3x3 (double inside)"""
    r = [D(v) for v in vec]
    theta = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    eye = [D(1), D(0), D(0), D(0), D(1), D(0), D(0), D(0), D(1)]
    if theta < DBL_EPS:
        return np.array(eye, F).reshape(3, 3)
    s, c = (D(v) for v in cr_sincos(theta))
    c1 = D(1) - c
    itheta = D(1) / theta if theta != 0 else D(0)
    rx, ry, rz = r[0] * itheta, r[1] * itheta, r[2] * itheta
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [D(0), -rz, ry, rz, D(0), -rx, -ry, rx, D(0)]
    return np.array([F(c * eye[k] + c1 * rrt[k] + s * r_x[k]) for k in range(9)], F).reshape(3, 3)


def centroid(P):
    """P 3x3 float32, one point per column: Pr, C"""
    C = np.zeros(3, F)
    for r in range(3):
        C[r] = scale32((P[r, 0] + P[r, 2]) + P[r, 1], 1.0 / 3)
    return (P - C[:, None]).astype(F), C


def compute_sim3(P1, P2, fix_scale):
    """ComputeSim3: R12 [3, 3], t12 [3], s12, T12 [3, 4], T21 [3, 4], float32"""
    with np.errstate(all="ignore"):
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = np.zeros((3, 3), F)
        for i in range(3):
            for j in range(3):
                s0 = D(0)
                for k in range(3):
                    s0 = s0 + D(Pr2[i, k]) * D(Pr1[j, k])
                M[i, j] = F(s0 * D(1))
        N11 = M[0, 0] + M[1, 1] + M[2, 2]
        N12, N13, N14 = M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
        N22 = M[0, 0] - M[1, 1] - M[2, 2]
        N23, N24 = M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]
        N33 = -M[0, 0] + M[1, 1] - M[2, 2]
        N34 = M[1, 2] + M[2, 1]
        N44 = -M[0, 0] - M[1, 1] + M[2, 2]
        _, V = jacobi4([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]])
        vec = [V[0][1], V[0][2], V[0][3]]
        n2 = D(0)
        for v in vec:
            n2 = n2 + D(v) * D(v)
        nrm = np.sqrt(n2)
        ang = D(cr_atan2(nrm, D(V[0][0])))
        alpha = (D(2) * ang) * (D(1) / nrm)
        vec = [scale32(v, alpha) for v in vec]
        R = rodrigues(vec)
        P3 = gemm_rows(R, Pr2.T.copy(), 1.0, [F(0)] * 3, 0.0).T.copy()       # P3[r, q]
        s = F(1)
        if not fix_scale:
            a, b = Pr1.reshape(9), P3.reshape(9)
            p = [D(a[k]) * D(b[k]) for k in range(9)]
            nom = D(0)
            nom = nom + (((p[0] + p[1]) + p[2]) + p[3])
            nom = nom + (((p[4] + p[5]) + p[6]) + p[7])
            nom = nom + p[8]
            den = D(0)
            for k in range(9):
                den = den + D(b[k] * b[k])
            s = F(nom / den)
        t = gemm_rows(R, O2, -D(s), O1, 1.0)
        sR = np.array([[scale32(R[r, q], D(s)) for q in range(3)] for r in range(3)], F)
        inv = D(1) / D(s)
        sRinv = np.array([[scale32(R[q, r], inv) for q in range(3)] for r in range(3)], F)
        tinv = gemm_rows(sRinv, t, -1.0, [F(0)] * 3, 0.0)
        T12 = np.concatenate([sR, t[:, None]], 1).astype(F)
        T21 = np.concatenate([sRinv, tinv[:, None]], 1).astype(F)
    return R, t, s, T12, T21


def canon(a):
    a = np.array(a, F)
    a[np.isnan(a)] = QNAN
    return a


class Corrs:
    """the constructor: camera points, image points, bounds of one solver"""

    def __init__(self, Tcw1, Tcw2, K1, K2, Xw1, Xw2, sigma2_1, sigma2_2):
        with np.errstate(all="ignore"):
            self.K1, self.K2 = np.asarray(K1, F), np.asarray(K2, F)
            self.c1 = apply34(Tcw1, np.asarray(Xw1, F).reshape(-1, 3))
            self.c2 = apply34(Tcw2, np.asarray(Xw2, F).reshape(-1, 3))
            self.p1, self.p2 = to_image(self.c1, self.K1), to_image(self.c2, self.K2)
            self.b1, self.b2 = bound32(sigma2_1), bound32(sigma2_2)
        self.N = len(self.c1)

    def check_inliers(self, T12, T21):
        with np.errstate(all="ignore"):
            q21 = to_image(apply34(T12, self.c2), self.K1)
            q12 = to_image(apply34(T21, self.c1), self.K2)
            self.last_projections = (q21, q12)

            def err(d):
                d = d.astype(D)
                s = D(0) + d[:, 0] * d[:, 0]
                s = s + d[:, 1] * d[:, 1]
                return s.astype(F)
            return (err(self.p1 - q21) < self.b1) & (err(q12 - self.p2) < self.b2)

    def hypothesis(self, smp, fix_scale):
        P1 = self.c1[smp].T.copy()
        P2 = self.c2[smp].T.copy()
        R, t, s, T12, T21 = compute_sim3(P1, P2, fix_scale)
        inl = self.check_inliers(T12, T21) if self.N else np.zeros(0, bool)
        return R, t, s, T12, inl


def solver_of(problems, s):
    o = problems["offsets"]
    a, b = int(o[s]), int(o[s + 1])
    return Corrs(problems["Tcw1"][s], problems["Tcw2"][s], problems["K1"][s], problems["K2"][s], problems["Xw1"][a:b],
                 problems["Xw2"][a:b], problems["sigma2_1"][a:b], problems["sigma2_2"][a:b])


def pack_mask(inl, words):
    m = np.zeros(words, np.uint64)
    for i in np.nonzero(inl)[0]:
        m[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return m


def table(problems, want_projections=False):
    """the whole table of a problem set in the layout of lib.sim3_ransac_host's result; with want_projections also the list of
    every projection array (FromCameraToImage's pair per solver, Project's pair per hypothesis), for tests that look for inf"""
    off = np.asarray(problems["offsets"], np.int64)
    n = len(off) - 1
    cap = np.maximum(np.asarray(problems["max_iterations"], np.int64).reshape(n), 1)
    words = (np.diff(off) + 63) // 64
    row0 = np.concatenate([[0], np.cumsum(cap)])
    mask0 = np.concatenate([[0], np.cumsum(cap * words)])
    rows = int(row0[-1])
    r = dict(iterations=np.zeros(n, np.int32), hypotheses=np.zeros(n, np.int32), row0=row0[:-1], words=words, mask0=mask0[:-1],
             sample=np.zeros((rows, 3), np.int32), R12=np.zeros((rows, 9), F), t12=np.zeros((rows, 3), F), s12=np.zeros(rows, F),
             T12=np.zeros((rows, 12), F), inliers=np.zeros(rows, np.int32), returns=np.zeros(rows, np.uint8),
             best=np.zeros(rows, np.int32), mask=np.zeros(int(mask0[-1]), np.uint64))
    proj = []
    for s in range(n):
        N = int(off[s + 1] - off[s])
        mi = int(problems["min_inliers"][s])
        it = ransac_iterations(N, problems["probability"][s], mi, problems["max_iterations"][s])
        r["iterations"][s] = it
        hyp = 0 if (N < mi or N < 3) else it
        r["hypotheses"][s] = hyp
        if not hyp:
            continue
        C = solver_of(problems, s)
        if want_projections:
            proj.append((C.p1, C.p2))                             # FromCameraToImage's
        smp = sample_triples(problems["seed"][s], N, hyp)
        best_n, best_i = 0, -1
        for h in range(hyp):
            row = int(row0[s]) + h
            R, t, sc, T12, inl = C.hypothesis(smp[h], bool(problems["fix_scale"][s]))
            if want_projections:
                proj.append(C.last_projections)
            cnt = int(inl.sum())
            r["sample"][row] = smp[h]
            r["R12"][row], r["t12"][row], r["s12"][row], r["T12"][row] = canon(R).reshape(9), canon(t), canon(sc), canon(T12).reshape(12)
            r["inliers"][row] = cnt
            w = int(words[s])
            m0 = int(mask0[s]) + h * w
            r["mask"][m0:m0 + w] = pack_mask(inl, w)
            if cnt >= best_n:
                best_n, best_i = cnt, h
                r["returns"][row] = 1 if cnt > mi else 0
            r["best"][row] = best_i
    return (r, proj) if want_projections else r


TABLE_KEYS = ("iterations", "hypotheses", "sample", "R12", "t12", "s12", "T12", "inliers", "returns", "best", "mask")


def tables_equal(a, b):
    """the names of the arrays whose bytes differ"""
    return [k for k in TABLE_KEYS if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


# ------------------------------------------------------------------------------------------------------------------------------
# iterate()
class Solver:
    """Sim3Solver as the reference runs it: iterate() computes its hypotheses one after the other (lines 144-211), with the
    solver's own rand() stream"""

    def __init__(self, problems, s, n1=None, indices1=None):
        o = problems["offsets"]
        self.C = solver_of(problems, s)
        self.N = int(o[s + 1] - o[s])
        self.indices1 = np.arange(self.N) if indices1 is None else np.asarray(indices1)
        self.n1 = self.N if n1 is None else n1
        self.fix = bool(problems["fix_scale"][s])
        self.min_inliers = int(problems["min_inliers"][s])
        self.max_its = ransac_iterations(self.N, problems["probability"][s], self.min_inliers, problems["max_iterations"][s])
        self.rng = GlibcRand(problems["seed"][s])
        self.n_iterations, self.best_inliers = 0, 0
        self.best = None

    def iterate(self, n_iterations):
        """-> (T12 or None, bNoMore, vbInliers, nInliers)"""
        vb = np.zeros(self.n1, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.n_iterations < self.max_its and cur < n_iterations:
            cur += 1
            self.n_iterations += 1
            avail = list(range(self.N))
            smp = []
            for _ in range(3):
                r = self.rng.random_int(0, len(avail) - 1)
                smp.append(avail[r])
                avail[r] = avail[-1]
                avail.pop()
            R, t, s, T12, inl = self.C.hypothesis(np.array(smp), self.fix)
            cnt = int(inl.sum())
            if cnt >= self.best_inliers:
                self.best_inliers = cnt
                self.best = (canon(R), canon(t), canon(s), canon(T12))
                if cnt > self.min_inliers:
                    vb[self.indices1[inl]] = True
                    return canon(T12), False, vb, cnt
        return None, self.n_iterations >= self.max_its, vb, 0

    def find(self):
        T, _, vb, n = self.iterate(self.max_its)
        return T, vb, n


class TableWalker:
    """the same interface over a finished table (lib.sim3_table of one solver): a cursor and nothing else"""

    def __init__(self, tab, N, min_inliers, n1=None, indices1=None):
        self.t, self.N, self.min_inliers = tab, N, min_inliers
        self.indices1 = np.arange(N) if indices1 is None else np.asarray(indices1)
        self.n1 = N if n1 is None else n1
        self.cursor = 0
        self.best = None

    def iterate(self, n_iterations):
        vb = np.zeros(self.n1, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        t = self.t
        rows = len(t["inliers"])                                # == iterations wherever the reference's loop is defined (N >= 3)
        while self.cursor < rows and cur < n_iterations:
            h = self.cursor
            cur += 1
            self.cursor += 1
            b = int(t["best"][h])
            self.best = (t["R12"][b].reshape(3, 3), t["t12"][b], t["s12"][b], t["T12"][b].reshape(3, 4))
            if t["returns"][h]:
                bits = np.unpackbits(t["mask"][h].view(np.uint8), bitorder="little")[:self.N].astype(bool)
                vb[self.indices1[bits]] = True
                return t["T12"][h].reshape(3, 4), False, vb, int(t["inliers"][h])
        return None, self.cursor >= rows, vb, 0

    def find(self):
        T, _, vb, n = self.iterate(self.t["iterations"])
        return T, vb, n


# ------------------------------------------------------------------------------------------------------------------------------
# scenes
def rot(axis, ang):
    axis = np.asarray(axis, D) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def pose(R, t):
    return np.concatenate([np.asarray(R, D), np.asarray(t, D).reshape(3, 1)], 1).astype(F).reshape(12)


K_DEFAULT = np.array([517.3, 516.5, 318.6, 255.3], F)


def random_solver(rng, N, fix_scale=False, min_inliers=20, max_iterations=300, probability=0.99, seed=1, outlier_frac=0.3,
                  scale=1.0, noise=0.0, levels=8, pose1=None):
    """One solver as a dict of per-solver fields and per-correspondence arrays.  Map 2 is map 1 moved by a similarity (s, R, t);
    the inliers are exact up to float rounding plus `noise`, the outliers' second points are moved so that both images see them
    >= 50 px away.  Returns (fields, truth) with truth = dict(inlier mask, s, R, t)."""
    Rcw1, Rcw2 = rot(rng.normal(size=3), rng.uniform(0, 0.3)), rot(rng.normal(size=3), rng.uniform(0, 0.3))
    tcw1, tcw2 = rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.2, 0.2, 3)
    if pose1 is not None:
        Rcw1, tcw1 = pose1
    # points in front of camera 1
    Pc1 = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.0, 1.0, N), rng.uniform(2.0, 6.0, N)], 1)
    Xw1 = (Pc1 - tcw1) @ Rcw1                                        # Rcw1^T (Pc1 - tcw1)
    # camera-frame similarity: Pc1 = s R Pc2 + t
    s = scale if not fix_scale else 1.0
    R12, t12 = rot(rng.normal(size=3), rng.uniform(0.05, 0.5)), rng.uniform(-0.3, 0.3, 3)
    Pc2 = ((Pc1 - t12) @ R12) / s
    inl = np.ones(N, bool)
    n_out = int(round(outlier_frac * N))
    if n_out:
        out_idx = rng.choice(N, n_out, replace=False)
        inl[out_idx] = False
        # >= 50 px at f ~ 517 and z <= 6 / s: a lateral move of 1.2 / s (>= 100 px) in the frame of camera 2, the same
        # displacement seen from camera 1 is s * 1.2 / s = 1.2 at z <= 6.5 (>= 90 px)
        ang = rng.uniform(0, 2 * math.pi, n_out)
        Pc2[out_idx, 0] += 1.2 / s * np.cos(ang)
        Pc2[out_idx, 1] += 1.2 / s * np.sin(ang)
    Pc2 = Pc2 + rng.normal(size=Pc2.shape) * noise
    Xw2 = (Pc2 - tcw2) @ Rcw2
    sig = (1.2 ** np.arange(levels)) ** 2
    f = dict(Tcw1=pose(Rcw1, tcw1), Tcw2=pose(Rcw2, tcw2), K1=K_DEFAULT.copy(), K2=K_DEFAULT.copy(), fix_scale=int(fix_scale),
             probability=probability, min_inliers=min_inliers, max_iterations=max_iterations, seed=seed,
             Xw1=Xw1.astype(F), Xw2=Xw2.astype(F), sigma2_1=sig[rng.integers(0, levels, N)].astype(F),
             sigma2_2=sig[rng.integers(0, levels, N)].astype(F))
    return f, dict(inliers=inl, s=s, R=R12, t=t12)


def pack(solvers):
    """a list of random_solver fields -> the problem-set dict of lib.sim3_ransac_host"""
    n = len(solvers)

    def col(k, dt, w=None):
        if n == 0:
            return np.zeros((0,) if w is None else (0, w), dt)
        return np.stack([np.asarray(s[k], dt) for s in solvers])

    def cat(k, w=None):
        parts = [np.asarray(s[k], F).reshape((-1,) if w is None else (-1, w)) for s in solvers]
        return np.concatenate(parts) if parts else np.zeros((0,) if w is None else (0, w), F)
    off = np.concatenate([[0], np.cumsum([len(s["sigma2_1"]) for s in solvers])]).astype(np.int32)
    return dict(Tcw1=col("Tcw1", F, 12), Tcw2=col("Tcw2", F, 12), K1=col("K1", F, 4), K2=col("K2", F, 4),
                fix_scale=col("fix_scale", np.uint8), probability=col("probability", D), min_inliers=col("min_inliers", np.int32),
                max_iterations=col("max_iterations", np.int32), seed=col("seed", np.uint32), offsets=off, Xw1=cat("Xw1", 3),
                Xw2=cat("Xw2", 3), sigma2_1=cat("sigma2_1"), sigma2_2=cat("sigma2_2"))


def degenerate_solvers(rng):
    """[repeated world points, three collinear points only (every sample is collinear), a point on a camera's z = 0 plane]"""
    out = []
    f, _ = random_solver(rng, 30, min_inliers=5, max_iterations=40, seed=3)
    f["Xw1"][:] = f["Xw1"][0]                                      # every sample repeats one point: N = 0, NaN hypotheses
    f["Xw2"][:] = f["Xw2"][0]
    out.append(f)
    f, _ = random_solver(rng, 3, min_inliers=0, max_iterations=6, seed=4)
    for k in ("Xw1", "Xw2"):
        f[k][1] = f[k][0] + F(0.5) * (f[k][2] - f[k][0])
    # exactly collinear in the camera frames too: identity poses, points on a coordinate line
    f["Tcw1"] = pose(np.eye(3), np.zeros(3))
    f["Tcw2"] = pose(np.eye(3), np.zeros(3))
    f["Xw1"] = np.array([[0, 0, 2], [0, 0, 3], [0, 0, 4]], F)
    f["Xw2"] = np.array([[0, 0, 2], [0, 0, 3], [0, 0, 4]], F)
    out.append(f)
    f, _ = random_solver(rng, 40, min_inliers=5, max_iterations=30, seed=5, outlier_frac=0.1)
    f["Tcw1"] = pose(np.eye(3), np.zeros(3))
    f["Xw1"][7, 2] = 0.0                                           # camera 1 sees it at z = 0 exactly
    f["Tcw2"] = pose(np.eye(3), np.zeros(3))
    f["Xw2"][11, 2] = 0.0
    out.append(f)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# tests/native/sim3_caller.cpp
def _kf_bytes(Tcw12, K, sig, octave, world, state):
    T = np.concatenate([np.asarray(Tcw12, F).reshape(12), np.array([0, 0, 0, 1], F)])
    return b"".join([T.tobytes(), np.asarray(K, F).tobytes(), np.asarray(sig, F).tobytes(), np.int32(len(octave)).tobytes(),
                     np.asarray(octave, np.int32).tobytes(), np.asarray(world, F).tobytes(), np.asarray(state, np.uint8).tobytes()])


def caller_scene(rng, fix_scale):
    """One current keyframe and three loop candidates for sim3_caller: (input bytes, problems as the adaptor compacts them,
    [mvnIndices1 per candidate], number of current keypoints).  Some map points are bad, missing or do not list their keyframe,
    some matches are empty; the second candidate is mostly outliers."""
    sig = ((F(1.2) ** np.arange(8, dtype=F)) ** 2).astype(F)
    pose1 = (rot(rng.normal(size=3), 0.2), rng.uniform(-0.2, 0.2, 3))
    sizes, fracs = (60, 45, 80), (0.3, 0.85, 0.3)
    cands = [random_solver(rng, n, fix_scale=fix_scale, min_inliers=20, max_iterations=300, seed=i + 1, outlier_frac=fr,
                           scale=1.0 if fix_scale else 1.25, pose1=pose1)[0] for i, (n, fr) in enumerate(zip(sizes, fracs))]
    n1 = sum(sizes) + 10
    oct1 = rng.integers(0, 8, n1)
    state1 = np.zeros(n1, np.uint8)
    state1[rng.choice(sum(sizes), 9, replace=False)] = [1, 1, 1, 2, 2, 2, 3, 3, 3]
    state1[sum(sizes):] = 2
    world1 = np.zeros((n1, 3), F)
    world1[:sum(sizes)] = np.concatenate([c["Xw1"] for c in cands])
    blob = [np.int32([3, int(fix_scale)]).tobytes(), _kf_bytes(cands[0]["Tcw1"], K_DEFAULT, sig, oct1, world1, state1)]
    solvers, indices = [], []
    start = 0
    for c, n in zip(cands, sizes):
        perm = rng.permutation(n)                                 # current key start + j is matched to candidate key perm[j]
        oct2 = rng.integers(0, 8, n)
        state2 = np.zeros(n, np.uint8)
        state2[rng.choice(n, 4, replace=False)] = [1, 1, 3, 3]    # a matched map point always exists: 2 does not occur here
        world2 = np.zeros((n, 3), F)
        world2[perm] = c["Xw2"]
        m12 = np.full(n1, -1, np.int32)
        m12[start:start + n] = perm
        m12[start + rng.choice(n, 3, replace=False)] = -1
        blob += [_kf_bytes(c["Tcw2"], K_DEFAULT, sig, oct2, world2, state2), m12.tobytes()]
        keep = [j for j in range(n1) if m12[j] >= 0 and state1[j] == 0 and state2[m12[j]] == 0]
        keep = np.array(keep, np.int64)
        f = dict(c)
        f.update(Xw1=world1[keep], Xw2=world2[m12[keep]], sigma2_1=sig[oct1[keep]], sigma2_2=sig[oct2[m12[keep]]])
        solvers.append(f)
        indices.append(keep)
        start += n
    return b"".join(blob), pack(solvers), indices, n1


def caller_expected(walkers):
    """the records sim3_caller writes, from one TableWalker per candidate: LoopClosing::ComputeSim3's loop, five iterations per
    candidate in turn, the third transform handed back accepted"""
    out = []
    discarded = [False] * len(walkers)
    left, handed, match = len(walkers), 0, False
    while left > 0 and not match:
        for i, w in enumerate(walkers):
            if discarded[i]:
                continue
            T, no_more, vb, n = w.iterate(5)
            if no_more:
                discarded[i] = True
                left -= 1
            v = np.zeros(29, F)
            if T is not None:
                R, t, s, _ = w.best
                v[:12] = np.asarray(T, F).reshape(12)
                v[15] = 1
                v[16:25], v[25:28], v[28] = np.asarray(R, F).reshape(9), t, s
            out += [np.int32([i, int(no_more), int(T is not None), n]).tobytes(), v.tobytes(), vb.astype(np.uint8).tobytes()]
            if T is not None:
                handed += 1
                if handed >= 3:
                    match = True
                    break
    return b"".join(out), handed
