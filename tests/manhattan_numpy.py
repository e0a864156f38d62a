"""An independent numpy restatement of the reference's Manhattan-frame tracker (src/Tracking.cc: ProjectSN2Conic :1198-1266,
ProjectSN2MF :1055-1196, TrackManhattanFrame :1336-1527, MeanShift :1529-1546) with the OpenCV pieces it calls (DESIGN.md
section 11), written from the reference text with float32 / float64 numpy operations only: element-wise float32 arrays for the
per-record float arithmetic, float64 for the double arithmetic, np.add.accumulate for MeanShift's sequential sums.  asin,
exp and tanf are the canonical routines of include/drfe_math.h, restated here as the same polynomials.

track(R, normals, dirs, n_calls) returns (R_out, info dict per call, rec_bits, line_bits, hits) where `hits` counts which
branches were taken (tests assert that every case of the issue was reached)."""
import collections

import numpy as np

f32, f64 = np.float32, np.float64
SIN_NORMAL = float.fromhex("0x1.9a7caf08cdfccp-3")
SIN_LINE = float.fromhex("0x1.a040c2f653a3cp-4")
SIN_MS = float.fromhex("0x1.fe4118cace77ep-3")
INLINE = 0x8000

_ASIN_C = [0.004660143486915096, 0.005153309682319905, 0.005740037670841924, 0.006447210311889649, 0.0073125258735988454,
           0.008390335809616815, 0.009761609529194078, 0.011551800896139705, 0.01396484375, 0.017352764423076924,
           0.022372159090909092, 0.030381944444444444, 0.044642857142857144, 0.075, 0.16666666666666666]
_EXP_C = [1.5619206968586225e-16, 2.8114572543455206e-15, 4.779477332387385e-14, 7.647163731819816e-13, 1.1470745597729725e-11,
          1.6059043836821613e-10, 2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06,
          2.48015873015873e-05, 0.0001984126984126984, 0.001388888888888889, 0.008333333333333333, 0.041666666666666664,
          0.16666666666666666, 0.5]
_SIN_C = [2.81145725434552076320e-15, -7.64716373181981647590e-13, 1.60590438368216145994e-10, -2.50521083854417187751e-08,
          2.75573192239858906526e-06, -1.98412698412698412698e-04, 8.33333333333333333333e-03, -1.66666666666666666667e-01]
_COS_C = [-1.56192069685862264622e-16, 4.77947733238738529744e-14, -1.14707455977297247139e-11, 2.08767569878680989792e-09,
          -2.75573192239858906526e-07, 2.48015873015873015873e-05, -1.38888888888888888889e-03, 4.16666666666666666667e-02,
          -5.00000000000000000000e-01]


def _horner(c, z):
    p = np.full_like(z, c[0])
    for v in c[1:]:
        p = p * z + f64(v)
    return p


def asin(x):
    x = np.asarray(x, f64)
    z = x * x
    return x + x * (z * _horner(_ASIN_C, z))


def exp(x):
    x = np.asarray(x, f64)
    kd = np.rint(x * f64(1.44269504088896338700))
    r = x - kd * f64(6.93147180369123816490e-01)
    r = r - kd * f64(1.90821492927058770002e-10)
    e = f64(1.0) + (r + (r * r) * _horner(_EXP_C, r))
    with np.errstate(invalid="ignore"):
        k = np.where(np.isnan(kd), 0, kd).astype(np.int64)
    return np.where(np.isnan(x), x, np.ldexp(e, k))


def tanf(xf):
    x = np.asarray(xf, f32).astype(f64)
    z = x * x
    sn = x + x * (z * _horner(_SIN_C, z))
    cs = f64(1.0) + z * _horner(_COS_C, z)
    return (sn / cs).astype(f32)


def _axis_rows(R, a):
    c = [(a + 3) % 3, (a + 4) % 3, (a + 5) % 3]
    return np.array([[R[r, c[k]] for r in range(3)] for k in range(3)], f32)


def _nini(M, N, D):
    """n_ini of the records (float32 products and sums) followed by the lines (double products, rounded to float)"""
    o = []
    for k in range(3):
        on = M[k, 0] * N[:, 0] + M[k, 1] * N[:, 1] + M[k, 2] * N[:, 2]
        ol = (f64(M[k, 0]) * D[:, 0] + f64(M[k, 1]) * D[:, 1] + f64(M[k, 2]) * D[:, 2]).astype(f32)
        o.append(np.concatenate([on.astype(f32), ol]))
    return o


def _lambda(o):
    return np.sqrt(o[0] * o[0] + o[1] * o[1]).astype(f64)


def _seqsum(v):
    return np.add.accumulate(np.concatenate([[f64(0.0)], np.asarray(v, f64)]))[-1]


def _svd_polar(A, hits):
    """cv::SVD::compute of a 3x3 CV_32F (JacobiSVDImpl_<float>), then U * VT through the small-matrix gemm"""
    eps = f32(2.0) * f32(1.1920928955078125e-07)
    minval = f64(1.17549435082228750797e-38)
    At = np.array(A, f32).T.copy()
    Vt = np.eye(3, dtype=f32)
    W = [f64(0)] * 3
    for i in range(3):
        sd = f64(0)
        for k in range(3):
            sd = sd + f64(At[i, k]) * f64(At[i, k])
        W[i] = sd
    for _ in range(30):
        changed = False
        for i in range(2):
            for j in range(i + 1, 3):
                a, b, p = W[i], W[j], f64(0)
                for k in range(3):
                    p = p + f64(At[i, k]) * f64(At[j, k])
                if abs(p) <= f64(eps) * np.sqrt(a * b):
                    continue
                p = p * f64(2)
                beta = a - b
                gamma = np.sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * f64(0.5)
                    s = f32(np.sqrt(delta / gamma))
                    c = f32(p / (gamma * f64(s) * f64(2)))
                else:
                    c = f32(np.sqrt((gamma + beta) / (gamma * f64(2))))
                    s = f32(p / (gamma * f64(c) * f64(2)))
                a = b = f64(0)
                for k in range(3):
                    t0 = c * At[i, k] + s * At[j, k]
                    t1 = -s * At[i, k] + c * At[j, k]
                    At[i, k], At[j, k] = t0, t1
                    a = a + f64(t0) * f64(t0)
                    b = b + f64(t1) * f64(t1)
                W[i], W[j] = a, b
                changed = True
                for k in range(3):
                    t0 = c * Vt[i, k] + s * Vt[j, k]
                    t1 = -s * Vt[i, k] + c * Vt[j, k]
                    Vt[i, k], Vt[j, k] = t0, t1
        if not changed:
            break
    for i in range(3):
        sd = f64(0)
        for k in range(3):
            sd = sd + f64(At[i, k]) * f64(At[i, k])
        W[i] = np.sqrt(sd)
    for i in range(2):
        j = i
        for k in range(i + 1, 3):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[[i, j]] = At[[j, i]]
            Vt[[i, j]] = Vt[[j, i]]
    state = 0x12345678
    for i in range(3):
        sd = W[i]
        ii = 0
        while ii < 100 and sd <= minval:
            hits["svd_zero_singular_value"] += 1
            val0 = f32(1.0 / 3)
            for k in range(3):
                state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
                At[i, k] = val0 if (state & 0xFFFFFFFF) & 256 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = f64(0)
                    for k in range(3):
                        sd = sd + f64(At[i, k] * At[j, k])
                    asum = f32(0)
                    for k in range(3):
                        t = f32(f64(At[i, k]) - sd * f64(At[j, k]))
                        At[i, k] = t
                        asum = asum + abs(t)
                    asum = f32(1) / asum if asum > eps * f32(100) else f32(0)
                    for k in range(3):
                        At[i, k] = At[i, k] * asum
            sd = f64(0)
            for k in range(3):
                sd = sd + f64(At[i, k]) * f64(At[i, k])
            sd = np.sqrt(sd)
            ii += 1
        s = f32(f64(1) / sd if sd > minval else f64(0))
        for k in range(3):
            At[i, k] = At[i, k] * s
    out = np.zeros((3, 3), f32)
    for r in range(3):
        for c in range(3):
            d = At[0, r] * Vt[0, c] + At[1, r] * Vt[1, c] + At[2, r] * Vt[2, c]
            out[r, c] = d + f32(0)
    return out


def _det3(m):
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def _track_once(R, N, D, call, rb, lb, hits):
    n, nl = len(N), len(D)
    info = dict(in_cone=[0, 0, 0], n_selected=[0, 0, 0], threshold=0, deficient=0, found=0, svd=0, density=[f32(0)] * 3)
    cone = []
    with np.errstate(invalid="ignore"):
        for a in (1, 2, 3):
            lam = _lambda(_nini(_axis_rows(R, a), N, D))
            m = np.concatenate([lam[:n] < SIN_NORMAL, lam[n:] < SIN_LINE])
            cone.append(m)
            info["in_cone"][a - 1] = int(m[:n].sum())
            rb[m[:n]] |= INLINE
            lb[m[n:]] |= INLINE
    hits["nan_records"] += int(np.isnan(N).any(axis=1).sum())
    hits["lines_in_cone"] += int(np.any([c[n:] for c in cone], axis=0).sum()) if nl else 0
    hits["lines_outside_cone"] += int((~np.any([c[n:] for c in cone], axis=0)).sum()) if nl else 0
    thr = n // 20
    a_, b_, c_ = info["in_cone"]
    if a_ > b_: a_, b_ = b_, a_
    if b_ > c_: b_, c_ = c_, b_
    if a_ > b_: a_, b_ = b_, a_
    if b_ < thr:
        thr = (b_ + a_) // 2
        info["deficient"] = 1
        hits["deficiency"] += 1
    info["threshold"] = thr
    for a in (1, 2, 3):
        M = _axis_rows(R, a)                       # R keeps the columns of the axes already found (R_cm aliases R_cm_update)
        idx = np.flatnonzero(cone[a - 1])
        with np.errstate(invalid="ignore", divide="ignore"):
            o = [v[idx] for v in _nini(M, N, D)]
            lam = _lambda(o)
            ms = lam < SIN_MS
            pushed = idx[ms]
            rb[pushed[pushed < n]] |= np.uint16(1 << (3 * call + a - 1))
            lb[pushed[pushed >= n] - n] |= np.uint16(1 << (3 * call + a - 1))
            lam, ox, oy, oz = lam[ms], o[0][ms].astype(f64), o[1][ms].astype(f64), o[2][ms].astype(f64)
            tan_alfa = lam / np.abs(o[2][ms]).astype(f64)
            alfa = asin(lam)
            mx = alfa / tan_alfa * ox / oz
            my = alfa / tan_alfa * oy / oz
            ok = ~np.isnan(mx) & ~np.isnan(my)
        hits["zero_lambda_dropped"] += int((~ok & (lam == 0)).sum())
        mx, my = mx[ok], my[ok]
        nm = np.sqrt(mx * mx + my * my)
        k = exp(f64(-20.0) * nm * nm)
        sel = len(mx)
        info["n_selected"][a - 1] = sel
        if sel <= thr:
            continue
        sx, sy, sk = _seqsum(k * mx), _seqsum(k * my), _seqsum(k)
        cx, cy = sx / sk, sy / sk
        info["density"][a - 1] = f32(sk / f64(sel))
        alfa = f32(np.sqrt(cx * cx + cy * cy))
        ta = tanf(alfa)[()] / alfa
        ma = [f32(f64(ta) * cx), f32(f64(ta) * cy), f32(1.0)]
        v = np.array([(M[0, r] * ma[0] + M[1, r] * ma[1] + M[2, r] * ma[2]) + f32(0) for r in range(3)], f32)
        s2 = f64(0)
        for r in range(3):
            s2 = s2 + f64(v[r]) * f64(v[r])
        inv = f32(f64(1.0) / np.sqrt(s2))
        col = (v * inv).astype(f32)
        total = f64(0)
        for r in range(3):
            total = total + f64(col[r])
        if total != 0:
            info["found"] |= 1 << (a - 1)
            R[:, a - 1] = col
    found = info["found"]
    nf = bin(found).count("1")
    if nf < 2:
        hits[f"found_{nf}"] += 1
        return info
    if nf == 2:
        ia, ib, ic = {3: (0, 1, 2), 6: (2, 1, 0), 5: (0, 2, 1)}[found]
        hits[f"pair_{found}"] += 1
        vc = _cross(R[:, ia].copy(), R[:, ib].copy())
        R[:, ic] = vc
        if abs(f64(_det3(R)) + f64(1)) < 0.5:
            R[:, ic] = -vc
            hits["det_flip"] += 1
    else:
        hits["found_3"] += 1
    R[:, :] = _svd_polar(R, hits)
    info["svd"] = 1
    return info


def track(R, normals, dirs=None, n_calls=3, hits=None):
    R = np.array(R, f32).reshape(3, 3).copy()
    N = np.ascontiguousarray(normals, f32).reshape(-1, 3)
    D = np.zeros((0, 3), f64) if dirs is None else np.ascontiguousarray(dirs, f64).reshape(-1, 3)
    hits = collections.Counter() if hits is None else hits
    rb = np.zeros(len(N), np.uint16)
    lb = np.zeros(len(D), np.uint16)
    infos = [_track_once(R, N, D, k, rb, lb, hits) for k in range(n_calls)]
    return R, infos, rb, lb, hits


def assert_equal_to_product(R_np, infos, rb, lb, R_c, info_c, rb_c, lb_c):
    """bit equality of a restatement result and a C-ABI result (lib.MANHATTAN_INFO_DTYPE info)"""
    assert np.array_equal(np.asarray(R_np, f32).view(np.uint32), np.asarray(R_c, f32).view(np.uint32)), (R_np, R_c)
    assert int(info_c["n_calls"]) == len(infos)
    for k, inf in enumerate(infos):
        ci = info_c["call"][k]
        assert list(ci["in_cone"]) == inf["in_cone"], (k, ci["in_cone"], inf["in_cone"])
        assert list(ci["n_selected"]) == inf["n_selected"], (k, ci["n_selected"], inf["n_selected"])
        assert int(ci["threshold"]) == inf["threshold"] and int(ci["deficient"]) == inf["deficient"]
        assert int(ci["found"]) == inf["found"] and int(ci["svd"]) == inf["svd"]
        assert np.array_equal(np.asarray(ci["density"], f32).view(np.uint32), np.array(inf["density"], f32).view(np.uint32))
    assert np.array_equal(rb, rb_c) and np.array_equal(lb, lb_c)
