/* sim3_core.h — the arithmetic of Sim3Solver (reference src/Sim3Solver.cc): the constructor's camera points, image points and
 * error bounds (:85-113), ComputeSim3 (:230-341, Horn 1987), Project and CheckInliers (:344-407), and iterate's bookkeeping
 * (:187-203) as a walk over finished inlier counts.  Shared by the host entry (sim3.cpp) and the device kernels
 * (sim3_kernels.hip) so that both produce the same bits; plain IEEE add / mul / div / sqrt, compiled with -ffp-contract=off on
 * both sides.  sin / cos of the double angle are cr_sincos.h's, the double atan2 is cr_atan2.h's: correctly rounded, or the
 * hypothesis is reported as not certified and finished with the host's libm.  The OpenCV readings are DESIGN.md section 16
 * (unpinned, as sections 11, 14 and 15). */
#ifndef DRFE_SIM3_CORE_H
#define DRFE_SIM3_CORE_H

#include "../../include/drfe.h"
#include "../../include/drfe_math.h"
#include "cr_atan2.h"

#include <float.h>
#include <stdint.h>

/* one correspondence of a solver: mvX3Dc1 / 2, mvP1im1 / mvP2im2, mvnMaxError1 / 2 converted to float as the comparison does */
struct Sim3Corr {
    float c1[3], c2[3], p1[2], p2[2], b1, b2;
};

/* Mat::convertTo(type, alpha) of a CV_32F element into CV_32F: a copy when alpha is 1 within DBL_EPSILON, else float
 * v * (float)alpha + (float)0.  What a scaled MatExpr (s * A, A / s, (s * A.t())) is assigned through. */
DRFE_HD float s3_scale(float v, double alpha)
{
    return fabs(alpha - 1.0) < DBL_EPSILON ? v : v * (float)alpha + 0.0f;
}

/* gemm(A, x, alpha, c, beta = 1 | no c) of a 3x3 by a 3-vector through the small-matrix path: float dot, then
 * (float)(t * alpha + c * beta) in double (no c: zerof * 0) */
DRFE_HD float s3_gemm_row(float a0, float a1, float a2, const float x[3], double alpha, float c, double beta)
{
    const float t = a0 * x[0] + a1 * x[1] + a2 * x[2];
    return (float)((double)t * alpha + (double)c * beta);
}

/* T.rowRange(0,3).colRange(0,3) * X + T.rowRange(0,3).col(3) for T = [A | b] 3x4 row-major */
DRFE_HD void s3_apply(const float T[12], const float X[3], float o[3])
{
    for (int r = 0; r < 3; r++) o[r] = s3_gemm_row(T[r * 4 + 0], T[r * 4 + 1], T[r * 4 + 2], X, 1.0, T[r * 4 + 3], 1.0);
}

/* FromCameraToImage / the tail of Project: K = (fx, fy, cx, cy) */
DRFE_HD void s3_to_image(const float P[3], const float K[4], float uv[2])
{
    const float invz = 1 / P[2];
    const float x = P[0] * invz, y = P[1] * invz;
    uv[0] = K[0] * x + K[2];
    uv[1] = K[1] * y + K[3];
}

/* mvnMaxError.push_back(9.210 * sigmaSquare) into a vector<size_t>, read back by `err < mvnMaxError[i]` as a float.  The entries
 * refuse a sigma2 whose product is not in [0, 2^63). */
DRFE_HD float s3_bound(float sigma2)
{
    return (float)(uint64_t)(9.210 * (double)sigma2);
}

DRFE_HD Sim3Corr s3_corr(const float Tcw1[12], const float Tcw2[12], const float K1[4], const float K2[4], const float Xw1[3],
                         const float Xw2[3], float sigma2_1, float sigma2_2)
{
    Sim3Corr c;
    s3_apply(Tcw1, Xw1, c.c1);
    s3_apply(Tcw2, Xw2, c.c2);
    s3_to_image(c.c1, K1, c.p1);
    s3_to_image(c.c2, K2, c.p2);
    c.b1 = s3_bound(sigma2_1);
    c.b2 = s3_bound(sigma2_2);
    return c;
}

/* Mat::dot of a 2x1 CV_32F with itself stored to float: double products summed in order */
DRFE_HD float s3_err(float d0, float d1)
{
    double s = 0.0;
    s += (double)d0 * (double)d0;
    s += (double)d1 * (double)d1;
    return (float)s;
}

/* CheckInliers for one correspondence under T12 (into camera 1) and T21 (into camera 2) */
DRFE_HD bool s3_inlier(const Sim3Corr& c, const float T12[12], const float T21[12], const float K1[4], const float K2[4])
{
    float P[3], q21[2], q12[2];
    s3_apply(T12, c.c2, P);
    s3_to_image(P, K1, q21);
    s3_apply(T21, c.c1, P);
    s3_to_image(P, K2, q12);
    const float e1 = s3_err(c.p1[0] - q21[0], c.p1[1] - q21[1]);
    const float e2 = s3_err(q12[0] - c.p2[0], q12[1] - c.p2[1]);
    return e1 < c.b1 && e2 < c.b2;
}

/* lapack.cpp's hypot of JacobiImpl_<float> */
DRFE_HD float s3_hypot(float a, float b)
{
    a = fabsf(a);
    b = fabsf(b);
    if (a > b) { b /= a; return a * sqrtf(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrtf(1 + a * a); }
    return 0;
}

/* cv::eigen of a symmetric 4x4 CV_32F: JacobiImpl_<float> — the largest off-diagonal element by the row / column maxima it
 * keeps, at most n * n * 30 rotations, stop at |pivot| <= FLT_EPSILON, then a selection sort by descending eigenvalue.  A in
 * (destroyed), W the eigenvalues, V the eigenvectors as rows. */
DRFE_HD void s3_jacobi4(float A[16], float W[4], float V[16])
{
    const int n = 4;
    const float eps = FLT_EPSILON;
    int indR[4] = {0, 0, 0, 0}, indC[4] = {0, 0, 0, 0};
    int i, k, m;
    float mv;
    for (i = 0; i < 16; i++) V[i] = 0.f;
    for (i = 0; i < n; i++) V[i * n + i] = 1.f;
    for (k = 0; k < n; k++) {
        W[k] = A[(n + 1) * k];
        if (k < n - 1) {
            for (m = k + 1, mv = fabsf(A[n * k + m]), i = k + 2; i < n; i++) {
                const float val = fabsf(A[n * k + i]);
                if (mv < val) mv = val, m = i;
            }
            indR[k] = m;
        }
        if (k > 0) {
            for (m = 0, mv = fabsf(A[k]), i = 1; i < k; i++) {
                const float val = fabsf(A[n * i + k]);
                if (mv < val) mv = val, m = i;
            }
            indC[k] = m;
        }
    }
    const int maxIters = n * n * 30;
    for (int iters = 0; iters < maxIters; iters++) {
        for (k = 0, mv = fabsf(A[indR[0]]), i = 1; i < n - 1; i++) {
            const float val = fabsf(A[n * i + indR[i]]);
            if (mv < val) mv = val, k = i;
        }
        int l = indR[k];
        for (i = 1; i < n; i++) {
            const float val = fabsf(A[n * indC[i] + i]);
            if (mv < val) mv = val, k = indC[i], l = i;
        }
        const float p = A[n * k + l];
        if (fabsf(p) <= eps) break;
        const float y = (float)((double)(W[l] - W[k]) * 0.5);
        float t = fabsf(y) + s3_hypot(p, y);
        float s = s3_hypot(p, t);
        const float c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        A[n * k + l] = 0;
        W[k] -= t;
        W[l] += t;
        float a0, b0;
#define S3_ROTATE(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
        for (i = 0; i < k; i++) S3_ROTATE(A[n * i + k], A[n * i + l]);
        for (i = k + 1; i < l; i++) S3_ROTATE(A[n * k + i], A[n * i + l]);
        for (i = l + 1; i < n; i++) S3_ROTATE(A[n * k + i], A[n * l + i]);
        for (i = 0; i < n; i++) S3_ROTATE(V[n * k + i], V[n * l + i]);
#undef S3_ROTATE
        for (int j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                for (m = idx + 1, mv = fabsf(A[n * idx + m]), i = idx + 2; i < n; i++) {
                    const float val = fabsf(A[n * idx + i]);
                    if (mv < val) mv = val, m = i;
                }
                indR[idx] = m;
            }
            if (idx > 0) {
                for (m = 0, mv = fabsf(A[idx]), i = 1; i < idx; i++) {
                    const float val = fabsf(A[n * i + idx]);
                    if (mv < val) mv = val, m = i;
                }
                indC[idx] = m;
            }
        }
    }
    for (k = 0; k < n - 1; k++) {
        m = k;
        for (i = k + 1; i < n; i++)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            float tmp = W[m]; W[m] = W[k]; W[k] = tmp;
            for (i = 0; i < n; i++) { tmp = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = tmp; }
        }
    }
}

/* cv::Rodrigues of a CV_32F rotation vector into a 3x3 CV_32F (cvRodrigues2: double inside).  sc = sin, cos of theta. */
DRFE_HD void s3_rodrigues(const float v[3], double theta, double s, double c, float R[9])
{
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; k++) R[k] = (float)I[k];
        return;
    }
    const double c1 = 1. - c;
    const double itheta = theta ? 1. / theta : 0.;
    const double rx = (double)v[0] * itheta, ry = (double)v[1] * itheta, rz = (double)v[2] * itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; k++) R[k] = (float)(c * I[k] + c1 * rrt[k] + s * r_x[k]);
}

/* ComputeCentroid: cv::reduce(SUM) over the three columns in reduceC_'s order ((p0 + p2) + p1, float), C / P.cols as a scaled
 * MatExpr, the columns minus C.  P and Pr are 3x3 row-major with one point per column. */
DRFE_HD void s3_centroid(const float P[9], float Pr[9], float C[3])
{
    for (int r = 0; r < 3; r++) {
        const float sum = (P[r * 3 + 0] + P[r * 3 + 2]) + P[r * 3 + 1];
        C[r] = s3_scale(sum, 1. / 3);
        for (int q = 0; q < 3; q++) Pr[r * 3 + q] = P[r * 3 + q] - C[r];
    }
}

/* ComputeSim3.  P1, P2: the sampled camera points, one per column.  Out: mR12i, mt12i, ms12i, and the upper 3x4 of mT12i and
 * mT21i.  Returns 1, or 0 when atan2 or sin / cos could not be certified (the outputs are then not to be used).  libm != 0
 * (host only) takes atan2, sin and cos from the host's libm instead: how a hypothesis that was not certified is finished. */
DRFE_HD int s3_horn(const float P1[9], const float P2[9], int fixScale, int libm, float R[9], float t[3], float* sOut, float T12[12],
                    float T21[12])
{
    float Pr1[9], Pr2[9], O1[3], O2[3], M[9];
    s3_centroid(P1, Pr1, O1);
    s3_centroid(P2, Pr2, O2);
    /* M = Pr2 * Pr1.t(): gemm with GEMM_2_T, double accumulation in order */
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s0 = 0.0;
            for (int k = 0; k < 3; k++) s0 += (double)Pr2[i * 3 + k] * (double)Pr1[j * 3 + k];
            M[i * 3 + j] = (float)(s0 * 1.0);
        }
    const float N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3];
    const float N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2];
    const float N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7], N44 = -M[0] - M[4] + M[8];
    float A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float W[4], V[16];
    s3_jacobi4(A, W, V);
    float vec[3] = {V[1], V[2], V[3]};
    /* cv::norm(vec): normL2Sqr in double, in order */
    double n2 = 0.0;
    for (int k = 0; k < 3; k++) n2 += (double)vec[k] * (double)vec[k];
    const double nrm = sqrt(n2);
    double ang, sn, cs;
    int ok = 1;
#if !defined(__HIP_DEVICE_COMPILE__)
    if (libm) ang = atan2(nrm, (double)V[0]);
    else
#endif
        ok = drfe_cr_atan2(nrm, (double)V[0], &ang);
    /* vec = 2 * ang * vec / norm(vec): one MatExpr whose scale is (2 * ang) * (1 / norm) */
    const double alpha = (2 * ang) * (1. / nrm);
    for (int k = 0; k < 3; k++) vec[k] = s3_scale(vec[k], alpha);
    const double rx = vec[0], ry = vec[1], rz = vec[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta != theta) sn = cs = theta;
    else if (theta < DBL_EPSILON) sn = 0.0, cs = 1.0;     /* not read */
#if !defined(__HIP_DEVICE_COMPILE__)
    else if (libm) sn = sin(theta), cs = cos(theta);
#endif
    else ok &= drfe_cr_sincos(theta, &sn, &cs);
    s3_rodrigues(vec, theta, sn, cs, R);
    /* P3 = mR12i * Pr2 */
    float P3[9];
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) {
            const float col[3] = {Pr2[q], Pr2[3 + q], Pr2[6 + q]};
            P3[r * 3 + q] = s3_gemm_row(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], col, 1.0, 0.f, 0.0);
        }
    float s = 1.0f;
    if (!fixScale) {
        /* Pr1.dot(P3): dotProd_'s groups of four double products; cv::pow(P3, 2) squares in float; den sums in double */
        double p[9];
        for (int k = 0; k < 9; k++) p[k] = (double)Pr1[k] * (double)P3[k];
        double nom = 0.0;
        nom += p[0] + p[1] + p[2] + p[3];
        nom += p[4] + p[5] + p[6] + p[7];
        nom += p[8];
        double den = 0;
        for (int k = 0; k < 9; k++) den += (double)(P3[k] * P3[k]);
        s = (float)(nom / den);
    }
    /* mt12i = O1 - ms12i * mR12i * O2: one gemm, alpha = -ms12i, C = O1 */
    for (int r = 0; r < 3; r++) t[r] = s3_gemm_row(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], O2, -(double)s, O1[r], 1.0);
    float sRinv[9];
    const double inv = 1.0 / (double)s;
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) {
            T12[r * 4 + q] = s3_scale(R[r * 3 + q], (double)s);
            sRinv[r * 3 + q] = s3_scale(R[q * 3 + r], inv);
        }
    for (int r = 0; r < 3; r++) {
        T12[r * 4 + 3] = t[r];
        for (int q = 0; q < 3; q++) T21[r * 4 + q] = sRinv[r * 3 + q];
        T21[r * 4 + 3] = s3_gemm_row(sRinv[r * 3], sRinv[r * 3 + 1], sRinv[r * 3 + 2], t, -1.0, 0.f, 0.0);
    }
    *sOut = s;
    return ok;
}

/* a NaN leaves the entries as the one quiet NaN 0x7FC00000: x86-64 and gfx950 give an invalid operation different signs */
DRFE_HD float s3_canon(float v)
{
    if (v == v) return v;
    const uint32_t q = 0x7FC00000u;
    float f;
    memcpy(&f, &q, 4);
    return f;
}

/* iterate's bookkeeping (:187-203) over the inlier counts of iterations 0 .. n-1: `>=` against the best so far, `>` against
 * mRansacMinInliers for handing the transform back */
DRFE_HD void s3_walk(const int32_t* count, int n, int minInliers, uint8_t* returns, int32_t* best)
{
    int bestCount = 0, bestIdx = -1;
    for (int h = 0; h < n; h++) {
        uint8_t ret = 0;
        if (count[h] >= bestCount) {
            bestCount = count[h];
            bestIdx = h;
            ret = count[h] > minInliers ? 1 : 0;
        }
        returns[h] = ret;
        best[h] = bestIdx;
    }
}

#endif
