/* init_core.h — the arithmetic of Initializer (reference src/Initializer.cc, the point-only Initialize at :49): ComputeH21 /
 * ComputeF21 (:231-308), CheckHomography / CheckFundamental (:310-473), the decompositions of ReconstructH / ReconstructF /
 * DecomposeE (:475-737, :914-934), CheckRT's per-match body with Triangulate (:739-752, :803-912) and the bookkeeping that ends
 * FindHomography / FindFundamental and the two Reconstruct functions, as walks over finished numbers.  Shared by the host entry
 * (init.cpp) and the device kernels (init_kernels.hip) so that both produce the same bits: plain IEEE add / mul / div / sqrt,
 * compiled with -ffp-contract=off on both sides, no transcendental (the acos of the parallax is init.cpp's host tail).  The
 * OpenCV pieces are restated from library knowledge and unpinned: DESIGN.md section 19.
 *
 * Matrices are row-major float[9] unless said otherwise. */
#ifndef DRFE_INIT_CORE_H
#define DRFE_INIT_CORE_H

#include "../../include/drfe.h"
#include "../../include/drfe_math.h"
#include "jacobi_svd_core.h"
#include "manhattan_core.h"
#include "triangulate_core.h"

#include <float.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define INIT_HDM __host__ __device__
#else
#define INIT_HDM
#endif

/* a small float matrix kept with a stride between its elements: 1 on the host, the lane count where every lane of a wavefront
 * keeps a matrix of its own in LDS (element-major, as pnp_core.h's PnpStrided) */
struct InitStrided {
    float* p;
    int stride;
    INIT_HDM float& operator[](int k) const { return p[(size_t)k * stride]; }
};

/* one match of a solver: mvKeys1[first].pt, mvKeys2[second].pt */
struct InitMatch {
    float u1, v1, u2, v2;
};

/* every NaN an entry stores is the quiet NaN 0x7FC00000 (a NaN's sign and payload differ between x86-64 and gfx950) */
DRFE_HD float init_canon(float v) { return v != v ? __builtin_nanf("") : v; }

/* isfinite of a float, from its bits */
DRFE_HD bool init_isfinite(float v)
{
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x7F800000u) != 0x7F800000u;
}

/* ---- OpenCV pieces -------------------------------------------------------------------------------------------------------- */

/* gemm's small-matrix path (flags == 0, 3 columns in A): a float dot left to right, then (float)(t * alpha + 0 * 0) */
DRFE_HD float init_gemm_out(float t, double alpha) { return (float)((double)t * alpha + 0.0 * 0.0); }
DRFE_HD void init_mm3(const float A[9], const float B[9], double alpha, float D[9])
{
    float T[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) T[r * 3 + c] = init_gemm_out(A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c], alpha);
    for (int k = 0; k < 9; k++) D[k] = T[k];
}
DRFE_HD void init_mv3(const float A[9], const float x[3], double alpha, float o[3])
{
    float T[3];
    for (int r = 0; r < 3; r++) T[r] = init_gemm_out(A[r * 3] * x[0] + A[r * 3 + 1] * x[1] + A[r * 3 + 2] * x[2], alpha);
    for (int k = 0; k < 3; k++) o[k] = T[k];
}
/* gemm with a transpose flag leaves the small-matrix path: GEMMSingleMul<float, double>, each element a double sum over k in
 * order, stored as (float)(s * 1).  ta: A is read transposed; tb: B is */
DRFE_HD void init_mm3_flag(const float A[9], bool ta, const float B[9], bool tb, float D[9])
{
    float T[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)(ta ? A[k * 3 + r] : A[r * 3 + k]) * (double)(tb ? B[c * 3 + k] : B[k * 3 + c]);
            T[r * 3 + c] = (float)(s * 1.0);
        }
    for (int k = 0; k < 9; k++) D[k] = T[k];
}
/* Mat * s, Mat / s, -Mat: convertTo with the double alpha, cvtScale in float (v * (float)alpha + 0.f), a plain copy when
 * |alpha - 1| < DBL_EPSILON */
DRFE_HD void init_scale(float* v, int n, double alpha)
{
    if (fabs(alpha - 1.0) < DBL_EPSILON) return;
    const float a = (float)alpha;
    for (int k = 0; k < n; k++) v[k] = v[k] * a + 0.0f;
}
/* cv::norm of a float 3-vector */
DRFE_HD double init_norm3(const float v[3]) { return sqrt(tr_dotd(v, v)); }

/* Mat::inv() of a 3x3 CV_32F (DECOMP_LU's closed form): the det3 macro as section 11 reads it (mf_det3, float) widened to double,
 * d = 1. / d, each cofactor a double difference of double products times d, stored to float; a zero determinant gives the zero
 * matrix */
DRFE_HD void init_inv3(const float S[9], float D[9])
{
    double d = (double)mf_det3(S);
    if (d == 0.) {
        for (int k = 0; k < 9; k++) D[k] = 0.f;
        return;
    }
    d = 1. / d;
#define INIT_S(r, c) ((double)S[(r) * 3 + (c)])
    float T[9];
    T[0] = (float)((INIT_S(1, 1) * INIT_S(2, 2) - INIT_S(1, 2) * INIT_S(2, 1)) * d);
    T[1] = (float)((INIT_S(0, 2) * INIT_S(2, 1) - INIT_S(0, 1) * INIT_S(2, 2)) * d);
    T[2] = (float)((INIT_S(0, 1) * INIT_S(1, 2) - INIT_S(0, 2) * INIT_S(1, 1)) * d);
    T[3] = (float)((INIT_S(1, 2) * INIT_S(2, 0) - INIT_S(1, 0) * INIT_S(2, 2)) * d);
    T[4] = (float)((INIT_S(0, 0) * INIT_S(2, 2) - INIT_S(0, 2) * INIT_S(2, 0)) * d);
    T[5] = (float)((INIT_S(0, 2) * INIT_S(1, 0) - INIT_S(0, 0) * INIT_S(1, 2)) * d);
    T[6] = (float)((INIT_S(1, 0) * INIT_S(2, 1) - INIT_S(1, 1) * INIT_S(2, 0)) * d);
    T[7] = (float)((INIT_S(0, 1) * INIT_S(2, 0) - INIT_S(0, 0) * INIT_S(2, 1)) * d);
    T[8] = (float)((INIT_S(0, 0) * INIT_S(1, 1) - INIT_S(0, 1) * INIT_S(1, 0)) * d);
#undef INIT_S
    for (int k = 0; k < 9; k++) D[k] = T[k];
}

/* JacobiSVDImpl_<float>'s sweeps and sort for n rows of m (row stride m) in At: jacobi_svd_core.h's drfe_jacobi_svd with the two
 * sizes apart.  W: the singular values in decreasing order; Vt (n x n) the accumulated rotations, not kept when !wantV (they feed
 * nothing else).  eps = 2 FLT_EPSILON, max(m, 30) = 30 sweeps for every m here (m <= 16). */
template <class TA, class TV>
DRFE_HD void init_jacobi_sweeps(TA At, int m, int n, double* W, TV Vt, bool wantV)
{
    const float eps = 2.0f * 1.1920928955078125e-07f;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const float t = At[i * m + k]; sd += (double)t * t; }
        W[i] = sd;
        if (wantV) {
            for (int k = 0; k < n; k++) Vt[i * n + k] = 0.f;
            Vt[i * n + i] = 1.f;
        }
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += (double)At[i * m + k] * At[j * m + k];
                if (fabs(p) <= (double)eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const float ai = At[i * m + k], aj = At[j * m + k];
                    const float t0 = c * ai + s * aj;
                    const float t1 = -s * ai + c * aj;
                    At[i * m + k] = t0; At[j * m + k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                if (wantV)
                    for (int k = 0; k < n; k++) {
                        const float vi = Vt[i * n + k], vj = Vt[j * n + k];
                        const float t0 = c * vi + s * vj;
                        const float t1 = -s * vi + c * vj;
                        Vt[i * n + k] = t0; Vt[j * n + k] = t1;
                    }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const float t = At[i * m + k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            for (int k = 0; k < m; k++) { const float t = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = t; }
            if (wantV)
                for (int k = 0; k < n; k++) { const float t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
        }
    }
}

/* the end of JacobiSVDImpl_<float>: rows 0 .. n1 - 1 of At become the left singular vectors.  Row i < n is divided by W[i]; a
 * row with W[i] <= FLT_MIN, and every row from n on (FULL_UV), is cv::RNG(0x12345678)'s +-1/m vector - one generator for the
 * whole call - orthogonalised twice against the rows before it (manhattan_core.h's mf_svd_polar, for any m) */
template <class TA>
DRFE_HD void init_left_vectors(TA At, int m, int n, int n1, const double* W)
{
    const float eps = 2.0f * 1.1920928955078125e-07f;
    const double minval = 1.17549435082228750797e-38;
    uint64_t rng = 0x12345678u;
    for (int i = 0; i < n1; i++) {
        double sd = i < n ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / m);
            for (int k = 0; k < m; k++) {
                rng = (uint64_t)(unsigned)rng * 4164903690u + (unsigned)(rng >> 32);
                At[i * m + k] = (((unsigned)rng) & 256) != 0 ? val0 : -val0;
            }
            for (int it = 0; it < 2; it++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    float asum = 0;
                    for (int k = 0; k < m; k++) {
                        const float t = (float)(At[i * m + k] - sd * At[j * m + k]);
                        At[i * m + k] = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const float t = At[i * m + k]; sd += (double)t * t; }
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
        for (int k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

/* cv::SVD::compute / cv::SVDecomp of a 3x3 CV_32F into w, u, vt: the shared drfe_jacobi_svd<3> on At = A^T, the left vectors as
 * above, u = At^T, w = (float)W */
DRFE_HD void init_svd3(const float A[9], float w[3], float u[9], float vt[9])
{
    float At[9];
    double W[3];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) At[i * 3 + k] = A[k * 3 + i];
    drfe_jacobi_svd<3>(At, W, vt);
    init_left_vectors(At, 3, 3, 3, W);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) u[r * 3 + c] = At[c * 3 + r];
    for (int i = 0; i < 3; i++) w[i] = (float)W[i];
}

/* ---- ComputeH21 / ComputeF21 ---------------------------------------------------------------------------------------------- */

/* the normalised points of one sampled match */
struct InitNorm {
    float x1, y1, x2, y2;
};

/* ComputeH21 (:231-271): the 16x9 system's At = A^T (9 rows of 16) in `big` (144 + 81 floats: At, then the 9x9 rotations),
 * vt.row(8).  m >= n, so vt is the accumulated rotations and U (with its cv::RNG rows 9 .. 15) is never read. */
template <class TA>
DRFE_HD void init_compute_h21(const InitNorm P[8], TA big, float Hn[9])
{
    for (int i = 0; i < 8; i++) {
        const float u1 = P[i].x1, v1 = P[i].y1, u2 = P[i].x2, v2 = P[i].y2;
        const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, -u2 * u1, -u2 * v1, -u2};
        for (int c = 0; c < 9; c++) {
            big[c * 16 + 2 * i] = r0[c];
            big[c * 16 + 2 * i + 1] = r1[c];
        }
    }
    double W[9];
    struct Off {
        TA a;
        int o;
        INIT_HDM float& operator[](int k) const { return a[o + k]; }
    };
    init_jacobi_sweeps(big, 16, 9, W, Off{big, 144}, true);
    for (int k = 0; k < 9; k++) Hn[k] = big[144 + 8 * 9 + k];
}

/* ComputeF21 (:273-308): the 8x9 system has m < n, so the roles swap: the routine runs on A itself (8 rows of 9, `big` holds 81
 * floats), vt's rows 0 .. 7 are the normalised rotated rows and row 8 - Fpre - is the FULL_UV vector cv::RNG starts and two rounds
 * of orthogonalisation finish.  Then the 3x3 SVD, w(2) = 0 and u * diag(w) * vt as two small gemms. */
template <class TA>
DRFE_HD void init_compute_fpre(const InitNorm P[8], TA big, float Fpre[9])
{
    for (int i = 0; i < 8; i++) {
        const float u1 = P[i].x1, v1 = P[i].y1, u2 = P[i].x2, v2 = P[i].y2;
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0f};
        for (int c = 0; c < 9; c++) big[i * 9 + c] = r[c];
    }
    double W[8];
    init_jacobi_sweeps(big, 9, 8, W, big, false);
    init_left_vectors(big, 9, 8, 9, W);
    for (int k = 0; k < 9; k++) Fpre[k] = big[72 + k];
}
template <class TA>
DRFE_HD void init_compute_f21(const InitNorm P[8], TA big, float Fn[9])
{
    float Fpre[9], w[3], u[9], vt[9];
    init_compute_fpre(P, big, Fpre);
    init_svd3(Fpre, w, u, vt);
    const float D[9] = {w[0], 0.f, 0.f, 0.f, w[1], 0.f, 0.f, 0.f, 0.f};
    float UD[9];
    init_mm3(u, D, 1.0, UD);
    init_mm3(UD, vt, 1.0, Fn);
}

/* Normalize's T (:795-799) from its four finished numbers */
DRFE_HD void init_T(float meanX, float meanY, float sX, float sY, float T[9])
{
    T[0] = sX; T[1] = 0.f; T[2] = -meanX * sX;
    T[3] = 0.f; T[4] = sY; T[5] = -meanY * sY;
    T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

/* one row of FindHomography (:164-166): H21i = T2inv * Hn * T1, H12i = H21i.inv() */
template <class TA>
DRFE_HD void init_row_h(const InitNorm P[8], const float T1[9], const float T2inv[9], TA big, float H21[9], float H12[9])
{
    float Hn[9], t[9];
    init_compute_h21(P, big, Hn);
    init_mm3(T2inv, Hn, 1.0, t);
    init_mm3(t, T1, 1.0, H21);
    init_inv3(H21, H12);
}
/* one row of FindFundamental (:215-217): F21i = T2t * Fn * T1 */
template <class TA>
DRFE_HD void init_row_f(const InitNorm P[8], const float T1[9], const float T2t[9], TA big, float F21[9])
{
    float Fn[9], t[9];
    init_compute_f21(P, big, Fn);
    init_mm3(T2t, Fn, 1.0, t);
    init_mm3(t, T1, 1.0, F21);
}

/* ---- CheckHomography / CheckFundamental ----------------------------------------------------------------------------------- */

/* invSigmaSquare = 1.0 / (sigma * sigma): the float product widened, a double division, rounded to float */
DRFE_HD float init_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

/* the two chi-square terms of one match (:346-384); in[k]: term k is at most th (a NaN term is: `chi > th` is false) */
DRFE_HD void init_chi_h(const float H[9], const float Hi[9], const InitMatch& m, float invS2, float chi[2], bool in[2])
{
    const float u1 = m.u1, v1 = m.v1, u2 = m.u2, v2 = m.v2;
    const float w2in1inv = (float)(1.0 / (double)(Hi[6] * u2 + Hi[7] * v2 + Hi[8]));
    const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
    const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    chi[0] = squareDist1 * invS2;
    const float w1in2inv = (float)(1.0 / (double)(H[6] * u1 + H[7] * v1 + H[8]));
    const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
    const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    chi[1] = squareDist2 * invS2;
    in[0] = !(chi[0] > 5.991f);
    in[1] = !(chi[1] > 5.991f);
}
DRFE_HD void init_chi_f(const float F[9], const InitMatch& m, float invS2, float chi[2], bool in[2])
{
    const float u1 = m.u1, v1 = m.v1, u2 = m.u2, v2 = m.v2;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    chi[0] = squareDist1 * invS2;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    chi[1] = squareDist2 * invS2;
    in[0] = !(chi[0] > 3.841f);
    in[1] = !(chi[1] > 3.841f);
}
/* score += th - chiSquare for the terms that are in, in the reference's order; thScore is 5.991 in both checks */
DRFE_HD float init_score_add(float score, const float chi[2], const bool in[2])
{
    if (in[0]) score += 5.991f - chi[0];
    if (in[1]) score += 5.991f - chi[1];
    return score;
}

/* the end of FindHomography / FindFundamental's loop (:170-175, :221-226) over the rows' finished scores: best[h] is the row that
 * holds the model after row h, strict `>` against a score that starts at 0, -1 before the first.  Returns the last best. */
DRFE_HD int init_walk_best(const float* score, int rows, int32_t* best)
{
    float s = 0.0f;
    int b = -1;
    for (int h = 0; h < rows; h++) {
        if (score[h] > s) { s = score[h]; b = h; }
        best[h] = b;
    }
    return b;
}

/* ---- ReconstructF / ReconstructH: the motion hypotheses ------------------------------------------------------------------- */

/* -Mat through convertTo(alpha = -1) */
DRFE_HD void init_neg(float* v, int n) { init_scale(v, n, -1.0); }

/* ReconstructF's E21 = K.t() * F21 * K (:484) and DecomposeE (:914-934) into the four hypotheses (R1, t), (R2, t), (R1, -t),
 * (R2, -t) of :499-502.  K.t() * F21 is a gemm with GEMM_1_T, u * W.t() one with GEMM_2_T. */
DRFE_HD void init_motions_f(const float F21[9], const float K[9], float R[4][9], float t[4][3])
{
    float E[9], tmp[9], w[3], u[9], vt[9];
    init_mm3_flag(K, true, F21, false, tmp);
    init_mm3(tmp, K, 1.0, E);
    init_svd3(E, w, u, vt);
    float t1[3] = {u[2], u[5], u[8]};
    init_scale(t1, 3, 1.0 / init_norm3(t1));
    const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float R1[9], R2[9];
    init_mm3(u, Wm, 1.0, tmp);
    init_mm3(tmp, vt, 1.0, R1);
    if ((double)mf_det3(R1) < 0) init_neg(R1, 9);
    init_mm3_flag(u, false, Wm, true, tmp);
    init_mm3(tmp, vt, 1.0, R2);
    if ((double)mf_det3(R2) < 0) init_neg(R2, 9);
    float t2[3] = {t1[0], t1[1], t1[2]};
    init_neg(t2, 3);
    for (int k = 0; k < 9; k++) { R[0][k] = R1[k]; R[1][k] = R2[k]; R[2][k] = R1[k]; R[3][k] = R2[k]; }
    for (int k = 0; k < 3; k++) { t[0][k] = t1[k]; t[1][k] = t1[k]; t[2][k] = t2[k]; t[3][k] = t2[k]; }
}

/* ReconstructH's eight hypotheses (:589-691); false when it leaves at the d1 / d2, d2 / d3 test.  The normals vn are computed by
 * the reference and never read. */
DRFE_HD bool init_motions_h(const float H21[9], const float K[9], float R[8][9], float t[8][3])
{
    float invK[9], A[9], tmp[9], w[3], U[9], Vt[9];
    init_inv3(K, invK);
    init_mm3(invK, H21, 1.0, tmp);
    init_mm3(tmp, K, 1.0, A);
    init_svd3(A, w, U, Vt);
    const float s = (float)((double)mf_det3(U) * (double)mf_det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    for (int i = 0; i < 8; i++) {
        const int q = i & 3;
        float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        float tp[3];
        if (i < 4) {
            Rp[0] = ctheta; Rp[2] = -stheta[q]; Rp[6] = stheta[q]; Rp[8] = ctheta;
            tp[0] = x1[q]; tp[1] = 0.f; tp[2] = -x3[q];
            init_scale(tp, 3, (double)(d1 - d3));
        } else {
            Rp[0] = cphi; Rp[2] = sphi[q]; Rp[4] = -1.f; Rp[6] = sphi[q]; Rp[8] = -cphi;
            tp[0] = x1[q]; tp[1] = 0.f; tp[2] = x3[q];
            init_scale(tp, 3, (double)(d1 + d3));
        }
        /* s * U * Rp * Vt: the scalar folds into the first gemm's alpha */
        init_mm3(U, Rp, (double)s, tmp);
        init_mm3(tmp, Vt, 1.0, R[i]);
        init_mv3(U, tp, 1.0, t[i]);
        init_scale(t[i], 3, 1.0 / init_norm3(t[i]));
    }
    return true;
}

/* ---- CheckRT -------------------------------------------------------------------------------------------------------------- */

/* what CheckRT computes before its loop (:808-831): fx, fy, cx, cy, P1 = K [I | 0], P2 = K [R | t], O2 = -R.t() * t, th2 */
struct InitCheck {
    float fx, fy, cx, cy, th2;
    float P1[12], P2[12], R[9], t[3], O2[3];
};
DRFE_HD void init_check_setup(const float K[9], const float R[9], const float t[3], float sigma, InitCheck* C)
{
    C->fx = K[0]; C->fy = K[4]; C->cx = K[2]; C->cy = K[5];
    C->th2 = (float)(4.0 * (double)(sigma * sigma));
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) C->P1[r * 4 + c] = K[r * 3 + c];
        C->P1[r * 4 + 3] = 0.f;
    }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            const float b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
            C->P2[r * 4 + c] = init_gemm_out(K[r * 3] * b0 + K[r * 3 + 1] * b1 + K[r * 3 + 2] * b2, 1.0);
        }
    for (int k = 0; k < 9; k++) C->R[k] = R[k];
    for (int k = 0; k < 3; k++) C->t[k] = t[k];
    /* -R.t(): the transpose materialised, then a gemm with alpha = -1 */
    for (int r = 0; r < 3; r++) C->O2[r] = init_gemm_out(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2], -1.0);
}

enum { INIT_PT_COUNTED = 1, INIT_PT_GOOD = 2 };

/* one inlier match of CheckRT's loop (:840-898): INIT_PT_COUNTED when it reaches nGood++ (X and *cosOut are then what the loop
 * stores and pushes), INIT_PT_GOOD when vbGood becomes true */
DRFE_HD int init_check_point(const InitCheck& C, const InitMatch& m, float X[3], float* cosOut)
{
    float A[16], At[16], Vt[16];
    double W[4];
    tr_arow(m.u1, C.P1 + 8, C.P1 + 0, A + 0);
    tr_arow(m.v1, C.P1 + 8, C.P1 + 4, A + 4);
    tr_arow(m.u2, C.P2 + 8, C.P2 + 0, A + 8);
    tr_arow(m.v2, C.P2 + 8, C.P2 + 4, A + 12);
    for (int i = 0; i < 4; i++)
        for (int k = 0; k < 4; k++) At[i * 4 + k] = A[k * 4 + i];
    drfe_jacobi_svd<4>(At, W, Vt);
    float p[3] = {Vt[12], Vt[13], Vt[14]};
    init_scale(p, 3, 1.0 / (double)Vt[15]);
    if (!init_isfinite(p[0]) || !init_isfinite(p[1]) || !init_isfinite(p[2])) return 0;
    const float n1[3] = {p[0] - 0.f, p[1] - 0.f, p[2] - 0.f};
    const float dist1 = (float)init_norm3(n1);
    const float n2[3] = {p[0] - C.O2[0], p[1] - C.O2[1], p[2] - C.O2[2]};
    const float dist2 = (float)init_norm3(n2);
    const float cosParallax = (float)(tr_dotd(n1, n2) / (double)(dist1 * dist2));
    const bool lowParallax = !((double)cosParallax < 0.99998);
    if (p[2] <= 0 && !lowParallax) return 0;
    float p2[3];
    for (int r = 0; r < 3; r++) {
        const float d = C.R[r * 3] * p[0] + C.R[r * 3 + 1] * p[1] + C.R[r * 3 + 2] * p[2];
        p2[r] = (float)((double)d * 1.0 + (double)C.t[r] * 1.0);
    }
    if (p2[2] <= 0 && !lowParallax) return 0;
    const float invZ1 = (float)(1.0 / (double)p[2]);
    const float im1x = C.fx * p[0] * invZ1 + C.cx, im1y = C.fy * p[1] * invZ1 + C.cy;
    const float squareError1 = (im1x - m.u1) * (im1x - m.u1) + (im1y - m.v1) * (im1y - m.v1);
    if (squareError1 > C.th2) return 0;
    const float invZ2 = (float)(1.0 / (double)p2[2]);
    const float im2x = C.fx * p2[0] * invZ2 + C.cx, im2y = C.fy * p2[1] * invZ2 + C.cy;
    const float squareError2 = (im2x - m.u2) * (im2x - m.u2) + (im2y - m.v2) * (im2y - m.v2);
    if (squareError2 > C.th2) return 0;
    X[0] = p[0]; X[1] = p[1]; X[2] = p[2];
    *cosOut = cosParallax;
    return INIT_PT_COUNTED | (lowParallax ? 0 : INIT_PT_GOOD);
}

/* the order std::sort's `<` gives the accepted cosines, as unsigned keys: -0 counts as +0 (they compare equal, so which of the
 * two a sort leaves at an index is not defined) and a NaN - which `<` cannot order - above every number.  The value a key stands
 * for is init_cos_value. */
DRFE_HD uint32_t init_cos_key(float c)
{
    if (c != c) return 0xFFFFFFFFu;
    if (c == 0.f) c = 0.f;
    union { float f; uint32_t u; } v;
    v.f = c;
    return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}
DRFE_HD float init_cos_value(uint32_t key)
{
    if (key == 0xFFFFFFFFu) return __builtin_nanf("");
    union { float f; uint32_t u; } v;
    v.u = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
    return v.f;
}

#endif
