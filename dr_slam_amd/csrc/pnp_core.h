/* pnp_core.h — the arithmetic of PnPsolver (reference src/PnPsolver.cc): EPnP's compute_pose (:477-525) with everything it
 * calls, CheckInliers (:308-339), and iterate's bookkeeping (:209-236) as two walks over finished inlier counts.  Shared by the
 * host entry (pnp.cpp) and the device kernels (pnp_kernels.hip) so that both produce the same bits: plain IEEE double add / mul /
 * div / sqrt, compiled with -ffp-contract=off on both sides, no transcendental.  The OpenCV pieces (MulTransposedR, the double
 * JacobiSVDImpl_, SVBkSb, cv::RNG) are restated from library knowledge and unpinned: DESIGN.md section 17.
 *
 * compute_pose keeps no per-correspondence array.  alphas and pcs are pure functions of a correspondence and a few small
 * matrices, so every sum over the correspondences recomputes them for the point it is at, in the reference's order.  How the
 * independent sums are spread (one after the other on the host and in the one-lane-per-hypothesis kernel, one per lane in the
 * refine kernel) is the policy's business; the order inside each sum is fixed here. */
#ifndef DRFE_PNP_CORE_H
#define DRFE_PNP_CORE_H

#include "../../include/drfe.h"
#include "../../include/drfe_math.h"

#include <float.h>
#include <stdint.h>
#include <string.h>

/* for member functions (DRFE_HD is for free ones) */
#if defined(__HIPCC__)
#define PNP_HDM __host__ __device__
#else
#define PNP_HDM
#endif

/* one correspondence of a solver: mvP2D, mvP3Dw, mvMaxError = sigma2 * th2 in float */
struct PnpCorr {
    float u, v, X[3], maxErr;
};

/* element k of a small matrix kept with a stride between its elements: 1 on the host, the lane count where every lane of a
 * wavefront keeps a matrix of its own in LDS (element-major, so a wavefront's accesses to element k are consecutive) */
struct PnpStrided {
    double* p;
    int stride;
    PNP_HDM double& operator[](int k) const { return p[(size_t)k * stride]; }
};

/* the correspondences one compute_pose runs over, as `slots` slots in the reference's order: the four sampled ones in draw order
 * (sample != null), or the set bits of a row's inlier mask in index order (Refine).  n of the slots are taken, `first` is the
 * first taken one's correspondence. */
struct PnpSel {
    const PnpCorr* corr;
    const int32_t* sample;
    const uint64_t* mask;
    int slots, n, first;
    PNP_HDM int at(int k) const
    {
        if (sample) return sample[k];
        return (mask[k >> 6] >> (k & 63)) & 1 ? k : -1;
    }
};

/* f(i, &s) for the taken slots of S in slot order: one ordered sum */
template <class F>
DRFE_HD double pnp_ordered_acc(const PnpSel& S, F f)
{
    double s = 0.0;
    for (int k = 0; k < S.slots; k++) {
        const int i = S.at(k);
        if (i >= 0) f(i, &s);
    }
    return s;
}
template <class F>
DRFE_HD double pnp_ordered_sum(const PnpSel& S, F term)
{
    return pnp_ordered_acc(S, [&](int i, double* s) { *s += term(i); });
}

/* every independent sum one after the other: put(e, f(e)) for e < K; and one ordered sum whose terms are expensive */
struct PnpSerial {
    template <int K, class F, class Put>
    PNP_HDM void sums(F f, Put put) const
    {
        for (int e = 0; e < K; e++) put(e, f(e));
    }
    template <class F>
    PNP_HDM double ordered_sum(const PnpSel& S, F term) const { return pnp_ordered_sum(S, term); }
};

/* cv::RNG::next (MWC, the multiplier of rng.hpp) */
DRFE_HD uint32_t pnp_rng_next(uint64_t* state)
{
    *state = (uint64_t)(uint32_t)*state * 4164903690u + (uint32_t)(*state >> 32);
    return (uint32_t)*state;
}

/* JacobiSVDImpl_<double> for an m x n matrix, m >= n, n1 = n: At holds A^T (n rows of m, row stride m) and is rotated in place;
 * on return W holds the singular values in decreasing order and At the left singular vectors as rows (the rotated rows
 * normalised; cv::RNG(0x12345678) vectors where a singular value is <= DBL_MIN), Vt (n x n, may be null: the rotations are then
 * not accumulated, which changes nothing else) the accumulated right rotations, all in W's order.  eps = 10 * DBL_EPSILON, at most
 * max(m, 30) sweeps.  hypot(p, beta) is canonicalised to sqrt(p * p + beta * beta) as in jacobi_svd_core.h. */
template <class TA>
DRFE_HD void pnp_jacobi_svd(TA At, int m, int n, double* W, double* Vt)
{
    const double eps = DBL_EPSILON * 10, minval = DBL_MIN;
    const int maxIter = m > 30 ? m : 30;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sd;
        if (Vt) {
            for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
            Vt[i * n + i] = 1;
        }
    }
    for (int iter = 0; iter < maxIter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += At[i * m + k] * At[j * m + k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const double ai = At[i * m + k], aj = At[j * m + k];
                    const double t0 = c * ai + s * aj;
                    const double t1 = -s * ai + c * aj;
                    At[i * m + k] = t0; At[j * m + k] = t1;
                    a += t0 * t0; b += t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                if (Vt) {
                    double *Vi = Vt + i * n, *Vj = Vt + j * n;
                    for (int k = 0; k < n; k++) {
                        const double t0 = c * Vi[k] + s * Vj[k];
                        const double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0; Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            for (int k = 0; k < m; k++) { const double t = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = t; }
            if (Vt)
                for (int k = 0; k < n; k++) { const double t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
        }
    }
    uint64_t rng = 0x12345678u;
    for (int i = 0; i < n; i++) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const double val0 = 1. / m;
            for (int k = 0; k < m; k++) At[i * m + k] = (pnp_rng_next(&rng) & 256) != 0 ? val0 : -val0;
            for (int iter = 0; iter < 2; iter++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    double asum = 0;
                    for (int k = 0; k < m; k++) {
                        const double t = At[i * m + k] - sd * At[j * m + k];
                        At[i * m + k] = t;
                        asum += fabs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
            sd = sqrt(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

/* SVBkSb's threshold: 2 * DBL_EPSILON * (w[0] + w[1] + ..), summed in order */
DRFE_HD double pnp_sv_threshold(const double* W, int n)
{
    double th = 0;
    for (int i = 0; i < n; i++) th += W[i];
    return th * (DBL_EPSILON * 2);
}

/* cvSolve(A, b, x, CV_SVD) for a 6 x n system: the SVD of A, then SVBkSb with one right-hand side */
DRFE_HD void pnp_svd_solve6(const double* A, int n, const double b[6], double* x)
{
    const int m = 6;
    double At[30], W[5], Vt[25];
    for (int i = 0; i < n; i++)
        for (int k = 0; k < m; k++) At[i * m + k] = A[k * n + i];
    pnp_jacobi_svd(At, m, n, W, Vt);
    for (int j = 0; j < n; j++) x[j] = 0;
    const double th = pnp_sv_threshold(W, n);
    for (int i = 0; i < n; i++) {
        double wi = W[i];
        if (fabs(wi) <= th) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < m; j++) s += At[i * m + j] * b[j];
        s *= wi;
        for (int j = 0; j < n; j++) x[j] = x[j] + s * Vt[i * n + j];
    }
}

/* cvInvert(A, Ainv, CV_SVD) of a 3x3: the SVD, then SVBkSb with no right-hand side (the identity) */
DRFE_HD void pnp_svd_invert3(const double A[9], double X[9])
{
    double At[9], W[3], Vt[9], buf[3];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) At[i * 3 + k] = A[k * 3 + i];
    pnp_jacobi_svd(At, 3, 3, W, Vt);
    for (int j = 0; j < 9; j++) X[j] = 0;
    const double th = pnp_sv_threshold(W, 3);
    for (int i = 0; i < 3; i++) {
        double wi = W[i];
        if (fabs(wi) <= th) continue;
        wi = 1 / wi;
        for (int j = 0; j < 3; j++) buf[j] = At[i * 3 + j] * wi;
        for (int r = 0; r < 3; r++) {
            const double s = Vt[i * 3 + r];
            for (int j = 0; j < 3; j++) X[r * 3 + j] = X[r * 3 + j] + s * buf[j];
        }
    }
}

/* qr_solve (:860-950) for the 6x4 system of gauss_newton, move for move.  When a column is all zero it returns early and leaves
 * X as it was: the caller's x is zero before the first round and stale afterwards (the reference reads an uninitialised stack
 * array there). */
DRFE_HD void pnp_qr_solve(double* pA, double* pb, double* pX)
{
    const int nr = 6, nc = 4;
    double A1[6], A2[6];
    double* ppAkk = pA;
    for (int k = 0; k < nc; k++) {
        double *ppAik = ppAkk, eta = fabs(*ppAik);
        for (int i = k + 1; i < nr; i++) {
            const double elt = fabs(*ppAik);
            if (eta < elt) eta = elt;
            ppAik += nc;
        }
        if (eta == 0) return;
        {
            double *q = ppAkk, sum = 0.0;
            const double inv_eta = 1. / eta;
            for (int i = k; i < nr; i++) {
                *q *= inv_eta;
                sum += *q * *q;
                q += nc;
            }
            double sigma = sqrt(sum);
            if (*ppAkk < 0) sigma = -sigma;
            *ppAkk += sigma;
            A1[k] = sigma * *ppAkk;
            A2[k] = -eta * sigma;
            for (int j = k + 1; j < nc; j++) {
                double *r = ppAkk, sum2 = 0;
                for (int i = k; i < nr; i++) {
                    sum2 += *r * r[j - k];
                    r += nc;
                }
                const double tau = sum2 / A1[k];
                r = ppAkk;
                for (int i = k; i < nr; i++) {
                    r[j - k] -= tau * *r;
                    r += nc;
                }
            }
        }
        ppAkk += nc + 1;
    }
    double* ppAjj = pA;
    for (int j = 0; j < nc; j++) {
        double *ppAij = ppAjj, tau = 0;
        for (int i = j; i < nr; i++) {
            tau += *ppAij * pb[i];
            ppAij += nc;
        }
        tau /= A1[j];
        ppAij = ppAjj;
        for (int i = j; i < nr; i++) {
            pb[i] -= tau * *ppAij;
            ppAij += nc;
        }
        ppAjj += nc + 1;
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double *ppAij = pA + i * nc + (i + 1), sum = 0;
        for (int j = i + 1; j < nc; j++) {
            sum += *ppAij * pX[j];
            ppAij++;
        }
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

/* gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838) */
DRFE_HD void pnp_gauss_newton(const double* L, const double* rho, double betas[4])
{
    double a[24], b[6], x[4] = {0, 0, 0, 0};
    for (int k = 0; k < 5; k++) {
        for (int i = 0; i < 6; i++) {
            const double* rowL = L + i * 10;
            double* rowA = a + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                             rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                             rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                             rowL[9] * betas[3] * betas[3]);
        }
        pnp_qr_solve(a, b, x);
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

DRFE_HD double pnp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

DRFE_HD double pnp_dist2(const double* p1, const double* p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

/* the three find_betas_approx_* (:667-758): which = 1, 2, 3 */
DRFE_HD void pnp_find_betas(int which, const double* L, const double* rho, double betas[4])
{
    double l[30], b[5];
    if (which == 1) {
        for (int i = 0; i < 6; i++) {
            l[i * 4 + 0] = L[i * 10 + 0]; l[i * 4 + 1] = L[i * 10 + 1]; l[i * 4 + 2] = L[i * 10 + 3]; l[i * 4 + 3] = L[i * 10 + 6];
        }
        pnp_svd_solve6(l, 4, rho, b);
        if (b[0] < 0) {
            betas[0] = sqrt(-b[0]);
            betas[1] = -b[1] / betas[0];
            betas[2] = -b[2] / betas[0];
            betas[3] = -b[3] / betas[0];
        } else {
            betas[0] = sqrt(b[0]);
            betas[1] = b[1] / betas[0];
            betas[2] = b[2] / betas[0];
            betas[3] = b[3] / betas[0];
        }
        return;
    }
    const int n = which == 2 ? 3 : 5;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < n; j++) l[i * n + j] = L[i * 10 + j];
    pnp_svd_solve6(l, n, rho, b);
    if (b[0] < 0) {
        betas[0] = sqrt(-b[0]);
        betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
    } else {
        betas[0] = sqrt(b[0]);
        betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = which == 2 ? 0.0 : b[3] / betas[0];
    betas[3] = 0.0;
}

/* compute_barycentric_coordinates' body for one correspondence (:423-433) */
DRFE_HD void pnp_alphas(const double ci[9], const double c0[3], const PnpCorr& q, double a[4])
{
    const double p0 = (double)q.X[0], p1 = (double)q.X[1], p2 = (double)q.X[2];
    for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * (p0 - c0[0]) + ci[3 * j + 1] * (p1 - c0[1]) + ci[3 * j + 2] * (p2 - c0[2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
}

/* compute_pcs' body for one correspondence (:468-474), negated where solve_for_sign negated the array */
DRFE_HD void pnp_pc(const double a[4], const double ccs[12], bool neg, double pc[3])
{
    for (int j = 0; j < 3; j++) {
        const double v = a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
        pc[j] = neg ? -v : v;
    }
}

/* element c of rows 2i (half = 0) and 2i + 1 (half = 1) of M (fill_M, :436-451) */
DRFE_HD double pnp_m(const double a[4], const double K[4], double u, double v, int half, int c)
{
    const int q = c / 3, r = c - 3 * q;
    if (half == 0) return r == 0 ? a[q] * K[0] : r == 1 ? 0.0 : a[q] * (K[2] - u);
    return r == 0 ? 0.0 : r == 1 ? a[q] * K[1] : a[q] * (K[3] - v);
}

/* compute_pose (:477-525) over the correspondences of S.  K = fu, fv, uc, vc.  big: room for the 12x12 (144 elements).  P: how
 * the independent sums are spread. */
template <class Pol, class Big>
DRFE_HD void pnp_compute_pose(const Pol& P, const PnpSel& S, const double K[4], Big big, double R[9], double t[3])
{
    const int n = S.n;
    const PnpCorr* corr = S.corr;
    double cws[4][3], c0[3];
    /* choose_control_points (:375-409) */
    P.template sums<3>([&](int j) { return pnp_ordered_sum(S, [&](int i) { return (double)corr[i].X[j]; }); },
                        [&](int j, double v) { c0[j] = v; });
    for (int j = 0; j < 3; j++) cws[0][j] = c0[j] / n;
    {
        /* cvMulTransposed(PW0, PW0tPW0, 1): the upper triangle, each element a sum over the rows in order, mirrored */
        double up[6], At[9], dc[3];
        P.template sums<6>([&](int e) {
            const int r = e < 3 ? 0 : e < 5 ? 1 : 2, c = e < 3 ? e : e < 5 ? e - 2 : 2;
            return pnp_ordered_sum(S, [&](int i) { return ((double)corr[i].X[r] - cws[0][r]) * ((double)corr[i].X[c] - cws[0][c]); });
        }, [&](int e, double v) { up[e] = v; });
        At[0] = up[0]; At[1] = At[3] = up[1]; At[2] = At[6] = up[2]; At[4] = up[3]; At[5] = At[7] = up[4]; At[8] = up[5];
        /* cvSVD(.., MODIFY_A | U_T) without V: dc the singular values, uct the left singular vectors as rows */
        pnp_jacobi_svd(At, 3, 3, dc, (double*)0);
        for (int i = 1; i < 4; i++) {
            const double k = sqrt(dc[i - 1] / n);
            for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * At[3 * (i - 1) + j];
        }
    }
    /* compute_barycentric_coordinates (:411-422) */
    double ci[9];
    {
        double cc[9];
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
        pnp_svd_invert3(cc, ci);
    }
    /* M^T M: 78 sums over the rows of M in order, mirrored into the 12x12, which is its own transpose */
    {
        P.template sums<78>([&](int e) {
            int r = 0, c = e;
            while (c >= 12 - r) { c -= 12 - r; r++; }
            c += r;
            return pnp_ordered_acc(S, [&](int i, double* s) {
                double a[4];
                pnp_alphas(ci, cws[0], corr[i], a);
                const double u = (double)corr[i].u, v = (double)corr[i].v;
                *s += pnp_m(a, K, u, v, 0, r) * pnp_m(a, K, u, v, 0, c);
                *s += pnp_m(a, K, u, v, 1, r) * pnp_m(a, K, u, v, 1, c);
            });
        }, [&](int e, double v) {
            int r = 0, c = e;
            while (c >= 12 - r) { c -= 12 - r; r++; }
            c += r;
            big[r * 12 + c] = v;
            big[c * 12 + r] = v;
        });
    }
    double vv[4][12];  /* v[0] .. v[3] = rows 11, 10, 9, 8 of ut */
    {
        double d[12];
        pnp_jacobi_svd(big, 12, 12, d, (double*)0);
        for (int i = 0; i < 4; i++)
            for (int k = 0; k < 12; k++) vv[i][k] = big[(11 - i) * 12 + k];
    }
    /* compute_L_6x10 (:760-800), compute_rho (:802-810) */
    double L[60], rho[6];
    {
        double dv[4][6][3];
        for (int i = 0; i < 4; i++) {
            int a = 0, b = 1;
            for (int j = 0; j < 6; j++) {
                dv[i][j][0] = vv[i][3 * a] - vv[i][3 * b];
                dv[i][j][1] = vv[i][3 * a + 1] - vv[i][3 * b + 1];
                dv[i][j][2] = vv[i][3 * a + 2] - vv[i][3 * b + 2];
                b++;
                if (b > 3) { a++; b = a + 1; }
            }
        }
        for (int i = 0; i < 6; i++) {
            double* row = L + 10 * i;
            row[0] = pnp_dot(dv[0][i], dv[0][i]);
            row[1] = 2.0f * pnp_dot(dv[0][i], dv[1][i]);
            row[2] = pnp_dot(dv[1][i], dv[1][i]);
            row[3] = 2.0f * pnp_dot(dv[0][i], dv[2][i]);
            row[4] = 2.0f * pnp_dot(dv[1][i], dv[2][i]);
            row[5] = pnp_dot(dv[2][i], dv[2][i]);
            row[6] = 2.0f * pnp_dot(dv[0][i], dv[3][i]);
            row[7] = 2.0f * pnp_dot(dv[1][i], dv[3][i]);
            row[8] = 2.0f * pnp_dot(dv[2][i], dv[3][i]);
            row[9] = pnp_dot(dv[3][i], dv[3][i]);
        }
        rho[0] = pnp_dist2(cws[0], cws[1]);
        rho[1] = pnp_dist2(cws[0], cws[2]);
        rho[2] = pnp_dist2(cws[0], cws[3]);
        rho[3] = pnp_dist2(cws[1], cws[2]);
        rho[4] = pnp_dist2(cws[1], cws[3]);
        rho[5] = pnp_dist2(cws[2], cws[3]);
    }
    double bestErr = 0;
    for (int which = 1; which <= 3; which++) {
        double betas[4], Rw[9], tw[3];
        pnp_find_betas(which, L, rho, betas);
        pnp_gauss_newton(L, rho, betas);
        /* compute_R_and_t (:651-662): compute_ccs, compute_pcs, solve_for_sign */
        double ccs[12];
        for (int k = 0; k < 12; k++) ccs[k] = 0.0f;
        for (int i = 0; i < 4; i++)
            for (int k = 0; k < 12; k++) ccs[k] += betas[i] * vv[i][k];
        bool neg = false;
        {
            double a[4], pc[3];
            pnp_alphas(ci, cws[0], corr[S.first], a);
            pnp_pc(a, ccs, false, pc);
            neg = pc[2] < 0.0;
        }
        /* estimate_R_and_t (:569-627) */
        double cen[6];
        P.template sums<6>([&](int e) {
            return pnp_ordered_sum(S, [&](int i) {
                if (e >= 3) return (double)corr[i].X[e - 3];
                double a[4], pc[3];
                pnp_alphas(ci, cws[0], corr[i], a);
                pnp_pc(a, ccs, neg, pc);
                return pc[e];
            });
        }, [&](int e, double v) { cen[e] = v; });
        for (int j = 0; j < 6; j++) cen[j] /= n;
        const double *pc0 = cen, *pw0 = cen + 3;
        double abt[9];
        P.template sums<9>([&](int e) {
            const int j = e / 3, k = e - 3 * j;
            return pnp_ordered_sum(S, [&](int i) {
                double a[4], pc[3];
                pnp_alphas(ci, cws[0], corr[i], a);
                pnp_pc(a, ccs, neg, pc);
                return (pc[j] - pc0[j]) * ((double)corr[i].X[k] - pw0[k]);
            });
        }, [&](int e, double v) { abt[e] = v; });
        {
            /* cvSVD(ABt, D, U, V, MODIFY_A): U[i][j] = At[j][i] of the left vectors' rows, V[i][j] = Vt[j][i] */
            double At[9], W[3], Vt[9];
            for (int i = 0; i < 3; i++)
                for (int k = 0; k < 3; k++) At[i * 3 + k] = abt[k * 3 + i];
            pnp_jacobi_svd(At, 3, 3, W, Vt);
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) Rw[i * 3 + j] = At[i] * Vt[j] + At[3 + i] * Vt[3 + j] + At[6 + i] * Vt[6 + j];
        }
        const double det = Rw[0] * Rw[4] * Rw[8] + Rw[1] * Rw[5] * Rw[6] + Rw[2] * Rw[3] * Rw[7] - Rw[2] * Rw[4] * Rw[6] -
                           Rw[1] * Rw[3] * Rw[8] - Rw[0] * Rw[5] * Rw[7];
        if (det < 0) {
            Rw[6] = -Rw[6];
            Rw[7] = -Rw[7];
            Rw[8] = -Rw[8];
        }
        tw[0] = pc0[0] - pnp_dot(Rw, pw0);
        tw[1] = pc0[1] - pnp_dot(Rw + 3, pw0);
        tw[2] = pc0[2] - pnp_dot(Rw + 6, pw0);
        /* reprojection_error (:550-567) */
        const double sum2 = P.ordered_sum(S, [&](int i) {
            const double pw[3] = {(double)corr[i].X[0], (double)corr[i].X[1], (double)corr[i].X[2]};
            const double Xc = pnp_dot(Rw, pw) + tw[0];
            const double Yc = pnp_dot(Rw + 3, pw) + tw[1];
            const double inv_Zc = 1.0 / (pnp_dot(Rw + 6, pw) + tw[2]);
            const double ue = K[2] + K[0] * Xc * inv_Zc;
            const double ve = K[3] + K[1] * Yc * inv_Zc;
            const double u = (double)corr[i].u, v = (double)corr[i].v;
            return sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
        });
        const double err = sum2 / n;
        /* N = 1; if (e2 < e1) N = 2; if (e3 < e[N]) N = 3 */
        if (which == 1 || err < bestErr) {
            bestErr = err;
            for (int k = 0; k < 9; k++) R[k] = Rw[k];
            for (int k = 0; k < 3; k++) t[k] = tw[k];
        }
    }
}

/* CheckInliers' body for one correspondence (:314-337) */
DRFE_HD bool pnp_inlier(const PnpCorr& q, const double R[9], const double t[3], const double K[4])
{
    const float Xc = (float)(R[0] * q.X[0] + R[1] * q.X[1] + R[2] * q.X[2] + t[0]);
    const float Yc = (float)(R[3] * q.X[0] + R[4] * q.X[1] + R[5] * q.X[2] + t[1]);
    const float invZc = (float)(1 / (R[6] * q.X[0] + R[7] * q.X[1] + R[8] * q.X[2] + t[2]));
    const double ue = K[2] + K[0] * Xc * invZc;
    const double ve = K[3] + K[1] * Yc * invZc;
    const float distX = (float)(q.u - ue);
    const float distY = (float)(q.v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < q.maxErr;
}

/* a NaN leaves the entries as the one quiet NaN 0x7FF8000000000000: x86-64 and gfx950 give an invalid operation different signs */
DRFE_HD double pnp_canon(double v)
{
    if (v == v) return v;
    const uint64_t q = 0x7FF8000000000000ull;
    double d;
    memcpy(&d, &q, 8);
    return d;
}

/* iterate's `>=` / `>` bookkeeping (:209-224) over the inlier counts of rows 0 .. n-1: best[h] the row that holds mBest* after
 * row h (-1: none yet), jobs the rows Refine has to run over (each distinct best row, in order).  Returns their number. */
DRFE_HD int pnp_walk_best(const int32_t* count, int n, int minInliers, int32_t* best, int32_t* jobs)
{
    int bestCount = 0, bestIdx = -1, nj = 0;
    for (int h = 0; h < n; h++) {
        if (count[h] >= minInliers && count[h] > bestCount) {
            bestCount = count[h];
            bestIdx = h;
            jobs[nj++] = h;
        }
        best[h] = bestIdx;
    }
    return nj;
}

/* Refine's `>` (:292) at every row that reaches it */
DRFE_HD void pnp_walk_returns(const int32_t* count, const int32_t* best, const int32_t* refined, int n, int minInliers, uint8_t* returns)
{
    for (int h = 0; h < n; h++) returns[h] = (count[h] >= minInliers && refined[best[h]] > minInliers) ? 1 : 0;
}

#endif
