/* jacobi_svd_core.h — the one-sided Jacobi SVD of OpenCV's JacobiSVDImpl_<float> for a square N x N CV_32F (N = 3: the
 * Manhattan-frame tracker's polar factor, manhattan_core.h; N = 4: linear triangulation, triangulate_core.h).  Shared by the
 * host entries and the device kernels so that both produce the same bits; plain IEEE add / mul / div / sqrt, compiled with
 * -ffp-contract=off on both sides.  DESIGN.md sections 11 and 15; the OpenCV reading is unpinned. */
#ifndef DRFE_JACOBI_SVD_CORE_H
#define DRFE_JACOBI_SVD_CORE_H

#include "../../include/drfe_math.h"

/* _SVDcompute's call for m = n = n1 = N (At = A^T, eps = 2 * FLT_EPSILON, at most max(N, 30) = 30 sweeps): on return W holds
 * the singular values sorted in decreasing order, At the rotated rows (A^T with its rows scaled by W, in W's order) and Vt the
 * accumulated right rotations, both permuted with W.  The left singular vectors (the normalisation of At and cv::RNG's random
 * vector for a zero singular value) are the caller's.  hypot(p, beta) is canonicalised to sqrt(p * p + beta * beta) (glibc's
 * last bit is host dependent).  VBLAS<float>::givens, which rotates Vt's rows four at a time when N = 4, computes b c - a s
 * where the scalar loop computes -s a + c b: the same IEEE value, so one loop serves both. */
template <int N>
DRFE_HD void drfe_jacobi_svd(float At[N * N], double W[N], float Vt[N * N])
{
    const float eps = 2.0f * 1.1920928955078125e-07f;
    for (int i = 0; i < N; i++) {
        double sd = 0;
        for (int k = 0; k < N; k++) { const float t = At[i * N + k]; sd += (double)t * t; }
        W[i] = sd;
        for (int k = 0; k < N; k++) Vt[i * N + k] = 0.f;
        Vt[i * N + i] = 1.f;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < N - 1; i++)
            for (int j = i + 1; j < N; j++) {
                float *Ai = At + i * N, *Aj = At + j * N;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < N; k++) p += (double)Ai[k] * Aj[k];
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
                for (int k = 0; k < N; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                float *Vi = Vt + i * N, *Vj = Vt + j * N;
                for (int k = 0; k < N; k++) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < N; i++) {
        double sd = 0;
        for (int k = 0; k < N; k++) { const float t = At[i * N + k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < N - 1; i++) {
        int j = i;
        for (int k = i + 1; k < N; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            for (int k = 0; k < N; k++) {
                float t = At[i * N + k]; At[i * N + k] = At[j * N + k]; At[j * N + k] = t;
                t = Vt[i * N + k]; Vt[i * N + k] = Vt[j * N + k]; Vt[j * N + k] = t;
            }
        }
    }
}

#endif
