/* sim3_kernels.hip — Sim3Solver's RANSAC (reference src/Sim3Solver.cc) on gfx950, every hypothesis of every solver of a call,
 * driven by sim3.cpp.  DESIGN.md section 16.
 *   k_sim3_prepare  one lane per correspondence: the two camera points, the two image points, the two bounds (Sim3Corr).
 *   k_sim3_horn     one lane per hypothesis: ComputeSim3 on its three sampled correspondences (Horn, the 4x4 Jacobi, Rodrigues in
 *                   float64); leaves R12, t12, s12, T12 in the table and T21 in scratch.
 *   k_sim3_count    workgroups over (solver, 32 hypotheses), one wavefront per hypothesis at a time: CheckInliers over the
 *                   correspondences 64 at a time (ransac_device.h).
 *   k_sim3_walk     one lane per solver: iterate's `>=` / `>` bookkeeping over its <= 300 counts in iteration order.
 * No float atomics and no sum across lanes: every float sum has the reference's order inside one lane.  -ffp-contract=off, as
 * the host entry. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sim3_internal.h"
#include "ransac_device.h"

#define SIM3_THREADS 256

__global__ __launch_bounds__(SIM3_THREADS) void k_sim3_prepare(const Sim3Launch L)
{
    const int i = blockIdx.x * SIM3_THREADS + threadIdx.x;
    if (i >= L.nCorr) return;
    const Sim3Solver& S = L.solver[L.corrSolver[i]];
    L.corr[i] = s3_corr(S.Tcw1, S.Tcw2, S.K1, S.K2, L.Xw1 + 3 * (size_t)i, L.Xw2 + 3 * (size_t)i, L.sig1[i], L.sig2[i]);
}

__global__ __launch_bounds__(64) void k_sim3_horn(const Sim3Launch L)
{
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= L.nHyp) return;
    const Sim3Solver& S = L.solver[L.hypSolver[w]];
    float P1[9], P2[9];
    for (int q = 0; q < 3; q++) {
        const Sim3Corr& c = L.corr[S.head.corr0 + L.sample[3 * (size_t)w + q]];
        for (int r = 0; r < 3; r++) {
            P1[r * 3 + q] = c.c1[r];
            P2[r * 3 + q] = c.c2[r];
        }
    }
    float R[9], t[3], s, T12[12], T21[12];
    const int ok = s3_horn(P1, P2, S.fixScale, 0, R, t, &s, T12, T21);
    for (int k = 0; k < 9; k++) L.R12[9 * (size_t)w + k] = s3_canon(R[k]);
    for (int k = 0; k < 3; k++) L.t12[3 * (size_t)w + k] = s3_canon(t[k]);
    L.s12[w] = s3_canon(s);
    for (int k = 0; k < 12; k++) {
        L.T12[12 * (size_t)w + k] = s3_canon(T12[k]);
        L.T21[12 * (size_t)w + k] = T21[k];
    }
    L.uncertified[w] = ok ? 0 : 1;
}

__global__ __launch_bounds__(SIM3_THREADS) void k_sim3_count(const Sim3Launch L)
{
    __shared__ Sim3Corr lds[DRFE_SIM3_LDS_CORR];
    const Sim3Solver& S = L.solver[blockIdx.y];
    const int lane = threadIdx.x & 63;
    ransac_count_rows<DRFE_SIM3_CHUNK, SIM3_THREADS>(S.head, L.corr + S.head.corr0, lds,
                                                    [&](const Sim3Corr* corr, int N, int h, size_t w) {
        float T12[12], T21[12];
        for (int k = 0; k < 12; k++) {
            T12[k] = L.T12[12 * w + k];
            T21[k] = L.T21[12 * w + k];
        }
        ransac_sweep(corr, N, lane, L.mask + S.head.mask0 + (size_t)h * S.head.words, L.inliers + w,
                     [&](const Sim3Corr& c) { return s3_inlier(c, T12, T21, S.K1, S.K2); });
    });
}

__global__ __launch_bounds__(64) void k_sim3_walk(const Sim3Launch L)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= L.nSolvers) return;
    const RansacSolverHead& S = L.solver[s].head;
    s3_walk(L.inliers + S.hyp0, S.hyp, S.minInliers, L.returns + S.hyp0, L.best + S.hyp0);
}

hipError_t drfe_launch_sim3(const Sim3Launch& L, hipStream_t s)
{
    if (L.nHyp <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sim3_prepare, dim3((L.nCorr + SIM3_THREADS - 1) / SIM3_THREADS), dim3(SIM3_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_sim3_horn, dim3((L.nHyp + 63) / 64), dim3(64), 0, s, L);
    hipLaunchKernelGGL(k_sim3_count, dim3((L.maxHyp + DRFE_SIM3_CHUNK - 1) / DRFE_SIM3_CHUNK, L.nSolvers), dim3(SIM3_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_sim3_walk, dim3((L.nSolvers + 63) / 64), dim3(64), 0, s, L);
    return hipGetLastError();
}
