/* pnp_kernels.hip — PnPsolver's RANSAC (reference src/PnPsolver.cc) on gfx950, every row of every solver of a call, driven by
 * pnp.cpp.  DESIGN.md section 17.
 *   k_pnp_solve4   one lane per row: EPnP's compute_pose on its four sampled correspondences.  The 12x12 that the Jacobi SVD
 *                  rotates lives in LDS, element-major over the 64 lanes (72 KiB a workgroup, two workgroups a CU).
 *   k_pnp_count    workgroups over (solver, 32 rows), one wavefront per row at a time: CheckInliers over the correspondences 64
 *                  at a time (ransac_device.h).
 *   k_pnp_best     one lane per solver: best[] over its counts in row order, and the rows Refine has to run over.
 *   k_pnp_jobs     one workgroup: the solvers' job counts summed by prefix into one compact job list of the call.
 *   k_pnp_refine   one wavefront per refine job (a bounded grid strides over the list): compute_pose over the inliers of the
 *                  job's row in index order.  Each of the
 *                  independent ordered sums (centroids, the 6 + 78 MulTransposed elements, pc0 / pw0, ABt) runs in one lane over
 *                  the correspondences in order; the terms of the reprojection error are computed 64 at a time and added in
 *                  order; the small solves run in every lane alike.  Then CheckInliers over all N, as k_pnp_count.
 *   k_pnp_returns  one lane per solver: Refine's `>` at every row that reaches it.
 * No float or double atomics; a sum is never split across lanes.  -ffp-contract=off, as the host entry. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "pnp_internal.h"
#include "ransac_device.h"

#define PNP_THREADS 256
/* workgroups of the refine launch: two fit a CU (72 KiB of LDS each), 256 CUs, four rounds' worth; they stride over the job list */
#define PNP_REFINE_GRID 2048

/* one wavefront: independent sum e in lane e % 64, handed to every lane; an ordered sum of expensive terms 64 terms at a time */
struct PnpWave {
    int lane;
    template <int K, class F, class Put>
    __device__ void sums(F f, Put put) const
    {
        for (int e0 = 0; e0 < K; e0 += 64) {
            const int e = e0 + lane;
            const double v = e < K ? f(e) : 0.0;
            const int cnt = K - e0 < 64 ? K - e0 : 64;
            for (int j = 0; j < cnt; j++) put(e0 + j, __shfl(v, j));
        }
    }
    template <class F>
    __device__ double ordered_sum(const PnpSel& S, F term) const
    {
        double s = 0.0;
        for (int base = 0; base < S.slots; base += 64) {
            const int k = base + lane;
            const int i = k < S.slots ? S.at(k) : -1;
            const double v = i >= 0 ? term(i) : 0.0;
            for (unsigned long long m = __ballot(i >= 0); m; m &= m - 1) s += __shfl(v, __ffsll(m) - 1);
        }
        return s;
    }
};

__global__ __launch_bounds__(64) void k_pnp_solve4(const PnpLaunch L)
{
    __shared__ double big[144 * 64];
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= L.nHyp) return;
    const PnpSolverRec& S = L.solver[L.hypSolver[w]];
    const int32_t* smp = L.sample + 4 * (size_t)w;
    const PnpSel sel{L.corr + S.head.corr0, smp, nullptr, 4, 4, smp[0]};
    double R[9], t[3];
    pnp_compute_pose(PnpSerial(), sel, S.K, PnpStrided{big + threadIdx.x, 64}, R, t);
    for (int k = 0; k < 9; k++) L.R[9 * (size_t)w + k] = pnp_canon(R[k]);
    for (int k = 0; k < 3; k++) L.t[3 * (size_t)w + k] = pnp_canon(t[k]);
}

/* CheckInliers of one row by one wavefront */
__device__ __forceinline__ void pnp_sweep(const PnpCorr* corr, int N, const double R[9], const double t[3], const double K[4],
                                          int lane, uint64_t* mask, int32_t* countOut)
{
    ransac_sweep(corr, N, lane, mask, countOut, [&](const PnpCorr& c) { return pnp_inlier(c, R, t, K); });
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_count(const PnpLaunch L)
{
    __shared__ PnpCorr lds[DRFE_PNP_LDS_CORR];
    const PnpSolverRec& S = L.solver[blockIdx.y];
    const int lane = threadIdx.x & 63;
    ransac_count_rows<DRFE_PNP_CHUNK, PNP_THREADS>(S.head, L.corr + S.head.corr0, lds,
                                                    [&](const PnpCorr* corr, int N, int h, size_t w) {
        double R[9], t[3];
        for (int k = 0; k < 9; k++) R[k] = L.R[9 * w + k];
        for (int k = 0; k < 3; k++) t[k] = L.t[3 * w + k];
        pnp_sweep(corr, N, R, t, S.K, lane, L.mask + S.head.mask0 + (size_t)h * S.head.words, L.inliers + w);
    });
}

__global__ __launch_bounds__(64) void k_pnp_best(const PnpLaunch L)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= L.nSolvers) return;
    const RansacSolverHead& S = L.solver[s].head;
    L.nJobs[s] = pnp_walk_best(L.inliers + S.hyp0, S.hyp, S.minInliers, L.best + S.hyp0, L.jobs + S.hyp0);
}

/* the call's job list: solver s's jobs at [base(s), base(s) + nJobs[s]), base the prefix sum of nJobs.  One workgroup; each thread
 * owns a contiguous run of solvers, thread 0 scans the 256 run totals. */
__global__ __launch_bounds__(PNP_THREADS) void k_pnp_jobs(const PnpLaunch L)
{
    __shared__ int32_t base[PNP_THREADS];
    const int per = (L.nSolvers + PNP_THREADS - 1) / PNP_THREADS;
    const int s0 = threadIdx.x * per, s1 = s0 + per < L.nSolvers ? s0 + per : L.nSolvers;
    int32_t sum = 0;
    for (int s = s0; s < s1; s++) sum += L.nJobs[s];
    base[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t acc = 0;
        for (int k = 0; k < PNP_THREADS; k++) { const int32_t v = base[k]; base[k] = acc; acc += v; }
        *L.totalJobs = acc;
    }
    __syncthreads();
    int32_t at = base[threadIdx.x];
    for (int s = s0; s < s1; s++) {
        const RansacSolverHead& S = L.solver[s].head;
        for (int j = 0; j < L.nJobs[s]; j++, at++) {
            L.jobSolver[at] = s;
            L.jobRow[at] = L.jobs[S.hyp0 + j];
        }
    }
}

__global__ __launch_bounds__(64) void k_pnp_refine(const PnpLaunch L)
{
    __shared__ double big[144 * 64];
    const int total = *L.totalJobs, lane = threadIdx.x;
    for (int job = blockIdx.x; job < total; job += gridDim.x) {     /* uniform over the workgroup, which is one wavefront */
        const PnpSolverRec& S = L.solver[L.jobSolver[job]];
        const int h = L.jobRow[job];
        const size_t w = (size_t)S.head.hyp0 + h;
        const uint64_t* rowMask = L.mask + S.head.mask0 + (size_t)h * S.head.words;
        int first = 0;
        for (int q = 0; q < S.head.words; q++)
            if (rowMask[q]) { first = q * 64 + __ffsll((unsigned long long)rowMask[q]) - 1; break; }
        const PnpCorr* corr = L.corr + S.head.corr0;
        const PnpSel sel{corr, nullptr, rowMask, S.head.n, L.inliers[w], first};
        double R[9], t[3];
        pnp_compute_pose(PnpWave{lane}, sel, S.K, PnpStrided{big + lane, 64}, R, t);
        if (lane == 0) {
            for (int k = 0; k < 9; k++) L.refR[9 * w + k] = pnp_canon(R[k]);
            for (int k = 0; k < 3; k++) L.refT[3 * w + k] = pnp_canon(t[k]);
        }
        pnp_sweep(corr, S.head.n, R, t, S.K, lane, L.refMask + S.head.mask0 + (size_t)h * S.head.words, L.refInliers + w);
    }
}

__global__ __launch_bounds__(64) void k_pnp_returns(const PnpLaunch L)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= L.nSolvers) return;
    const RansacSolverHead& S = L.solver[s].head;
    pnp_walk_returns(L.inliers + S.hyp0, L.best + S.hyp0, L.refInliers + S.hyp0, S.hyp, S.minInliers, L.returns + S.hyp0);
}

hipError_t drfe_launch_pnp(const PnpLaunch& L, hipStream_t s)
{
    if (L.nHyp <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pnp_solve4, dim3((L.nHyp + 63) / 64), dim3(64), 0, s, L);
    hipLaunchKernelGGL(k_pnp_count, dim3((L.maxHyp + DRFE_PNP_CHUNK - 1) / DRFE_PNP_CHUNK, L.nSolvers), dim3(PNP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_pnp_best, dim3((L.nSolvers + 63) / 64), dim3(64), 0, s, L);
    hipLaunchKernelGGL(k_pnp_jobs, dim3(1), dim3(PNP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_pnp_refine, dim3(L.nHyp < PNP_REFINE_GRID ? L.nHyp : PNP_REFINE_GRID), dim3(64), 0, s, L);
    hipLaunchKernelGGL(k_pnp_returns, dim3((L.nSolvers + 63) / 64), dim3(64), 0, s, L);
    return hipGetLastError();
}

/* CheckInliers of n correspondences under one pose by one wavefront: the test hook behind drfe_debug_pnp_inliers_device */
__global__ __launch_bounds__(64) void k_pnp_sweep_one(const PnpCorr* corr, int n, const double* Rt, const double* K, uint64_t* mask,
                                                      int32_t* count)
{
    double R[9], t[3], Kd[4];
    for (int k = 0; k < 9; k++) R[k] = Rt[k];
    for (int k = 0; k < 3; k++) t[k] = Rt[9 + k];
    for (int k = 0; k < 4; k++) Kd[k] = K[k];
    pnp_sweep(corr, n, R, t, Kd, threadIdx.x, mask, count);
}

hipError_t drfe_launch_pnp_sweep_one(const PnpCorr* corr, int n, const double* Rt, const double* K, uint64_t* mask, int32_t* count,
                                     hipStream_t s)
{
    hipLaunchKernelGGL(k_pnp_sweep_one, dim3(1), dim3(64), 0, s, corr, n, Rt, K, mask, count);
    return hipGetLastError();
}
