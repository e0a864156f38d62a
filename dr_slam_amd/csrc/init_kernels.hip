/* init_kernels.hip — Initializer's RANSAC and reconstruction (reference src/Initializer.cc) on gfx950, every row of every solver
 * of a call, driven by init.cpp.  DESIGN.md section 19.
 *   k_init_solve    one lane per (model, row), the H rows first: ComputeH21 or ComputeF21 on the row's eight matches, then H21i
 *                   and its inverse, or F21i.  The 16x9 with its 9x9 rotations, or the 8x9 with its ninth row, lives in LDS,
 *                   element-major over the 64 lanes (225 floats a lane, 56.25 KiB a workgroup, two workgroups a CU).
 *   k_init_score    workgroups over (solver, 32 rows, model), one wavefront per row at a time (ransac_device.h): CheckHomography
 *                   or CheckFundamental over the matches 64 at a time.  The ballot of the test is the mask word; the two
 *                   chi-square terms of a match are computed across the lanes and added to the score in index order.
 *   k_init_best     one lane per (solver, model): best[] over the scores in row order.
 *   k_init_motions  one lane per solver: RH, the branch and the 4 or 8 motion hypotheses.
 *   k_init_check    one wavefront per (solver, motion hypothesis): CheckRT over the inliers of the best row, Triangulate in the
 *                   lane, nGood by popcount, vP3D / vbGood scattered by the reference key (a match's key is unique), the selected
 *                   cosine by a radix rank selection over the accepted cosines' keys in LDS.
 * No float atomics; a sum is never split across lanes; no transcendental.  -ffp-contract=off, as the host entry. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "init_internal.h"
#include "ransac_device.h"

#define INIT_THREADS 256

__global__ __launch_bounds__(64) void k_init_solve(const InitLaunch L)
{
    __shared__ float big[225 * 64];
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= 2 * L.nHyp) return;
    const bool isF = g >= L.nHyp;
    const int w = isF ? g - L.nHyp : g;
    const InitSolverRec& S = L.solver[L.hypSolver[w]];
    const InitNorm* norm = L.norm + S.head.corr0;
    const int32_t* smp = L.sample + 8 * (size_t)w;
    InitNorm pts[8];
    for (int q = 0; q < 8; q++) pts[q] = norm[smp[q]];
    const InitStrided mem{big + threadIdx.x, 64};
    if (!isF) {
        float H21[9], H12[9];
        init_row_h(pts, S.T1, S.T2inv, mem, H21, H12);
        for (int k = 0; k < 9; k++) {
            L.H21[9 * (size_t)w + k] = init_canon(H21[k]);
            L.H12[9 * (size_t)w + k] = H12[k];
        }
    } else {
        float F21[9];
        init_row_f(pts, S.T1, S.T2t, mem, F21);
        for (int k = 0; k < 9; k++) L.F21[9 * (size_t)w + k] = init_canon(F21[k]);
    }
}

/* one row's check by one wavefront: chi(match, chi[2], in[2]) per lane, the mask words and the score by lane 0 */
template <class Chi>
__device__ __forceinline__ void init_sweep(const InitMatch* match, int N, int lane, uint64_t* mask, float* scoreOut, Chi chi)
{
    float score = 0.f;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        float c[2] = {0.f, 0.f};
        bool in[2] = {false, false};
        if (i < N) chi(match[i], c, in);
        const unsigned long long m0 = __ballot(in[0]), m1 = __ballot(in[1]);
        if (lane == 0) mask[base >> 6] = m0 & m1;
        const float t0 = 5.991f - c[0], t1 = 5.991f - c[1];
        const int cnt = N - base < 64 ? N - base : 64;
        for (int j = 0; j < cnt; j++) {                          /* uniform over the wavefront */
            const float a0 = __shfl(t0, j), a1 = __shfl(t1, j);
            if ((m0 >> j) & 1) score += a0;
            if ((m1 >> j) & 1) score += a1;
        }
    }
    if (lane == 0) *scoreOut = init_canon(score);
}

__global__ __launch_bounds__(INIT_THREADS) void k_init_score(const InitLaunch L)
{
    __shared__ InitMatch lds[DRFE_INIT_LDS_MATCH];
    const InitSolverRec& S = L.solver[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const bool isF = blockIdx.z == 1;
    ransac_count_rows<DRFE_INIT_CHUNK, INIT_THREADS>(S.head, L.match + S.head.corr0, lds,
                                                      [&](const InitMatch* match, int N, int h, size_t w) {
        float A[9], B[9];
        uint64_t* mask = (isF ? L.maskF : L.maskH) + S.head.mask0 + (size_t)h * S.head.words;
        if (isF) {
            for (int k = 0; k < 9; k++) A[k] = L.F21[9 * w + k];
            init_sweep(match, N, lane, mask, L.scoreF + w,
                       [&](const InitMatch& m, float* c, bool* in) { init_chi_f(A, m, S.invSigma2, c, in); });
        } else {
            for (int k = 0; k < 9; k++) { A[k] = L.H21[9 * w + k]; B[k] = L.H12[9 * w + k]; }
            init_sweep(match, N, lane, mask, L.scoreH + w,
                       [&](const InitMatch& m, float* c, bool* in) { init_chi_h(A, B, m, S.invSigma2, c, in); });
        }
    });
}

__global__ __launch_bounds__(64) void k_init_best(const InitLaunch L)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= 2 * L.nSolvers) return;
    const int s = g >> 1;
    const RansacSolverHead& S = L.solver[s].head;
    if (S.hyp == 0) return;
    if (g & 1) {
        const int b = init_walk_best(L.scoreF + S.hyp0, S.hyp, L.bestF + S.hyp0);
        L.lastF[s] = b;
        L.SF[s] = b >= 0 ? L.scoreF[S.hyp0 + b] : 0.f;
    } else {
        const int b = init_walk_best(L.scoreH + S.hyp0, S.hyp, L.bestH + S.hyp0);
        L.lastH[s] = b;
        L.SH[s] = b >= 0 ? L.scoreH[S.hyp0 + b] : 0.f;
    }
}

__global__ __launch_bounds__(64) void k_init_motions(const InitLaunch L)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= L.nSolvers) return;
    const InitSolverRec& S = L.solver[s];
    if (S.head.hyp == 0) return;
    int32_t branch, flags;
    float RH;
    init_pick_branch(L.SH[s], L.SF[s], S.head.n, &RH, &branch, &flags);
    int nm = 0;
    if (branch != DRFE_INIT_BRANCH_NONE) {
        const bool H = branch == DRFE_INIT_BRANCH_H;
        const float* model = H ? L.H21 + 9 * ((size_t)S.head.hyp0 + L.lastH[s]) : L.F21 + 9 * ((size_t)S.head.hyp0 + L.lastF[s]);
        float M[9];
        for (int k = 0; k < 9; k++) M[k] = model[k];
        nm = init_solver_motions(S.K, branch, M, L.mR + 72 * (size_t)s, L.mt + 24 * (size_t)s, &flags);
    }
    L.RH[s] = RH;
    L.branch[s] = branch;
    L.flags[s] = flags;
    L.motions[s] = nm;
}

__global__ __launch_bounds__(64) void k_init_check(const InitLaunch L)
{
    __shared__ uint32_t keys[DRFE_INIT_MAX_KEYS];
    const int s = blockIdx.y, m = blockIdx.x, lane = threadIdx.x;
    const InitSolverRec& S = L.solver[s];
    if (S.head.hyp == 0 || m >= L.motions[s]) return;             /* uniform over the workgroup, which is one wavefront */
    const bool H = L.branch[s] == DRFE_INIT_BRANCH_H;
    const int row = H ? L.lastH[s] : L.lastF[s];
    const uint64_t* mask = (H ? L.maskH : L.maskF) + S.head.mask0 + (size_t)row * S.head.words;
    const InitMatch* match = L.match + S.head.corr0;
    const int32_t* first = L.first + S.head.corr0;
    const size_t at = 8 * (size_t)S.key10 + (size_t)m * S.nKeys1;
    InitCheck C;
    init_check_setup(S.K, L.mR + 72 * (size_t)s + 9 * m, L.mt + 24 * (size_t)s + 3 * m, S.sigma, &C);
    const int N = S.head.n;
    int nGood = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        int code = 0;
        float X[3], c = 0.f;
        if (i < N && ((mask[base >> 6] >> lane) & 1)) code = init_check_point(C, match[i], X, &c);
        const bool counted = code & INIT_PT_COUNTED;
        const unsigned long long word = __ballot(counted);
        if (counted) {
            const size_t k = at + (size_t)first[i];
            for (int q = 0; q < 3; q++) L.mP3D[3 * k + q] = init_canon(X[q]);
            if (code & INIT_PT_GOOD) L.mVbGood[k] = 1;
            keys[nGood + __popcll(word & ((1ull << lane) - 1))] = init_cos_key(c);
        }
        nGood += __popcll(word);
    }
    __syncthreads();
    if (nGood == 0) return;
    /* the key of rank min(50, nGood - 1): bit by bit from the top, counting the keys that agree with the prefix and have a 0 */
    int k = nGood - 1 < 50 ? nGood - 1 : 50;
    uint32_t prefix = 0;
    bool nan = false;
    for (int bit = 31; bit >= 0; bit--) {
        int cnt = 0;
        for (int base = 0; base < nGood; base += 64) {
            const int j = base + lane;
            const uint32_t key = j < nGood ? keys[j] : 0u;
            cnt += __popcll(__ballot(j < nGood && ((key ^ prefix) >> bit) == 0));
            if (bit == 31) nan = nan || __ballot(j < nGood && key == 0xFFFFFFFFu) != 0;
        }
        if (k >= cnt) { k -= cnt; prefix |= 1u << bit; }
    }
    if (lane == 0) {
        L.mGood[8 * (size_t)s + m] = nGood;
        L.mCos[8 * (size_t)s + m] = init_cos_value(prefix);
        L.mStatus[8 * (size_t)s + m] = nan ? DRFE_INIT_MOTION_NAN_COS : 0;
    }
}

/* k_init_check alone, over branch, motions, lastH / lastF, the masks and mR / mt as they lie in L (drfe_debug_init_check_rt) */
hipError_t drfe_launch_init_check(const InitLaunch& L, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_check, dim3(8, L.nSolvers), dim3(64), 0, s, L);
    return hipGetLastError();
}

hipError_t drfe_launch_init(const InitLaunch& L, hipStream_t s)
{
    if (L.nHyp <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_solve, dim3((2 * L.nHyp + 63) / 64), dim3(64), 0, s, L);
    hipLaunchKernelGGL(k_init_score, dim3((L.maxHyp + DRFE_INIT_CHUNK - 1) / DRFE_INIT_CHUNK, L.nSolvers, 2), dim3(INIT_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_init_best, dim3((2 * L.nSolvers + 63) / 64), dim3(64), 0, s, L);
    hipLaunchKernelGGL(k_init_motions, dim3((L.nSolvers + 63) / 64), dim3(64), 0, s, L);
    hipLaunchKernelGGL(k_init_check, dim3(8, L.nSolvers), dim3(64), 0, s, L);
    return hipGetLastError();
}
