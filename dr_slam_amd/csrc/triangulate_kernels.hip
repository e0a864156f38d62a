/* triangulate_kernels.hip — LocalMapping::CreateNewMapPoints / CreateNewMapLines2's per-match body (reference
 * src/LocalMapping.cc:383-538, 875-1026) on gfx950, driven by triangulate.cpp.  DESIGN.md section 15.
 *   k_tri_match  one lane per match: the branch, the point (the 4x4 Jacobi SVD in float64, or the stereo unprojection) or the
 *                line's endpoints (triangulate_core.h), every gate, the status byte.  Compacting the SVD-branch matches into a
 *                launch of their own was measured and not adopted.
 * -ffp-contract=off, as the host entries. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "triangulate_internal.h"

#define TRI_THREADS 256

__device__ __forceinline__ void tri_write(const TriLaunch& L, int i, int st, int br, const float* X)
{
    L.status[i] = (uint8_t)st;
    L.branch[i] = (uint8_t)br;
    const int w = L.line ? 6 : 3;
    const bool ok = (st & 0x7F) == DRFE_TRI_ACCEPTED;
    for (int k = 0; k < w; k++) L.x3d[(size_t)w * i + k] = ok ? X[k] : 0.f;
}

__global__ __launch_bounds__(TRI_THREADS) void k_tri_match(const TriLaunch L)
{
    const int i = blockIdx.x * TRI_THREADS + threadIdx.x;
    if (i >= L.n) return;
    const TriMatch m = L.match[i];
    float X[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (m.kf1 < 0) {
        tri_write(L, i, DRFE_TRI_BASELINE, DRFE_TRI_BRANCH_NONE, X);
        return;
    }
    const int o1 = L.V.off[m.kf1], g1 = o1 + m.idx1, g2 = L.V.off[m.kf2] + m.idx2;
    int br = 0, st;
    if (L.line) {
        const int q2 = m.idx2 < L.V.off[m.kf1 + 1] - o1 ? o1 + m.idx2 : -1;
        st = tr_line(L.V, m.kf1, m.kf2, g1, g2, q2, X, X + 3, &br);
    } else {
        st = tr_point(L.V, m.kf1, m.kf2, g1, g2, X, &br);
    }
    tri_write(L, i, st, br, X);
}

/* the test hook behind drfe_debug_triangulate_math_device: drfe_math.h's canonical atan2f / cosf as this file compiles them,
 * one lane per element, the expressions of the host hook (and of tr_point's stereo parallax for which == 2) */
__global__ __launch_bounds__(TRI_THREADS) void k_tri_math(int which, const float* __restrict__ y, const float* __restrict__ x, int n,
                                                          float* __restrict__ out)
{
    const int i = blockIdx.x * TRI_THREADS + threadIdx.x;
    if (i >= n) return;
    out[i] = which == 0 ? drfe_atan2f(y[i], x[i]) : which == 1 ? drfe_cosf(y[i]) : drfe_cosf(2 * drfe_atan2f(y[i] / 2, x[i]));
}

hipError_t drfe_launch_triangulate_math(int which, const float* y, const float* x, int n, float* out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tri_math, dim3((n + TRI_THREADS - 1) / TRI_THREADS), dim3(TRI_THREADS), 0, s, which, y, x, n, out);
    return hipGetLastError();
}

hipError_t drfe_launch_triangulate(const TriLaunch& L, hipStream_t s)
{
    if (L.n <= 0) return hipSuccess;
    const int blocks = (L.n + TRI_THREADS - 1) / TRI_THREADS;
    hipLaunchKernelGGL(k_tri_match, dim3(blocks), dim3(TRI_THREADS), 0, s, L);
    return hipGetLastError();
}
