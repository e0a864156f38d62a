/* map_upkeep_kernels.hip — MapPoint / MapLine descriptor and normal upkeep (reference src/MapPoint.cc:288-411,
 * src/MapLine.cpp:241-362) on gfx950, driven by map_upkeep.cpp.  DESIGN.md section 14.
 *   k_mu_items       one lane per item: the normal and distance band (map_upkeep_core.h, observations in order), the status
 *                    byte, the frustum record, and best = -1 / zero bytes where no device descriptor kernel writes them;
 *   k_mu_desc_group  items of at most G descriptor rows, 256 / G items per workgroup: lane l of a group holds row l, row j comes
 *                    to every lane by ds_bpermute, the G x G distances go to LDS, each row's median is a rank selection
 *                    (bisection on the value, 9 counting passes), and the group's minimum of (median << 16) | row picks the
 *                    first row with the least median;
 *   k_mu_desc_wg     one workgroup per item of up to DRFE_UPKEEP_DEVICE_ROWS rows: the rows in LDS, one thread per row,
 *                    distances recomputed in every selection pass (N^2 does not fit), the minimum over the workgroup.
 * Integer work only in the descriptor kernels; -ffp-contract=off for the float chains. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "map_upkeep_internal.h"
#include "map_upkeep_core.h"

#define MU_THREADS 256

/* k-th smallest (0-based) of the n distances of row `lane` in a column-major n x G block (entry (lane, j) at D[j * G + lane]):
 * the least v in [0, 256] with #{d <= v} > k */
template <int G>
__device__ __forceinline__ int mu_select(const uint16_t* D, int lane, int n, int k)
{
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
        for (int j = 0; j < n; j++) cnt += D[j * G + lane] <= mid ? 1 : 0;
        if (cnt > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void mu_load_row(const uint4* rows, int r, uint32_t w[8])
{
    const uint4 a = rows[2 * (size_t)r], b = rows[2 * (size_t)r + 1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

__device__ __forceinline__ void mu_store_desc(uint4* desc, int item, const uint32_t w[8])
{
    desc[2 * (size_t)item] = make_uint4(w[0], w[1], w[2], w[3]);
    desc[2 * (size_t)item + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}

template <int G>
__global__ __launch_bounds__(MU_THREADS) void k_mu_desc_group(const MuItem* __restrict__ items, const int32_t* __restrict__ list,
                                                              int count, const uint4* __restrict__ rows,
                                                              const int32_t* __restrict__ rowObs, int32_t* __restrict__ best,
                                                              uint4* __restrict__ desc)
{
    __shared__ uint16_t D[MU_THREADS * G];                /* per group: G x G, column-major */
    const int g = threadIdx.x / G, l = threadIdx.x % G, base = threadIdx.x - l;
    const int slot = blockIdx.x * (MU_THREADS / G) + g;
    int item = -1, nr = 0, row0 = 0;
    if (slot < count) {
        item = list[slot];
        const MuItem it = items[item];
        nr = it.nrows;
        row0 = it.row0;
    }
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (l < nr) mu_load_row(rows, row0 + l, w);
    uint16_t* Dg = D + g * G * G;
    /* every lane runs every trip (ds_bpermute reads lanes of the own group only); j >= nr gives distances nobody reads.  With
     * one group per wavefront (G == 64) nr is wave-uniform and bounds the loop. */
    const int trips = G == 64 ? nr : G;
    for (int j = 0; j < trips; j++) {
        uint32_t r[8];
        for (int k = 0; k < 8; k++) r[k] = (uint32_t)__shfl((int)w[k], base + j, 64);
        const int d = mu_hamming(w, r);
        if (l < nr && j < nr) Dg[j * G + l] = (uint16_t)d;
    }
    __syncthreads();
    uint32_t key = 0xFFFFFFFFu;
    if (l < nr) key = mu_key(mu_select<G>(Dg, l, nr, mu_median_rank(nr)), l);
    if (G == 64) {
        key = drfe_wave_min_u32(key);
    } else {
        for (int m = G / 2; m >= 1; m >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, m, G));
    }
    const int win = (int)(key & 0xFFFFu);
    if (nr > 0 && l == win) {
        best[item] = rowObs[row0 + win];
        mu_store_desc(desc, item, w);
    }
}

__global__ __launch_bounds__(MU_THREADS) void k_mu_desc_wg(const MuItem* __restrict__ items, const int32_t* __restrict__ list,
                                                           const uint4* __restrict__ rows, const int32_t* __restrict__ rowObs,
                                                           int32_t* __restrict__ best, uint4* __restrict__ desc)
{
    extern __shared__ uint4 R[];                           /* 2 x uint4 per row */
    __shared__ uint32_t wmin[MU_THREADS / 64];
    const int item = list[blockIdx.x];
    const MuItem it = items[item];
    const int nr = it.nrows, k = mu_median_rank(nr);
    for (int q = threadIdx.x; q < 2 * nr; q += MU_THREADS) R[q] = rows[2 * (size_t)it.row0 + q];
    __syncthreads();
    uint32_t key = 0xFFFFFFFFu;
    for (int r = threadIdx.x; r < nr; r += MU_THREADS) {
        uint32_t w[8];
        mu_load_row(R, r, w);
        int lo = 0, hi = 256;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
            for (int j = 0; j < nr; j++) {
                uint32_t o[8];
                mu_load_row(R, j, o);
                cnt += mu_hamming(w, o) <= mid ? 1 : 0;
            }
            if (cnt > k) hi = mid;
            else lo = mid + 1;
        }
        key = min(key, mu_key(lo, r));
    }
    key = drfe_wave_min_u32(key);
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = wmin[0];
        for (int v = 1; v < MU_THREADS / 64; v++) m = min(m, wmin[v]);
        const int win = (int)(m & 0xFFFFu);
        best[item] = rowObs[it.row0 + win];
        desc[2 * (size_t)item] = R[2 * win];
        desc[2 * (size_t)item + 1] = R[2 * win + 1];
    }
}

template <bool Line>
__global__ __launch_bounds__(MU_THREADS) void k_mu_items(const MuLaunch L)
{
    const int i = blockIdx.x * MU_THREADS + threadIdx.x;
    if (i >= L.n) return;
    const MuItem it = L.items[i];
    uint8_t st = 0;
    if (it.flags & MU_HAS_ROWS) st |= DRFE_UPKEEP_DESCRIPTOR;
    if (!(it.flags & MU_DEVICE_DESC)) {
        L.best[i] = -1;
        L.desc[2 * (size_t)i] = make_uint4(0, 0, 0, 0);
        L.desc[2 * (size_t)i + 1] = make_uint4(0, 0, 0, 0);
    }
    float maxD = 0.f, minD = 0.f;
    const bool normal = (L.what & DRFE_UPKEEP_NORMAL) && (it.flags & MU_ACTIVE);
    if (normal) st |= DRFE_UPKEEP_NORMAL;
    const float* OwRef = L.kfCenter + 3 * (size_t)it.refKf;
    if (!Line) {
        const float* X = static_cast<const float*>(L.world) + 3 * (size_t)i;
        float nrm[3] = {0.f, 0.f, 0.f};
        if (normal) {
            for (int o = it.obs0; o < it.obs0 + it.nobs; o++) mu_point_obs(nrm, X, L.kfCenter + 3 * (size_t)L.obsKf[o]);
            mu_point_finish(nrm, it.nobs, X, OwRef, L.scale[it.level], L.scale[L.nLevels - 1], &maxD, &minD);
        }
        float* N = static_cast<float*>(L.normal) + 3 * (size_t)i;
        N[0] = nrm[0]; N[1] = nrm[1]; N[2] = nrm[2];
        if (L.frustum) {
            drfe_frustum_point* f = static_cast<drfe_frustum_point*>(L.frustum) + i;
            for (int k = 0; k < 3; k++) {
                f->world[k] = normal ? X[k] : 0.f;
                f->normal[k] = nrm[k];
            }
            f->min_distance = 0.8f * minD;
            f->max_distance = 1.2f * maxD;
        }
    } else {
        const double* P = static_cast<const double*>(L.world) + 6 * (size_t)i;
        double nrm[3] = {0.0, 0.0, 0.0};
        if (normal) {
            for (int o = it.obs0; o < it.obs0 + it.nobs; o++) mu_line_obs(nrm, P, L.kfCenter + 3 * (size_t)L.obsKf[o]);
            mu_line_finish(nrm, it.nobs, P, OwRef, L.scale[it.level], L.scale[L.nLevels - 1], &maxD, &minD);
        }
        double* N = static_cast<double*>(L.normal) + 3 * (size_t)i;
        N[0] = nrm[0]; N[1] = nrm[1]; N[2] = nrm[2];
        if (L.frustum) {
            drfe_frustum_line* f = static_cast<drfe_frustum_line*>(L.frustum) + i;
            for (int k = 0; k < 6; k++) f->world[k] = normal ? P[k] : 0.0;
            for (int k = 0; k < 3; k++) f->normal[k] = nrm[k];
            f->min_distance = 0.8f * minD;
            f->max_distance = 1.2f * maxD;
        }
    }
    L.maxD[i] = maxD;
    L.minD[i] = minD;
    L.status[i] = st;
}

hipError_t drfe_launch_map_upkeep(const MuLaunch& L, hipStream_t s)
{
    if (L.n <= 0) return hipSuccess;
    const int blocks = (L.n + MU_THREADS - 1) / MU_THREADS;
    if (L.line) hipLaunchKernelGGL(k_mu_items<true>, dim3(blocks), dim3(MU_THREADS), 0, s, L);
    else hipLaunchKernelGGL(k_mu_items<false>, dim3(blocks), dim3(MU_THREADS), 0, s, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (L.count[MU_B4] > 0)
        hipLaunchKernelGGL(k_mu_desc_group<4>, dim3((L.count[MU_B4] + 63) / 64), dim3(MU_THREADS), 0, s, L.items, L.list[MU_B4],
                           L.count[MU_B4], L.rows, L.rowObs, L.best, L.desc);
    if (L.count[MU_B16] > 0)
        hipLaunchKernelGGL(k_mu_desc_group<16>, dim3((L.count[MU_B16] + 15) / 16), dim3(MU_THREADS), 0, s, L.items, L.list[MU_B16],
                           L.count[MU_B16], L.rows, L.rowObs, L.best, L.desc);
    if (L.count[MU_B64] > 0)
        hipLaunchKernelGGL(k_mu_desc_group<64>, dim3((L.count[MU_B64] + 3) / 4), dim3(MU_THREADS), 0, s, L.items, L.list[MU_B64],
                           L.count[MU_B64], L.rows, L.rowObs, L.best, L.desc);
    if (L.count[MU_BWG] > 0) {
        /* rows of up to DRFE_UPKEEP_DEVICE_ROWS items in LDS: above the 64 KiB default */
        static const hipError_t attr = hipFuncSetAttribute((const void*)k_mu_desc_wg, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                           DRFE_UPKEEP_DEVICE_ROWS * 32);
        if (attr != hipSuccess) return attr;
        hipLaunchKernelGGL(k_mu_desc_wg, dim3(L.count[MU_BWG]), dim3(MU_THREADS), (size_t)L.maxRowsWg * 32, s, L.items,
                           L.list[MU_BWG], L.rows, L.rowObs, L.best, L.desc);
    }
    return hipGetLastError();
}
