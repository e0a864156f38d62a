/* plane_match_kernels.hip — plane association (PlaneMatcher::SearchMapByCoefficients, reference src/PlaneMatcher.cpp:11-91,
 * and Map::FlagMatchedPlanePoints, src/Map.cc:406-431) of a batch of frames against device-resident maps, on gfx950.
 *
 * Four launches on one stream, no inter-workgroup flags inside a launch:
 *   k_pm_gate    one workgroup per frame plane q: the world coefficients, the angle with every plane of its map, and for the
 *                pairs that pass the gate (and whose map plane is not bad) one work item per PM_CHUNK points of the cloud,
 *                appended to a work list through an atomic counter (the list order does not matter: see below);
 *   k_pm_dist    a grid-stride loop over the work list: 256 lanes take PointDistanceFromPlane's per-point term of their chunk
 *                as a u32 key (plane_match_core.h), a wavefront min, then one atomicMin per wavefront into the pair's key.
 *                A minimum of floats is order-free, so the result equals the reference's sequential scan bit for bit;
 *   k_pm_decide  one lane per frame plane replays the reference's sequential decision over (angle, distance) in
 *                vpMapPlanes order; the found count per frame is an integer atomicAdd;
 *   k_pm_flags   (flag_points) one workgroup per (matched frame plane, PM_FLAG_POINTS map points): sticky byte flags (an OR,
 *                order-free) and the pair count, a wavefront sum then one atomicAdd.
 * The accumulators (keys, counter, counts, flags) are reset by memsets on the stream before the launches (plane_match.cpp).
 * All arithmetic is plane_match_core.h, shared with the host entry; -ffp-contract=off. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "post_internal.h"
#include "plane_match_core.h"

#define PM_THREADS 256
#define PM_DIST_GRID 2048         /* workgroups of the grid-stride distance pass (8 per CU) */

__global__ __launch_bounds__(PM_THREADS) void k_pm_gate(PmLaunch L)
{
    const int q = blockIdx.x;
    const int f = L.qFrame[q], m = L.qMap[q], pb = L.planeOff[m], M = L.planeOff[m + 1] - pb, pr = L.qPair[q];
    float pM[4];
    pm_world_coef(L.Tcw + 16 * (size_t)f, L.coefs + 4 * (size_t)q, pM);
    for (int j = threadIdx.x; j < M; j += PM_THREADS) {
        const int gj = pb + j;
        const float a = pm_angle(pM, L.mapCoefs + 4 * (size_t)gj);
        L.angle[pr + j] = a;
        if (L.mapBad[gj] || !pm_gate(a, L.params.aTh)) continue;
        const int nch = (L.cloudEnd[gj] - L.cloudBeg[gj] + PM_CHUNK - 1) / PM_CHUNK;
        if (nch == 0) continue;
        const uint32_t base = atomicAdd(L.counter, (uint32_t)nch);
        for (int c = 0; c < nch; c++)
            if (base + c < (uint32_t)L.workCap) L.work[base + c] = make_int4(q, gj, pr + j, c);
    }
}

__global__ __launch_bounds__(PM_THREADS) void k_pm_dist(PmLaunch L)
{
    const uint32_t n = min(*L.counter, (uint32_t)L.workCap);
    for (uint32_t it = blockIdx.x; it < n; it += gridDim.x) {
        const int4 w = L.work[it];
        float pM[4];
        pm_world_coef(L.Tcw + 16 * (size_t)L.qFrame[w.x], L.coefs + 4 * (size_t)w.x, pM);
        const int lo = L.cloudBeg[w.y] + w.w * PM_CHUNK, hi = min(lo + PM_CHUNK, L.cloudEnd[w.y]);
        uint32_t k = PM_NO_DISTANCE_BITS;
        for (int p = lo + (int)threadIdx.x; p < hi; p += PM_THREADS) {
            const float* xyz = L.cloud + 3 * (size_t)p;
            k = min(k, pm_point_key(pM, xyz[0], xyz[1], xyz[2]));
        }
        k = drfe_wave_min_u32(k);
        if ((threadIdx.x & 63) == 0 && k < PM_NO_DISTANCE_BITS) atomicMin(L.key + w.z, k);
    }
}

__global__ void k_pm_decide(PmLaunch L)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= L.Q) return;
    const int m = L.qMap[q], pb = L.planeOff[m], M = L.planeOff[m + 1] - pb, pr = L.qPair[q];
    if (pm_decide(L.params, L.angle + pr, L.key + pr, L.mapBad + pb, M, L.mapOut + q, L.parOut + q, L.verOut + q))
        atomicAdd(L.nmatches + L.qFrame[q], 1);
}

__global__ __launch_bounds__(PM_THREADS) void k_pm_flags(PmLaunch L)
{
    const int q = blockIdx.x;
    if (L.mapOut[q] < 0) return;
    const int m = L.qMap[q], p0 = L.pointOff[m], n = L.pointOff[m + 1] - p0;
    const int lo = blockIdx.y * PM_FLAG_POINTS;
    if (lo >= n) return;
    const int hi = min(lo + PM_FLAG_POINTS, n);
    float pM[4];
    pm_world_coef(L.Tcw + 16 * (size_t)L.qFrame[q], L.coefs + 4 * (size_t)q, pM);
    int cnt = 0;
    for (int p = lo + (int)threadIdx.x; p < hi; p += PM_THREADS) {
        const float* xyz = L.points + 3 * (size_t)(p0 + p);
        if (pm_flag_point(pM, xyz[0], xyz[1], xyz[2])) {
            L.flags[p0 + p] = 1;
            cnt++;
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(L.npairs + L.qFrame[q], cnt);
}

hipError_t drfe_launch_plane_match(const PmLaunch& L, hipStream_t s)
{
    if (L.Q <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pm_gate, dim3(L.Q), dim3(PM_THREADS), 0, s, L);
    if (L.workCap > 0)
        hipLaunchKernelGGL(k_pm_dist, dim3(min(L.workCap, PM_DIST_GRID)), dim3(PM_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_pm_decide, dim3((L.Q + 63) / 64), dim3(64), 0, s, L);
    if (L.flagPoints && L.maxPts > 0)
        hipLaunchKernelGGL(k_pm_flags, dim3(L.Q, (L.maxPts + PM_FLAG_POINTS - 1) / PM_FLAG_POINTS), dim3(PM_THREADS), 0, s, L);
    return hipGetLastError();
}
