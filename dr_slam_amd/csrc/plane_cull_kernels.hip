/* plane_cull_kernels.hip — the distance half of LocalMapping::MapPlaneCulling (reference src/LocalMapping.cc:239-263 with
 * Map::PointDistanceFromPlane, src/Map.cc:433-448) over one device-resident map, on gfx950.
 *
 *   k_pc_pairs  one lane per pair i < j: the angle, the key reset to PM_NO_DISTANCE_BITS, and where both planes are alive,
 *               the gate passes and plane j's cloud is not empty, row i is appended to column j's list through an integer
 *               atomic counter (the list order does not matter: every pair has its own key);
 *   k_pc_dist   one workgroup per (column j, PC_CHUNK points of its cloud, tile of gated rows): each lane keeps its
 *               PC_POINTS_PER_LANE points in registers, the tile's row coefficients are staged once in LDS (wave-uniform
 *               reads), and per row a wavefront min then one atomicMin per wavefront goes into the pair's key.  A cloud point
 *               is loaded once per row tile, not once per pair.  A minimum of floats is order-free, so the result equals the
 *               reference's sequential scan bit for bit (plane_match_kernels.hip).
 * The walk over the rows, the merges and the rebuilds stay on the host (plane_cull.cpp); a column whose cloud was rebuilt is
 * recomputed with k_pc_dist alone.  Plain vector stores and integer atomics only.  All arithmetic is plane_cull_core.h,
 * shared with the host entry; -ffp-contract=off. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "plane_map_internal.h"
#include "plane_cull_core.h"

__global__ __launch_bounds__(PC_THREADS) void k_pc_pairs(PcLaunch L)
{
    const int j = blockIdx.y, i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (j >= L.P || i >= j) return;
    const int gi = L.pb + i, gj = L.pb + j, at = pc_pair_index(i, j);
    const float a = pm_angle(L.mapCoefs + 4 * (size_t)gi, L.mapCoefs + 4 * (size_t)gj);
    L.angle[at] = a;
    L.key[at] = PM_NO_DISTANCE_BITS;
    if (L.mapBad[gi] || L.mapBad[gj] || !pc_gate(a, L.aTh) || L.cloudEnd[gj] <= L.cloudBeg[gj]) return;
    const int slot = atomicAdd(L.rowCount + j, 1);          /* at most j rows: the list is column j's slice of the triangle */
    L.rowList[pc_pair_index(0, j) + slot] = i;
}

__global__ __launch_bounds__(PC_THREADS) void k_pc_dist(PcLaunch L, int col0)
{
    __shared__ float sCoef[PC_ROW_TILE][4];
    __shared__ int sRow[PC_ROW_TILE];
    const int j = col0 + blockIdx.y;
    if (j >= L.P) return;
    const int nrows = min(L.rowCount[j], j), r0 = blockIdx.z * L.tile;
    if (r0 >= nrows) return;
    const int gj = L.pb + j;
    const int lo = L.cloudBeg[gj] + blockIdx.x * PC_CHUNK, hi = min(lo + PC_CHUNK, L.cloudEnd[gj]);
    if (lo >= hi) return;
    const int nt = min(L.tile, nrows - r0);
    if ((int)threadIdx.x < nt) {
        const int i = L.rowList[pc_pair_index(0, j) + r0 + threadIdx.x];
        sRow[threadIdx.x] = i;
        for (int k = 0; k < 4; k++) sCoef[threadIdx.x][k] = L.mapCoefs[4 * (size_t)(L.pb + i) + k];
    }
    __syncthreads();
    float x[PC_POINTS_PER_LANE], y[PC_POINTS_PER_LANE], z[PC_POINTS_PER_LANE];
    int np = 0;
#pragma unroll
    for (int k = 0; k < PC_POINTS_PER_LANE; k++) {
        const int p = lo + k * PC_THREADS + (int)threadIdx.x;
        if (p < hi) {
            const float* xyz = L.cloud + 3 * (size_t)p;
            x[k] = xyz[0]; y[k] = xyz[1]; z[k] = xyz[2];
            np = k + 1;
        }
    }
    for (int r = 0; r < nt; r++) {
        uint32_t key = PM_NO_DISTANCE_BITS;
#pragma unroll
        for (int k = 0; k < PC_POINTS_PER_LANE; k++)
            if (k < np) key = min(key, pc_point_key(sCoef[r], x[k], y[k], z[k]));
        key = drfe_wave_min_u32(key);
        if ((threadIdx.x & 63) == 0 && key < PM_NO_DISTANCE_BITS) atomicMin(L.key + pc_pair_index(sRow[r], j), key);
    }
}

hipError_t drfe_launch_plane_cull_pairs(const PcLaunch& L, hipStream_t s)
{
    if (L.P < 2) return hipSuccess;
    hipLaunchKernelGGL(k_pc_pairs, dim3((L.P + PC_THREADS - 1) / PC_THREADS, L.P), dim3(PC_THREADS), 0, s, L);
    return hipGetLastError();
}

hipError_t drfe_launch_plane_cull_dist(const PcLaunch& L, int col0, int ncols, int maxChunks, int maxRows, hipStream_t s)
{
    if (ncols < 1 || maxChunks < 1 || maxRows < 1) return hipSuccess;
    const int tiles = (maxRows + L.tile - 1) / L.tile;
    hipLaunchKernelGGL(k_pc_dist, dim3(maxChunks, ncols, tiles), dim3(PC_THREADS), 0, s, L, col0);
    return hipGetLastError();
}
