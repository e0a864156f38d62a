/* create_kernels.hip — map-point and map-line creation on the device.  A chunk is a run of the call's
 * creations of one kind, a lane per creation, CREATE_TILE of them a workgroup; its observations are a flat entry space of two
 * entries per creation, a lane per entry.
 *
 *   k_create_count  a lane per creation takes its kept observers, 1 or 2 (create_observers): their number in front of it inside
 *                   its tile is its thread index plus the rank of its "two" flag (ballot inside the wave, wave totals across the
 *                   workgroup); the tile's total goes to the tile array.
 *   k_create_scan   one workgroup: the exclusive prefix of the tile totals, in place.
 *   k_create_clear  a lane per entry: clears the claim word of the row entry it names and reports what the entry displaces - the
 *                   slot of the creation that named the same row entry last before it in the call (the host's `prev`), else the
 *                   slot the resident row holds, which no launch has written yet.
 *   k_create_claim  atomicMax of the entry's walk rank (+ 1) on that claim word: the later creation holds the row.
 *   k_create_item   a lane per creation: the observers in slot order, the stereo flags and the octave from the resident attribute
 *                   block, the centres and scales from the resident geometry block, UpdateNormalAndDepth (create_point_normal),
 *                   and the new slot of every per-slot section, written into the room the host granted behind the stored slots.
 *   k_create_rows   the claimant of a row entry stores the new slot into the resident match row.
 *
 * The hand-offs are the launches, in stream order.  A maximum does not show the order of its atomics; every other word is written
 * by one lane, or by several with the same value (the cleared claim word).  Nothing a lane reads of the resident blocks is written
 * by the call before the launch that reads it: the rows are read in k_create_clear and written in k_create_rows; the stored
 * slots' sections are only appended to.  Bounds: slot0 + t and obs0 + (observers before) stay inside the granted room, which the
 * host sized from the same counts. */
#include "lmap_device.h"

namespace {

/* the claim word and the row entry an observation entry names */
__device__ inline int32_t row_word(const CreateLaunch& L, int32_t e)
{
    const int32_t* rowOff = L.kind == FUSE_POINT ? L.I.kfMpOff : L.I.kfMlOff;
    return rowOff[L.kf[e]] + L.idx[e];
}

__device__ inline int32_t* row_of(const CreateLaunch& L)
{
    return const_cast<int32_t*>(L.kind == FUSE_POINT ? L.I.kfMp : L.I.kfMl);
}

__global__ __launch_bounds__(CREATE_TILE) void k_create_count(CreateLaunch L)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    const int32_t t = L.t0 + blockIdx.x * CREATE_TILE + threadIdx.x;
    const bool in = t < L.t1;
    const bool two = in && L.cnt[t] == 2 && L.kf[2 * t + 1] != L.kf[2 * t];
    int total;
    unsigned long long ballot;
    const int twosBefore = block_rank(two, shWave, &total, &ballot);
    if (in) L.local[t - L.t0] = (int32_t)threadIdx.x + twosBefore;
    if (threadIdx.x == 0) {
        const int32_t left = L.t1 - (L.t0 + (int32_t)blockIdx.x * CREATE_TILE);
        L.tile[blockIdx.x] = (left < CREATE_TILE ? left : CREATE_TILE) + total;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_create_scan(CreateLaunch L, int tiles)
{
    __shared__ int32_t sh[LMAP_THREADS];
    int32_t carry = 0;
    for (int base = 0; base < tiles; base += LMAP_THREADS) {
        const int g = base + threadIdx.x;
        const int32_t v = g < tiles ? L.tile[g] : 0;
        int32_t total;
        const int32_t before = block_excl_scan(v, sh, &total);
        if (g < tiles) L.tile[g] = carry + before;
        carry += total;
    }
}

__global__ __launch_bounds__(CREATE_TILE) void k_create_clear(CreateLaunch L)
{
    const int32_t e = 2 * L.t0 + blockIdx.x * CREATE_TILE + threadIdx.x;
    if (e >= 2 * L.t1) return;
    if ((e & 1) >= L.cnt[e >> 1]) {
        L.displaced[e] = -1;
        return;
    }
    const int32_t w = row_word(L, e);
    L.claim[w] = 0;
    L.displaced[e] = L.prev[e] >= 0 ? L.slot0 + L.prev[e] : row_of(L)[w];
}

__global__ __launch_bounds__(CREATE_TILE) void k_create_claim(CreateLaunch L)
{
    const int32_t e = 2 * L.t0 + blockIdx.x * CREATE_TILE + threadIdx.x;
    if (e >= 2 * L.t1 || (e & 1) >= L.cnt[e >> 1]) return;
    atomicMax(L.claim + row_word(L, e), e + 1);
}

__global__ __launch_bounds__(CREATE_TILE) void k_create_item(CreateLaunch L)
{
    const int32_t t = L.t0 + blockIdx.x * CREATE_TILE + threadIdx.x;
    if (t >= L.t1) return;
    int32_t oKf[2], oIdx[2];
    const int32_t m = create_observers(L.cnt[t], L.kf + 2 * t, L.idx + 2 * t, oKf, oIdx);
    const int32_t off = L.obs0 + L.tile[blockIdx.x] + L.local[t - L.t0];
    const size_t s = (size_t)(L.slot0 + t);
    if (L.kind == FUSE_LINE) {
        const_cast<uint8_t*>(L.I.mlBad)[s] = 0;
        const_cast<int32_t*>(L.R.found[1])[s] = 1;
        const_cast<int32_t*>(L.R.visible[1])[s] = 1;
        const_cast<int64_t*>(L.R.first[1])[s] = L.first[t];
        const_cast<int32_t*>(L.R.mlNObs)[s] = m;
        for (int32_t o = 0; o < m; o++) {
            const_cast<int32_t*>(L.R.mlObs)[off + o] = oKf[o];
            const_cast<int32_t*>(L.R.mlObsIdx)[off + o] = oIdx[o];
        }
        const_cast<int32_t*>(L.R.mlObsOff)[s + 1] = off + m;
        return;
    }
    int32_t nObs = 0;
    for (int32_t o = 0; o < m; o++) nObs += fuse_obs_weight(FUSE_POINT, L.A.stereo[L.I.kfMpOff[oKf[o]] + oIdx[o]]);
    const int32_t ref = L.ref[t];
    const int32_t level = L.A.octave[L.I.kfMpOff[ref] + create_ref_index(m, oKf, oIdx, ref)];
    const_cast<uint8_t*>(L.I.mpBad)[s] = 0;
    for (int32_t o = 0; o < m; o++) {
        const_cast<int32_t*>(L.I.obs)[off + o] = oKf[o];
        const_cast<int32_t*>(L.A.obsIdx)[off + o] = oIdx[o];
    }
    const_cast<int32_t*>(L.I.obsOff)[s + 1] = off + m;
    const_cast<int32_t*>(L.A.nObs)[s] = nObs;
    const_cast<int32_t*>(L.R.found[0])[s] = 1;
    const_cast<int32_t*>(L.R.visible[0])[s] = 1;
    const_cast<int64_t*>(L.R.first[0])[s] = L.first[t];
    const float X[3] = {L.world[3 * (size_t)t], L.world[3 * (size_t)t + 1], L.world[3 * (size_t)t + 2]};
    if (L.geo) {
        for (int k = 0; k < 3; k++) const_cast<float*>(L.G.mpWorld)[3 * s + k] = X[k];
        const_cast<int32_t*>(L.G.mpRef)[s] = ref;
        const_cast<int32_t*>(L.G.mpLevel)[s] = level;
        const_cast<int32_t*>(L.G.mpBy)[s] = 0;
        const_cast<int32_t*>(L.G.mpByRef)[s] = 0;
    }
    if (L.normals) {
        float nrm[3], maxD, minD;
        const uint8_t status = create_point_normal(L.G.kfOw, L.G.scale, L.G.nLevels, X, m, oKf, ref, level, nrm, &maxD, &minD);
        for (int k = 0; k < 3; k++) L.nrm[3 * (size_t)t + k] = nrm[k];
        L.maxD[t] = maxD;
        L.minD[t] = minD;
        L.status[t] = status;
    }
}

__global__ __launch_bounds__(CREATE_TILE) void k_create_rows(CreateLaunch L)
{
    const int32_t e = 2 * L.t0 + blockIdx.x * CREATE_TILE + threadIdx.x;
    if (e >= 2 * L.t1 || (e & 1) >= L.cnt[e >> 1]) return;
    const int32_t w = row_word(L, e);
    if (L.claim[w] == e + 1) row_of(L)[w] = L.slot0 + (e >> 1);
}

}  // namespace

hipError_t drfe_launch_create_chunk(const CreateLaunch& L, hipStream_t s)
{
    const int32_t n = L.t1 - L.t0;
    if (n <= 0) return hipSuccess;
    const int tiles = (n + CREATE_TILE - 1) / CREATE_TILE, entryTiles = (2 * n + CREATE_TILE - 1) / CREATE_TILE;
    hipLaunchKernelGGL(k_create_count, dim3(tiles), dim3(CREATE_TILE), 0, s, L);
    hipLaunchKernelGGL(k_create_scan, dim3(1), dim3(LMAP_THREADS), 0, s, L, tiles);
    hipLaunchKernelGGL(k_create_clear, dim3(entryTiles), dim3(CREATE_TILE), 0, s, L);
    hipLaunchKernelGGL(k_create_claim, dim3(entryTiles), dim3(CREATE_TILE), 0, s, L);
    hipLaunchKernelGGL(k_create_item, dim3(tiles), dim3(CREATE_TILE), 0, s, L);
    hipLaunchKernelGGL(k_create_rows, dim3(entryTiles), dim3(CREATE_TILE), 0, s, L);
    return hipGetLastError();
}
