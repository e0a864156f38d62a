/* recent_kernels.hip — LocalMapping::MapPointCulling and MapLineCulling on the device.  A chunk is a run of
 * the flat entry space (the point list, then the line list), a lane per entry:
 *
 *   k_recent_claim    the verdict of every entry from the state the chunk found (recent_core.h); an entry that culls lowers its
 *                     item's claim word to its list position, so that the first occurrence of a handle carries the verdict.
 *   k_recent_verdict  the action of every entry (a later occurrence of a culled item is "was bad"), the observations its verdict
 *                     erases, and per workgroup the totals: kept points, kept lines, culled items, erased observations.
 *   k_recent_scan     one workgroup: the exclusive prefix of those totals over the chunk's workgroups, on top of what the chunks
 *                     before left in the head words.
 *   k_recent_pack     the surviving lists, the culled entries and the offsets of their erased observations, all in list order
 *                     (rank by ballot inside a wave, scan over the workgroup); the bad flag of every culled item into the
 *                     resident image.
 *   k_recent_erase    the erased observations of all culled items as one flat index space over a grid: a search in the offsets
 *                     per lane, then the store of -1 into the resident match row and the record (key frame, index).  Equal
 *                     stores are the only shared writes.
 *
 * A later chunk finds the bad flags the earlier ones stored, which is what the reference's walk finds there. */
#include "lmap_device.h"

namespace {

__device__ inline int entry_verdict(const RecentLaunch& L, int kind, int32_t s)
{
    if (kind == RECENT_POINT ? L.I.mpBad[s] : L.I.mlBad[s]) return RECENT_WAS_BAD;
    const int32_t nObs = kind == RECENT_POINT ? L.A.nObs[s] : L.R.mlNObs[s];
    return recent_verdict(kind, L.R.found[kind][s], L.R.visible[kind][s], L.R.first[kind][s], nObs, L.current, L.monocular);
}

__global__ __launch_bounds__(RECENT_TILE) void k_recent_claim(RecentLaunch L)
{
    const int e = L.e0 + blockIdx.x * RECENT_TILE + threadIdx.x;
    if (e >= L.e1) return;
    const int kind = e < L.nPts ? RECENT_POINT : RECENT_LINE;
    const int32_t s = L.item[e];
    if (recent_culls(entry_verdict(L, kind, s))) atomicMin(&L.claim[kind][s], e);
}

__global__ __launch_bounds__(RECENT_TILE) void k_recent_verdict(RecentLaunch L)
{
    __shared__ int32_t sErased;
    const int e = L.e0 + blockIdx.x * RECENT_TILE + threadIdx.x;
    const bool valid = e < L.e1;
    if (threadIdx.x == 0) sErased = 0;
    int action = -1, kind = RECENT_POINT;
    int32_t cnt = 0;
    if (valid) {
        kind = e < L.nPts ? RECENT_POINT : RECENT_LINE;
        const int32_t s = L.item[e];
        action = entry_verdict(L, kind, s);
        if (recent_culls(action)) {
            if (L.claim[kind][s] != e) action = RECENT_WAS_BAD;        /* culled by an earlier entry of the list */
            else cnt = kind == RECENT_POINT ? L.I.obsOff[s + 1] - L.I.obsOff[s] : L.R.mlObsOff[s + 1] - L.R.mlObsOff[s];
        }
        L.action[e] = (uint8_t)action;
        L.cnt[e - L.e0] = cnt;
    }
    const int keptP = __syncthreads_count(action == RECENT_KEPT && kind == RECENT_POINT);
    const int keptL = __syncthreads_count(action == RECENT_KEPT && kind == RECENT_LINE);
    const int culled = __syncthreads_count(recent_culls(action));
    if (cnt) atomicAdd(&sErased, cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        RecentGroup G;
        G.v[RECENT_HEAD_KEPT_P] = keptP;
        G.v[RECENT_HEAD_KEPT_L] = keptL;
        G.v[RECENT_HEAD_CULLED] = culled;
        G.v[RECENT_HEAD_ERASED] = sErased;
        L.group[blockIdx.x] = G;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_recent_scan(RecentLaunch L, int groups)
{
    __shared__ int32_t sh[LMAP_THREADS];
    int32_t carry[RECENT_HEAD_BASE];
    for (int i = 0; i < RECENT_HEAD_BASE; i++) carry[i] = L.head[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < RECENT_HEAD_BASE; i++) L.head[RECENT_HEAD_BASE + i] = carry[i];
    for (int base = 0; base < groups; base += LMAP_THREADS) {
        const int g = base + threadIdx.x;
        RecentGroup G = {};
        if (g < groups) G = L.group[g];
        for (int i = 0; i < RECENT_HEAD_BASE; i++) {
            int32_t total;
            const int32_t before = block_excl_scan(G.v[i], sh, &total);
            G.v[i] = carry[i] + before;
            carry[i] += total;
        }
        if (g < groups) L.group[g] = G;
    }
    if (threadIdx.x == 0)
        for (int i = 0; i < RECENT_HEAD_BASE; i++) L.head[i] = carry[i];
}

__global__ __launch_bounds__(RECENT_TILE) void k_recent_pack(RecentLaunch L)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    __shared__ int32_t sh[LMAP_THREADS];
    const int e = L.e0 + blockIdx.x * RECENT_TILE + threadIdx.x;
    const bool valid = e < L.e1;
    const RecentGroup G = L.group[blockIdx.x];
    const int action = valid ? (int)L.action[e] : -1;
    const int kind = e < L.nPts ? RECENT_POINT : RECENT_LINE;
    const int32_t cnt = valid ? L.cnt[e - L.e0] : 0;
    int total;
    unsigned long long ballot;
    for (int k = 0; k < 2; k++) {
        const bool kept = action == RECENT_KEPT && kind == k;
        const int r = block_rank(kept, shWave, &total, &ballot);
        if (kept) L.kept[k][G.v[RECENT_HEAD_KEPT_P + k] + r] = L.handle[e];
    }
    const bool culls = recent_culls(action);
    const int r = block_rank(culls, shWave, &total, &ballot);
    int32_t erased;
    const int32_t before = block_excl_scan(cnt, sh, &erased);
    if (culls) {
        const int32_t s = L.item[e];
        L.culledEntry[G.v[RECENT_HEAD_CULLED] + r] = e;
        L.erOff[G.v[RECENT_HEAD_CULLED] + r] = G.v[RECENT_HEAD_ERASED] + before;
        const_cast<uint8_t*>(kind == RECENT_POINT ? L.I.mpBad : L.I.mlBad)[s] = 1;
    }
}

__global__ __launch_bounds__(RECENT_ERASE_TILE) void k_recent_erase(RecentLaunch L)
{
    const int32_t t1 = L.head[RECENT_HEAD_ERASED], c0 = L.head[RECENT_HEAD_BASE + RECENT_HEAD_CULLED], c1 = L.head[RECENT_HEAD_CULLED];
    const int64_t stride = (int64_t)gridDim.x * RECENT_ERASE_TILE;
    for (int64_t t = (int64_t)L.head[RECENT_HEAD_BASE + RECENT_HEAD_ERASED] + blockIdx.x * RECENT_ERASE_TILE + threadIdx.x; t < t1; t += stride) {
        /* the last culled item of the chunk whose offset is not above t: the one with an observation there */
        int32_t lo = c0, hi = c1;
        while (hi - lo > 1) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (L.erOff[mid] <= t) lo = mid;
            else hi = mid;
        }
        const int32_t e = L.culledEntry[lo], s = L.item[e], k = (int32_t)t - L.erOff[lo];
        int32_t kf, idx;
        if (e < L.nPts) {
            const int32_t o = L.I.obsOff[s] + k;
            kf = L.I.obs[o];
            idx = L.A.obsIdx[o];
            const_cast<int32_t*>(L.I.kfMp)[L.I.kfMpOff[kf] + idx] = -1;
        } else {
            const int32_t o = L.R.mlObsOff[s] + k;
            kf = L.R.mlObs[o];
            idx = L.R.mlObsIdx[o];
            const_cast<int32_t*>(L.I.kfMl)[L.I.kfMlOff[kf] + idx] = -1;
        }
        L.erKf[t] = kf;
        L.erIdx[t] = idx;
    }
}

}  // namespace

hipError_t drfe_launch_recent_chunk(const RecentLaunch& L, int64_t eraseBound, hipStream_t s)
{
    const int n = L.e1 - L.e0;
    if (n <= 0) return hipSuccess;
    const int groups = (n + RECENT_TILE - 1) / RECENT_TILE;
    hipLaunchKernelGGL(k_recent_claim, dim3(groups), dim3(RECENT_TILE), 0, s, L);
    hipLaunchKernelGGL(k_recent_verdict, dim3(groups), dim3(RECENT_TILE), 0, s, L);
    hipLaunchKernelGGL(k_recent_scan, dim3(1), dim3(LMAP_THREADS), 0, s, L, groups);
    hipLaunchKernelGGL(k_recent_pack, dim3(groups), dim3(RECENT_TILE), 0, s, L);
    if (eraseBound > 0) {
        const int64_t want = (eraseBound + RECENT_ERASE_TILE - 1) / RECENT_ERASE_TILE;
        hipLaunchKernelGGL(k_recent_erase, dim3((unsigned)(want < RECENT_ERASE_GROUPS ? want : RECENT_ERASE_GROUPS)), dim3(RECENT_ERASE_TILE), 0, s, L);
    }
    return hipGetLastError();
}
