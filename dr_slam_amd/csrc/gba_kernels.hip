/* gba_kernels.hip — the map update of LoopClosing::RunGlobalBundleAdjustment on the device.
 *
 *   k_gba_compose   one workgroup, round after round over the unstamped depth: a lane per key frame of the round composes its
 *                   mTcwGBA from its parent's finished one, its parent's stored pose and its own (gba_compose of gba_core.h).  The
 *                   stored poses are only read; a barrier ends each round.  A round wider than the workgroup is strided over.
 *                   It takes the stamp.
 *   k_gba_commit    a lane per visited key frame, in the host's FIFO list: mTcwBefGBA = the stored pose, the pose and its centre =
 *                   mTcwGBA, into the two resident blocks, and the record of the key frame.
 *   k_gba_move      a lane per point slot of the chunk: the point rule (gba_point), the position in place, the kind byte, and the
 *                   moved points of the workgroup.
 *   k_gba_scan      one workgroup: the exclusive prefix of those counts.
 *   k_gba_pack      a lane per point slot again: the rank of its kind byte among the workgroup's (ballot, prefix), its record at
 *                   the workgroup's offset: ascending slot.
 *
 * The hand-offs are the launches, in stream order, and the barrier between rounds.  Every visited key frame is in the list once
 * and every point is its own lane's, so no two lanes write one item. */
#include "lmap_device.h"

namespace {

__global__ __launch_bounds__(LMAP_THREADS) void k_gba_compose(GbaLaunch L)
{
    for (int d = 0; d < L.nRounds; d++) {
        const int i1 = L.roundOff[d + 1];
        for (int i = L.roundOff[d] + threadIdx.x; i < i1; i += LMAP_THREADS) {
            const size_t s = (size_t)L.roundKf[i], pa = (size_t)L.roundParent[i];
            float T[16];
            gba_compose(L.G.kfTcw + 16 * s, L.G.kfTcw + 16 * pa, L.B.kfTcwGBA + 16 * pa, T);
            for (int k = 0; k < 16; k++) L.B.kfTcwGBA[16 * s + k] = T[k];
            L.B.kfStamp[s] = L.loop;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_gba_commit(GbaLaunch L)
{
    const int v = blockIdx.x * LMAP_THREADS + threadIdx.x;
    if (v >= L.nV) return;
    const size_t s = (size_t)L.list[v];
    float T[16], Ow[3];
    for (int k = 0; k < 16; k++) {
        const float old = L.G.kfTcw[16 * s + k];
        T[k] = L.B.kfTcwGBA[16 * s + k];
        L.B.kfBef[16 * s + k] = old;
        L.outBef[16 * (size_t)v + k] = old;
        L.outPose[16 * (size_t)v + k] = T[k];
        L.G.kfTcw[16 * s + k] = T[k];
    }
    camera_centre_kf(T, Ow);
    for (int k = 0; k < 3; k++) L.G.kfOw[3 * s + k] = Ow[k];
    L.B.kfHasBef[s] = 1;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_gba_move(GbaLaunch L)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    const int q = blockIdx.x * GBA_TILE + threadIdx.x, n = L.p1 - L.p0;
    int kind = GBA_POINT_STAYS;
    if (q < n) {
        const size_t p = (size_t)(L.p0 + q);
        const int32_t stamp = L.B.mpStamp[p];
        uint8_t bad = L.I.mpBad[p];
        int32_t r = -1, refStamp = 0;
        if (!bad && stamp != L.loop) {
            r = L.G.mpRef[p];
            /* a point without a reference slot stays: the host has refused the call where the reference would have read it */
            if (r >= 0) refStamp = L.B.kfStamp[r];
            else bad = 1;
        }
        float X[3], Xn[3];
        for (int k = 0; k < 3; k++) X[k] = L.G.mpWorld[3 * p + k];
        const size_t rr = r >= 0 ? (size_t)r : 0;
        kind = gba_point(bad, stamp, refStamp, L.loop, L.B.mpPosGBA + 3 * p, X, L.B.kfBef + 16 * rr, L.G.kfTcw + 16 * rr, Xn);
        if (kind != GBA_POINT_STAYS)
            for (int k = 0; k < 3; k++) L.G.mpWorld[3 * p + k] = Xn[k];
        L.kind[q] = (uint8_t)kind;
    }
    int tot;
    unsigned long long b;
    block_rank(kind != GBA_POINT_STAYS, shWave, &tot, &b);
    if (threadIdx.x == 0) L.groupCnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_gba_scan(GbaLaunch L, int nGroups)
{
    __shared__ int32_t sh[LMAP_THREADS];
    const int tid = threadIdx.x;
    int32_t carry = 0;
    for (int j0 = 0; j0 < nGroups; j0 += LMAP_THREADS) {
        const int j = j0 + tid;
        const int32_t v = j < nGroups ? L.groupCnt[j] : 0;
        int32_t tot;
        const int32_t ex = block_excl_scan(v, sh, &tot);
        if (j < nGroups) L.groupCnt[j] = carry + ex;
        carry += tot;
    }
    if (tid == 0) L.groupCnt[nGroups] = carry;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_gba_pack(GbaLaunch L)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    const int q = blockIdx.x * GBA_TILE + threadIdx.x, n = L.p1 - L.p0;
    const uint8_t kind = q < n ? L.kind[q] : (uint8_t)GBA_POINT_STAYS;
    int tot;
    unsigned long long b;
    const int r = block_rank(kind != GBA_POINT_STAYS, shWave, &tot, &b);
    if (kind == GBA_POINT_STAYS) return;
    const size_t o = (size_t)(L.groupCnt[blockIdx.x] + r), p = (size_t)(L.p0 + q);
    if (o >= (size_t)L.pkCap) return;          /* the host counted fewer: it compares the totals and refuses */
    L.pkItem[o] = (int32_t)p;
    for (int k = 0; k < 3; k++) L.pkWorld[3 * o + k] = L.G.mpWorld[3 * p + k];
    L.pkKind[o] = kind;
}

int groups(int n) { return (n + LMAP_THREADS - 1) / LMAP_THREADS; }

}  // namespace

hipError_t drfe_launch_gba_keyframes(const GbaLaunch& L, hipStream_t s)
{
    if (L.nV <= 0) return hipSuccess;
    if (L.nRounds > 0) hipLaunchKernelGGL(k_gba_compose, dim3(1), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_gba_commit, dim3(groups(L.nV)), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}

hipError_t drfe_launch_gba_points(const GbaLaunch& L, hipStream_t s)
{
    const int n = L.p1 - L.p0;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gba_move, dim3(groups(n)), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_gba_scan, dim3(1), dim3(LMAP_THREADS), 0, s, L, groups(n));
    hipLaunchKernelGGL(k_gba_pack, dim3(groups(n)), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}
