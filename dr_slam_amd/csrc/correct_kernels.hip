/* correct_kernels.hip — LoopClosing::CorrectLoop's Sim3 propagation on the device.
 *
 *   k_correct_pose     a lane per called key frame: CorrectedSim3, NonCorrectedSim3, the inverse, the new pose and its centre
 *                      (corr_keyframe of correct_core.h), by position in rank order.
 *   k_correct_claim    grid (row tile, position): every entry of the called match rows that the walk would move takes its point
 *                      with an atomicMin of its walk rank.
 *   k_correct_count    a workgroup per position: the entries that hold their point's minimum.
 *   k_correct_scan     one workgroup: the exclusive prefix of those counts.
 *   k_correct_move     a workgroup per position of the chunk, a lane per entry of a pass: the two maps in f64, then the walk over
 *                      the point's observations with the centre each observer has at that moment of the reference's loop; the
 *                      records are compacted in walk order.
 *   k_correct_scatter  a lane per record: position and stamps into the image.
 *   k_correct_poses    a lane per called key frame, after the last chunk: pose and centre into the image.
 *
 * The hand-offs are the launches, in stream order.  A minimum has one value, so the order of the atomics cannot show.  A moved
 * point is read and written by its one claiming entry only; the stored poses and centres are read by every chunk and replaced
 * after the last. */
#include "lmap_device.h"

namespace {

__global__ __launch_bounds__(LMAP_THREADS) void k_correct_pose(CorrLaunch L)
{
    const int j = blockIdx.x * LMAP_THREADS + threadIdx.x;
    if (j >= L.n) return;
    float TwcCur[16];
    pose_inverse_kf(L.G.kfTcw + 16 * (size_t)L.called[L.curPos], TwcCur);
    SoSim3 Scw;
    corr_sim3_from8(L.Scw, Scw);
    CorrKf K;
    corr_keyframe(L.G.kfTcw + 16 * (size_t)L.called[j], j == L.curPos, TwcCur, Scw, K);
    L.kf[j] = K;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_correct_claim(CorrLaunch L)
{
    const int j = blockIdx.y, i = blockIdx.x * CORRECT_TILE + threadIdx.x;
    const int32_t kf = L.called[j];
    const int r0 = L.I.kfMpOff[kf], len = L.I.kfMpOff[kf + 1] - r0;
    if (i >= len) return;
    const int32_t p = L.I.kfMp[r0 + i];
    if (corr_entry_moves(p, L.I.mpBad, L.G.mpBy, L.cur)) atomicMin(&L.claim[p], lmap_walk_rank(j, i, L.rowStride));
}

/* an entry moves its point when it made the claim: a null, bad or stamped entry made none, and no rank is LMAP_NO_CLAIM */
__device__ inline bool corr_kept(const CorrLaunch& L, int32_t p, int j, int i)
{
    return p >= 0 && L.claim[p] == lmap_walk_rank(j, i, L.rowStride);
}

__global__ __launch_bounds__(LMAP_THREADS) void k_correct_count(CorrLaunch L)
{
    __shared__ int32_t sCnt;
    const int j = blockIdx.x;
    const int32_t kf = L.called[j];
    const int r0 = L.I.kfMpOff[kf], len = L.I.kfMpOff[kf + 1] - r0;
    if (threadIdx.x == 0) sCnt = 0;
    __syncthreads();
    int32_t c = 0;
    for (int i = threadIdx.x; i < len; i += CORRECT_TILE) c += corr_kept(L, L.I.kfMp[r0 + i], j, i) ? 1 : 0;
    if (c) atomicAdd(&sCnt, c);
    __syncthreads();
    if (threadIdx.x == 0) L.cnt[j] = sCnt;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_correct_scan(CorrLaunch L)
{
    __shared__ int32_t sh[LMAP_THREADS];
    const int tid = threadIdx.x;
    int32_t carry = 0;
    for (int j0 = 0; j0 < L.n; j0 += LMAP_THREADS) {
        const int j = j0 + tid;
        const int32_t v = j < L.n ? L.cnt[j] : 0;
        int32_t tot;
        const int32_t ex = block_excl_scan(v, sh, &tot);
        if (j < L.n) L.off[j] = carry + ex;
        carry += tot;
    }
    if (tid == 0) L.off[L.n] = carry;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_correct_move(CorrLaunch L)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    const int j = L.j0 + blockIdx.x;
    const int32_t kf = L.called[j];
    const int r0 = L.I.kfMpOff[kf], len = L.I.kfMpOff[kf + 1] - r0;
    const CorrKf& K = L.kf[j];
    int32_t at = L.off[j] - L.off[L.j0];
    for (int i0 = 0; i0 < len; i0 += CORRECT_TILE) {
        const int i = i0 + threadIdx.x;
        int32_t p = -1;
        bool keep = false;
        if (i < len) {
            p = L.I.kfMp[r0 + i];
            keep = corr_kept(L, p, j, i);
        }
        float Xn[3], nrm[3], maxD = 0.0f, minD = 0.0f;
        uint8_t status = 0;
        if (keep) {
            corr_point(K.nonCorrected, K.swi, L.G.mpWorld + 3 * (size_t)p, Xn);
            status = corr_normal(L.G, L.I.obsOff, L.I.obs, L.pos, L.kf, p, j, Xn, nrm, &maxD, &minD);
        }
        int tot;
        unsigned long long b;
        const int r = block_rank(keep, shWave, &tot, &b);
        if (keep) {
            const size_t o = (size_t)(at + r);
            L.pkItem[o] = p;
            L.pkBy[o] = j;
            for (int k = 0; k < 3; k++) {
                L.pkWorld[3 * o + k] = Xn[k];
                L.pkNormal[3 * o + k] = nrm[k];
            }
            L.pkMax[o] = maxD;
            L.pkMin[o] = minD;
            L.pkStatus[o] = status;
        }
        at += tot;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_correct_scatter(CorrLaunch L)
{
    const int count = L.off[L.j1] - L.off[L.j0];
    for (int o = blockIdx.x * LMAP_THREADS + threadIdx.x; o < count; o += gridDim.x * LMAP_THREADS) {
        const int32_t p = L.pkItem[o];
        for (int k = 0; k < 3; k++) L.G.mpWorld[3 * (size_t)p + k] = L.pkWorld[3 * (size_t)o + k];
        L.G.mpBy[p] = L.cur;
        L.G.mpByRef[p] = L.calledHandle[L.pkBy[o]];
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_correct_poses(CorrLaunch L)
{
    const int j = blockIdx.x * LMAP_THREADS + threadIdx.x;
    if (j >= L.n) return;
    const size_t s = (size_t)L.called[j];
    for (int k = 0; k < 16; k++) L.G.kfTcw[16 * s + k] = L.kf[j].Tiw[k];
    for (int k = 0; k < 3; k++) L.G.kfOw[3 * s + k] = L.kf[j].Ow[k];
}

int groups(int n) { return (n + LMAP_THREADS - 1) / LMAP_THREADS; }

}  // namespace

hipError_t drfe_launch_correct_plan(const CorrLaunch& L, hipStream_t s)
{
    if (L.n <= 0) return hipSuccess;
    const int tiles = L.maxRow > 0 ? (L.maxRow + CORRECT_TILE - 1) / CORRECT_TILE : 1;
    hipLaunchKernelGGL(k_correct_pose, dim3(groups(L.n)), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_correct_claim, dim3(tiles, L.n), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_correct_count, dim3(L.n), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_correct_scan, dim3(1), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}

hipError_t drfe_launch_correct_chunk(const CorrLaunch& L, hipStream_t s)
{
    if (L.j1 <= L.j0) return hipSuccess;
    hipLaunchKernelGGL(k_correct_move, dim3(L.j1 - L.j0), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_correct_scatter, dim3(256), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}

hipError_t drfe_launch_correct_poses(const CorrLaunch& L, hipStream_t s)
{
    if (L.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_correct_poses, dim3(groups(L.n)), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}
