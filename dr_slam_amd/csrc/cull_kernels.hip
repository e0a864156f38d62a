/* cull_kernels.hip — LocalMapping::KeyFrameCulling on the device.
 *
 *   k_cull_record  grid (row tile, position of the chunk): every key frame of the chunk side by side against the working state as
 *                  the chunk finds it.  Per entry the record of cull_core.h (the depth test and, over the observers of its point
 *                  that are not called, how many there are and how many count) and what the entry counts for right now
 *                  (cull_replay); per key frame the sums of that: nMPs, nRedundant and the observers walked.
 *   k_cull_walk    one workgroup walks the chunk's key frames in call order.  Until the first key frame of the chunk is culled
 *                  the sums stand as they are and a key frame costs one load.  After that, the lanes look over the row for an
 *                  entry that was nulled or whose point lost an observation since the records (cull_entry_changed); only then
 *                  the row is counted again, cull_replay against the working state, the counts meeting in LDS.  Every lane takes
 *                  the same verdict.  A culled key frame's row is erased by the same lanes, a point at most once (an exchange on
 *                  its claim word), which is all that a later key frame of the call reads.
 *
 * The working state (match rows, bad flags, counters, live flags) is scratch that the host copies from the resident image before
 * the first chunk; it lives across the chunks of a call.  The hand-off between two key frames is __syncthreads(): one workgroup,
 * so a workgroup-scope fence orders the plain stores of one key frame's erasure before the loads of the next. */
#include "lmap_device.h"

namespace {

__global__ __launch_bounds__(CULL_TILE) void k_cull_record(CullLaunch L)
{
    __shared__ int32_t sMPs, sRedundant, sWalked;
    const int j = L.j0 + blockIdx.y, i = blockIdx.x * CULL_TILE + threadIdx.x;
    const int32_t k = L.called[j];
    const int len = L.S.kfMpOff[k + 1] - L.S.kfMpOff[k];
    if ((int)(blockIdx.x * CULL_TILE) >= len || (L.S.kfFlags[k] & CULL_KF_ORIGIN)) return;    /* the same for the whole workgroup */
    if (threadIdx.x == 0) sMPs = sRedundant = sWalked = 0;
    __syncthreads();
    if (i < len) {
        const CullRecord R = cull_record(L.S, L.pos, k, i, L.monocular);
        L.rec[L.recOff[j] - L.recOff[L.j0] + i] = R;
        int32_t walked = 0;
        const int v = cull_replay(L.S, L.pos, R, k, i, &walked);
        if (v > 0) atomicAdd(&sMPs, 1);
        if (v > 1) atomicAdd(&sRedundant, 1);
        if (walked) atomicAdd(&sWalked, walked);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sMPs) atomicAdd(&L.spec[j].nMPs, sMPs);
        if (sRedundant) atomicAdd(&L.spec[j].nRedundant, sRedundant);
        if (sWalked) atomicAdd(&L.spec[j].walked, (unsigned long long)sWalked);
    }
}

__global__ __launch_bounds__(CULL_WALK_THREADS) void k_cull_walk(CullLaunch L)
{
    __shared__ int32_t sMPs, sRedundant, sDied;
    __shared__ unsigned long long sWalked;
    const int tid = threadIdx.x;
    bool culledSince = false;                  /* since the chunk's records; the same for every lane */
    for (int j = L.j0; j < L.j1; j++) {
        const int32_t k = L.called[j];
        const uint8_t flags = L.S.kfFlags[k];
        int32_t* out = L.out + (size_t)CULL_OUT_WORDS * j;
        if (flags & CULL_KF_ORIGIN) {          /* the same for every lane */
            if (tid == 0) {
                out[0] = out[1] = out[3] = out[4] = out[5] = 0;
                out[2] = CULL_ORIGIN;
            }
            continue;
        }
        const int r0 = L.S.kfMpOff[k], len = L.S.kfMpOff[k + 1] - r0;
        const CullRecord* rec = L.rec + (L.recOff[j] - L.recOff[L.j0]);
        int again = 0;
        if (culledSince) {
            int changed = 0;
            for (int i = tid; i < len; i += CULL_WALK_THREADS) changed |= cull_entry_changed(L.S, L.touched, rec[i], k, i) ? 1 : 0;
            again = __syncthreads_or(changed);
        }
        int32_t nMPs, nRedundant, nDied = 0;
        unsigned long long nWalked;
        if (!again) {
            nMPs = L.spec[j].nMPs;
            nRedundant = L.spec[j].nRedundant;
            nWalked = L.spec[j].walked;
        } else {
            if (tid == 0) {
                sMPs = sRedundant = 0;
                sWalked = 0ull;
            }
            __syncthreads();
            int32_t m = 0, r = 0, walked = 0;
            for (int i = tid; i < len; i += CULL_WALK_THREADS) {
                const int v = cull_replay(L.S, L.pos, rec[i], k, i, &walked);
                m += v > 0;
                r += v > 1;
            }
            if (m) atomicAdd(&sMPs, m);
            if (r) atomicAdd(&sRedundant, r);
            if (walked) atomicAdd(&sWalked, (unsigned long long)walked);
            __syncthreads();
            nMPs = sMPs;
            nRedundant = sRedundant;
            nWalked = sWalked;
        }
        const int action = cull_action(cull_verdict(nRedundant, nMPs), flags);
        if (action == CULL_CULLED) {           /* the same for every lane */
            if (tid == 0) sDied = 0;
            __syncthreads();
            int32_t died = 0;
            for (int i = tid; i < len; i += CULL_WALK_THREADS) {
                const int32_t q = L.S.row[r0 + i];
                if (q < 0) continue;
                if (atomicExch(&L.claim[q], j) == j) continue;     /* a second entry of the row with the same point */
                int32_t front;
                const int res = cull_erase(L.S, k, q, &front);
                if (res) L.touched[q] = 1;
                died += res == 3;
            }
            if (died) atomicAdd(&sDied, died);
            __syncthreads();
            nDied = sDied;
            culledSince = true;
        }
        if (tid == 0) {
            out[0] = nMPs;
            out[1] = nRedundant;
            out[2] = action;
            out[3] = nDied;
            out[4] = (int32_t)(nWalked & 0xffffffffull);
            out[5] = (int32_t)(nWalked >> 32);
        }
        if (again || action == CULL_CULLED) __syncthreads();       /* the LDS words are set again by the next key frame */
    }
}

}  // namespace

hipError_t drfe_launch_cull_chunk(const CullLaunch& L, hipStream_t s)
{
    if (L.j1 <= L.j0) return hipSuccess;
    if (L.maxRow > 0) {
        const int tiles = (L.maxRow + CULL_TILE - 1) / CULL_TILE;
        hipLaunchKernelGGL(k_cull_record, dim3(tiles, L.j1 - L.j0), dim3(CULL_TILE), 0, s, L);
    }
    hipLaunchKernelGGL(k_cull_walk, dim3(1), dim3(CULL_WALK_THREADS), 0, s, L);
    return hipGetLastError();
}
