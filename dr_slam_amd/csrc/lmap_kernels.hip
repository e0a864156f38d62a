/* lmap_kernels.hip — Tracking::UpdateLocalMap of every frame of a call on the device.
 *
 *   k_lmap_vote     a workgroup per query.  Lanes stride over the frame's points; each adds 1 per observation into the query's
 *                   histogram over key-frame slots (LDS up to LMAP_LDS_KFS stored key frames, else a zeroed row of global scratch;
 *                   integer atomic adds only).  Bad points are compacted into the nulled list in keypoint order, the others are
 *                   flagged in the in-frame row.  The listed slots (a vote and not bad) are compacted in slot order = rank order,
 *                   their ballots are the mark words, pKFmax is a reduction on (votes, lowest slot).  One lane then runs the
 *                   expansion loop of lmap_core.h, which is sequential by definition and at most 81 iterations long.
 *   k_lmap_claim    grid (rows, query, points | lines): every entry of the local key frames' match rows takes its item with an
 *                   atomicMin of its walk rank.
 *   k_lmap_count    same grid: the kept entries of each local key frame (those that hold their item's minimum).
 *   k_lmap_scan     per (query, kind): exclusive prefix of those counts over the local list; the query's totals.
 *   k_lmap_offsets  one workgroup: the four CSR offset arrays of the call.
 *   k_lmap_write    same grid as the claim: order-preserving compaction of the kept entries into the packed lists, with the
 *                   in-frame flag of each.
 *   k_lmap_pack     per query: the local key frames and the nulled indices into their packed lists.
 *
 * The hand-offs are the launches, in stream order; no workgroup waits on another.  Which atomic arrives first cannot show: adds
 * commute and a minimum has one value. */
#include "lmap_device.h"

namespace {

template <bool LDS>
__global__ __launch_bounds__(LMAP_THREADS) void k_lmap_vote(LmapLaunch L)
{
    __shared__ int32_t sHist[LDS ? LMAP_LDS_KFS : 1];
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    __shared__ int32_t sVotes[LMAP_THREADS], sSlot[LMAP_THREADS];
    __shared__ int32_t sCounter;
    const int q = blockIdx.x, tid = threadIdx.x, nK = L.I.nK;
    const size_t histBase = (size_t)q * (size_t)nK;
    if (LDS)
        for (int s = tid; s < nK; s += LMAP_THREADS) sHist[s] = 0;
    if (tid == 0) sCounter = 0;
    __syncthreads();
    /* the vote (:3450-3462) */
    const int p0 = L.ptOff[q], nPt = L.ptOff[q + 1] - p0;
    uint8_t* inP = L.inFrame[0] + (size_t)q * (size_t)L.I.nP;
    int nNulled = 0;
    for (int i0 = 0; i0 < nPt; i0 += LMAP_THREADS) {
        const int i = i0 + tid;
        int what = 0;
        int32_t p = -1;
        if (i < nPt) {
            p = L.pts[p0 + i];
            what = lmap_frame_point(p, L.I.mpBad);
        }
        if (what == 1) {
            inP[p] = 1;
            for (int o = L.I.obsOff[p]; o < L.I.obsOff[p + 1]; o++) {
                const int32_t kf = L.I.obs[o];
                if (LDS)
                    atomicAdd(&sHist[kf], 1);
                else
                    atomicAdd(&L.hist[histBase + kf], 1);
            }
        }
        int tot;
        unsigned long long b;
        const int r = block_rank(what == 2, shWave, &tot, &b);
        if (what == 2) L.nulledTmp[p0 + nNulled + r] = i;
        nNulled += tot;
    }
    uint8_t* inL = L.inFrame[1] + (size_t)q * (size_t)L.I.nL;
    for (int i = L.lnOff[q] + tid; i < L.lnOff[q + 1]; i += LMAP_THREADS) {
        const int32_t l = L.lns[i];
        if (l >= 0) inL[l] = 1;
    }
    __syncthreads();
    /* the vote loop over the counter in rank order (:3474-3488) */
    int32_t* list = L.list + (size_t)q * (size_t)L.rowK;
    uint32_t* mark = L.mark + (size_t)q * (size_t)L.markWords;
    int nListed = 0;
    int32_t myCounter = 0, bv = 0, bs = 0x7fffffff;
    for (int s0 = 0; s0 < nK; s0 += LMAP_THREADS) {
        const int s = s0 + tid;
        bool listed = false;
        if (s < nK) {
            const int32_t v = LDS ? sHist[s] : __hip_atomic_load(&L.hist[histBase + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v > 0) myCounter++;
            listed = lmap_listed(v, L.I.kfBad[s]);
            if (listed && lmap_better(v, s, bv, bs)) {
                bv = v;
                bs = s;
            }
        }
        int tot;
        unsigned long long b;
        const int r = block_rank(listed, shWave, &tot, &b);
        if ((tid & 63) == 0) {
            const int w0 = (s0 + (tid & ~63)) >> 5;
            if (w0 < L.markWords) mark[w0] = (uint32_t)b;
            if (w0 + 1 < L.markWords) mark[w0 + 1] = (uint32_t)(b >> 32);
        }
        if (listed) list[nListed + r] = s;
        nListed += tot;
    }
    if (myCounter) atomicAdd(&sCounter, myCounter);
    sVotes[tid] = bv;
    sSlot[tid] = bs;
    __syncthreads();
    for (int w = LMAP_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w && lmap_better(sVotes[tid + w], sSlot[tid + w], sVotes[tid], sSlot[tid])) {
            sVotes[tid] = sVotes[tid + w];
            sSlot[tid] = sSlot[tid + w];
        }
        __syncthreads();
    }
    const int32_t counter = sCounter;
    LmapQueryRec R;
    R.nItems[0] = R.nItems[1] = 0;
    R.nNulled = nNulled;
    R.pad[0] = R.pad[1] = R.pad[2] = 0;
    if (counter == 0) {
        /* the early return (:3464): the list stays as the previous frame left it */
        const int v0 = L.prevOff[q], nPrev = L.prevOff[q + 1] - v0;
        for (int i = tid; i < nPrev; i += LMAP_THREADS) list[i] = L.prev[v0 + i];
        if (tid == 0) {
            R.nKf = nPrev;
            R.refKf = -1;
            R.rec[0] = R.rec[1] = R.rec[2] = R.rec[3] = 0;
            L.rec[q] = R;
        }
        return;
    }
    if (tid == 0) {
        const int32_t added = lmap_expand(L.I, list, nListed, mark);
        R.nKf = nListed + added;
        R.refKf = sVotes[0] > 0 ? sSlot[0] : -1;
        R.rec[0] = counter;
        R.rec[1] = nListed;
        R.rec[2] = added;
        R.rec[3] = sVotes[0];
        L.rec[q] = R;
    }
}

struct Gather {
    int kind, q, nKf, nItems, stride;
    const int32_t* rowOff;
    const int32_t* row;
    const uint8_t* bad;
    const int32_t* list;
    size_t base, rowBase;
    __device__ Gather(const LmapLaunch& L)
    {
        kind = blockIdx.z;
        q = blockIdx.y;
        nItems = kind ? L.I.nL : L.I.nP;
        stride = L.rowStride[kind];
        rowOff = kind ? L.I.kfMlOff : L.I.kfMpOff;
        row = kind ? L.I.kfMl : L.I.kfMp;
        bad = kind ? L.I.mlBad : L.I.mpBad;
        nKf = L.rec[q].nKf;
        rowBase = (size_t)q * (size_t)L.rowK;
        list = L.list + rowBase;
        base = (size_t)q * (size_t)nItems;
    }
};

__global__ __launch_bounds__(LMAP_THREADS) void k_lmap_claim(LmapLaunch L)
{
    const Gather G(L);
    int32_t* claim = L.claim[G.kind] + G.base;
    for (int j = blockIdx.x; j < G.nKf; j += gridDim.x) {
        const int32_t kf = G.list[j];
        const int r0 = G.rowOff[kf], len = G.rowOff[kf + 1] - r0;
        for (int i = threadIdx.x; i < len; i += LMAP_GATHER_ENTRIES) {
            const int32_t item = G.row[r0 + i];
            /* a bad item is never listed: its claim is not needed */
            if (item >= 0 && !G.bad[item]) atomicMin(&claim[item], lmap_walk_rank(j, i, G.stride));
        }
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_lmap_count(LmapLaunch L)
{
    __shared__ int32_t sCnt;
    const Gather G(L);
    const int32_t* claim = L.claim[G.kind] + G.base;
    if (threadIdx.x == 0) sCnt = 0;
    __syncthreads();
    for (int j = blockIdx.x; j < G.nKf; j += gridDim.x) {
        const int32_t kf = G.list[j];
        const int r0 = G.rowOff[kf], len = G.rowOff[kf + 1] - r0;
        int32_t c = 0;
        for (int i = threadIdx.x; i < len; i += LMAP_GATHER_ENTRIES)
            c += lmap_entry_kept(G.row[r0 + i], lmap_walk_rank(j, i, G.stride), claim, G.bad) ? 1 : 0;
        if (c) atomicAdd(&sCnt, c);
        __syncthreads();
        if (threadIdx.x == 0) {
            L.cnt[G.kind][G.rowBase + j] = sCnt;
            sCnt = 0;
        }
        __syncthreads();
    }
}

/* grid (query, kind) */
__global__ __launch_bounds__(LMAP_THREADS) void k_lmap_scan(LmapLaunch L)
{
    __shared__ int32_t sh[LMAP_THREADS];
    const int q = blockIdx.x, kind = blockIdx.y, tid = threadIdx.x;
    const int nKf = L.rec[q].nKf;
    int32_t* cnt = L.cnt[kind] + (size_t)q * (size_t)L.rowK;
    int32_t carry = 0;
    for (int j0 = 0; j0 < nKf; j0 += LMAP_THREADS) {
        const int j = j0 + tid;
        const int32_t v = j < nKf ? cnt[j] : 0;
        int32_t tot;
        const int32_t ex = block_excl_scan(v, sh, &tot);
        if (j < nKf) cnt[j] = carry + ex;
        carry += tot;
    }
    if (tid == 0) L.rec[q].nItems[kind] = carry;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_lmap_offsets(LmapLaunch L)
{
    __shared__ int32_t sh[LMAP_THREADS];
    const int tid = threadIdx.x;
    for (int f = 0; f < 4; f++) {
        int32_t carry = 0;
        for (int q0 = 0; q0 < L.nQ; q0 += LMAP_THREADS) {
            const int q = q0 + tid;
            int32_t v = 0;
            if (q < L.nQ) v = f == 0 ? L.rec[q].nKf : f == 3 ? L.rec[q].nNulled : L.rec[q].nItems[f - 1];
            int32_t tot;
            const int32_t ex = block_excl_scan(v, sh, &tot);
            if (q < L.nQ) L.off[f][q] = carry + ex;
            carry += tot;
        }
        if (tid == 0) L.off[f][L.nQ] = carry;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_lmap_write(LmapLaunch L)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    const Gather G(L);
    const int32_t* claim = L.claim[G.kind] + G.base;
    const uint8_t* inFrame = L.inFrame[G.kind] + G.base;
    const int32_t qOut = L.off[1 + G.kind][G.q];
    for (int j = blockIdx.x; j < G.nKf; j += gridDim.x) {
        const int32_t kf = G.list[j];
        const int r0 = G.rowOff[kf], len = G.rowOff[kf + 1] - r0;
        int32_t at = qOut + L.cnt[G.kind][G.rowBase + j];
        for (int i0 = 0; i0 < len; i0 += LMAP_GATHER_ENTRIES) {
            const int i = i0 + threadIdx.x;
            int32_t item = -1;
            bool keep = false;
            if (i < len) {
                item = G.row[r0 + i];
                keep = lmap_entry_kept(item, lmap_walk_rank(j, i, G.stride), claim, G.bad);
            }
            int tot;
            unsigned long long b;
            const int r = block_rank(keep, shWave, &tot, &b);
            if (keep) {
                L.packedItem[G.kind][at + r] = item;
                L.packedIn[G.kind][at + r] = inFrame[item];
            }
            at += tot;
        }
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_lmap_pack(LmapLaunch L)
{
    const int q = blockIdx.x, tid = threadIdx.x;
    const int nKf = L.rec[q].nKf, nNulled = L.rec[q].nNulled;
    const int32_t* list = L.list + (size_t)q * (size_t)L.rowK;
    for (int i = tid; i < nKf; i += LMAP_THREADS) L.packedKf[L.off[0][q] + i] = list[i];
    const int p0 = L.ptOff[q];
    for (int i = tid; i < nNulled; i += LMAP_THREADS) L.packedNulled[L.off[3][q] + i] = L.nulledTmp[p0 + i];
}

}  // namespace

hipError_t drfe_launch_lmap(const LmapLaunch& L, hipStream_t s)
{
    if (L.nQ <= 0) return hipSuccess;
    const int rows = L.rowK < 1 ? 1 : (L.rowK < LMAP_GATHER_ROWS ? L.rowK : LMAP_GATHER_ROWS);
    if (L.I.nK <= LMAP_LDS_KFS)
        hipLaunchKernelGGL(k_lmap_vote<true>, dim3(L.nQ), dim3(LMAP_THREADS), 0, s, L);
    else
        hipLaunchKernelGGL(k_lmap_vote<false>, dim3(L.nQ), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_lmap_claim, dim3(rows, L.nQ, 2), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_lmap_count, dim3(rows, L.nQ, 2), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_lmap_scan, dim3(L.nQ, 2), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_lmap_offsets, dim3(1), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_lmap_write, dim3(rows, L.nQ, 2), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_lmap_pack, dim3(L.nQ), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}
