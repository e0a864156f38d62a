/* conn_kernels.hip — KeyFrame::UpdateConnections of every key frame of a call on the device, the closed form
 * of conn_core.h.
 *
 *   k_conn_vote     a workgroup per called key frame k.  Lanes stride over k's match row; each voting entry adds 1 per observation
 *                   but k's own into the histogram over key-frame slots (LDS up to LMAP_LDS_KFS stored key frames, else a zeroed
 *                   row of global scratch; integer atomic adds only).  The counter is compacted in slot order = rank order,
 *                   pKFmax is a reduction on (votes, lowest slot), the listed keys are ranked against each other tile by tile
 *                   (keys are distinct, so a key's place is the number of larger ones), the fallback lists pKFmax alone.
 *   k_conn_edges    a workgroup per called key frame, a lane per counter entry: a listed entry is an AddConnection on its key
 *                   frame j; the value it meets is found by binary search in C_j (j called earlier) or in j's stored row.
 *   k_conn_touched  one workgroup: the touched slots in ascending order, the offsets of the packed counters.
 *   k_conn_count    a workgroup per touched key frame j: the edges that land on j (a binary search for j in every called key
 *                   frame's counter), the size of j's final rows, which list it ends with, its parent and flag.
 *   k_conn_offsets  one workgroup: the offsets of the packed rows.
 *   k_conn_rows     a workgroup per touched key frame: base row and edges scattered into a row over slots (LDS or global
 *                   scratch; one writer per slot), compacted in slot order into the final weights; then the list: the full sort
 *                   of those, the listed keys of its own call, or the stored one.
 *   k_conn_pack     per called key frame: its counter into the packed list.
 *
 * The hand-offs are the launches, in stream order; no workgroup waits on another.  Which atomic arrives first cannot show: the adds
 * commute, and the touched marks are stores of the same byte. */
#include "lmap_device.h"

namespace {

/* lmap_device.h's rank without the wave's ballot */
__device__ int block_rank(bool flag, int32_t* shWave, int* total)
{
    unsigned long long ballot;
    return ::block_rank(flag, shWave, total, &ballot);
}

/* The pairs (kf, w)[0 .. n) - with listedOnly those of at least CONN_TH - in descending key order: into keys, or into the pair
 * arrays.  Every thread of the workgroup calls it. */
__device__ void rank_sort(const int32_t* kf, const int32_t* w, int n, bool listedOnly, uint64_t* sKey, uint64_t* keys, int32_t* outKf,
                          int32_t* outW)
{
    const int tid = threadIdx.x;
    for (int c0 = 0; c0 < n; c0 += LMAP_THREADS) {
        const int c = c0 + tid;
        uint64_t my = 0;                       /* no key is 0: weights are positive */
        if (c < n && (!listedOnly || conn_listed(w[c]))) my = conn_key(w[c], kf[c]);
        int rank = 0;
        for (int e0 = 0; e0 < n; e0 += CONN_SORT_TILE) {
            const int e = e0 + tid;
            __syncthreads();
            sKey[tid] = (e < n && (!listedOnly || conn_listed(w[e]))) ? conn_key(w[e], kf[e]) : 0;
            __syncthreads();
            if (my) {
                const int m = n - e0 < CONN_SORT_TILE ? n - e0 : CONN_SORT_TILE;
                for (int i = 0; i < m; i++) rank += sKey[i] > my ? 1 : 0;
            }
        }
        if (my) {
            if (keys) {
                keys[rank] = my;
            } else {
                outKf[rank] = conn_key_slot(my);
                outW[rank] = conn_key_weight(my);
            }
        }
    }
}

/* grid: the called key frames [p0, p0 + gridDim.x) */
template <bool LDS>
__global__ __launch_bounds__(LMAP_THREADS) void k_conn_vote(ConnLaunch L, int p0)
{
    __shared__ int32_t sHist[LDS ? LMAP_LDS_KFS : 1];
    __shared__ uint64_t sKey[CONN_SORT_TILE];
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    __shared__ int32_t sVotes[LMAP_THREADS], sSlot[LMAP_THREADS];
    const int p = p0 + blockIdx.x, tid = threadIdx.x, nK = L.I.nK;
    const int32_t k = L.called[p];
    int32_t* gHist = L.hist + (size_t)blockIdx.x * (size_t)nK;
    if (LDS)
        for (int s = tid; s < nK; s += LMAP_THREADS) sHist[s] = 0;
    __syncthreads();
    /* the vote (:377-398) */
    const int r0 = L.I.kfMpOff[k], len = L.I.kfMpOff[k + 1] - r0;
    for (int i = tid; i < len; i += LMAP_THREADS) {
        const int32_t pt = L.I.kfMp[r0 + i];
        if (!conn_point_votes(pt, L.I.mpBad)) continue;
        for (int o = L.I.obsOff[pt]; o < L.I.obsOff[pt + 1]; o++) {
            const int32_t kf = L.I.obs[o];
            if (!conn_obs_votes(kf, k)) continue;
            if (LDS)
                atomicAdd(&sHist[kf], 1);
            else
                atomicAdd(&gHist[kf], 1);
        }
    }
    __syncthreads();
    /* the walk over the counter in rank order (:411-424): the counter itself, nmax and pKFmax */
    const int32_t cap0 = L.capOff[p], cap = L.capOff[p + 1] - cap0;
    int32_t* cKf = L.cntKf + cap0;
    int32_t* cW = L.cntW + cap0;
    int nC = 0, nListed = 0;
    int32_t bv = 0, bs = 0x7fffffff;
    for (int s0 = 0; s0 < nK; s0 += LMAP_THREADS) {
        const int s = s0 + tid;
        int32_t v = 0;
        if (s < nK) v = LDS ? sHist[s] : __hip_atomic_load(&gHist[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v > 0 && conn_better(v, s, bv, bs)) {
            bv = v;
            bs = s;
        }
        int tot;
        const int r = block_rank(v > 0, shWave, &tot);
        /* the host's bound holds for every graph; the test keeps a wrong bound from writing past the region */
        if (v > 0 && nC + r < cap) {
            cKf[nC + r] = s;
            cW[nC + r] = v;
        }
        nC += tot;
        int totL;
        (void)block_rank(conn_listed(v), shWave, &totL);
        nListed += totL;
    }
    sVotes[tid] = bv;
    sSlot[tid] = bs;
    __syncthreads();
    for (int w = LMAP_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w && conn_better(sVotes[tid + w], sSlot[tid + w], sVotes[tid], sSlot[tid])) {
            sVotes[tid] = sVotes[tid + w];
            sSlot[tid] = sSlot[tid + w];
        }
        __syncthreads();
    }
    const int32_t nmax = sVotes[0], best = nmax > 0 ? sSlot[0] : -1;
    if (nC > cap) nC = cap;
    uint64_t* lst = L.lst + cap0;
    if (nC > 0) {
        if (nListed > 0)
            rank_sort(cKf, cW, nC, true, sKey, lst, nullptr, nullptr);
        else if (tid == 0)
            lst[0] = conn_key(nmax, best);     /* the fallback (:426-430) */
    }
    __syncthreads();
    if (tid == 0) {
        ConnRec R;
        R.nC = nC;
        R.nL = nC > 0 ? (nListed > 0 ? nListed : 1) : 0;
        R.nmax = nmax;
        R.best = best;
        L.rec[p] = R;
        /* the first connection (:448-453): the parent is the front of the list */
        L.newParent[p] = nC > 0 && L.G.first[k] ? conn_key_slot(lst[0]) : -1;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_conn_edges(ConnLaunch L)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    const int32_t k = L.called[p];
    const ConnRec R = L.rec[p];
    const int32_t cap0 = L.capOff[p];
    if (tid == 0) L.mark[k] = 1;
    const bool fallback = !conn_listed(R.nmax);
    for (int c = tid; c < R.nC; c += LMAP_THREADS) {
        const int32_t j = L.cntKf[cap0 + c], w = L.cntW[cap0 + c];
        uint8_t f = 0;
        if (conn_listed(w) || (fallback && j == R.best)) {
            const int32_t pj = L.pos[j], nCj = pj >= 0 ? L.rec[pj].nC : 0;
            const int32_t* row;
            const int32_t* rowW;
            int32_t n;
            if (conn_prior_in_counter(pj, nCj, p)) {
                row = L.cntKf + L.capOff[pj];
                rowW = L.cntW + L.capOff[pj];
                n = nCj;
            } else {
                row = L.G.wKf + L.G.wOff[j];
                rowW = L.G.wW + L.G.wOff[j];
                n = L.G.wOff[j + 1] - L.G.wOff[j];
            }
            const int32_t at = conn_find(row, n, k);
            f = conn_changes(at >= 0, at >= 0 ? rowW[at] : 0, w) ? 2 : 1;
            L.mark[j] = 1;
        }
        L.chg[cap0 + c] = f;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_conn_touched(ConnLaunch L)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    __shared__ int32_t sh[LMAP_THREADS];
    const int tid = threadIdx.x, nK = L.I.nK;
    int nT = 0;
    for (int s0 = 0; s0 < nK; s0 += LMAP_THREADS) {
        const int s = s0 + tid;
        const bool on = s < nK && L.mark[s];
        int tot;
        const int r = block_rank(on, shWave, &tot);
        if (on) L.touched[nT + r] = s;
        nT += tot;
    }
    int32_t carry = 0;
    for (int p0 = 0; p0 < L.n; p0 += LMAP_THREADS) {
        const int p = p0 + tid;
        const int32_t v = p < L.n ? L.rec[p].nC : 0;
        int32_t tot;
        const int32_t ex = block_excl_scan(v, sh, &tot);
        if (p < L.n) L.cntOff[p] = carry + ex;
        carry += tot;
    }
    if (tid == 0) {
        L.cntOff[L.n] = carry;
        L.head[CONN_HEAD_TOUCHED] = nT;
        L.head[CONN_HEAD_COUNTER] = carry;
    }
}

/* what a touched key frame's rows start from: its own counter when it was called with one, else its stored weights */
struct Base {
    int32_t pj, nCj, len;
    const int32_t* kf;
    const int32_t* w;
    __device__ Base(const ConnLaunch& L, int32_t j)
    {
        pj = L.pos[j];
        nCj = pj >= 0 ? L.rec[pj].nC : 0;
        if (nCj > 0) {
            kf = L.cntKf + L.capOff[pj];
            w = L.cntW + L.capOff[pj];
            len = nCj;
        } else {
            kf = L.G.wKf + L.G.wOff[j];
            w = L.G.wW + L.G.wOff[j];
            len = L.G.wOff[j + 1] - L.G.wOff[j];
        }
    }
};

/* the edge of called key frame p onto j that is in j's final row: its index in p's counter, or -1 */
__device__ int32_t landing_edge(const ConnLaunch& L, const Base& B, int32_t j, int p)
{
    if (p == B.pj || !conn_edge_applies(B.pj, B.nCj, p)) return -1;
    const int32_t cap0 = L.capOff[p];
    const int32_t c = conn_find(L.cntKf + cap0, L.rec[p].nC, j);
    return c >= 0 && L.chg[cap0 + c] ? cap0 + c : -1;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_conn_count(ConnLaunch L)
{
    __shared__ int32_t sAdd, sChanged;
    const int tid = threadIdx.x, nT = L.head[CONN_HEAD_TOUCHED];
    for (int t = blockIdx.x; t < nT; t += gridDim.x) {
        const int32_t j = L.touched[t];
        const Base B(L, j);
        if (tid == 0) sAdd = sChanged = 0;
        __syncthreads();
        int32_t add = 0, changed = 0;
        for (int p = tid; p < L.n; p += LMAP_THREADS) {
            const int32_t e = landing_edge(L, B, j, p);
            if (e < 0) continue;
            if (conn_find(B.kf, B.len, L.called[p]) < 0) add++;
            if (L.chg[e] == 2) changed = 1;
        }
        if (add) atomicAdd(&sAdd, add);
        if (changed) atomicOr(&sChanged, 1);
        __syncthreads();
        if (tid == 0) {
            const bool own = B.nCj > 0;
            const int mode = conn_list_mode(own, sChanged != 0);
            const int32_t nW = B.len + sAdd;
            L.tMode[t] = mode;
            L.wOff[t] = nW;
            L.oOff[t] = mode == CONN_LIST_FULL ? nW : (mode == CONN_LIST_OWN ? L.rec[B.pj].nL : L.G.oOff[j + 1] - L.G.oOff[j]);
            const int32_t np = B.pj >= 0 ? L.newParent[B.pj] : -1;
            L.tParent[t] = np >= 0 ? np : L.I.kfParent[j];
            L.tFirst[t] = L.G.first[j] && !own ? 1 : 0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_conn_offsets(ConnLaunch L)
{
    __shared__ int32_t sh[LMAP_THREADS];
    const int tid = threadIdx.x, nT = L.head[CONN_HEAD_TOUCHED];
    for (int f = 0; f < 2; f++) {
        int32_t* off = f ? L.oOff : L.wOff;
        int32_t carry = 0;
        for (int t0 = 0; t0 < nT; t0 += LMAP_THREADS) {
            const int t = t0 + tid;
            const int32_t v = t < nT ? off[t] : 0;
            int32_t tot;
            const int32_t ex = block_excl_scan(v, sh, &tot);
            if (t < nT) off[t] = carry + ex;
            carry += tot;
        }
        if (tid == 0) {
            off[nT] = carry;
            L.head[f ? CONN_HEAD_ORDERED : CONN_HEAD_WEIGHTS] = carry;
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(LMAP_THREADS) void k_conn_rows(ConnLaunch L)
{
    __shared__ int32_t sRow[LDS ? LMAP_LDS_KFS : 1];
    __shared__ uint64_t sKey[CONN_SORT_TILE];
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    const int tid = threadIdx.x, nK = L.I.nK, nT = L.head[CONN_HEAD_TOUCHED];
    int32_t* row = LDS ? sRow : L.dense + (size_t)blockIdx.x * (size_t)nK;
    for (int t = blockIdx.x; t < nT; t += gridDim.x) {
        const int32_t j = L.touched[t];
        const Base B(L, j);
        __syncthreads();
        for (int s = tid; s < nK; s += LMAP_THREADS) row[s] = 0;
        __syncthreads();
        for (int i = tid; i < B.len; i += LMAP_THREADS) row[B.kf[i]] = B.w[i];
        __syncthreads();
        /* an edge overwrites the base entry of its key frame; the called key frames are distinct */
        for (int p = tid; p < L.n; p += LMAP_THREADS) {
            const int32_t e = landing_edge(L, B, j, p);
            if (e >= 0) row[L.called[p]] = L.cntW[e];
        }
        __syncthreads();
        const int32_t w0 = L.wOff[t], nW = L.wOff[t + 1] - w0;
        int at = 0;
        for (int s0 = 0; s0 < nK; s0 += LMAP_THREADS) {
            const int s = s0 + tid;
            const int32_t v = s < nK ? row[s] : 0;
            int tot;
            const int r = block_rank(v > 0, shWave, &tot);
            if (v > 0 && at + r < nW) {
                L.pkWKf[w0 + at + r] = s;
                L.pkWW[w0 + at + r] = v;
            }
            at += tot;
        }
        __syncthreads();
        const int32_t o0 = L.oOff[t], nO = L.oOff[t + 1] - o0;
        const int mode = L.tMode[t];
        if (mode == CONN_LIST_FULL) {
            rank_sort(L.pkWKf + w0, L.pkWW + w0, nW, false, sKey, nullptr, L.pkOKf + o0, L.pkOW + o0);
        } else if (mode == CONN_LIST_OWN) {
            const uint64_t* lst = L.lst + L.capOff[B.pj];
            for (int i = tid; i < nO; i += LMAP_THREADS) {
                L.pkOKf[o0 + i] = conn_key_slot(lst[i]);
                L.pkOW[o0 + i] = conn_key_weight(lst[i]);
            }
        } else {
            const int32_t g0 = L.G.oOff[j];
            for (int i = tid; i < nO; i += LMAP_THREADS) {
                L.pkOKf[o0 + i] = L.G.oKf[g0 + i];
                L.pkOW[o0 + i] = L.G.oW[g0 + i];
            }
        }
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_conn_pack(ConnLaunch L)
{
    const int p = blockIdx.x;
    const int32_t cap0 = L.capOff[p], at = L.cntOff[p], nC = L.rec[p].nC;
    for (int i = threadIdx.x; i < nC; i += LMAP_THREADS) {
        L.pkCntKf[at + i] = L.cntKf[cap0 + i];
        L.pkCntW[at + i] = L.cntW[cap0 + i];
    }
}

}  // namespace

hipError_t drfe_launch_conn(const ConnLaunch& L, hipStream_t s)
{
    if (L.n <= 0) return hipSuccess;
    const int nK = L.I.nK;
    const bool lds = nK <= LMAP_LDS_KFS;
    hipError_t e = hipMemsetAsync(L.mark, 0, (size_t)nK, s);
    if (e != hipSuccess) return e;
    for (int p0 = 0; p0 < L.n; p0 += L.chunk) {
        const int m = L.n - p0 < L.chunk ? L.n - p0 : L.chunk;
        if (lds) {
            hipLaunchKernelGGL(k_conn_vote<true>, dim3(m), dim3(LMAP_THREADS), 0, s, L, p0);
        } else {
            e = hipMemsetAsync(L.hist, 0, sizeof(int32_t) * (size_t)m * (size_t)nK, s);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k_conn_vote<false>, dim3(m), dim3(LMAP_THREADS), 0, s, L, p0);
        }
    }
    const int groups = nK < CONN_ROW_GROUPS ? nK : CONN_ROW_GROUPS;
    hipLaunchKernelGGL(k_conn_edges, dim3(L.n), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_conn_touched, dim3(1), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_conn_count, dim3(groups), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_conn_offsets, dim3(1), dim3(LMAP_THREADS), 0, s, L);
    if (lds)
        hipLaunchKernelGGL(k_conn_rows<true>, dim3(groups), dim3(LMAP_THREADS), 0, s, L);
    else
        hipLaunchKernelGGL(k_conn_rows<false>, dim3(groups), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_conn_pack, dim3(L.n), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}
