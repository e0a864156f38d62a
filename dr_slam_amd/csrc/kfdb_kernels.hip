/* kfdb_kernels.hip — KeyFrameDatabase's loop and relocalisation queries on the device: a workgroup per
 * query, key frames across its lanes.
 *
 *   k_kfdb_count   stage 1: one sorted-merge walk per (query, key frame) gives the common-word count, the smallest shared word and
 *                  L1Scoring::score's ordered double sum (inside one lane); stage 2: maxCommonWords, the threshold, minScore of a
 *                  loop query from its covisible list; the listed / scored marks.
 *   k_kfdb_select  stage 3 is the score kept from the walk; stage 4: the kept key frames compacted and ranked by (smallest shared
 *                  word, sequence number), the order in which the reference meets them; stage 5: the neighbour accumulation;
 *                  stage 6: the retain threshold, first-occurrence de-duplication and an order-preserving compaction.
 *   k_kfdb_commit  relocalisation: the resident mRelocScore takes the score of the last query of the call that scored the key frame.
 *   k_kfdb_pack    the candidate lists of all queries into one CSR.
 *
 * A relocalisation query reads a stale mRelocScore from the marks and scores of the earlier queries of the call, which
 * k_kfdb_count has finished for all of them before k_kfdb_select starts, so the queries of a call run side by side. */
#include "kfdb_internal.h"

namespace {

__device__ int32_t block_max_i32(int32_t v, int32_t* sh)
{
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int w = KFDB_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w && sh[tid + w] > sh[tid]) sh[tid] = sh[tid + w];
        __syncthreads();
    }
    return sh[0];
}

__device__ int32_t block_sum_i32(int32_t v, int32_t* sh)
{
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int w = KFDB_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    return sh[0];
}

/* the largest of the lanes' values: what `if (acc > best) best = acc` over any order leaves (no NaN reaches it) */
__device__ float block_max_f32(float v, float* sh)
{
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int w = KFDB_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w && sh[tid + w] > sh[tid]) sh[tid] = sh[tid + w];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(KFDB_THREADS) void k_kfdb_count(KfdbLaunch L)
{
    __shared__ int32_t sh[KFDB_THREADS];
    const int q = blockIdx.x, tid = threadIdx.x, nS = L.nSlots;
    const size_t base = (size_t)q * (size_t)nS;
    uint8_t* flag = L.flag + base;
    if (!L.reloc) {
        for (int i = L.connOff[q] + tid; i < L.connOff[q + 1]; i += KFDB_THREADS) flag[L.conn[i]] = KFDB_F_CONNECTED;
        __syncthreads();
    }
    const int q0 = L.qOff[q], nQw = L.qOff[q + 1] - q0;
    int32_t myMax = 0, myListed = 0;
    for (int s = tid; s < nS; s += KFDB_THREADS) {
        const int w0 = L.wordOff[s], nK = L.wordOff[s + 1] - w0;
        int32_t c = 0, f = -1;
        double sum = 0.0;
        if (nK > 0) kfdb_walk(L.qIds + q0, L.qVals + q0, nQw, L.wordIds + w0, L.wordVals + w0, nK, &c, &f, &sum);
        L.cnt[base + s] = c;
        L.first[base + s] = f;
        L.score[base + s] = kfdb_score(sum);
        uint8_t fl = flag[s];
        const bool visible = L.seq[s] >= 0 && L.from[s] <= q;
        if (visible && c > 0 && !(fl & KFDB_F_CONNECTED)) {
            fl |= KFDB_F_LISTED;
            myListed++;
            if (c > myMax) myMax = c;
        }
        flag[s] = fl;
    }
    const int32_t maxCommon = block_max_i32(myMax, sh);
    const int32_t listed = block_sum_i32(myListed, sh);
    const int32_t minCommon = kfdb_min_common(maxCommon);
    int32_t myScored = 0;
    for (int s = tid; s < nS; s += KFDB_THREADS) {
        const uint8_t fl = flag[s];
        if ((fl & KFDB_F_LISTED) && L.cnt[base + s] > minCommon) {
            flag[s] = fl | KFDB_F_SCORED;
            myScored++;
        }
    }
    const int32_t scored = block_sum_i32(myScored, sh);
    if (tid == 0) {
        float minScore = 0.0f;
        if (!L.reloc) {
            if (L.useCov[q]) {
                /* src/LoopClosing.cc:139-151 */
                minScore = 1.0f;
                for (int i = L.covOff[q]; i < L.covOff[q + 1]; i++) {
                    const float sc = L.score[base + L.cov[i]];
                    if (sc < minScore) minScore = sc;
                }
            } else {
                minScore = L.minScoreIn[q];
            }
        }
        KfdbQueryRec R;
        R.listed = listed;
        R.scored = scored;
        R.kept = 0;
        R.maxCommon = maxCommon;
        R.minCommon = minCommon;
        R.nCand = 0;
        R.uninit = 0;
        R.pad = 0;
        R.minScore = minScore;
        R.pad2 = 0.0f;
        L.rec[q] = R;
    }
}

/* the neighbour test of a query and the score it reads (kfdb_accumulate) */
struct KfdbLook {
    const KfdbLaunch& L;
    int q;
    size_t base;
    int32_t uninit;
    __device__ bool operator()(int32_t nb, float* s)
    {
        const uint8_t fl = L.flag[base + nb];
        if (!L.reloc) {
            /* mnLoopQuery == id (listed) and mnLoopWords > minCommonWords */
            if (!(fl & KFDB_F_SCORED)) return false;
            *s = L.score[base + nb];
            return true;
        }
        /* mnRelocQuery == id: in the inverted file and shares a word */
        if (!(fl & KFDB_F_LISTED)) return false;
        if (fl & KFDB_F_SCORED) {
            *s = L.score[base + nb];
            return true;
        }
        /* not scored by this query: what the latest earlier query that scored it left, else the resident value */
        for (int k = q - 1; k >= 0; k--) {
            const size_t at = (size_t)k * (size_t)L.nSlots + (size_t)nb;
            if (L.flag[at] & KFDB_F_SCORED) {
                *s = L.score[at];
                return true;
            }
        }
        if (L.relocWritten[nb]) {
            *s = L.relocScore[nb];
        } else {
            *s = 0.0f;
            uninit++;
        }
        return true;
    }
};

__global__ __launch_bounds__(KFDB_THREADS) void k_kfdb_select(KfdbLaunch L)
{
    __shared__ int32_t sh[KFDB_THREADS];
    __shared__ float shf[KFDB_THREADS];
    __shared__ int32_t sKept, sUninit;
    const int q = blockIdx.x, tid = threadIdx.x, nS = L.nSlots;
    const size_t base = (size_t)q * (size_t)nS;
    const uint8_t* flag = L.flag + base;
    const float minScore = L.rec[q].minScore;
    if (tid == 0) {
        sKept = 0;
        sUninit = 0;
    }
    __syncthreads();
    /* lScoreAndMatch, in any order */
    for (int s = tid; s < nS; s += KFDB_THREADS)
        if ((flag[s] & KFDB_F_SCORED) && (L.reloc || L.score[base + s] >= minScore)) L.keptTmp[base + atomicAdd(&sKept, 1)] = s;
    __syncthreads();
    const int nKept = sKept;
    /* its order: the rank of (smallest shared word, sequence number) among the kept; the pairs are distinct */
    for (int e = tid; e < nKept; e += KFDB_THREADS) {
        const int32_t s = L.keptTmp[base + e];
        const int32_t fs = L.first[base + s];
        const int64_t qs = L.seq[s];
        int r = 0;
        for (int j = 0; j < nKept; j++) {
            const int32_t t = L.keptTmp[base + j];
            r += kfdb_before(L.first[base + t], L.seq[t], fs, qs);
        }
        L.keptOrd[base + r] = s;
    }
    __syncthreads();
    float myBest = L.reloc ? 0.0f : minScore;
    KfdbLook look{L, q, base, 0};
    for (int e = tid; e < nKept; e += KFDB_THREADS) {
        const int32_t s = L.keptOrd[base + e];
        float a;
        int32_t b;
        kfdb_accumulate(L.score[base + s], s, L.nbr + (size_t)KFDB_NEIGHBOURS * (size_t)s, look, &a, &b);
        L.acc[base + e] = a;
        L.best[base + e] = b;
        if (a > myBest) myBest = a;
    }
    if (look.uninit) atomicAdd(&sUninit, look.uninit);
    const float retain = kfdb_retain(block_max_f32(myBest, shf));
    /* the first entry that elects each key frame */
    for (int e = tid; e < nKept; e += KFDB_THREADS)
        if (L.acc[base + e] > retain) atomicMin(L.minEntry + base + L.best[base + e], e);
    __syncthreads();
    int nCand = 0;
    for (int e0 = 0; e0 < nKept; e0 += KFDB_THREADS) {
        const int e = e0 + tid;
        int32_t b = -1;
        int keep = 0;
        if (e < nKept && L.acc[base + e] > retain) {
            b = L.best[base + e];
            keep = __hip_atomic_load(L.minEntry + base + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == e;
        }
        /* inclusive scan of keep over the chunk */
        __syncthreads();
        sh[tid] = keep;
        __syncthreads();
        for (int w = 1; w < KFDB_THREADS; w <<= 1) {
            const int32_t add = tid >= w ? sh[tid - w] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        if (keep) L.cand[base + nCand + sh[tid] - 1] = b;
        nCand += sh[KFDB_THREADS - 1];
    }
    __syncthreads();
    if (tid == 0) {
        L.rec[q].kept = nKept;
        L.rec[q].nCand = nCand;
        L.rec[q].uninit = sUninit;
    }
}

__global__ __launch_bounds__(KFDB_THREADS) void k_kfdb_commit(KfdbLaunch L)
{
    const int s = blockIdx.x * KFDB_THREADS + threadIdx.x;
    if (s >= L.nSlots) return;
    for (int k = L.nQueries - 1; k >= 0; k--) {
        const size_t at = (size_t)k * (size_t)L.nSlots + (size_t)s;
        if (L.flag[at] & KFDB_F_SCORED) {
            L.relocScore[s] = L.score[at];
            L.relocWritten[s] = 1;
            return;
        }
    }
}

__global__ __launch_bounds__(KFDB_THREADS) void k_kfdb_pack(KfdbLaunch L)
{
    __shared__ int32_t sh[KFDB_THREADS];
    const int q = blockIdx.x, tid = threadIdx.x;
    int32_t mine = 0;
    for (int k = tid; k < q; k += KFDB_THREADS) mine += L.rec[k].nCand;
    const int32_t off = block_sum_i32(mine, sh);
    const int32_t n = L.rec[q].nCand;
    const size_t base = (size_t)q * (size_t)L.nSlots;
    for (int i = tid; i < n; i += KFDB_THREADS) L.candPacked[off + i] = L.cand[base + i];
    if (tid == 0) {
        L.candOff[q] = off;
        if (q == L.nQueries - 1) L.candOff[q + 1] = off + n;
    }
}

}  // namespace

hipError_t drfe_launch_kfdb(const KfdbLaunch& L, hipStream_t s)
{
    if (L.nQueries <= 0 || L.nSlots <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_kfdb_count, dim3(L.nQueries), dim3(KFDB_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_kfdb_select, dim3(L.nQueries), dim3(KFDB_THREADS), 0, s, L);
    if (L.reloc) hipLaunchKernelGGL(k_kfdb_commit, dim3((L.nSlots + KFDB_THREADS - 1) / KFDB_THREADS), dim3(KFDB_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_kfdb_pack, dim3(L.nQueries), dim3(KFDB_THREADS), 0, s, L);
    return hipGetLastError();
}
