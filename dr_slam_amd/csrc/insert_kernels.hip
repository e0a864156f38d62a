/* insert_kernels.hip — the item loops of LocalMapping::ProcessNewKeyFrame on the device.  The rows of a call
 * are one flat entry space (insert_core.h), a lane per entry.  A chunk is a run of called key frames:
 *
 *   k_insert_claim    every entry that names an item lowers the claim word of (its key frame, the item) to its row index, so that
 *                     the first occurrence of an item inside one row is known.
 *   k_insert_verdict  the action of every entry from the resident image (ins_verdict): the bad flag, a scan of the item's resident
 *                     observers for the key frame, the claim.  An ADDED entry adds its weight to the item's nObs in the resident
 *                     attribute (recent-list) block and, with normals, sets its key frame's bit in the point's adder word.
 *
 * After the last chunk, over the whole entry space:
 *
 *   k_insert_count    per workgroup the ADDED and RECENT entries of each kind.
 *   k_insert_scan     one workgroup: their exclusive prefix over the workgroups, the totals into the head words.
 *   k_insert_pack     the ADDED entries and the RECENT items of each kind in walk order (rank by ballot inside a wave, scan over
 *                     the workgroup).
 *   k_insert_normals  a lane per ADDED point entry, over a grid: UpdateNormalAndDepth over the resident observers merged with the
 *                     adders at or before its key frame (ins_point_normal); every ordered sum stays inside the lane.
 *
 * The hand-offs are the launches, in stream order.  A minimum, a set bit and an integer sum do not show the order of their
 * atomics; nothing a verdict reads is written by the call. */
#include "lmap_device.h"

namespace {

struct Entry {
    int32_t j, i, kind, kf, item;
};

__device__ inline Entry entry_of(const InsertLaunch& L, int32_t e)
{
    Entry E;
    const int32_t q = ins_segment(L.segOff, 2 * L.n, e);
    E.kind = q >= L.n ? FUSE_LINE : FUSE_POINT;
    E.j = q - (E.kind == FUSE_LINE ? L.n : 0);
    E.i = e - L.segOff[q];
    E.kf = L.called[E.j];
    E.item = E.kind == FUSE_POINT ? L.I.kfMp[L.I.kfMpOff[E.kf] + E.i] : L.I.kfMl[L.I.kfMlOff[E.kf] + E.i];
    return E;
}

__device__ inline int32_t* claim_word(const InsertLaunch& L, const Entry& E)
{
    return L.claim[E.kind] + (size_t)(E.j - L.j0) * (size_t)(E.kind == FUSE_POINT ? L.I.nP : L.I.nL) + (size_t)E.item;
}

__global__ __launch_bounds__(INSERT_TILE) void k_insert_claim(InsertLaunch L, int32_t e0, int32_t e1)
{
    const int32_t e = e0 + blockIdx.x * INSERT_TILE + threadIdx.x;
    if (e >= e1) return;
    const Entry E = entry_of(L, e);
    if (E.item >= 0) atomicMin(claim_word(L, E), E.i);
}

__global__ __launch_bounds__(INSERT_TILE) void k_insert_verdict(InsertLaunch L, int32_t e0, int32_t e1)
{
    const int32_t e = e0 + blockIdx.x * INSERT_TILE + threadIdx.x;
    if (e >= e1) return;
    const Entry E = entry_of(L, e);
    int action = INS_NULL;
    if (E.item >= 0) {
        const bool point = E.kind == FUSE_POINT;
        const uint8_t bad = point ? L.I.mpBad[E.item] : L.I.mlBad[E.item];
        bool observes = false;
        if (!bad)
            observes = point ? ins_observes(L.I.obs, L.I.obsOff[E.item], L.I.obsOff[E.item + 1], E.kf)
                             : ins_observes(L.R.mlObs, L.R.mlObsOff[E.item], L.R.mlObsOff[E.item + 1], E.kf);
        action = ins_verdict(E.item, bad, observes, *claim_word(L, E) == E.i);
        if (action == INS_ADDED) {
            if (point) {
                atomicAdd(const_cast<int32_t*>(L.A.nObs) + E.item, fuse_obs_weight(FUSE_POINT, L.A.stereo[L.I.kfMpOff[E.kf] + E.i]));
                if (L.normals) {
                    const int32_t r = L.rankOf[E.j];
                    atomicOr(L.adders + (size_t)E.item * (size_t)L.words + (size_t)(r >> 5), 1u << (r & 31));
                }
            } else {
                atomicAdd(const_cast<int32_t*>(L.R.mlNObs) + E.item, fuse_obs_weight(FUSE_LINE, 0));
            }
        }
    }
    L.action[e] = (uint8_t)action;
}

/* the class of an entry among the head words, or -1 */
__device__ inline int entry_class(const InsertLaunch& L, int32_t e, int32_t total)
{
    if (e >= total) return -1;
    const int a = L.action[e];
    if (a != INS_ADDED && a != INS_RECENT) return -1;
    const int line = e >= L.segOff[L.n] ? 2 : 0;
    return line + (a == INS_ADDED ? INSERT_HEAD_ADDED_P : INSERT_HEAD_RECENT_P);
}

__global__ __launch_bounds__(INSERT_TILE) void k_insert_count(InsertLaunch L, int32_t total)
{
    const int c = entry_class(L, blockIdx.x * INSERT_TILE + threadIdx.x, total);
    InsertGroup G;
    for (int k = 0; k < INSERT_HEAD_WORDS; k++) G.v[k] = __syncthreads_count(c == k);
    if (threadIdx.x == 0) L.group[blockIdx.x] = G;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_insert_scan(InsertLaunch L, int groups)
{
    __shared__ int32_t sh[LMAP_THREADS];
    int32_t carry[INSERT_HEAD_WORDS] = {0, 0, 0, 0};
    for (int base = 0; base < groups; base += LMAP_THREADS) {
        const int g = base + threadIdx.x;
        InsertGroup G = {};
        if (g < groups) G = L.group[g];
        for (int k = 0; k < INSERT_HEAD_WORDS; k++) {
            int32_t total;
            const int32_t before = block_excl_scan(G.v[k], sh, &total);
            G.v[k] = carry[k] + before;
            carry[k] += total;
        }
        if (g < groups) L.group[g] = G;
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < INSERT_HEAD_WORDS; k++) L.head[k] = carry[k];
}

__global__ __launch_bounds__(INSERT_TILE) void k_insert_pack(InsertLaunch L, int32_t total)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    const int32_t e = blockIdx.x * INSERT_TILE + threadIdx.x;
    const int c = entry_class(L, e, total);
    const InsertGroup G = L.group[blockIdx.x];
    for (int k = 0; k < INSERT_HEAD_WORDS; k++) {
        int tot;
        unsigned long long ballot;
        const int r = block_rank(c == k, shWave, &tot, &ballot);
        if (c != k) continue;
        const int kind = k >> 1;
        if (k & 1) L.recent[kind][G.v[k] + r] = entry_of(L, e).item;
        else L.addEntry[kind][G.v[k] + r] = e;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_insert_normals(InsertLaunch L)
{
    const int32_t count = L.head[INSERT_HEAD_ADDED_P];
    for (int32_t t = blockIdx.x * LMAP_THREADS + threadIdx.x; t < count; t += gridDim.x * LMAP_THREADS) {
        const Entry E = entry_of(L, L.addEntry[FUSE_POINT][t]);
        const InsAdders A{L.adders + (size_t)E.item * (size_t)L.words, L.words, L.byRank, L.called, E.j};
        float nrm[3], maxD, minD;
        const uint8_t status = ins_point_normal(L.G, L.I.obsOff, L.I.obs, A, E.item, nrm, &maxD, &minD);
        for (int k = 0; k < 3; k++) L.nrm[3 * (size_t)t + k] = nrm[k];
        L.maxD[t] = maxD;
        L.minD[t] = minD;
        L.status[t] = status;
    }
}

int groups_of(int32_t n) { return (n + INSERT_TILE - 1) / INSERT_TILE; }

}  // namespace

hipError_t drfe_launch_insert_chunk(const InsertLaunch& L, const int32_t* hostSegOff, hipStream_t s)
{
    /* the chunk's point rows and its line rows are two runs of the entry space */
    for (int kind = 0; kind < 2; kind++) {
        const int32_t e0 = hostSegOff[kind * L.n + L.j0], e1 = hostSegOff[kind * L.n + L.j1];
        if (e1 > e0) hipLaunchKernelGGL(k_insert_claim, dim3(groups_of(e1 - e0)), dim3(INSERT_TILE), 0, s, L, e0, e1);
    }
    for (int kind = 0; kind < 2; kind++) {
        const int32_t e0 = hostSegOff[kind * L.n + L.j0], e1 = hostSegOff[kind * L.n + L.j1];
        if (e1 > e0) hipLaunchKernelGGL(k_insert_verdict, dim3(groups_of(e1 - e0)), dim3(INSERT_TILE), 0, s, L, e0, e1);
    }
    return hipGetLastError();
}

hipError_t drfe_launch_insert_finish(const InsertLaunch& L, const int32_t* hostSegOff, hipStream_t s)
{
    const int32_t total = hostSegOff[2 * L.n];
    if (total <= 0) return hipSuccess;
    const int groups = groups_of(total);
    hipLaunchKernelGGL(k_insert_count, dim3(groups), dim3(INSERT_TILE), 0, s, L, total);
    hipLaunchKernelGGL(k_insert_scan, dim3(1), dim3(LMAP_THREADS), 0, s, L, groups);
    hipLaunchKernelGGL(k_insert_pack, dim3(groups), dim3(INSERT_TILE), 0, s, L, total);
    if (L.normals && hostSegOff[L.n] > 0) {
        const int want = groups_of(hostSegOff[L.n]);
        hipLaunchKernelGGL(k_insert_normals, dim3(want < INSERT_NORMAL_GROUPS ? want : INSERT_NORMAL_GROUPS), dim3(LMAP_THREADS), 0, s, L);
    }
    return hipGetLastError();
}
