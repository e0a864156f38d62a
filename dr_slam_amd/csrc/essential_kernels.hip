/* essential_kernels.hip — what surrounds the solver of Optimizer::OptimizeEssentialGraph on the device.
 *
 * The edge builder:
 *   k_ess_vertices  a lane per vertex: vScw from its row of the corrected table or its stored pose, the non-corrected Sim3, both
 *                   inverses (ess_vertex of essential_core.h), and vScw as the vertex's record.
 *   k_ess_units     one wavefront per unit.  A row of LoopConnections: a lane per member, the weight test by binary search in the
 *                   key's weights row.  A key frame of the map: its parent, its loop-edge row (a lane per member, smaller handles
 *                   kept), then its ordered row - the first entry below 100 by ballot, the end() rule, a lane per prefix entry with
 *                   binary searches in the children row, the loop-edge row and the pair list of the loop connections.  The rank of
 *                   a kept entry among the wavefront's ballot keeps the in-row order; the descriptors (other end, kind) go to the
 *                   unit's region of the host's bound, the count and the emptied flag to the unit's words.
 *   k_ess_scan      one workgroup: the exclusive prefix of the counts over the units in order, the total, the emptied prefixes.
 *   k_ess_write     a lane per edge of the total: its unit by binary search in the prefix, its descriptor, Sji = Sjw * Swi in f64
 *                   (ess_measure), its record at its place in the reference's addEdge order.
 * The commit:
 *   k_ess_poses     a lane per stored key frame: a named one gets vScw, vCorrectedSwc, its pose and centre in place in the
 *                   resident geometry and its record (ess_pose); any other the default-constructed pair.
 *   k_ess_points    a lane per point slot of the chunk: nIDr (its handle into a slot by binary search), the two maps, the position
 *                   in place, UpdateNormalAndDepth over its observers at the centres the launch before left, and its record at
 *                   the workgroup's offset (the host's count) plus its rank among the workgroup's ballots: ascending slot.
 *
 * The hand-offs are the launches, in stream order.  A unit's descriptors are its wavefront's, an edge and a point are their lane's,
 * a key frame is named once: no two lanes write one item.  Every index is inside what the host sized: a unit writes at most its
 * bound (one descriptor per row entry), an edge below the total, a record below pkCap. */
#include "lmap_device.h"

namespace {

__global__ __launch_bounds__(LMAP_THREADS) void k_ess_vertices(EssEdgesLaunch L)
{
    const int v = blockIdx.x * LMAP_THREADS + threadIdx.x;
    if (v >= L.nV) return;
    const size_t s = (size_t)L.vert[v];
    const int32_t row = L.tab[s];
    EssKf K;
    ess_vertex(row < 0 ? nullptr : L.corrected + 8 * (size_t)row, row < 0 ? nullptr : L.nonCorrected + 8 * (size_t)row, L.G.kfTcw + 16 * s, K);
    L.kf[s] = K;
    corr_sim3_to8(K.scw, L.outScw + 8 * (size_t)v);
}

/* the kept lanes of one pass write their descriptors behind the n the unit has so far; returns their number */
__device__ inline int ess_emit(const EssEdgesLaunch& L, int32_t base, int32_t room, int n, bool keep, int32_t other, int kind, int lane)
{
    const unsigned long long b = __ballot(keep);
    const int at = n + __popcll(b & ((1ull << lane) - 1ull));
    if (keep && at < room) {
        L.dTo[base + at] = other;
        L.dKind[base + at] = (uint8_t)kind;
    }
    return __popcll(b);
}

__global__ __launch_bounds__(LMAP_THREADS) void k_ess_units(EssEdgesLaunch L)
{
    const int lane = threadIdx.x & (ESS_WAVE - 1);
    const int u = blockIdx.x * ESS_WAVES + (threadIdx.x >> 6);
    if (u >= L.nU) return;                             /* the whole wavefront leaves */
    const int32_t base = L.capOff[u], room = L.capOff[u + 1] - base;
    int n = 0, emptied = 0;
    if (u < L.nLc) {
        const int32_t i = L.lcKey[u], e0 = L.lcOff[u], len = L.lcOff[u + 1] - e0;
        for (int32_t p = 0; p < len; p += ESS_WAVE) {
            const int32_t e = p + lane;
            const int32_t j = e < len ? L.lcKf[e0 + e] : -1;
            const bool keep = e < len && ess_lc_kept(L.C.wOff, L.C.wKf, L.C.wW, i, j, L.cur, L.loop);
            n += ess_emit(L, base, room, n, keep, j, ESS_KIND_LOOP_CONNECTION, lane);
        }
    } else {
        const int32_t i = L.vert[u - L.nLc], pa = L.I.kfParent[i];
        if (pa >= 0) n += ess_emit(L, base, room, n, lane == 0, pa, ESS_KIND_SPANNING_TREE, lane);
        const int32_t l0 = L.E.leOff[i], nLe = L.E.leOff[i + 1] - l0, hi = L.kfHandle[i];
        for (int32_t p = 0; p < nLe; p += ESS_WAVE) {
            const int32_t e = p + lane;
            const int32_t m = e < nLe ? L.E.le[l0 + e] : -1;
            const bool keep = e < nLe && L.kfHandle[m] < hi;
            n += ess_emit(L, base, room, n, keep, m, ESS_KIND_LOOP_EDGE, lane);
        }
        const int32_t o0 = L.C.oOff[i], len = L.C.oOff[i + 1] - o0;
        int32_t first = len;
        for (int32_t p = 0; p < len; p += ESS_WAVE) {
            const int32_t e = p + lane;
            const unsigned long long below = __ballot(e < len && L.C.oW[o0 + e] < ESS_MIN_FEAT);
            if (below) {
                first = p + __ffsll((long long)below) - 1;
                break;
            }
        }
        const int32_t pre = ess_prefix(first, len);
        emptied = len > 0 && first == len;
        const int32_t c0 = L.I.childOff[i], nCh = L.I.childOff[i + 1] - c0;
        for (int32_t p = 0; p < pre; p += ESS_WAVE) {
            const int32_t e = p + lane;
            const int32_t other = e < pre ? L.C.oKf[o0 + e] : -1;
            const bool keep = e < pre && ess_covis_kept(L.I.child + c0, nCh, L.E.le + l0, nLe, L.I.kfBad, L.kfHandle, pa, i, other) &&
                              !ess_inserted(L.pairKey, L.pairI, L.pairJ, L.nPairs, L.C.wOff, L.C.wKf, L.C.wW, i, other, L.cur, L.loop);
            n += ess_emit(L, base, room, n, keep, other, ESS_KIND_COVISIBILITY, lane);
        }
    }
    if (lane == 0) {
        L.cnt[u] = n < room ? n : room;
        L.emptied[u] = (uint8_t)emptied;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_ess_scan(EssEdgesLaunch L)
{
    __shared__ int32_t sh[LMAP_THREADS];
    const int tid = threadIdx.x;
    int32_t carry = 0, empt = 0;
    for (int j0 = 0; j0 < L.nU; j0 += LMAP_THREADS) {
        const int j = j0 + tid;
        const int32_t v = j < L.nU ? L.cnt[j] : 0;
        int32_t tot;
        const int32_t ex = block_excl_scan(v, sh, &tot);
        if (j < L.nU) L.cnt[j] = carry + ex;
        carry += tot;
        block_excl_scan(j < L.nU ? (int32_t)L.emptied[j] : 0, sh, &tot);
        empt += tot;
    }
    if (tid == 0) {
        L.cnt[L.nU] = carry;
        L.cnt[L.nU + 1] = empt;
    }
}

__global__ __launch_bounds__(LMAP_THREADS) void k_ess_write(EssEdgesLaunch L, int32_t total)
{
    const int e = blockIdx.x * ESS_TILE + threadIdx.x;
    if (e >= total || e >= L.bound) return;
    /* the last unit whose offset is not above e: cnt[0 .. nU] ascends, units without edges repeat an offset */
    int32_t lo = 0, hi = L.nU;
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (L.cnt[mid] <= e) lo = mid;
        else hi = mid;
    }
    const int32_t u = lo, d = L.capOff[u] + (e - L.cnt[u]);
    if (d < 0 || d >= L.bound) return;
    const int32_t i = u < L.nLc ? L.lcKey[u] : L.vert[u - L.nLc], j = L.dTo[d];
    const int kind = L.dKind[d];
    double m[8];
    ess_measure(L.kf[i], L.kf[j], kind, m);
    L.eFrom[e] = i;
    L.eTo[e] = j;
    for (int k = 0; k < 8; k++) L.eMeas[8 * (size_t)e + k] = m[k];
    L.eKind[e] = (uint8_t)kind;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_ess_poses(EssCommitLaunch L)
{
    const int s = blockIdx.x * LMAP_THREADS + threadIdx.x;
    if (s >= L.I.nK) return;
    const int32_t a = L.posOf[s];
    EssMove M;
    ess_identity(M.scw);
    ess_identity(M.swc);
    if (a >= 0) {
        float T[16], Ow[3];
        double w[8];
        corr_sim3_from8(L.scw + 8 * (size_t)a, M.scw);
        ess_pose(L.optimised + 8 * (size_t)a, M.swc, T, Ow);
        corr_sim3_to8(M.swc, w);
        for (int k = 0; k < 16; k++) {
            L.G.kfTcw[16 * (size_t)s + k] = T[k];
            L.outTiw[16 * (size_t)a + k] = T[k];
        }
        for (int k = 0; k < 3; k++) L.G.kfOw[3 * (size_t)s + k] = Ow[k];
        for (int k = 0; k < 8; k++) L.outSwc[8 * (size_t)a + k] = w[k];
    }
    L.mv[s] = M;
}

__global__ __launch_bounds__(LMAP_THREADS) void k_ess_points(EssCommitLaunch L)
{
    __shared__ int32_t shWave[LMAP_THREADS / 64];
    const int q = blockIdx.x * ESS_TILE + threadIdx.x, n = L.p1 - L.p0;
    const size_t p = (size_t)(L.p0 + (q < n ? q : 0));
    bool moves = q < n && !L.I.mpBad[p];
    int32_t idr = 0, r = -1;
    if (moves) {
        /* the host has refused the call where either lookup would miss */
        const int32_t ref = L.G.mpRef[p];
        idr = ess_ref_handle(L.G.mpBy[p], L.G.mpByRef[p], ref >= 0 ? L.kfHandle[ref] : -1, L.cur);
        const int32_t k = ess_find(L.hSorted, L.I.nK, idr);
        r = k >= 0 ? L.hSlot[k] : -1;
        if (ref < 0 || r < 0) moves = false;
    }
    float Xn[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f}, maxD = 0.0f, minD = 0.0f;
    uint8_t st = 0;
    if (moves) {
        float X[3];
        for (int k = 0; k < 3; k++) X[k] = L.G.mpWorld[3 * p + k];
        const EssMove M = L.mv[r];
        corr_point(M.scw, M.swc, X, Xn);
        for (int k = 0; k < 3; k++) L.G.mpWorld[3 * p + k] = Xn[k];
        st = ess_normal(L.G, L.G.kfOw, L.I.obsOff, L.I.obs, (int32_t)p, Xn, nrm, &maxD, &minD);
    }
    int tot;
    unsigned long long b;
    const int rank = block_rank(moves, shWave, &tot, &b);
    if (!moves) return;
    const size_t o = (size_t)(L.grpOff[blockIdx.x] + rank);
    if (o >= (size_t)L.pkCap) return;                  /* the host counted fewer: it sized the arrays from its own count */
    L.pkItem[o] = (int32_t)p;
    L.pkRef[o] = idr;
    for (int k = 0; k < 3; k++) {
        L.pkWorld[3 * o + k] = Xn[k];
        L.pkNormal[3 * o + k] = nrm[k];
    }
    L.pkMax[o] = maxD;
    L.pkMin[o] = minD;
    L.pkStatus[o] = st;
}

int groups(int n) { return (n + LMAP_THREADS - 1) / LMAP_THREADS; }

}  // namespace

hipError_t drfe_launch_essential_plan(const EssEdgesLaunch& L, hipStream_t s)
{
    if (L.nV > 0) hipLaunchKernelGGL(k_ess_vertices, dim3(groups(L.nV)), dim3(LMAP_THREADS), 0, s, L);
    if (L.nU > 0) hipLaunchKernelGGL(k_ess_units, dim3((L.nU + ESS_WAVES - 1) / ESS_WAVES), dim3(LMAP_THREADS), 0, s, L);
    hipLaunchKernelGGL(k_ess_scan, dim3(1), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}

hipError_t drfe_launch_essential_write(const EssEdgesLaunch& L, int32_t total, hipStream_t s)
{
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ess_write, dim3(groups(total)), dim3(LMAP_THREADS), 0, s, L, total);
    return hipGetLastError();
}

hipError_t drfe_launch_essential_poses(const EssCommitLaunch& L, hipStream_t s)
{
    if (L.I.nK <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ess_poses, dim3(groups(L.I.nK)), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}

hipError_t drfe_launch_essential_points(const EssCommitLaunch& L, hipStream_t s)
{
    const int n = L.p1 - L.p0;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ess_points, dim3(groups(n)), dim3(LMAP_THREADS), 0, s, L);
    return hipGetLastError();
}
