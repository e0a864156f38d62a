/* map_upkeep.cpp — MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth and MapLine::ComputeDistinctiveDescriptors /
 * UpdateAverageDir (reference src/MapPoint.cc:288-411, src/MapLine.cpp:241-362) behind the C-ABI of include/drfe.h: the two
 * host entries (no context) and the two batch entries (map_upkeep_kernels.hip).  Both sides evaluate map_upkeep_core.h;
 * DESIGN.md section 14. */
#include "map_upkeep_internal.h"
#include "map_upkeep_core.h"
#include "hip_buf.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

struct MuBuffers {
    PinnedBuf<char> hin, hout;         /* staging: one copy each way */
    DevBuf<char> din, dout;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

void drfe_map_upkeep_free(drfe_ctx* c)
{
    delete c->mu;
    c->mu = nullptr;
}

namespace {

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

bool kf_bad(const drfe_upkeep_keyframes* k, int32_t kf) { return k->bad && k->bad[kf]; }

bool active(const drfe_upkeep_items* it, int i)
{
    return !(it->bad && it->bad[i]) && it->obs_offsets[i + 1] > it->obs_offsets[i];
}

/* all-or-nothing validation of a call */
int check_args(int what, const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, const drfe_upkeep_out* o, std::string& err)
{
    err = "map_upkeep: invalid argument";
    if (what < 1 || what > 3 || !k || !it || !o || it->n < 0 || k->n < 0) return DRFE_ERR_INVALID;
    if (it->n == 0) return DRFE_OK;
    if (!o->status || !it->obs_offsets || it->obs_offsets[0] != 0) return DRFE_ERR_INVALID;
    for (int i = 0; i < it->n; i++)
        if (it->obs_offsets[i + 1] < it->obs_offsets[i]) { err = "map_upkeep: decreasing obs_offsets"; return DRFE_ERR_INVALID; }
    const int T = it->obs_offsets[it->n];
    if (T > 0 && !it->obs_kf) return DRFE_ERR_INVALID;
    for (int q = 0; q < T; q++)
        if (it->obs_kf[q] < 0 || it->obs_kf[q] >= k->n) { err = "map_upkeep: obs_kf out of range"; return DRFE_ERR_INVALID; }
    if ((what & DRFE_UPKEEP_DESCRIPTOR) && T > 0 && !it->obs_desc) return DRFE_ERR_INVALID;
    if (what & DRFE_UPKEEP_NORMAL) {
        if (!it->world || !it->ref_kf || !it->ref_level || !k->scale_factors || k->n_levels < 1 || (k->n > 0 && !k->center))
            return DRFE_ERR_INVALID;
        for (int i = 0; i < it->n; i++) {
            if (!active(it, i)) continue;
            if (it->ref_kf[i] < 0 || it->ref_kf[i] >= k->n || it->ref_level[i] < 0 || it->ref_level[i] >= k->n_levels) {
                err = "map_upkeep: ref_kf or ref_level out of range";
                return DRFE_ERR_INVALID;
            }
        }
    }
    return DRFE_OK;
}

/* ComputeDistinctiveDescriptors of item i on the host: the rows of non-bad keyframes in order, every distance, each row's
 * median by counting (the k-th smallest of integers in [0, 256]), the first strict minimum.  -1 when there is no row. */
int best_obs_host(const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, int i, std::vector<uint32_t>& rows,
                  std::vector<int32_t>& obs, std::vector<uint16_t>& D)
{
    rows.clear();
    obs.clear();
    const int o0 = it->obs_offsets[i], o1 = it->obs_offsets[i + 1];
    for (int q = o0; q < o1; q++) {
        if (kf_bad(k, it->obs_kf[q])) continue;
        uint32_t w[8];
        std::memcpy(w, it->obs_desc + 32 * (size_t)q, 32);
        rows.insert(rows.end(), w, w + 8);
        obs.push_back(q - o0);
    }
    const int N = (int)obs.size();
    if (!N) return -1;
    D.assign((size_t)N * N, 0);
    for (int a = 0; a < N; a++)
        for (int b = a + 1; b < N; b++)
            D[(size_t)a * N + b] = D[(size_t)b * N + a] = (uint16_t)mu_hamming(&rows[8 * (size_t)a], &rows[8 * (size_t)b]);
    const int kth = mu_median_rank(N);
    uint32_t bestKey = 0xFFFFFFFFu;
    for (int a = 0; a < N; a++) {
        int hist[257] = {0};
        for (int b = 0; b < N; b++) hist[D[(size_t)a * N + b]]++;
        int v = 0, acc = hist[0];
        while (acc <= kth) acc += hist[++v];
        bestKey = std::min(bestKey, mu_key(v, a));
    }
    return (int)(bestKey & 0xFFFFu);
}

/* item i's descriptor half into the outputs (best_obs / desc; -1 and zeros when unchanged) */
void desc_host(const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, int i, const drfe_upkeep_out* o, std::vector<uint32_t>& rows,
               std::vector<int32_t>& obs, std::vector<uint16_t>& D)
{
    const int r = active(it, i) ? best_obs_host(k, it, i, rows, obs, D) : -1;
    if (o->best_obs) o->best_obs[i] = r < 0 ? -1 : obs[r];
    if (o->desc) {
        if (r < 0) std::memset(o->desc + 32 * (size_t)i, 0, 32);
        else std::memcpy(o->desc + 32 * (size_t)i, &rows[8 * (size_t)r], 32);
    }
    if (r >= 0) o->status[i] |= DRFE_UPKEEP_DESCRIPTOR;
}

/* item i's normal half (zeros when not computed) */
template <bool Line>
void normal_host(int what, const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, int i, const drfe_upkeep_out* o)
{
    typedef typename std::conditional<Line, double, float>::type T;
    T nrm[3] = {0, 0, 0};
    float maxD = 0.f, minD = 0.f;
    const bool on = (what & DRFE_UPKEEP_NORMAL) && active(it, i);
    const int o0 = it->obs_offsets[i], o1 = it->obs_offsets[i + 1];
    if (on) {
        const float* OwRef = k->center + 3 * (size_t)it->ref_kf[i];
        const float levelScale = k->scale_factors[it->ref_level[i]], lastScale = k->scale_factors[k->n_levels - 1];
        if constexpr (Line) {
            const double* P = static_cast<const double*>(it->world) + 6 * (size_t)i;
            double* n = reinterpret_cast<double*>(nrm);
            for (int q = o0; q < o1; q++) mu_line_obs(n, P, k->center + 3 * (size_t)it->obs_kf[q]);
            mu_line_finish(n, o1 - o0, P, OwRef, levelScale, lastScale, &maxD, &minD);
        } else {
            const float* X = static_cast<const float*>(it->world) + 3 * (size_t)i;
            float* n = reinterpret_cast<float*>(nrm);
            for (int q = o0; q < o1; q++) mu_point_obs(n, X, k->center + 3 * (size_t)it->obs_kf[q]);
            mu_point_finish(n, o1 - o0, X, OwRef, levelScale, lastScale, &maxD, &minD);
        }
        o->status[i] |= DRFE_UPKEEP_NORMAL;
    }
    if (o->normal) std::memcpy(static_cast<T*>(o->normal) + 3 * (size_t)i, nrm, sizeof(nrm));
    if (o->max_distance) o->max_distance[i] = maxD;
    if (o->min_distance) o->min_distance[i] = minD;
    if (o->frustum) {
        if constexpr (Line) {
            drfe_frustum_line& f = static_cast<drfe_frustum_line*>(o->frustum)[i];
            std::memset(&f, 0, sizeof(f));
            if (on) std::memcpy(f.world, static_cast<const double*>(it->world) + 6 * (size_t)i, 48);
            std::memcpy(f.normal, nrm, sizeof(nrm));
            f.min_distance = 0.8f * minD;
            f.max_distance = 1.2f * maxD;
        } else {
            drfe_frustum_point& f = static_cast<drfe_frustum_point*>(o->frustum)[i];
            std::memset(&f, 0, sizeof(f));
            if (on) std::memcpy(f.world, static_cast<const float*>(it->world) + 3 * (size_t)i, 12);
            std::memcpy(f.normal, nrm, sizeof(nrm));
            f.min_distance = 0.8f * minD;
            f.max_distance = 1.2f * maxD;
        }
    }
}

template <bool Line>
int upkeep_host(int what, const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, drfe_upkeep_out* o)
{
    std::string err;
    const int rc = check_args(what, k, it, o, err);
    if (rc) return rc;
    std::vector<uint32_t> rows;
    std::vector<int32_t> obs;
    std::vector<uint16_t> D;
    for (int i = 0; i < it->n; i++) {
        o->status[i] = 0;
        if (what & DRFE_UPKEEP_DESCRIPTOR) {
            desc_host(k, it, i, o, rows, obs, D);
        } else {
            if (o->best_obs) o->best_obs[i] = -1;
            if (o->desc) std::memset(o->desc + 32 * (size_t)i, 0, 32);
        }
        normal_host<Line>(what, k, it, i, o);
    }
    return DRFE_OK;
}

/* the device path: one staging copy, four kernels at most, one copy back; descriptors of items above the device's row cap
 * are computed here while the kernels run */
template <bool Line>
int upkeep_batch(drfe_ctx* c, int what, const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, drfe_upkeep_out* o, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    int rc = check_args(what, k, it, o, c->err);
    if (rc) return rc;
    MuBuffers* b = c->mu;
    if (!b) { b = new MuBuffers(); c->mu = b; }
    b->stats[0]++;
    const int n = it->n;
    if (n == 0) return DRFE_OK;
    b->stats[1] += n;
    const int T = it->obs_offsets[n];
    const bool wantDesc = (what & DRFE_UPKEEP_DESCRIPTOR) != 0, wantNormal = (what & DRFE_UPKEEP_NORMAL) != 0;
    /* plan: items, their rows, the buckets */
    std::vector<MuItem> items((size_t)n);
    std::vector<int32_t> lists[MU_BUCKETS], hostDesc;
    int64_t R = 0;
    int maxWg = 0;
    for (int i = 0; i < n; i++) {
        MuItem& m = items[(size_t)i];
        const int o0 = it->obs_offsets[i], o1 = it->obs_offsets[i + 1];
        m = MuItem{o0, o1 - o0, 0, 0, 0, 0, 0, 0};
        if (!active(it, i)) continue;
        m.flags = MU_ACTIVE;
        if (wantNormal) { m.refKf = it->ref_kf[i]; m.level = it->ref_level[i]; }
        if (!wantDesc) continue;
        int nr = 0;
        for (int q = o0; q < o1; q++) nr += kf_bad(k, it->obs_kf[q]) ? 0 : 1;
        if (!nr) continue;
        m.flags |= MU_HAS_ROWS;
        if (nr > DRFE_UPKEEP_DEVICE_ROWS) { hostDesc.push_back(i); continue; }
        m.flags |= MU_DEVICE_DESC;
        m.row0 = (int32_t)R;
        m.nrows = nr;
        R += nr;
        const int bk = nr <= 4 ? MU_B4 : nr <= 16 ? MU_B16 : nr <= 64 ? MU_B64 : MU_BWG;
        lists[bk].push_back(i);
        if (bk == MU_BWG) maxWg = std::max(maxWg, nr);
    }
    if (R > INT32_MAX / 32) { c->err = "map_upkeep: too many descriptor rows in one call"; return DRFE_ERR_CAPACITY; }
    /* staging layout (16-byte aligned sections) */
    const size_t wsz = Line ? 48 : 12, nsz = Line ? 24 : 12, fsz = Line ? sizeof(drfe_frustum_line) : sizeof(drfe_frustum_point);
    const size_t oItems = 0, oCent = align16(oItems + (size_t)n * sizeof(MuItem)), oScale = align16(oCent + (size_t)k->n * 12),
                 oWorld = align16(oScale + (wantNormal ? (size_t)k->n_levels * 4 : 0)),
                 oObsKf = align16(oWorld + (wantNormal ? (size_t)n * wsz : 0)), oRows = align16(oObsKf + (wantNormal ? (size_t)T * 4 : 0)),
                 oRowObs = align16(oRows + (size_t)R * 32), oLists = align16(oRowObs + (size_t)R * 4);
    size_t oList[MU_BUCKETS], inEnd = oLists;
    for (int bk = 0; bk < MU_BUCKETS; bk++) { oList[bk] = inEnd; inEnd = align16(inEnd + lists[bk].size() * 4); }
    const size_t pBest = 0, pDesc = align16((size_t)n * 4), pNormal = align16(pDesc + (size_t)n * 32), pMax = align16(pNormal + (size_t)n * nsz),
                 pMin = align16(pMax + (size_t)n * 4), pStatus = align16(pMin + (size_t)n * 4), pFrustum = align16(pStatus + (size_t)n),
                 outEnd = align16(pFrustum + (o->frustum ? (size_t)n * fsz : 0));
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, b->hin.grow(inEnd));
    HIPCHK(c, b->din.grow(inEnd));
    HIPCHK(c, b->hout.grow(outEnd));
    HIPCHK(c, b->dout.grow(outEnd));
    char* h = b->hin;
    std::memcpy(h + oItems, items.data(), (size_t)n * sizeof(MuItem));
    if (wantNormal) {
        if (k->n) std::memcpy(h + oCent, k->center, (size_t)k->n * 12);
        std::memcpy(h + oScale, k->scale_factors, (size_t)k->n_levels * 4);
        std::memcpy(h + oWorld, it->world, (size_t)n * wsz);
        if (T) std::memcpy(h + oObsKf, it->obs_kf, (size_t)T * 4);
    }
    for (int bk = 0; bk < MU_BUCKETS; bk++) {
        if (!lists[bk].empty()) std::memcpy(h + oList[bk], lists[bk].data(), lists[bk].size() * 4);
        for (int i : lists[bk]) {
            const MuItem& m = items[(size_t)i];
            char* rd = h + oRows + 32 * (size_t)m.row0;
            int32_t* ro = reinterpret_cast<int32_t*>(h + oRowObs) + m.row0;
            for (int q = m.obs0, r = 0; q < m.obs0 + m.nobs; q++) {
                if (kf_bad(k, it->obs_kf[q])) continue;
                std::memcpy(rd + 32 * (size_t)r, it->obs_desc + 32 * (size_t)q, 32);
                ro[r++] = q - m.obs0;
            }
        }
    }
    char* d = b->din;
    char* dO = b->dout;
    HIPCHK(c, hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, s));
    MuLaunch L{};
    L.items = reinterpret_cast<const MuItem*>(d + oItems);
    L.n = n; L.what = what; L.line = Line ? 1 : 0; L.nLevels = k->n_levels;
    L.kfCenter = reinterpret_cast<const float*>(d + oCent);
    L.scale = reinterpret_cast<const float*>(d + oScale);
    L.world = d + oWorld;
    L.obsKf = reinterpret_cast<const int32_t*>(d + oObsKf);
    L.rows = reinterpret_cast<const uint4*>(d + oRows);
    L.rowObs = reinterpret_cast<const int32_t*>(d + oRowObs);
    for (int bk = 0; bk < MU_BUCKETS; bk++) {
        L.list[bk] = reinterpret_cast<const int32_t*>(d + oList[bk]);
        L.count[bk] = (int)lists[bk].size();
    }
    L.maxRowsWg = maxWg;
    L.best = reinterpret_cast<int32_t*>(dO + pBest);
    L.desc = reinterpret_cast<uint4*>(dO + pDesc);
    L.normal = dO + pNormal;
    L.maxD = reinterpret_cast<float*>(dO + pMax);
    L.minD = reinterpret_cast<float*>(dO + pMin);
    L.status = reinterpret_cast<uint8_t*>(dO + pStatus);
    L.frustum = o->frustum ? dO + pFrustum : nullptr;
    hipError_t e = drfe_launch_map_upkeep(L, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b->hout, dO, outEnd, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { c->err = std::string("map_upkeep batch: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
    /* the host's share while the device works: descriptors of items above the row cap */
    std::vector<uint32_t> rows;
    std::vector<int32_t> obs, bestH((size_t)hostDesc.size());
    std::vector<uint16_t> D;
    std::vector<uint8_t> descH(32 * hostDesc.size());
    for (size_t q = 0; q < hostDesc.size(); q++) {
        const int r = best_obs_host(k, it, hostDesc[q], rows, obs, D);
        bestH[q] = obs[r];
        std::memcpy(&descH[32 * q], &rows[8 * (size_t)r], 32);
    }
    HIPCHK(c, hipStreamSynchronize(s));
    const char* ho = b->hout;
    if (o->best_obs) std::memcpy(o->best_obs, ho + pBest, (size_t)n * 4);
    if (o->desc) std::memcpy(o->desc, ho + pDesc, (size_t)n * 32);
    if (o->normal) std::memcpy(o->normal, ho + pNormal, (size_t)n * nsz);
    if (o->max_distance) std::memcpy(o->max_distance, ho + pMax, (size_t)n * 4);
    if (o->min_distance) std::memcpy(o->min_distance, ho + pMin, (size_t)n * 4);
    std::memcpy(o->status, ho + pStatus, (size_t)n);
    if (o->frustum) std::memcpy(o->frustum, ho + pFrustum, (size_t)n * fsz);
    for (size_t q = 0; q < hostDesc.size(); q++) {
        if (o->best_obs) o->best_obs[hostDesc[q]] = bestH[q];
        if (o->desc) std::memcpy(o->desc + 32 * (size_t)hostDesc[q], &descH[32 * q], 32);
    }
    for (int bk = 0; bk < MU_BUCKETS; bk++) b->stats[2 + bk] += (int64_t)lists[bk].size();
    b->stats[6] += (int64_t)hostDesc.size();
    if (wantNormal)
        for (int i = 0; i < n; i++) b->stats[7] += items[(size_t)i].flags & MU_ACTIVE ? 1 : 0;
    return DRFE_OK;
}

}  // namespace

extern "C" {

int drfe_map_point_upkeep_host(int what, const drfe_upkeep_keyframes* kfs, const drfe_upkeep_items* items, drfe_upkeep_out* out)
{
    return upkeep_host<false>(what, kfs, items, out);
}

int drfe_map_line_upkeep_host(int what, const drfe_upkeep_keyframes* kfs, const drfe_upkeep_items* items, drfe_upkeep_out* out)
{
    return upkeep_host<true>(what, kfs, items, out);
}

int drfe_map_point_upkeep_batch(drfe_ctx* ctx, int what, const drfe_upkeep_keyframes* kfs, const drfe_upkeep_items* items,
                                drfe_upkeep_out* out, void* stream)
{
    return upkeep_batch<false>(ctx, what, kfs, items, out, stream);
}

int drfe_map_line_upkeep_batch(drfe_ctx* ctx, int what, const drfe_upkeep_keyframes* kfs, const drfe_upkeep_items* items,
                               drfe_upkeep_out* out, void* stream)
{
    return upkeep_batch<true>(ctx, what, kfs, items, out, stream);
}

int drfe_map_upkeep_stats(drfe_ctx* c, int64_t* stats)
{
    if (!c || !stats) return DRFE_ERR_INVALID;
    if (c->mu) std::memcpy(stats, c->mu->stats, sizeof(c->mu->stats));
    else std::memset(stats, 0, 8 * sizeof(int64_t));
    return DRFE_OK;
}

}  // extern "C"
