/* map_upkeep.cpp — MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth and MapLine::ComputeDistinctiveDescriptors /
 * UpdateAverageDir (reference src/MapPoint.cc:288-411, src/MapLine.cpp:241-362) behind the C-ABI of include/drfe.h: the two
 * host entries (no context) and the two batch entries (map_upkeep_kernels.hip).  Both sides evaluate map_upkeep_core.h;
 * DESIGN.md section 14. */
#include "map_upkeep_internal.h"
#include "map_upkeep_core.h"
#include "hip_buf.h"
#include "stage_layout.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

struct MuBuffers {
    StagePair io;                      /* staging: one copy each way */
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

void drfe_map_upkeep_free(drfe_ctx* c)
{
    delete c->mu;
    c->mu = nullptr;
}

namespace {

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
    using W = std::conditional_t<Line, double, float>;          /* world coordinates and normals */
    using Fr = std::conditional_t<Line, drfe_frustum_line, drfe_frustum_point>;
    const size_t nn = (size_t)n, nNormal = wantNormal ? 1 : 0;
    StageLayout<16> in, out;
    const auto sItems = in.add<MuItem>(nn);
    const auto sCent = in.add<float>(nNormal * k->n * 3), sScale = in.add<float>(nNormal * k->n_levels);
    const auto sWorld = in.add<W>(nNormal * nn * (Line ? 6 : 3));
    const auto sObsKf = in.add<int32_t>(nNormal * T);
    const auto sRows = in.add<uint4>((size_t)R * 2);
    const auto sRowObs = in.add<int32_t>((size_t)R);
    Section<int32_t> sList[MU_BUCKETS];
    for (int bk = 0; bk < MU_BUCKETS; bk++) sList[bk] = in.add<int32_t>(lists[bk].size());
    const auto sBest = out.add<int32_t>(nn);
    const auto sDesc = out.add<uint4>(nn * 2);
    const auto sNormal = out.add<W>(nn * 3);
    const auto sMax = out.add<float>(nn), sMin = out.add<float>(nn);
    const auto sStatus = out.add<uint8_t>(nn);
    const auto sFrustum = out.add<Fr>(o->frustum ? nn : 0);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, b->io.grow(in.bytes(), out.bytes()));
    char* h = b->io.hin;
    sItems.put(h, items.data());
    sCent.put(h, k->center);
    sScale.put(h, k->scale_factors);
    sWorld.put(h, it->world);
    sObsKf.put(h, it->obs_kf);
    for (int bk = 0; bk < MU_BUCKETS; bk++) {
        sList[bk].put(h, lists[bk].data());
        for (int i : lists[bk]) {
            const MuItem& m = items[(size_t)i];
            uint4* rd = sRows.at(h) + 2 * (size_t)m.row0;
            int32_t* ro = sRowObs.at(h) + m.row0;
            for (int q = m.obs0, r = 0; q < m.obs0 + m.nobs; q++) {
                if (kf_bad(k, it->obs_kf[q])) continue;
                std::memcpy(rd + 2 * (size_t)r, it->obs_desc + 32 * (size_t)q, 32);
                ro[r++] = q - m.obs0;
            }
        }
    }
    const char* d = b->io.din;
    char* dO = b->io.dout;
    HIPCHK(c, hipMemcpyAsync(b->io.din, h, in.bytes(), hipMemcpyHostToDevice, s));
    MuLaunch L{};
    L.items = sItems.at(d);
    L.n = n; L.what = what; L.line = Line ? 1 : 0; L.nLevels = k->n_levels;
    L.kfCenter = sCent.at(d);
    L.scale = sScale.at(d);
    L.world = sWorld.at(d);
    L.obsKf = sObsKf.at(d);
    L.rows = sRows.at(d);
    L.rowObs = sRowObs.at(d);
    for (int bk = 0; bk < MU_BUCKETS; bk++) {
        L.list[bk] = sList[bk].at(d);
        L.count[bk] = (int)lists[bk].size();
    }
    L.maxRowsWg = maxWg;
    L.best = sBest.at(dO);
    L.desc = sDesc.at(dO);
    L.normal = sNormal.at(dO);
    L.maxD = sMax.at(dO);
    L.minD = sMin.at(dO);
    L.status = sStatus.at(dO);
    L.frustum = o->frustum ? sFrustum.at(dO) : nullptr;
    hipError_t e = drfe_launch_map_upkeep(L, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b->io.hout, dO, out.bytes(), hipMemcpyDeviceToHost, s);
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
    const char* ho = b->io.hout;
    sBest.get(ho, o->best_obs);
    sDesc.get(ho, o->desc);
    sNormal.get(ho, o->normal);
    sMax.get(ho, o->max_distance);
    sMin.get(ho, o->min_distance);
    sStatus.get(ho, o->status);
    sFrustum.get(ho, o->frustum);
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
