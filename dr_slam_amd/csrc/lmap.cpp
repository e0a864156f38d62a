/* lmap.cpp — Tracking::UpdateLocalMap (reference src/Tracking.cc:3383-3541) on the local-map store (lmap_store.h), behind the
 * C-ABI of include/drfe.h: the argument checks, the host walk, the device entry (lmap_kernels.hip) and the counters.  Both sides
 * read the same image and evaluate lmap_core.h.  A call is checked as a whole and committed only when its results fit the caller's
 * arrays.  DESIGN.md section 25. */
#include "lmap_call.h"

#include <algorithm>
#include <cstring>
#include <map>

using namespace lmap_store;

namespace {

/* a checked call, in slots */
struct Call {
    int n = 0;
    std::vector<int32_t> ptOff, pts, lnOff, lns, prevOff, prev;
    int64_t lastId = 0;
    int32_t maxPrev = 0, maxPts = 0;
};

struct Result {
    std::vector<int32_t> kfOff, kfs, ref, mpOff, mps, mlOff, mls, nuOff, nulled, record;
    std::vector<uint8_t> mpIn, mlIn;
    void start()
    {
        kfOff.assign(1, 0);
        mpOff.assign(1, 0);
        mlOff.assign(1, 0);
        nuOff.assign(1, 0);
    }
};

int slots_of(drfe_lmap* db, const std::unordered_map<int32_t, int32_t>& map, const int32_t* h, int n, bool allowNull, const char* what,
             std::vector<int32_t>& out)
{
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        if (h[i] == -1 && allowNull) {
            out[(size_t)i] = -1;
            continue;
        }
        const auto it = map.find(h[i]);
        if (it == map.end()) return lmap_fail(db, DRFE_ERR_INVALID, std::string("lmap: a query names an unknown ") + what + " handle");
        out[(size_t)i] = it->second;
    }
    return DRFE_OK;
}

int plan(drfe_lmap* db, const drfe_lmap_queries* q, const drfe_lmap_out* o, Call& C)
{
    if (!q || q->n < 0 || !o) return lmap_fail(db, DRFE_ERR_INVALID, "lmap: invalid argument");
    if (q->n > DRFE_LMAP_MAX_QUERIES) return lmap_fail(db, DRFE_ERR_INVALID, "lmap: more than DRFE_LMAP_MAX_QUERIES queries in a call");
    if (o->kf_capacity < 0 || o->mp_capacity < 0 || o->ml_capacity < 0 || o->nulled_capacity < 0 || !o->kf_offsets || !o->ref_kf ||
        !o->mp_offsets || !o->ml_offsets || !o->nulled_offsets || !o->record || (o->kf_capacity > 0 && !o->kfs) ||
        (o->mp_capacity > 0 && (!o->mps || !o->mp_in_frame)) || (o->ml_capacity > 0 && (!o->mls || !o->ml_in_frame)) ||
        (o->nulled_capacity > 0 && !o->nulled))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap: invalid output arrays");
    const int n = q->n;
    C.n = n;
    if (n == 0) return DRFE_OK;
    if (!q->frame_id) return lmap_fail(db, DRFE_ERR_INVALID, "lmap: invalid argument");
    int64_t last = db->lastId;
    for (int k = 0; k < n; k++) {
        if (q->frame_id[k] == 0 || q->frame_id[k] <= last)
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap: a frame id is 0 or does not exceed the last id used on this store");
        last = q->frame_id[k];
    }
    C.lastId = last;
    if (!lmap_offsets_ok(q->point_offsets, n) || (q->point_offsets[n] > 0 && !q->points))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap: point_offsets do not start at 0 or decrease");
    if (q->line_offsets && (!lmap_offsets_ok(q->line_offsets, n) || (q->line_offsets[n] > 0 && !q->lines)))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap: line_offsets do not start at 0 or decrease");
    if (q->prev_kf_offsets && (!lmap_offsets_ok(q->prev_kf_offsets, n) || (q->prev_kf_offsets[n] > 0 && !q->prev_kfs)))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap: prev_kf_offsets do not start at 0 or decrease");
    int rc = lmap_build_image(db);
    if (rc) return rc;
    const Image& G = db->img;
    C.ptOff.assign(q->point_offsets, q->point_offsets + n + 1);
    rc = slots_of(db, G.mpSlot, q->points, C.ptOff[(size_t)n], true, "map-point", C.pts);
    if (rc) return rc;
    if (q->line_offsets) {
        C.lnOff.assign(q->line_offsets, q->line_offsets + n + 1);
        rc = slots_of(db, G.mlSlot, q->lines, C.lnOff[(size_t)n], true, "map-line", C.lns);
        if (rc) return rc;
    } else {
        C.lnOff.assign((size_t)n + 1, 0);
    }
    if (q->prev_kf_offsets) {
        C.prevOff.assign(q->prev_kf_offsets, q->prev_kf_offsets + n + 1);
        rc = slots_of(db, G.kfSlot, q->prev_kfs, C.prevOff[(size_t)n], false, "key-frame", C.prev);
        if (rc) return rc;
    } else {
        C.prevOff.assign((size_t)n + 1, 0);
    }
    for (int k = 0; k < n; k++) {
        C.maxPrev = std::max(C.maxPrev, C.prevOff[(size_t)k + 1] - C.prevOff[(size_t)k]);
        C.maxPts = std::max(C.maxPts, C.ptOff[(size_t)k + 1] - C.ptOff[(size_t)k]);
    }
    return DRFE_OK;
}

/* the reference's loops, query after query, with stamps for mnTrackReferenceForFrame */
void run_host(drfe_lmap* db, const Call& C, Result& R)
{
    lmap_host_views(db);
    const LmapImage I = db->hView;
    const int n = C.n;
    R.start();
    R.ref.assign((size_t)n, -1);
    R.record.assign((size_t)n * 4, 0);
    std::vector<int32_t> votes((size_t)I.nK), list;
    std::vector<uint32_t> mark(((size_t)I.nK + 31) / 32);
    std::vector<int32_t>&stampP = db->stampP, &stampL = db->stampL, &inP = db->inP, &inL = db->inL;
    if (stampP.size() != (size_t)I.nP || stampL.size() != (size_t)I.nL || db->serial > 0x7fffffff - n) {
        stampP.assign((size_t)I.nP, 0);
        inP.assign((size_t)I.nP, 0);
        stampL.assign((size_t)I.nL, 0);
        inL.assign((size_t)I.nL, 0);
        db->serial = 0;
    }
    for (int q = 0; q < n; q++) {
        const int32_t k = ++db->serial;
        std::fill(votes.begin(), votes.end(), 0);
        for (int i = C.ptOff[(size_t)q]; i < C.ptOff[(size_t)q + 1]; i++) {
            const int32_t p = C.pts[(size_t)i];
            const int what = lmap_frame_point(p, I.mpBad);
            if (what == 2) R.nulled.push_back(i - C.ptOff[(size_t)q]);
            if (what != 1) continue;
            inP[(size_t)p] = k;
            for (int o = I.obsOff[p]; o < I.obsOff[p + 1]; o++) votes[(size_t)I.obs[o]]++;
        }
        R.nuOff.push_back((int32_t)R.nulled.size());
        for (int i = C.lnOff[(size_t)q]; i < C.lnOff[(size_t)q + 1]; i++)
            if (C.lns[(size_t)i] >= 0) inL[(size_t)C.lns[(size_t)i]] = k;
        int32_t counter = 0, bv = 0, bs = 0x7fffffff;
        list.clear();
        std::fill(mark.begin(), mark.end(), 0u);
        for (int32_t s = 0; s < I.nK; s++) {
            const int32_t v = votes[(size_t)s];
            if (v > 0) counter++;
            if (!lmap_listed(v, I.kfBad[s])) continue;
            if (lmap_better(v, s, bv, bs)) {
                bv = v;
                bs = s;
            }
            list.push_back(s);
            lmap_mark(mark.data(), s);
        }
        if (counter == 0) {
            list.assign(C.prev.begin() + C.prevOff[(size_t)q], C.prev.begin() + C.prevOff[(size_t)q + 1]);
        } else {
            const int32_t nListed = (int32_t)list.size();
            list.resize((size_t)I.nK);
            const int32_t added = lmap_expand(I, list.data(), nListed, mark.data());
            list.resize((size_t)(nListed + added));
            R.ref[(size_t)q] = bv > 0 ? bs : -1;
            R.record[4 * (size_t)q + 0] = counter;
            R.record[4 * (size_t)q + 1] = nListed;
            R.record[4 * (size_t)q + 2] = added;
            R.record[4 * (size_t)q + 3] = bv;
        }
        R.kfs.insert(R.kfs.end(), list.begin(), list.end());
        R.kfOff.push_back((int32_t)R.kfs.size());
        for (const int32_t kf : list) {
            for (int i = I.kfMpOff[kf]; i < I.kfMpOff[kf + 1]; i++) {
                const int32_t p = I.kfMp[i];
                if (p < 0 || stampP[(size_t)p] == k || I.mpBad[p]) continue;
                stampP[(size_t)p] = k;
                R.mps.push_back(p);
                R.mpIn.push_back(inP[(size_t)p] == k ? 1 : 0);
            }
            for (int i = I.kfMlOff[kf]; i < I.kfMlOff[kf + 1]; i++) {
                const int32_t l = I.kfMl[i];
                if (l < 0 || stampL[(size_t)l] == k || I.mlBad[l]) continue;
                stampL[(size_t)l] = k;
                R.mls.push_back(l);
                R.mlIn.push_back(inL[(size_t)l] == k ? 1 : 0);
            }
        }
        R.mpOff.push_back((int32_t)R.mps.size());
        R.mlOff.push_back((int32_t)R.mls.size());
    }
}

/* bytes of device scratch one query takes, its packed results included */
int64_t query_scratch(const drfe_lmap* db, const Call& C, int32_t rowK)
{
    const Image& G = db->img;
    const int64_t nK = (int64_t)G.kfHandle.size(), nP = (int64_t)G.mpHandle.size(), nL = (int64_t)G.mlHandle.size();
    return (nK > LMAP_LDS_KFS ? 4 * nK : 0) + 4 * ((nK + 31) / 32) + 16 * (int64_t)rowK + 10 * (nP + nL) + 8 * (int64_t)C.maxPts + 256;
}

int32_t row_k(const drfe_lmap* db, const Call& C) { return std::max((int32_t)db->img.kfHandle.size(), C.maxPrev); }

/* the device can run the call: a query fits the scratch budget and the walk ranks fit an int32 */
bool device_fits(const drfe_lmap* db, const Call& C)
{
    const int32_t rowK = row_k(db, C);
    const int64_t stride = (int64_t)std::max(db->img.maxRow[0], db->img.maxRow[1]) + 1;
    return query_scratch(db, C, rowK) <= db->scratchBytes && (int64_t)rowK * stride < (int64_t)LMAP_NO_CLAIM;
}

/* queries [k0, k1) of the call: one staging block up, the launches, the offsets and records back, then exactly the lists */
int run_chunk(LmapCall& call, const Call& C, int k0, int k1, int32_t rowK, Result& R)
{
    drfe_lmap* db = call.db;
    const Image& G = db->img;
    const size_t nQ = (size_t)(k1 - k0), nK = G.kfHandle.size(), nP = G.mpHandle.size(), nL = G.mlHandle.size();
    const size_t markWords = (nK + 31) / 32;
    const int32_t pt0 = C.ptOff[(size_t)k0], ln0 = C.lnOff[(size_t)k0], pv0 = C.prevOff[(size_t)k0];
    const size_t nPts = (size_t)(C.ptOff[(size_t)k1] - pt0), nLns = (size_t)(C.lnOff[(size_t)k1] - ln0), nPrev = (size_t)(C.prevOff[(size_t)k1] - pv0);
    StageLayout<16> in, out, scr;
    const auto sPtOff = in.add<int32_t>(nQ + 1);
    const auto sPts = in.add<int32_t>(nPts);
    const auto sLnOff = in.add<int32_t>(nQ + 1);
    const auto sLns = in.add<int32_t>(nLns);
    const auto sPrevOff = in.add<int32_t>(nQ + 1);
    const auto sPrev = in.add<int32_t>(nPrev);
    const auto oRec = out.add<LmapQueryRec>(nQ);
    const auto oOff = out.add<int32_t>(4 * (nQ + 1));
    /* zeroed: the global histogram (when the LDS one is too small) and the in-frame rows */
    const auto xHist = scr.add<int32_t>(nK > LMAP_LDS_KFS ? nQ * nK : 0);
    const auto xInP = scr.add<uint8_t>(nQ * nP);
    const auto xInL = scr.add<uint8_t>(nQ * nL);
    const size_t zeroEnd = scr.bytes();
    /* LMAP_NO_CLAIM bytes */
    const auto xClaimP = scr.add<int32_t>(nQ * nP);
    const auto xClaimL = scr.add<int32_t>(nQ * nL);
    const size_t claimEnd = scr.bytes();
    const auto xMark = scr.add<uint32_t>(nQ * markWords);
    const auto xList = scr.add<int32_t>(nQ * (size_t)rowK);
    const auto xCntP = scr.add<int32_t>(nQ * (size_t)rowK);
    const auto xCntL = scr.add<int32_t>(nQ * (size_t)rowK);
    const auto xNulledTmp = scr.add<int32_t>(nPts);
    const auto xKf = scr.add<int32_t>(nQ * (size_t)rowK);
    const auto xMp = scr.add<int32_t>(nQ * nP);
    const auto xMl = scr.add<int32_t>(nQ * nL);
    const auto xNulled = scr.add<int32_t>(nPts);
    const auto xMpIn = scr.add<uint8_t>(nQ * nP);
    const auto xMlIn = scr.add<uint8_t>(nQ * nL);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, ho] = call.at;
    for (size_t k = 0; k <= nQ; k++) {
        sPtOff.at(h)[k] = C.ptOff[(size_t)k0 + k] - pt0;
        sLnOff.at(h)[k] = C.lnOff[(size_t)k0 + k] - ln0;
        sPrevOff.at(h)[k] = C.prevOff[(size_t)k0 + k] - pv0;
    }
    sPts.put(h, C.pts.data() + pt0);
    sLns.put(h, C.lns.data() + ln0);
    sPrev.put(h, C.prev.data() + pv0);
    if (const int rc = call.send()) return rc;
    hipError_t e = zeroEnd ? hipMemsetAsync(dS, 0, zeroEnd, call.st) : hipSuccess;
    if (e == hipSuccess && claimEnd > zeroEnd) e = hipMemsetAsync(dS + zeroEnd, LMAP_NO_CLAIM & 0xff, claimEnd - zeroEnd, call.st);
    LmapLaunch L{};
    L.I = db->dView;
    L.nQ = (int32_t)nQ;
    L.rowK = rowK;
    L.rowStride[0] = G.maxRow[0] + 1;
    L.rowStride[1] = G.maxRow[1] + 1;
    L.markWords = (int32_t)markWords;
    L.ptOff = sPtOff.at(d);
    L.pts = sPts.at(d);
    L.lnOff = sLnOff.at(d);
    L.lns = sLns.at(d);
    L.prevOff = sPrevOff.at(d);
    L.prev = sPrev.at(d);
    L.hist = xHist.at(dS);
    L.mark = xMark.at(dS);
    L.list = xList.at(dS);
    L.cnt[0] = xCntP.at(dS);
    L.cnt[1] = xCntL.at(dS);
    L.claim[0] = xClaimP.at(dS);
    L.claim[1] = xClaimL.at(dS);
    L.inFrame[0] = xInP.at(dS);
    L.inFrame[1] = xInL.at(dS);
    L.nulledTmp = xNulledTmp.at(dS);
    L.rec = oRec.at(dO);
    for (int f = 0; f < 4; f++) L.off[f] = oOff.at(dO) + (size_t)f * (nQ + 1);
    L.packedKf = xKf.at(dS);
    L.packedItem[0] = xMp.at(dS);
    L.packedItem[1] = xMl.at(dS);
    L.packedIn[0] = xMpIn.at(dS);
    L.packedIn[1] = xMlIn.at(dS);
    L.packedNulled = xNulled.at(dS);
    if (e == hipSuccess) e = drfe_launch_lmap(L, call.st);
    if (const int rc = call.back(e)) return rc;
    const LmapQueryRec* rec = oRec.at(ho);
    const int32_t* off = oOff.at(ho);
    const size_t tKf = (size_t)off[nQ], tMp = (size_t)off[2 * nQ + 1], tMl = (size_t)off[3 * nQ + 2], tNu = (size_t)off[4 * nQ + 3];
    LmapFetch f;
    const auto lKf = f.add(xKf.at(dS), tKf);
    const auto lMp = f.add(xMp.at(dS), tMp);
    const auto lMl = f.add(xMl.at(dS), tMl);
    const auto lNu = f.add(xNulled.at(dS), tNu);
    const auto lMpIn = f.add(xMpIn.at(dS), tMp);
    const auto lMlIn = f.add(xMlIn.at(dS), tMl);
    if (const int rc = call.fetch(f)) return rc;
    const int32_t bKf = R.kfOff.back(), bMp = R.mpOff.back(), bMl = R.mlOff.back(), bNu = R.nuOff.back();
    for (size_t k = 0; k < nQ; k++) {
        R.kfOff.push_back(bKf + off[k + 1]);
        R.mpOff.push_back(bMp + off[(nQ + 1) + k + 1]);
        R.mlOff.push_back(bMl + off[2 * (nQ + 1) + k + 1]);
        R.nuOff.push_back(bNu + off[3 * (nQ + 1) + k + 1]);
        R.ref.push_back(rec[k].refKf);
        for (int f = 0; f < 4; f++) R.record.push_back(rec[k].rec[f]);
    }
    R.kfs.insert(R.kfs.end(), f.at(lKf), f.at(lKf) + tKf);
    R.mps.insert(R.mps.end(), f.at(lMp), f.at(lMp) + tMp);
    R.mls.insert(R.mls.end(), f.at(lMl), f.at(lMl) + tMl);
    R.nulled.insert(R.nulled.end(), f.at(lNu), f.at(lNu) + tNu);
    R.mpIn.insert(R.mpIn.end(), f.at(lMpIn), f.at(lMpIn) + tMp);
    R.mlIn.insert(R.mlIn.end(), f.at(lMlIn), f.at(lMlIn) + tMl);
    return DRFE_OK;
}

int run_device(drfe_lmap* db, const Call& C, Result& R, void* stream)
{
    LmapCall call{db, "lmap"};
    if (const int rc = call.begin(LMAP_NEED_IMAGE, stream)) return rc;
    const int32_t rowK = row_k(db, C);
    const int64_t perQuery = query_scratch(db, C, rowK);
    const int chunk = (int)std::min<int64_t>(C.n, std::max<int64_t>(1, db->scratchBytes / perQuery));
    R.start();
    for (int k0 = 0; k0 < C.n; k0 += chunk) {
        if (const int rc = run_chunk(call, C, k0, std::min(C.n, k0 + chunk), rowK, R)) return rc;
    }
    return DRFE_OK;
}

/* results into the caller's arrays and the call into the store's id and counters, or neither */
int finish(drfe_lmap* db, const Call& C, const Result& R, drfe_lmap_out* o, bool onDevice)
{
    const int n = C.n;
    const Image& G = db->img;
    o->kf_offsets[0] = o->mp_offsets[0] = o->ml_offsets[0] = o->nulled_offsets[0] = 0;
    if (n == 0) return DRFE_OK;
    const int32_t tKf = R.kfOff[(size_t)n], tMp = R.mpOff[(size_t)n], tMl = R.mlOff[(size_t)n], tNu = R.nuOff[(size_t)n];
    if (tKf > o->kf_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap: more local key frames than kf_capacity");
    if (tMp > o->mp_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap: more local points than mp_capacity");
    if (tMl > o->ml_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap: more local lines than ml_capacity");
    if (tNu > o->nulled_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap: more nulled points than nulled_capacity");
    for (int k = 0; k < n; k++) {
        o->kf_offsets[k + 1] = R.kfOff[(size_t)k + 1];
        o->mp_offsets[k + 1] = R.mpOff[(size_t)k + 1];
        o->ml_offsets[k + 1] = R.mlOff[(size_t)k + 1];
        o->nulled_offsets[k + 1] = R.nuOff[(size_t)k + 1];
        o->ref_kf[k] = R.ref[(size_t)k] >= 0 ? G.kfHandle[(size_t)R.ref[(size_t)k]] : -1;
    }
    std::memcpy(o->record, R.record.data(), sizeof(int32_t) * 4 * (size_t)n);
    for (int32_t i = 0; i < tKf; i++) o->kfs[i] = G.kfHandle[(size_t)R.kfs[(size_t)i]];
    for (int32_t i = 0; i < tMp; i++) o->mps[i] = G.mpHandle[(size_t)R.mps[(size_t)i]];
    for (int32_t i = 0; i < tMl; i++) o->mls[i] = G.mlHandle[(size_t)R.mls[(size_t)i]];
    if (tMp) std::memcpy(o->mp_in_frame, R.mpIn.data(), (size_t)tMp);
    if (tMl) std::memcpy(o->ml_in_frame, R.mlIn.data(), (size_t)tMl);
    if (tNu) std::memcpy(o->nulled, R.nulled.data(), sizeof(int32_t) * (size_t)tNu);
    db->lastId = C.lastId;
    db->stats[0]++;
    db->stats[1] += n;
    if (onDevice) db->stats[2]++;
    db->stats[4] += tKf;
    db->stats[5] += tMp;
    db->stats[6] += tMl;
    db->stats[7] += tNu;
    return DRFE_OK;
}

/* mode: 0 host, 1 device, 2 by the crossover */
int entry(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* o, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap: a device call on a store without a context");
    Call C;
    int rc = plan(db, q, o, C);
    if (rc) return rc;
    bool dev = mode == 1;
    if (mode == 2) dev = db->ctx && C.n >= DRFE_LMAP_DEVICE_FROM && device_fits(db, C);
    if (C.n == 0) dev = false;
    if (dev && !device_fits(db, C))
        return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap: one query does not fit the configured device scratch (or its walk ranks an int32)");
    Result R;
    if (dev) {
        rc = run_device(db, C, R, stream);
        if (rc) return rc;
    } else if (C.n > 0) {
        run_host(db, C, R);
    }
    return finish(db, C, R, o, dev);
}

}  // namespace

extern "C" {

int drfe_lmap_limits(int32_t* out4)
{
    if (!out4) return DRFE_ERR_INVALID;
    out4[0] = LMAP_LDS_KFS;
    out4[1] = LMAP_THREADS;
    out4[2] = LMAP_GATHER_ENTRIES;
    out4[3] = DRFE_LMAP_DEVICE_FROM;
    return DRFE_OK;
}

int drfe_lmap_update_host(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* o) { return entry(db, q, o, 0, nullptr); }
int drfe_lmap_update_device(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* o, void* stream) { return entry(db, q, o, 1, stream); }
int drfe_lmap_update_batch(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* o, void* stream) { return entry(db, q, o, 2, stream); }

int drfe_lmap_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::stats, stats); }

}  // extern "C"
