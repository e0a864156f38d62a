/* lmap_correct.cpp — the Sim3 propagation of LoopClosing::CorrectLoop (reference src/LoopClosing.cc:480-562) on the local-map
 * store, behind the C-ABI of include/drfe.h: the geometry setters and getters, the geometry image, the checks, the host walk, the
 * device entry (correct_kernels.hip), the commit and the counters.  Both sides evaluate correct_core.h.  A call is checked as a
 * whole and committed only when its results fit the caller's arrays.  DESIGN.md section 27. */
#include "lmap_call.h"

#include <algorithm>
#include <cstring>

using namespace lmap_store;

/* the geometry by slot, after the image */
int lmap_build_geo(drfe_lmap* db)
{
    const int rc = lmap_build_image(db);
    if (rc) return rc;
    if (!db->geoDirty) return DRFE_OK;
    const Image& G = db->img;
    GeoImage& E = db->geo;
    const size_t nK = G.kfHandle.size(), nP = G.mpHandle.size();
    const int32_t nLevels = (int32_t)db->scales.size();
    E.kfHas.assign(nK, 0);
    E.kfTcw.assign(16 * nK, 0.0f);
    E.kfOw.assign(3 * nK, 0.0f);
    E.mpHas.assign(nP, 0);
    E.mpWorld.assign(3 * nP, 0.0f);
    E.mpRef.assign(nP, -1);
    E.mpLevel.assign(nP, 0);
    E.mpBy.assign(nP, 0);
    E.mpByRef.assign(nP, 0);
    bool complete = nLevels > 0;
    for (size_t s = 0; s < nK; s++) {
        const auto it = db->kfPose.find(G.kfHandle[s]);
        if (it == db->kfPose.end()) {
            complete = false;
            continue;
        }
        E.kfHas[s] = 1;
        std::memcpy(&E.kfTcw[16 * s], it->second.data(), sizeof(float) * 16);
        camera_centre_kf(&E.kfTcw[16 * s], &E.kfOw[3 * s]);
    }
    for (size_t s = 0; s < nP; s++) {
        const auto it = db->mpGeo.find(G.mpHandle[s]);
        if (it == db->mpGeo.end()) {
            complete = false;
            continue;
        }
        const MpGeo& P = it->second;
        E.mpHas[s] = 1;
        std::memcpy(&E.mpWorld[3 * s], P.X, sizeof(P.X));
        const auto r = G.kfSlot.find(P.ref);
        if (r != G.kfSlot.end()) E.mpRef[s] = r->second;
        E.mpLevel[s] = P.level;
        E.mpBy[s] = P.by;
        E.mpByRef[s] = P.byRef;
        if (E.mpRef[s] < 0 || !E.kfHas[(size_t)E.mpRef[s]] || P.level < 0 || P.level >= nLevels) complete = false;
    }
    E.complete = complete;
    db->geoDirty = false;
    db->blk[drfe_lmap::GEO].stale_all();
    return DRFE_OK;
}

namespace {

/* a checked call: the called key frames by position (rank order) */
struct CorrPlan {
    int32_t n = 0, cur = 0, curPos = -1, maxRow = 0;
    int64_t sumRows = 0;
    SoSim3 Scw;
    std::vector<int32_t> called, calledHandle, pos, posOfArg;
};

/* what a call leaves, in slots and positions */
struct CorrResult {
    std::vector<CorrKf> kf;
    std::vector<int32_t> item, by;
    std::vector<float> world, normal, maxD, minD;
    std::vector<uint8_t> status;
    int chunks = 0;
};

bool corr_out_ok(const drfe_lmap_correct_out* o)
{
    return o && o->points_capacity >= 0 && o->walk_pos && o->corrected && o->non_corrected && o->Tiw && o->n_points &&
           (o->points_capacity == 0 ||
            (o->points && o->claimed_by && o->world && o->normal && o->max_distance && o->min_distance && o->status));
}

/* the handles of a call into positions; refuses a duplicate, an unknown handle and, when cur is given, a list without it */
int corr_positions(drfe_lmap* db, int32_t n, const int32_t* handles, const int32_t* cur, CorrPlan& C)
{
    if (n <= 0 || !handles) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_correct: invalid argument");
    if (n > DRFE_LMAP_MAX_QUERIES) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_correct: more than DRFE_LMAP_MAX_QUERIES key frames in a call");
    const int rc = lmap_build_geo(db);
    if (rc) return rc;
    const Image& G = db->img;
    C.n = n;
    std::vector<std::pair<int32_t, int32_t>> order;   /* (slot, index in the call) */
    C.pos.assign(G.kfHandle.size(), -1);
    for (int a = 0; a < n; a++) {
        const auto it = G.kfSlot.find(handles[a]);
        if (it == G.kfSlot.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_correct: the call names an unknown key-frame handle");
        if (C.pos[(size_t)it->second] >= 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_correct: the call names a key frame twice");
        C.pos[(size_t)it->second] = 0;
        order.emplace_back(it->second, a);
    }
    std::sort(order.begin(), order.end());
    C.called.resize((size_t)n);
    C.calledHandle.resize((size_t)n);
    C.posOfArg.resize((size_t)n);
    for (int j = 0; j < n; j++) {
        const int32_t s = order[(size_t)j].first;
        C.called[(size_t)j] = s;
        C.calledHandle[(size_t)j] = G.kfHandle[(size_t)s];
        C.pos[(size_t)s] = j;
        C.posOfArg[(size_t)order[(size_t)j].second] = j;
        const int32_t len = G.kfMpOff[(size_t)s + 1] - G.kfMpOff[(size_t)s];
        C.maxRow = std::max(C.maxRow, len);
        C.sumRows += len;
        if (cur && G.kfHandle[(size_t)s] == *cur) C.curPos = j;
    }
    if (cur && C.curPos < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_correct: the current key frame is not among the called");
    return DRFE_OK;
}

/* DRFE_ERR_STATE and the name of the item when the call would read geometry that is not there */
int corr_check(drfe_lmap* db, const CorrPlan& C)
{
    const Image& G = db->img;
    const GeoImage& E = db->geo;
    if (E.complete) return DRFE_OK;
    const int32_t nLevels = (int32_t)db->scales.size();
    if (nLevels <= 0) return lmap_fail(db, DRFE_ERR_STATE, "lmap_correct: the store has no scale factors");
    auto lacks = [&](const char* kind, int32_t h, const std::string& of) {
        return lmap_fail(db, DRFE_ERR_STATE, std::string("lmap_correct: ") + kind + " " + std::to_string(h) + of + " has no geometry");
    };
    for (int j = 0; j < C.n; j++) {
        const int32_t k = C.called[(size_t)j];
        if (!E.kfHas[(size_t)k]) return lacks("key frame", G.kfHandle[(size_t)k], "");
    }
    for (int j = 0; j < C.n; j++) {
        const int32_t k = C.called[(size_t)j];
        for (int32_t i = G.kfMpOff[(size_t)k]; i < G.kfMpOff[(size_t)k + 1]; i++) {
            const int32_t p = G.kfMp[(size_t)i];
            if (p < 0 || G.mpBad[(size_t)p]) continue;
            const int32_t h = G.mpHandle[(size_t)p];
            if (!E.mpHas[(size_t)p]) return lacks("map point", h, "");
            if (E.mpBy[(size_t)p] == C.cur) continue;
            const std::string of = ", of map point " + std::to_string(h) + ",";
            for (int32_t o = G.obsOff[(size_t)p]; o < G.obsOff[(size_t)p + 1]; o++)
                if (!E.kfHas[(size_t)G.obs[(size_t)o]]) return lacks("observing key frame", G.kfHandle[(size_t)G.obs[(size_t)o]], of);
            const int32_t r = E.mpRef[(size_t)p];
            if (r < 0)
                return lmap_fail(db, DRFE_ERR_STATE, "lmap_correct: the reference key frame " + std::to_string(db->mpGeo.at(h).ref) +
                                                    " of map point " + std::to_string(h) + " is unknown");
            if (!E.kfHas[(size_t)r]) return lacks("reference key frame", G.kfHandle[(size_t)r], of);
            if (E.mpLevel[(size_t)p] < 0 || E.mpLevel[(size_t)p] >= nLevels)
                return lmap_fail(db, DRFE_ERR_STATE, "lmap_correct: ref_level of map point " + std::to_string(h) + " is not a level of the store");
        }
    }
    return DRFE_OK;
}

/* the reference's loops: every key frame's Sim3 pair first, then key frame after key frame its points and its pose */
void corr_host(drfe_lmap* db, const CorrPlan& C, CorrResult& R)
{
    lmap_host_views(db);
    const LmapImage I = db->hView;
    const CorrImage V = db->hCorr;
    float TwcCur[16];
    pose_inverse_kf(V.kfTcw + 16 * (size_t)C.called[(size_t)C.curPos], TwcCur);
    R.kf.resize((size_t)C.n);
    for (int j = 0; j < C.n; j++) corr_keyframe(V.kfTcw + 16 * (size_t)C.called[(size_t)j], j == C.curPos, TwcCur, C.Scw, R.kf[(size_t)j]);
    std::vector<uint8_t> moved((size_t)I.nP, 0);   /* mnCorrectedByKF == cur, set by this call */
    for (int j = 0; j < C.n; j++) {
        const int32_t k = C.called[(size_t)j];
        const CorrKf& K = R.kf[(size_t)j];
        for (int32_t i = I.kfMpOff[k]; i < I.kfMpOff[k + 1]; i++) {
            const int32_t p = I.kfMp[i];
            if (!corr_entry_moves(p, I.mpBad, V.mpBy, C.cur) || moved[(size_t)p]) continue;
            moved[(size_t)p] = 1;
            float Xn[3], nrm[3], maxD, minD;
            corr_point(K.nonCorrected, K.swi, V.mpWorld + 3 * (size_t)p, Xn);
            const uint8_t st = corr_normal(V, I.obsOff, I.obs, C.pos.data(), R.kf.data(), p, j, Xn, nrm, &maxD, &minD);
            R.item.push_back(p);
            R.by.push_back(j);
            R.world.insert(R.world.end(), Xn, Xn + 3);
            R.normal.insert(R.normal.end(), nrm, nrm + 3);
            R.maxD.push_back(maxD);
            R.minD.push_back(minD);
            R.status.push_back(st);
        }
    }
}

/* how a device call divides the scratch: the claims and counts are shared, a chunk adds the packed records of its rows */
struct CorrFit {
    int64_t fixed = 0, whole = 0, least = 0;
    bool fits = false;
};

CorrFit corr_fit(const drfe_lmap* db, const CorrPlan& C)
{
    CorrFit F;
    F.fixed = 4 * (int64_t)db->img.mpHandle.size() + 4 * (int64_t)C.n + 1024;
    F.whole = F.fixed + CORRECT_ENTRY_BYTES * C.sumRows;
    F.least = F.fixed + CORRECT_ENTRY_BYTES * (int64_t)C.maxRow;
    F.fits = F.least <= db->scratchBytes && (int64_t)C.n * ((int64_t)C.maxRow + 1) < (int64_t)LMAP_NO_CLAIM;
    return F;
}

/* The plan launches and the totals back, the capacity test, then chunk after chunk its records back; the image on the device is
 * written only after the capacity test.  A HIP failure in between leaves the device copy to be sent again. */
int corr_device(drfe_lmap* db, const CorrPlan& C, const CorrFit& F, int32_t capacity, CorrResult& R, void* stream)
{
    LmapCall call{db, "lmap correct"};
    if (const int rc = call.begin(LMAP_NEED_GEO, stream)) return rc;
    const Image& G = db->img;
    const size_t n = (size_t)C.n, nK = G.kfHandle.size(), nP = G.mpHandle.size();
    /* rows of a chunk: as many positions as the budget holds, one at least */
    const int64_t room = std::min<int64_t>(db->scratchBytes, F.whole) - F.fixed;
    int64_t chunkRows = 0, rows = 0;
    for (size_t j = 0; j < n; j++) {
        const int64_t len = G.kfMpOff[(size_t)C.called[j] + 1] - G.kfMpOff[(size_t)C.called[j]];
        if (rows + len > room / CORRECT_ENTRY_BYTES) rows = 0;
        rows += len;
        chunkRows = std::max(chunkRows, rows);
    }
    StageLayout<16> in, out, scr;
    const auto sCalled = in.add<int32_t>(n);
    const auto sHandle = in.add<int32_t>(n);
    const auto sPos = in.add<int32_t>(nK);
    const auto oKf = out.add<CorrKf>(n);
    const auto oOff = out.add<int32_t>(n + 1);
    const auto xClaim = scr.add<int32_t>(nP);
    const auto xCnt = scr.add<int32_t>(n);
    const auto xItem = scr.add<int32_t>((size_t)chunkRows);
    const auto xBy = scr.add<int32_t>((size_t)chunkRows);
    const auto xWorld = scr.add<float>(3 * (size_t)chunkRows);
    const auto xNormal = scr.add<float>(3 * (size_t)chunkRows);
    const auto xMax = scr.add<float>((size_t)chunkRows);
    const auto xMin = scr.add<float>((size_t)chunkRows);
    const auto xStatus = scr.add<uint8_t>((size_t)chunkRows);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, ho] = call.at;
    sCalled.put(h, C.called.data());
    sHandle.put(h, C.calledHandle.data());
    sPos.put(h, C.pos.data());
    if (const int rc = call.send()) return rc;
    hipError_t e = nP ? hipMemsetAsync(xClaim.at(dS), LMAP_NO_CLAIM & 0xff, xClaim.bytes(), call.st) : hipSuccess;
    CorrLaunch L{};
    L.I = db->dView;
    L.G = db->dCorr;
    L.n = C.n;
    L.cur = C.cur;
    L.curPos = C.curPos;
    L.rowStride = C.maxRow + 1;
    L.maxRow = C.maxRow;
    corr_sim3_to8(C.Scw, L.Scw);
    L.called = sCalled.at(d);
    L.calledHandle = sHandle.at(d);
    L.pos = sPos.at(d);
    L.claim = xClaim.at(dS);
    L.cnt = xCnt.at(dS);
    L.kf = oKf.at(dO);
    L.off = oOff.at(dO);
    L.pkItem = xItem.at(dS);
    L.pkBy = xBy.at(dS);
    L.pkWorld = xWorld.at(dS);
    L.pkNormal = xNormal.at(dS);
    L.pkMax = xMax.at(dS);
    L.pkMin = xMin.at(dS);
    L.pkStatus = xStatus.at(dS);
    if (e == hipSuccess) e = drfe_launch_correct_plan(L, call.st);
    if (const int rc = call.back(e)) return rc;
    R.kf.assign(oKf.at(ho), oKf.at(ho) + n);
    const std::vector<int32_t> off(oOff.at(ho), oOff.at(ho) + n + 1);
    const int64_t total = off[n];
    if (total < 0 || total > C.sumRows) return lmap_fail(db, DRFE_ERR_STATE, "lmap correct device call: totals past their bounds");
    if (total > capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_correct: more moved points than points_capacity");
    R.item.resize((size_t)total);
    R.by.resize((size_t)total);
    R.world.resize(3 * (size_t)total);
    R.normal.resize(3 * (size_t)total);
    R.maxD.resize((size_t)total);
    R.minD.resize((size_t)total);
    R.status.resize((size_t)total);
    LmapWrites writes(db->blk[drfe_lmap::GEO]);
    LmapFetch f;
    const auto lItem = f.add(xItem.at(dS), (size_t)chunkRows);
    const auto lBy = f.add(xBy.at(dS), (size_t)chunkRows);
    const auto lWorld = f.add(xWorld.at(dS), 3 * (size_t)chunkRows);
    const auto lNormal = f.add(xNormal.at(dS), 3 * (size_t)chunkRows);
    const auto lMax = f.add(xMax.at(dS), (size_t)chunkRows);
    const auto lMin = f.add(xMin.at(dS), (size_t)chunkRows);
    const auto lStatus = f.add(xStatus.at(dS), (size_t)chunkRows);
    if (const int rc = call.room(f)) return rc;
    for (size_t j0 = 0; j0 < n;) {
        size_t j1 = j0;
        rows = 0;
        while (j1 < n) {
            const int64_t len = G.kfMpOff[(size_t)C.called[j1] + 1] - G.kfMpOff[(size_t)C.called[j1]];
            if (j1 > j0 && rows + len > room / CORRECT_ENTRY_BYTES) break;
            rows += len;
            j1++;
        }
        L.j0 = (int32_t)j0;
        L.j1 = (int32_t)j1;
        const size_t b = (size_t)off[j0], cnt = (size_t)(off[j1] - off[j0]);
        f.set(cnt, lItem, lBy, lMax, lMin, lStatus);
        f.set(3 * cnt, lWorld, lNormal);
        if (const int rc = call.fetch(f, drfe_launch_correct_chunk(L, call.st))) return rc;
        f.get(lItem, R.item.data() + b);
        f.get(lBy, R.by.data() + b);
        f.get(lWorld, R.world.data() + 3 * b);
        f.get(lNormal, R.normal.data() + 3 * b);
        f.get(lMax, R.maxD.data() + b);
        f.get(lMin, R.minD.data() + b);
        f.get(lStatus, R.status.data() + b);
        R.chunks++;
        j0 = j1;
    }
    if (const int rc = call.drain(drfe_launch_correct_poses(L, call.st))) return rc;
    writes.done();
    return DRFE_OK;
}

/* results into the caller's arrays and poses, positions and stamps into the store, or neither */
int corr_finish(drfe_lmap* db, const CorrPlan& C, const CorrResult& R, drfe_lmap_correct_out* o, bool onDevice)
{
    const Image& G = db->img;
    GeoImage& E = db->geo;
    const size_t total = R.item.size();
    if ((int64_t)total > o->points_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_correct: more moved points than points_capacity");
    for (int a = 0; a < C.n; a++) {
        const int32_t j = C.posOfArg[(size_t)a];
        const CorrKf& K = R.kf[(size_t)j];
        o->walk_pos[a] = j;
        corr_sim3_to8(K.corrected, o->corrected + 8 * (size_t)a);
        corr_sim3_to8(K.nonCorrected, o->non_corrected + 8 * (size_t)a);
        std::memcpy(o->Tiw + 16 * (size_t)a, K.Tiw, sizeof(K.Tiw));
    }
    *o->n_points = (int32_t)total;
    int64_t noObs = 0;
    for (size_t t = 0; t < total; t++) {
        o->points[t] = G.mpHandle[(size_t)R.item[t]];
        o->claimed_by[t] = C.calledHandle[(size_t)R.by[t]];
        noObs += R.status[t] == 0;
    }
    if (total) {
        std::memcpy(o->world, R.world.data(), 12 * total);
        std::memcpy(o->normal, R.normal.data(), 12 * total);
        std::memcpy(o->max_distance, R.maxD.data(), 4 * total);
        std::memcpy(o->min_distance, R.minD.data(), 4 * total);
        std::memcpy(o->status, R.status.data(), total);
    }
    /* the commit, against the image the call read */
    for (size_t t = 0; t < total; t++) {
        const size_t p = (size_t)R.item[t];
        MpGeo& P = db->mpGeo.at(o->points[t]);
        std::memcpy(P.X, &R.world[3 * t], sizeof(P.X));
        P.by = C.cur;
        P.byRef = o->claimed_by[t];
        std::memcpy(&E.mpWorld[3 * p], P.X, sizeof(P.X));
        E.mpBy[p] = P.by;
        E.mpByRef[p] = P.byRef;
    }
    for (int j = 0; j < C.n; j++) {
        const size_t s = (size_t)C.called[(size_t)j];
        const CorrKf& K = R.kf[(size_t)j];
        std::memcpy(db->kfPose.at(C.calledHandle[(size_t)j]).data(), K.Tiw, sizeof(K.Tiw));
        std::memcpy(&E.kfTcw[16 * s], K.Tiw, sizeof(K.Tiw));
        std::memcpy(&E.kfOw[3 * s], K.Ow, sizeof(K.Ow));
    }
    if (!onDevice) db->blk[drfe_lmap::GEO].stale_all();
    int64_t* st = db->corrStats;
    st[0]++;
    st[1] += C.n;
    if (onDevice) st[2]++;
    st[3] += (int64_t)total;
    st[4] += noObs;
    st[5] += C.sumRows;
    st[6] += R.chunks;
    return DRFE_OK;
}

/* mode: 0 host, 1 device, 2 by the crossover */
int corr_entry(drfe_lmap* db, int32_t cur, const double* Scw, int32_t n, const int32_t* handles, drfe_lmap_correct_out* o, int mode,
               void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_correct: a device call on a store without a context");
    if (!Scw || !corr_out_ok(o)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_correct: invalid argument");
    CorrPlan C;
    C.cur = cur;
    corr_sim3_from8(Scw, C.Scw);
    int rc = corr_positions(db, n, handles, &cur, C);
    if (rc) return rc;
    rc = corr_check(db, C);
    if (rc) return rc;
    bool dev = mode == 1 || (mode == 2 && db->ctx && n >= DRFE_LMAP_CORRECT_DEVICE_FROM);
    CorrFit F;
    if (dev) {
        F = corr_fit(db, C);
        if (!F.fits && mode == 1)
            return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_correct: the longest called row does not fit the configured device scratch (or the walk ranks an int32)");
        dev = F.fits;
    }
    CorrResult R;
    if (dev) {
        rc = corr_device(db, C, F, o->points_capacity, R, stream);
        if (rc) return rc;
    } else {
        corr_host(db, C, R);
    }
    return corr_finish(db, C, R, o, dev);
}

}  // namespace

extern "C" {

int drfe_lmap_set_scales(drfe_lmap* db, int32_t n_levels, const float* scale_factors)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (n_levels <= 0 || !scale_factors) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_scales: invalid argument");
    db->scales.assign(scale_factors, scale_factors + n_levels);
    db->geoDirty = true;
    return DRFE_OK;
}

int drfe_lmap_get_scales(drfe_lmap* db, int32_t capacity, int32_t* n_levels, float* scale_factors)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!n_levels || capacity < 0 || (capacity > 0 && !scale_factors)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_scales: invalid argument");
    *n_levels = (int32_t)db->scales.size();
    if (*n_levels > capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_get_scales: more levels than capacity");
    if (*n_levels) std::memcpy(scale_factors, db->scales.data(), sizeof(float) * db->scales.size());
    return DRFE_OK;
}

int drfe_lmap_set_poses(drfe_lmap* db, int32_t count, const int32_t* handles, const float* Tcw)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !Tcw))) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_poses: invalid argument");
    for (int i = 0; i < count; i++)
        if (handles[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_poses: a negative handle");
    for (int i = 0; i < count; i++) std::memcpy(db->kfPose[handles[i]].data(), Tcw + 16 * (size_t)i, sizeof(float) * 16);
    if (count) db->geoDirty = true;
    return DRFE_OK;
}

int drfe_lmap_get_poses(drfe_lmap* db, int32_t count, const int32_t* handles, float* Tcw, float* Ow, float* Twc)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && !handles)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_poses: invalid argument");
    for (int i = 0; i < count; i++)
        if (db->kfPose.find(handles[i]) == db->kfPose.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_poses: a handle without a pose");
    for (int i = 0; i < count; i++) {
        const float* T = db->kfPose.at(handles[i]).data();
        if (Tcw) std::memcpy(Tcw + 16 * (size_t)i, T, sizeof(float) * 16);
        if (Ow) camera_centre_kf(T, Ow + 3 * (size_t)i);
        if (Twc) pose_inverse_kf(T, Twc + 16 * (size_t)i);
    }
    return DRFE_OK;
}

int drfe_lmap_set_point_geometry(drfe_lmap* db, const drfe_lmap_point_geometry* r)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!r || r->count < 0 || (r->count > 0 && (!r->handle || !r->world || !r->ref_kf || !r->ref_level)))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_point_geometry: invalid argument");
    for (int i = 0; i < r->count; i++)
        if (r->handle[i] < 0 || r->ref_kf[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_point_geometry: a negative handle");
    for (int i = 0; i < r->count; i++) {
        MpGeo& P = db->mpGeo[r->handle[i]];
        std::memcpy(P.X, r->world + 3 * (size_t)i, sizeof(P.X));
        P.ref = r->ref_kf[i];
        P.level = r->ref_level[i];
        P.by = r->corrected_by ? r->corrected_by[i] : 0;
        P.byRef = r->corrected_ref ? r->corrected_ref[i] : 0;
    }
    if (r->count) db->geoDirty = true;
    return DRFE_OK;
}

int drfe_lmap_get_point_geometry(drfe_lmap* db, int32_t count, const int32_t* handles, float* world, int32_t* ref_kf, int32_t* ref_level,
                                 int32_t* corrected_by, int32_t* corrected_ref)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && !handles)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_point_geometry: invalid argument");
    for (int i = 0; i < count; i++)
        if (db->mpGeo.find(handles[i]) == db->mpGeo.end())
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_point_geometry: a handle without geometry");
    for (int i = 0; i < count; i++) {
        const MpGeo& P = db->mpGeo.at(handles[i]);
        if (world) std::memcpy(world + 3 * (size_t)i, P.X, sizeof(P.X));
        if (ref_kf) ref_kf[i] = P.ref;
        if (ref_level) ref_level[i] = P.level;
        if (corrected_by) corrected_by[i] = P.by;
        if (corrected_ref) corrected_ref[i] = P.byRef;
    }
    return DRFE_OK;
}

int drfe_lmap_correct_host(drfe_lmap* db, int32_t cur, const double* Scw, int32_t n, const int32_t* handles, drfe_lmap_correct_out* o)
{
    return corr_entry(db, cur, Scw, n, handles, o, 0, nullptr);
}
int drfe_lmap_correct_device(drfe_lmap* db, int32_t cur, const double* Scw, int32_t n, const int32_t* handles, drfe_lmap_correct_out* o,
                             void* stream)
{
    return corr_entry(db, cur, Scw, n, handles, o, 1, stream);
}
int drfe_lmap_correct_batch(drfe_lmap* db, int32_t cur, const double* Scw, int32_t n, const int32_t* handles, drfe_lmap_correct_out* o,
                            void* stream)
{
    return corr_entry(db, cur, Scw, n, handles, o, 2, stream);
}

int drfe_lmap_correct_limits(int32_t* out4)
{
    if (!out4) return DRFE_ERR_INVALID;
    out4[0] = CORRECT_TILE;
    out4[1] = DRFE_LMAP_CORRECT_DEVICE_FROM;
    out4[2] = CORRECT_ENTRY_BYTES;
    out4[3] = LMAP_THREADS;
    return DRFE_OK;
}

int drfe_lmap_correct_scratch(drfe_lmap* db, int32_t n, const int32_t* handles, int64_t* out3)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!out3) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_correct_scratch: invalid argument");
    CorrPlan C;
    const int rc = corr_positions(db, n, handles, nullptr, C);
    if (rc) return rc;
    const CorrFit F = corr_fit(db, C);
    out3[0] = F.whole;
    out3[1] = F.least;
    out3[2] = F.fixed;
    return DRFE_OK;
}

int drfe_lmap_correct_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::corrStats, stats); }

}  // extern "C"
