/* lmap_gba.cpp — the map update that ends LoopClosing::RunGlobalBundleAdjustment (reference src/LoopClosing.cc:722-783) on the
 * local-map store, behind the C-ABI of include/drfe.h: the setters and getters of mTcwGBA, mTcwBefGBA, mPosGBA and the stamps,
 * that state by slot, the integer walk with its checks, the host entry, the device entry (gba_kernels.hip), the commit and the
 * counters.  Both sides evaluate gba_core.h.  A call is checked as a whole before anything is written.  DESIGN.md section 29. */
#include "lmap_call.h"

#include <algorithm>
#include <cstring>

using namespace lmap_store;

namespace {

/* the state by slot, after the geometry */
int build_gba(drfe_lmap* db)
{
    const int rc = lmap_build_geo(db);
    if (rc) return rc;
    if (!db->gbaDirty) return DRFE_OK;
    const Image& G = db->img;
    GbaAttr& A = db->gba;
    const size_t nK = G.kfHandle.size(), nP = G.mpHandle.size();
    A.kfTcwGBA.assign(16 * nK, 0.0f);
    A.kfBef.assign(16 * nK, 0.0f);
    A.kfStamp.assign(nK, 0);
    A.kfHasT.assign(nK, 0);
    A.kfHasBef.assign(nK, 0);
    A.mpPosGBA.assign(3 * nP, 0.0f);
    A.mpStamp.assign(nP, 0);
    A.mpHasPos.assign(nP, 0);
    if (!db->kfGba.empty())
        for (size_t s = 0; s < nK; s++) {
            const auto it = db->kfGba.find(G.kfHandle[s]);
            if (it == db->kfGba.end()) continue;
            const KfGba& K = it->second;
            std::memcpy(&A.kfTcwGBA[16 * s], K.T, sizeof(K.T));
            std::memcpy(&A.kfBef[16 * s], K.bef, sizeof(K.bef));
            A.kfStamp[s] = K.stamp;
            A.kfHasT[s] = K.hasT;
            A.kfHasBef[s] = K.hasBef;
        }
    if (!db->mpGba.empty())
        for (size_t s = 0; s < nP; s++) {
            const auto it = db->mpGba.find(G.mpHandle[s]);
            if (it == db->mpGba.end()) continue;
            const MpGba& P = it->second;
            std::memcpy(&A.mpPosGBA[3 * s], P.X, sizeof(P.X));
            A.mpStamp[s] = P.stamp;
            A.mpHasPos[s] = P.hasX;
        }
    db->gbaDirty = false;
    db->blk[drfe_lmap::GBA].stale_all();
    return DRFE_OK;
}

/* the checked walk of a call: the visited key frames in FIFO order and the composed ones by round */
struct GbaPlan {
    int32_t loop = 0, maxDepth = 0;
    std::vector<int32_t> list, parentV, at;    /* slots by position; position of the parent or -1; position by slot or -1 */
    std::vector<uint8_t> composed;
    std::vector<int32_t> roundOff, roundKf, roundParent;
    /* the points, from the check */
    int64_t nKind[3] = {0, 0, 0}, skippedRef = 0;
    int64_t chunkPts = 0;
    std::vector<int32_t> chunkMoved;           /* moved points of each chunk of chunkPts slots */
};

struct GbaResult {
    std::vector<float> pose, bef;              /* 16 per position */
    std::vector<int32_t> item;                 /* point slots */
    std::vector<float> world;
    std::vector<uint8_t> kind;
};

bool gba_out_ok(const drfe_lmap_gba_out* o)
{
    return o && o->keyframes_capacity >= 0 && o->points_capacity >= 0 && o->n_keyframes && o->n_points &&
           (o->keyframes_capacity == 0 || (o->keyframes && o->Tcw && o->TcwBef && o->composed)) &&
           (o->points_capacity == 0 || (o->points && o->world && o->kind));
}

/* :723-746 on integers: the FIFO, the stamps, who is composed from whom and at which unstamped depth.  O(key frames). */
int gba_walk(drfe_lmap* db, int32_t nOrigins, const int32_t* origins, GbaPlan& W)
{
    const Image& G = db->img;
    const GeoImage& E = db->geo;
    const GbaAttr& A = db->gba;
    const size_t nK = G.kfHandle.size();
    auto kfName = [&](int32_t s) { return "key frame " + std::to_string(G.kfHandle[(size_t)s]); };
    W.at.assign(nK, -1);
    std::vector<int32_t> depth;
    for (int a = 0; a < nOrigins; a++) {
        const auto it = G.kfSlot.find(origins[a]);
        if (it == G.kfSlot.end())
            return lmap_fail(db, DRFE_ERR_STATE, "lmap_gba: the origin key frame " + std::to_string(origins[a]) + " is unknown");
        if (W.at[(size_t)it->second] >= 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_gba: the call names an origin twice");
        W.at[(size_t)it->second] = (int32_t)W.list.size();
        W.list.push_back(it->second);
        W.parentV.push_back(-1);
        W.composed.push_back(0);
        depth.push_back(0);
    }
    for (size_t v = 0; v < W.list.size(); v++) {
        const int32_t s = W.list[v];
        if (!E.kfHas[(size_t)s]) return lmap_fail(db, DRFE_ERR_STATE, "lmap_gba: the visited " + kfName(s) + " has no pose");
        if (!W.composed[v] && !A.kfHasT[(size_t)s])
            return lmap_fail(db, DRFE_ERR_STATE, "lmap_gba: the visited " + kfName(s) + " has no TcwGBA");
        for (int32_t i = G.childOff[(size_t)s]; i < G.childOff[(size_t)s + 1]; i++) {
            const int32_t c = G.child[(size_t)i];
            if (W.at[(size_t)c] >= 0) return lmap_fail(db, DRFE_ERR_STATE, "lmap_gba: the " + kfName(c) + " would be visited twice");
            const uint8_t comp = A.kfStamp[(size_t)c] != W.loop;
            const int32_t d = comp ? depth[v] + 1 : 0;
            W.at[(size_t)c] = (int32_t)W.list.size();
            W.list.push_back(c);
            W.parentV.push_back((int32_t)v);
            W.composed.push_back(comp);
            depth.push_back(d);
            W.maxDepth = std::max(W.maxDepth, d);
        }
    }
    /* the composed key frames by depth, in list order within one */
    W.roundOff.assign((size_t)W.maxDepth + 1, 0);
    for (size_t v = 0; v < W.list.size(); v++)
        if (depth[v] > 0) W.roundOff[(size_t)depth[v]]++;
    for (int d = 1; d <= W.maxDepth; d++) W.roundOff[(size_t)d] += W.roundOff[(size_t)d - 1];
    W.roundKf.resize((size_t)W.roundOff[(size_t)W.maxDepth]);
    W.roundParent.resize(W.roundKf.size());
    std::vector<int32_t> fill(W.roundOff.begin(), W.roundOff.end());
    for (size_t v = 0; v < W.list.size(); v++)
        if (depth[v] > 0) {
            const size_t o = (size_t)fill[(size_t)depth[v] - 1]++;
            W.roundKf[o] = W.list[v];
            W.roundParent[o] = W.list[(size_t)W.parentV[v]];
        }
    return DRFE_OK;
}

/* :749-783 over every point slot.  With R the positions are computed from the poses of R (the host entry); without it the pass
 * only checks and counts (the device entry).  The store is not written. */
int gba_points(drfe_lmap* db, GbaPlan& W, GbaResult* R)
{
    const Image& G = db->img;
    const GeoImage& E = db->geo;
    const GbaAttr& A = db->gba;
    const size_t nP = G.mpHandle.size();
    auto mpName = [&](size_t p) { return "map point " + std::to_string(G.mpHandle[p]); };
    W.chunkMoved.assign(W.chunkPts > 0 ? (nP + (size_t)W.chunkPts - 1) / (size_t)W.chunkPts : 0, 0);
    for (size_t p = 0; p < nP; p++) {
        const uint8_t bad = G.mpBad[p];
        const int32_t stamp = A.mpStamp[p];
        int32_t r = -1, v = -1, refStamp = 0;
        /* a point that is not bad either moves, and its position is part of its geometry, or is asked for its reference key frame */
        if (!bad && !E.mpHas[p]) return lmap_fail(db, DRFE_ERR_STATE, "lmap_gba: the " + mpName(p) + " has no geometry");
        if (!bad && stamp != W.loop) {
            r = E.mpRef[p];
            if (r < 0)
                return lmap_fail(db, DRFE_ERR_STATE, "lmap_gba: the reference key frame " + std::to_string(db->mpGeo.at(G.mpHandle[p]).ref) +
                                                    " of " + mpName(p) + " is unknown");
            v = W.at[(size_t)r];
            refStamp = v >= 0 && W.composed[(size_t)v] ? W.loop : A.kfStamp[(size_t)r];
        }
        const int kind = gba_point_kind(bad, stamp, refStamp, W.loop);
        if (kind == GBA_POINT_STAYS) {
            W.skippedRef += !bad;
            continue;
        }
        const float *bef = nullptr, *Tcw = nullptr;
        if (kind == GBA_POINT_POS) {
            if (!A.mpHasPos[p]) return lmap_fail(db, DRFE_ERR_STATE, "lmap_gba: the " + mpName(p) + " holds the stamp and has no PosGBA");
        } else {
            const std::string of = "lmap_gba: the reference key frame " + std::to_string(G.kfHandle[(size_t)r]) + " of " + mpName(p);
            if (!E.kfHas[(size_t)r]) return lmap_fail(db, DRFE_ERR_STATE, of + " has no pose");
            if (v < 0 && !A.kfHasBef[(size_t)r]) return lmap_fail(db, DRFE_ERR_STATE, of + " was not reached and has no TcwBefGBA");
            if (R) {
                bef = v >= 0 ? &R->bef[16 * (size_t)v] : &A.kfBef[16 * (size_t)r];
                Tcw = v >= 0 ? &R->pose[16 * (size_t)v] : &E.kfTcw[16 * (size_t)r];
            }
        }
        W.nKind[kind]++;
        if (W.chunkPts > 0) W.chunkMoved[p / (size_t)W.chunkPts]++;
        if (R) {
            float Xn[3];
            gba_point(bad, stamp, refStamp, W.loop, &A.mpPosGBA[3 * p], &E.mpWorld[3 * p], bef, Tcw, Xn);
            R->item.push_back((int32_t)p);
            R->world.insert(R->world.end(), Xn, Xn + 3);
            R->kind.push_back((uint8_t)kind);
        }
    }
    return DRFE_OK;
}

/* the poses of the walk, top-down in list order: a parent stands before its children */
void gba_poses_host(drfe_lmap* db, const GbaPlan& W, GbaResult& R)
{
    const GeoImage& E = db->geo;
    const GbaAttr& A = db->gba;
    const size_t nV = W.list.size();
    R.pose.resize(16 * nV);
    R.bef.resize(16 * nV);
    for (size_t v = 0; v < nV; v++) {
        const size_t s = (size_t)W.list[v];
        std::memcpy(&R.bef[16 * v], &E.kfTcw[16 * s], sizeof(float) * 16);
        if (W.composed[v]) {
            const size_t pv = (size_t)W.parentV[v];
            gba_compose(&E.kfTcw[16 * s], &E.kfTcw[16 * (size_t)W.list[pv]], &R.pose[16 * pv], &R.pose[16 * v]);
        } else {
            std::memcpy(&R.pose[16 * v], &A.kfTcwGBA[16 * s], sizeof(float) * 16);
        }
    }
}

struct GbaFit {
    int64_t fixed = GBA_FIXED_BYTES, whole = 0, least = 0, chunkPts = 0;
    bool fits = false;
};

GbaFit gba_fit(const drfe_lmap* db)
{
    GbaFit F;
    const int64_t nP = (int64_t)db->img.mpHandle.size();
    F.whole = F.fixed + GBA_POINT_BYTES * nP;
    F.least = F.fixed + GBA_POINT_BYTES * std::min<int64_t>(nP, 1);
    F.fits = F.least <= db->scratchBytes;
    F.chunkPts = F.fits ? std::min<int64_t>(nP, (db->scratchBytes - F.fixed) / GBA_POINT_BYTES) : 0;
    return F;
}

/* The key-frame launches and their records back, then chunk after chunk of point slots its records back.  Everything the call
 * could be refused for has been checked, so the resident blocks are written from the first launch on; a HIP failure in between
 * leaves both to be sent again. */
int gba_device(drfe_lmap* db, const GbaPlan& W, GbaResult& R, void* stream)
{
    LmapCall call{db, "lmap gba"};
    if (const int rc = call.begin(LMAP_NEED_GBA, stream)) return rc;
    const size_t nV = W.list.size(), nP = db->img.mpHandle.size(), chunk = (size_t)W.chunkPts;
    const size_t nGroups = (chunk + GBA_TILE - 1) / GBA_TILE;
    const int64_t total = W.nKind[1] + W.nKind[2];
    size_t most = 0;
    for (const int32_t m : W.chunkMoved) most = std::max(most, (size_t)m);
    StageLayout<16> in, out, scr;
    const auto sList = in.add<int32_t>(nV);
    const auto sOff = in.add<int32_t>(W.roundOff.size());
    const auto sKf = in.add<int32_t>(W.roundKf.size());
    const auto sPar = in.add<int32_t>(W.roundParent.size());
    const auto oPose = out.add<float>(16 * nV);
    const auto oBef = out.add<float>(16 * nV);
    const auto xKind = scr.add<uint8_t>(chunk);
    const auto xCnt = scr.add<int32_t>(nGroups + 1);
    const auto xItem = scr.add<int32_t>(most);
    const auto xWorld = scr.add<float>(3 * most);
    const auto xPk = scr.add<uint8_t>(most);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, ho] = call.at;
    LmapFetch f;
    const auto lTot = f.add(xCnt.at(dS), 1);
    const auto lItem = f.add(xItem.at(dS), most);
    const auto lWorld = f.add(xWorld.at(dS), 3 * most);
    const auto lKind = f.add(xPk.at(dS), most);
    if (const int rc = call.room(f)) return rc;
    sList.put(h, W.list.data());
    sOff.put(h, W.roundOff.data());
    sKf.put(h, W.roundKf.data());
    sPar.put(h, W.roundParent.data());
    if (const int rc = call.send()) return rc;
    GbaLaunch L{};
    L.I = db->dView;
    L.G = db->dCorr;
    L.B = db->dGba;
    L.loop = W.loop;
    L.nV = (int32_t)nV;
    L.nRounds = W.maxDepth;
    L.pkCap = (int32_t)most;
    L.list = sList.at(d);
    L.roundOff = sOff.at(d);
    L.roundKf = sKf.at(d);
    L.roundParent = sPar.at(d);
    L.kind = xKind.at(dS);
    L.groupCnt = xCnt.at(dS);
    L.pkItem = xItem.at(dS);
    L.pkWorld = xWorld.at(dS);
    L.pkKind = xPk.at(dS);
    L.outPose = oPose.at(dO);
    L.outBef = oBef.at(dO);
    LmapWrites writes(db->blk[drfe_lmap::GEO], &db->blk[drfe_lmap::GBA]);
    if (const int rc = call.back(drfe_launch_gba_keyframes(L, call.st))) return rc;
    R.pose.assign(oPose.at(ho), oPose.at(ho) + 16 * nV);
    R.bef.assign(oBef.at(ho), oBef.at(ho) + 16 * nV);
    R.item.resize((size_t)total);
    R.world.resize(3 * (size_t)total);
    R.kind.resize((size_t)total);
    size_t b = 0;
    for (size_t p0 = 0, k = 0; p0 < nP; p0 += chunk, k++) {
        const size_t p1 = std::min(nP, p0 + chunk), cnt = (size_t)W.chunkMoved[k];
        L.p0 = (int32_t)p0;
        L.p1 = (int32_t)p1;
        f.set(lTot, xCnt.at(dS) + (p1 - p0 + GBA_TILE - 1) / GBA_TILE, 1);
        f.set(cnt, lItem, lKind);
        f.set(3 * cnt, lWorld);
        if (const int rc = call.fetch(f, drfe_launch_gba_points(L, call.st))) return rc;
        if ((size_t)*f.at(lTot) != cnt) return lmap_fail(db, DRFE_ERR_STATE, "lmap gba device call: the moved points of a chunk are not the host's count");
        f.get(lItem, R.item.data() + b);
        f.get(lWorld, R.world.data() + 3 * b);
        f.get(lKind, R.kind.data() + b);
        b += cnt;
    }
    writes.done();
    return DRFE_OK;
}

/* results into the caller's arrays, and poses, mTcwBefGBA, composed mTcwGBA, stamps and positions into the store */
void gba_finish(drfe_lmap* db, const GbaPlan& W, const GbaResult& R, drfe_lmap_gba_out* o, bool onDevice)
{
    const Image& G = db->img;
    GeoImage& E = db->geo;
    GbaAttr& A = db->gba;
    const size_t nV = W.list.size(), total = R.item.size();
    *o->n_keyframes = (int32_t)nV;
    *o->n_points = (int32_t)total;
    int64_t nComposed = 0;
    for (size_t v = 0; v < nV; v++) {
        const size_t s = (size_t)W.list[v];
        const int32_t hnd = G.kfHandle[s];
        const float *T = &R.pose[16 * v], *B = &R.bef[16 * v];
        o->keyframes[v] = hnd;
        o->composed[v] = W.composed[v];
        std::memcpy(o->Tcw + 16 * v, T, sizeof(float) * 16);
        std::memcpy(o->TcwBef + 16 * v, B, sizeof(float) * 16);
        std::memcpy(db->kfPose.at(hnd).data(), T, sizeof(float) * 16);
        std::memcpy(&E.kfTcw[16 * s], T, sizeof(float) * 16);
        camera_centre_kf(T, &E.kfOw[3 * s]);
        KfGba& K = db->kfGba[hnd];
        std::memcpy(K.bef, B, sizeof(K.bef));
        K.hasBef = 1;
        std::memcpy(&A.kfBef[16 * s], B, sizeof(K.bef));
        A.kfHasBef[s] = 1;
        if (W.composed[v]) {
            nComposed++;
            std::memcpy(K.T, T, sizeof(K.T));
            K.hasT = 1;
            K.stamp = W.loop;
            std::memcpy(&A.kfTcwGBA[16 * s], T, sizeof(K.T));
            A.kfHasT[s] = 1;
            A.kfStamp[s] = W.loop;
        }
    }
    for (size_t t = 0; t < total; t++) {
        const size_t p = (size_t)R.item[t];
        o->points[t] = G.mpHandle[p];
        o->kind[t] = R.kind[t];
        std::memcpy(o->world + 3 * t, &R.world[3 * t], sizeof(float) * 3);
        std::memcpy(db->mpGeo.at(o->points[t]).X, &R.world[3 * t], sizeof(float) * 3);
        std::memcpy(&E.mpWorld[3 * p], &R.world[3 * t], sizeof(float) * 3);
    }
    if (!onDevice) {
        db->blk[drfe_lmap::GEO].stale_all();
        db->blk[drfe_lmap::GBA].stale_all();
    }
    int64_t* st = db->gbaStats;
    st[0]++;
    if (onDevice) st[1]++;
    st[2] += (int64_t)nV;
    st[3] += nComposed;
    st[4] = std::max<int64_t>(st[4], W.maxDepth);
    st[5] += W.nKind[1];
    st[6] += W.nKind[2];
    st[7] += W.skippedRef;
}

/* mode: 0 host, 1 device, 2 by the crossover */
int gba_entry(drfe_lmap* db, int32_t loop, int32_t nOrigins, const int32_t* origins, drfe_lmap_gba_out* o, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_gba: a device call on a store without a context");
    if (nOrigins <= 0 || !origins || !gba_out_ok(o)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_gba: invalid argument");
    int rc = build_gba(db);
    if (rc) return rc;
    GbaPlan W;
    W.loop = loop;
    rc = gba_walk(db, nOrigins, origins, W);
    if (rc) return rc;
    bool dev = mode == 1 || (mode == 2 && db->ctx && (int64_t)db->img.mpHandle.size() >= (int64_t)DRFE_LMAP_GBA_DEVICE_FROM);
    if (dev) {
        const GbaFit F = gba_fit(db);
        if (!F.fits && mode == 1) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_gba: the configured device scratch does not hold one point slot");
        dev = F.fits;
        W.chunkPts = F.chunkPts;
    }
    GbaResult R;
    if (!dev) {
        W.chunkPts = 0;
        gba_poses_host(db, W, R);
    }
    rc = gba_points(db, W, dev ? nullptr : &R);
    if (rc) return rc;
    if ((int64_t)W.list.size() > o->keyframes_capacity)
        return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_gba: more visited key frames than keyframes_capacity");
    if (W.nKind[1] + W.nKind[2] > o->points_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_gba: more moved points than points_capacity");
    if (dev) {
        rc = gba_device(db, W, R, stream);
        if (rc) return rc;
    }
    gba_finish(db, W, R, o, dev);
    return DRFE_OK;
}

/* a setter's row into the state by slot when that is current, so that an edit costs no rebuild; the setter marks the block, once */
template <class F>
void patch_slot(drfe_lmap* db, const std::unordered_map<int32_t, int32_t>& slots, int32_t handle, F&& f)
{
    if (db->imgDirty || db->gbaDirty) {
        db->gbaDirty = true;
        return;
    }
    const auto it = slots.find(handle);
    if (it != slots.end()) f((size_t)it->second);
}

}  // namespace

extern "C" {

int drfe_lmap_set_gba_keyframes(drfe_lmap* db, int32_t count, const int32_t* handles, const float* TcwGBA, const int32_t* stamp)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !TcwGBA || !stamp))) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_gba_keyframes: invalid argument");
    for (int i = 0; i < count; i++)
        if (handles[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_gba_keyframes: a negative handle");
    GbaAttr& A = db->gba;
    for (int i = 0; i < count; i++) {
        KfGba& K = db->kfGba[handles[i]];
        std::memcpy(K.T, TcwGBA + 16 * (size_t)i, sizeof(K.T));
        K.hasT = 1;
        K.stamp = stamp[i];
        patch_slot(db, db->img.kfSlot, handles[i], [&](size_t s) {
            std::memcpy(&A.kfTcwGBA[16 * s], K.T, sizeof(K.T));
            A.kfHasT[s] = 1;
            A.kfStamp[s] = K.stamp;
        });
    }
    if (count) db->blk[drfe_lmap::GBA].stale_all();
    return DRFE_OK;
}

int drfe_lmap_set_gba_points(drfe_lmap* db, int32_t count, const int32_t* handles, const float* PosGBA, const int32_t* stamp)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !PosGBA || !stamp))) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_gba_points: invalid argument");
    for (int i = 0; i < count; i++)
        if (handles[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_gba_points: a negative handle");
    GbaAttr& A = db->gba;
    for (int i = 0; i < count; i++) {
        MpGba& P = db->mpGba[handles[i]];
        std::memcpy(P.X, PosGBA + 3 * (size_t)i, sizeof(P.X));
        P.hasX = 1;
        P.stamp = stamp[i];
        patch_slot(db, db->img.mpSlot, handles[i], [&](size_t s) {
            std::memcpy(&A.mpPosGBA[3 * s], P.X, sizeof(P.X));
            A.mpHasPos[s] = 1;
            A.mpStamp[s] = P.stamp;
        });
    }
    if (count) db->blk[drfe_lmap::GBA].stale_all();
    return DRFE_OK;
}

int drfe_lmap_get_gba_keyframes(drfe_lmap* db, int32_t count, const int32_t* handles, float* TcwGBA, int32_t* stamp, float* TcwBefGBA,
                                uint8_t* has_TcwGBA, uint8_t* has_TcwBefGBA)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && !handles)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_gba_keyframes: invalid argument");
    for (int i = 0; i < count; i++)
        if (db->kfGba.find(handles[i]) == db->kfGba.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_gba_keyframes: a handle without state");
    for (int i = 0; i < count; i++) {
        const KfGba& K = db->kfGba.at(handles[i]);
        if (TcwGBA) std::memcpy(TcwGBA + 16 * (size_t)i, K.T, sizeof(K.T));
        if (stamp) stamp[i] = K.stamp;
        if (TcwBefGBA) std::memcpy(TcwBefGBA + 16 * (size_t)i, K.bef, sizeof(K.bef));
        if (has_TcwGBA) has_TcwGBA[i] = K.hasT;
        if (has_TcwBefGBA) has_TcwBefGBA[i] = K.hasBef;
    }
    return DRFE_OK;
}

int drfe_lmap_get_gba_points(drfe_lmap* db, int32_t count, const int32_t* handles, float* PosGBA, int32_t* stamp, uint8_t* has_PosGBA)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && !handles)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_gba_points: invalid argument");
    for (int i = 0; i < count; i++)
        if (db->mpGba.find(handles[i]) == db->mpGba.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_gba_points: a handle without state");
    for (int i = 0; i < count; i++) {
        const MpGba& P = db->mpGba.at(handles[i]);
        if (PosGBA) std::memcpy(PosGBA + 3 * (size_t)i, P.X, sizeof(P.X));
        if (stamp) stamp[i] = P.stamp;
        if (has_PosGBA) has_PosGBA[i] = P.hasX;
    }
    return DRFE_OK;
}

int drfe_lmap_gba_host(drfe_lmap* db, int32_t loop, int32_t n_origins, const int32_t* origins, drfe_lmap_gba_out* out)
{
    return gba_entry(db, loop, n_origins, origins, out, 0, nullptr);
}
int drfe_lmap_gba_device(drfe_lmap* db, int32_t loop, int32_t n_origins, const int32_t* origins, drfe_lmap_gba_out* out, void* stream)
{
    return gba_entry(db, loop, n_origins, origins, out, 1, stream);
}
int drfe_lmap_gba_batch(drfe_lmap* db, int32_t loop, int32_t n_origins, const int32_t* origins, drfe_lmap_gba_out* out, void* stream)
{
    return gba_entry(db, loop, n_origins, origins, out, 2, stream);
}

int drfe_lmap_gba_limits(int32_t* out6)
{
    if (!out6) return DRFE_ERR_INVALID;
    out6[0] = GBA_TILE;
    out6[1] = DRFE_LMAP_GBA_DEVICE_FROM;
    out6[2] = 0;
    out6[3] = GBA_POINT_BYTES;
    out6[4] = GBA_FIXED_BYTES;
    out6[5] = 64;
    return DRFE_OK;
}

int drfe_lmap_gba_scratch(drfe_lmap* db, int64_t* out3)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!out3) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_gba_scratch: invalid argument");
    const int rc = lmap_build_image(db);
    if (rc) return rc;
    const GbaFit F = gba_fit(db);
    out3[0] = F.whole;
    out3[1] = F.least;
    out3[2] = F.fixed;
    return DRFE_OK;
}

int drfe_lmap_gba_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::gbaStats, stats); }

}  // extern "C"
