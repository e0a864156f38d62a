/* lmap_create.cpp — map-point and map-line creation on the local-map store: the tail of LocalMapping::CreateNewMapPoints and
 * CreateNewMapLines2 (reference src/LocalMapping.cc:522-535, :1019-1031) with MapPoint::AddObservation and UpdateNormalAndDepth
 * (src/MapPoint.cc:124-138, :376-417), MapLine::AddObservation (src/MapLine.cpp:91-100) and KeyFrame::AddMapPoint / AddMapLine
 * (src/KeyFrame.cc:287-291, :849-853), behind the C-ABI of include/drfe.h: the checks, the walk, the commit into the rows by handle,
 * the append to everything the store keeps by slot, the room in the resident blocks and the counters.  The rules are create_core.h's.
 * A call is checked as a whole before anything is written, on the host, before the device entry (create_kernels.hip) launches
 * anything.  Both entries evaluate create_core.h.  DESIGN.md section 34.  Parity with a build of the reference's files is not
 * pinned: they cannot be built here. */
#include "lmap_call.h"
#include "create_core.h"

#include <algorithm>
#include <cstring>
#include <unordered_set>

using namespace lmap_store;

namespace {

/* one checked creation, in slots: the call's observations and the observers it keeps, in list order */
struct Creation {
    int32_t handle = 0, n = 0, m = 0, ref = 0, level = 0, nObs = 0;
    int32_t kf[2] = {0, 0}, idx[2] = {0, 0}, oKf[2] = {0, 0}, oIdx[2] = {0, 0};
    int32_t prev[2] = {-1, -1};        /* the creation of the call that named the same row entry last before, or -1 */
    int64_t first = 0;
};

struct CreatePlan {
    std::vector<Creation> c[2];        /* points, lines */
    bool normals = false;
    bool append[2] = {true, true};     /* the handles of the kind qualify for the append */
};

bool call_ok(const drfe_lmap_create_call* c)
{
    if (!c || c->n_points < 0 || c->n_lines < 0 || c->displaced_capacity[0] < 0 || c->displaced_capacity[1] < 0 || c->record_capacity < 0) return false;
    if (c->n_points > 0 && (!c->point_handle || !c->point_n_obs || !c->point_obs_kf || !c->point_obs_index || !c->point_ref_kf ||
                            !c->point_first_kf || !c->point_world || !c->point_displaced))
        return false;
    if (c->n_points > 0 && c->normal && (!c->max_distance || !c->min_distance || !c->status)) return false;
    if (c->n_lines > 0 && (!c->line_handle || !c->line_n_obs || !c->line_obs_kf || !c->line_obs_index || !c->line_ref_kf || !c->line_first_kf ||
                           !c->line_displaced))
        return false;
    return true;
}

/* every refusal of a call but the capacities; the images it reads are current */
int create_plan(drfe_lmap* db, const drfe_lmap_create_call* c, CreatePlan& P)
{
    int rc = lmap_build_recent(db);
    P.normals = c->normal != nullptr && c->n_points > 0;
    if (!rc && P.normals) rc = lmap_build_geo(db);
    if (rc) return rc;
    lmap_host_views(db);
    const Image& G = db->img;
    const CullAttr& A = db->cull;
    const GeoImage& E = db->geo;
    const std::string who = "lmap_create: ";
    const int32_t nLevels = (int32_t)db->scales.size();
    for (int kind = 0; kind < 2; kind++) {
        const bool point = kind == FUSE_POINT;
        const int32_t n = point ? c->n_points : c->n_lines;
        const int32_t *handle = point ? c->point_handle : c->line_handle, *nObs = point ? c->point_n_obs : c->line_n_obs,
                      *oKf = point ? c->point_obs_kf : c->line_obs_kf, *oIdx = point ? c->point_obs_index : c->line_obs_index,
                      *ref = point ? c->point_ref_kf : c->line_ref_kf;
        const int64_t* first = point ? c->point_first_kf : c->line_first_kf;
        const std::vector<int32_t>&rowOff = point ? G.kfMpOff : G.kfMlOff, &stored = point ? G.mpHandle : G.mlHandle;
        const char* name = point ? "map point " : "map line ";
        std::unordered_set<int32_t> seen;
        std::unordered_map<int32_t, int32_t> holder;   /* row entry (flat) -> the creation that named it last */
        if (n > (1 << 28)) return lmap_fail(db, DRFE_ERR_INVALID, who + "more than 2^28 creations of a kind in a call");
        int32_t above = stored.empty() ? -1 : stored.back();
        P.c[kind].reserve((size_t)n);
        for (int32_t t = 0; t < n; t++) {
            const std::string it = who + name + std::to_string(handle[t]);
            Creation K;
            K.handle = handle[t];
            if (K.handle < 0) return lmap_fail(db, DRFE_ERR_INVALID, it + ": a negative handle");
            if (point ? db->mp.count(K.handle) != 0 : db->ml.count(K.handle) != 0) return lmap_fail(db, DRFE_ERR_INVALID, it + " is in the store already");
            if (!seen.insert(K.handle).second) return lmap_fail(db, DRFE_ERR_INVALID, it + " stands twice in the call");
            if (K.handle <= above) P.append[kind] = false;
            above = K.handle;
            K.n = nObs[t];
            if (K.n < 1 || K.n > 2) return lmap_fail(db, DRFE_ERR_INVALID, it + ": 1 or 2 observations, not " + std::to_string(K.n));
            K.ref = -1;
            for (int32_t o = 0; o < K.n; o++) {
                const int32_t kh = oKf[2 * (size_t)t + o];
                const auto ks = G.kfSlot.find(kh);
                if (ks == G.kfSlot.end()) return lmap_fail(db, DRFE_ERR_INVALID, it + ": unknown key frame " + std::to_string(kh));
                K.kf[o] = ks->second;
                K.idx[o] = oIdx[2 * (size_t)t + o];
                if (K.idx[o] < 0 || K.idx[o] >= rowOff[(size_t)K.kf[o] + 1] - rowOff[(size_t)K.kf[o]])
                    return lmap_fail(db, DRFE_ERR_INVALID, it + ": index " + std::to_string(K.idx[o]) + " is outside the row of key frame " + std::to_string(kh));
                if (kh == ref[t]) K.ref = K.kf[o];
                const auto was = holder.find(rowOff[(size_t)K.kf[o]] + K.idx[o]);
                if (was != holder.end()) K.prev[o] = was->second;
                holder[rowOff[(size_t)K.kf[o]] + K.idx[o]] = t;
            }
            if (K.ref < 0) return lmap_fail(db, DRFE_ERR_INVALID, it + ": the reference key frame " + std::to_string(ref[t]) + " is not among its observations");
            K.first = first[t];
            K.m = create_observers(K.n, K.kf, K.idx, K.oKf, K.oIdx);
            if (!point) {
                K.nObs = K.m;
                P.c[kind].push_back(K);
                continue;
            }
            for (int32_t o = 0; o < K.m; o++) {
                if (A.kfHas[(size_t)K.oKf[o]] != 2)
                    return lmap_fail(db, DRFE_ERR_STATE, it + ": key frame " + std::to_string(G.kfHandle[(size_t)K.oKf[o]]) + " has no culling attributes that fit its row");
                K.nObs += fuse_obs_weight(FUSE_POINT, A.stereo[(size_t)(G.kfMpOff[(size_t)K.oKf[o]] + K.oIdx[o])]);
            }
            K.level = A.octave[(size_t)(G.kfMpOff[(size_t)K.ref] + create_ref_index(K.m, K.oKf, K.oIdx, K.ref))];
            if (P.normals) {
                if (nLevels <= 0) return lmap_fail(db, DRFE_ERR_STATE, who + "the store has no scales");
                for (int32_t o = 0; o < K.m; o++)
                    if (!E.kfHas[(size_t)K.oKf[o]])
                        return lmap_fail(db, DRFE_ERR_STATE, it + ": observer " + std::to_string(G.kfHandle[(size_t)K.oKf[o]]) + " has no pose");
                if (K.level < 0 || K.level >= nLevels) return lmap_fail(db, DRFE_ERR_STATE, it + ": octave " + std::to_string(K.level) + " is outside the scales");
            }
            P.c[kind].push_back(K);
        }
    }
    return DRFE_OK;
}

/* The new items of one kind into everything that is kept by slot, at the end.  The slot of creation t is base + t. */
void append_slots(drfe_lmap* db, const CreatePlan& P, const drfe_lmap_create_call* c, int kind, bool onDevice)
{
    std::vector<size_t> touched;       /* the row entries written, for the upload after a host call */
    Image& G = db->img;
    CullAttr& A = db->cull;
    RecentAttr& Q = db->rec;
    GeoImage& E = db->geo;
    GbaAttr& B = db->gba;
    const int32_t nLevels = (int32_t)db->scales.size();
    for (size_t t = 0; t < P.c[kind].size(); t++) {
        const Creation& K = P.c[kind][t];
        if (kind == FUSE_POINT) {
            const int32_t s = (int32_t)G.mpHandle.size();
            G.mpHandle.push_back(K.handle);
            G.mpSlot[K.handle] = s;
            G.mpBad.push_back(0);
            G.obs.insert(G.obs.end(), K.oKf, K.oKf + K.m);
            G.obsOff.push_back((int32_t)G.obs.size());
            A.mpHas.push_back(1);
            A.nObs.push_back(K.nObs);
            A.obsIdx.insert(A.obsIdx.end(), K.oIdx, K.oIdx + K.m);
            A.live.insert(A.live.end(), (size_t)K.m, 1);
            Q.mpHas.push_back(1);
            Q.mpFound.push_back(1);
            Q.mpVisible.push_back(1);
            Q.mpFirst.push_back(K.first);
            if (!db->geoDirty) {
                E.mpHas.push_back(1);
                E.mpWorld.insert(E.mpWorld.end(), c->point_world + 3 * t, c->point_world + 3 * t + 3);
                E.mpRef.push_back(K.ref);
                E.mpLevel.push_back(K.level);
                E.mpBy.push_back(0);
                E.mpByRef.push_back(0);
                if (!E.kfHas[(size_t)K.ref] || K.level < 0 || K.level >= nLevels) E.complete = false;
            }
            if (!db->gbaDirty) {
                B.mpPosGBA.insert(B.mpPosGBA.end(), 3, 0.0f);
                B.mpStamp.push_back(0);
                B.mpHasPos.push_back(0);
            }
            if (db->stampP.size() + 1 == G.mpHandle.size()) {
                db->stampP.push_back(0);
                db->inP.push_back(0);
            }
            for (int32_t o = 0; o < K.n; o++) {
                const size_t e = (size_t)(G.kfMpOff[(size_t)K.kf[o]] + K.idx[o]);
                G.kfMp[e] = s;
                touched.push_back(e);
            }
        } else {
            const int32_t s = (int32_t)G.mlHandle.size();
            G.mlHandle.push_back(K.handle);
            G.mlSlot[K.handle] = s;
            G.mlBad.push_back(0);
            Q.mlHas.push_back(1);
            Q.mlFound.push_back(1);
            Q.mlVisible.push_back(1);
            Q.mlFirst.push_back(K.first);
            Q.mlNObs.push_back(K.nObs);
            Q.mlObs.insert(Q.mlObs.end(), K.oKf, K.oKf + K.m);
            Q.mlObsIdx.insert(Q.mlObsIdx.end(), K.oIdx, K.oIdx + K.m);
            Q.mlObsOff.push_back((int32_t)Q.mlObs.size());
            if (db->stampL.size() + 1 == G.mlHandle.size()) {
                db->stampL.push_back(0);
                db->inL.push_back(0);
            }
            for (int32_t o = 0; o < K.n; o++) {
                const size_t e = (size_t)(G.kfMlOff[(size_t)K.kf[o]] + K.idx[o]);
                G.kfMl[e] = s;
                touched.push_back(e);
            }
        }
    }
    if (onDevice) return;
    /* one copy per touched row entry with the next upload; sending the section as one run past some tens of entries is the next
     * thing to do here */
    for (const size_t e : touched) db->blk[drfe_lmap::ROWS].stale_at(kind == FUSE_POINT ? db->secKfMp : db->secKfMl, e);
}

/* UpdateNormalAndDepth of every created point, on the host: the records of the call */
void host_records(drfe_lmap* db, const CreatePlan& P, drfe_lmap_create_call* c)
{
    const CorrImage& C = db->hCorr;
    for (size_t t = 0; t < P.c[0].size(); t++) {
        const Creation& K = P.c[0][t];
        c->status[t] = create_point_normal(C.kfOw, C.scale, C.nLevels, c->point_world + 3 * t, K.m, K.oKf, K.ref, K.level, c->normal + 3 * t,
                                           &c->max_distance[t], &c->min_distance[t]);
    }
}

/* The sections of the resident blocks the call appends to, with the elements each gains per created point, kept point observer,
 * created line and kept line observer.  f(block, section, elements after the call). */
template <class F>
void appended_sections(drfe_lmap* db, const CreatePlan& P, F&& f)
{
    Image& G = db->img;
    CullAttr& A = db->cull;
    RecentAttr& Q = db->rec;
    GeoImage& E = db->geo;
    GbaAttr& B = db->gba;
    size_t nP = P.c[0].size(), nL = P.c[1].size(), oP = 0, oL = 0;
    for (const Creation& K : P.c[0]) oP += (size_t)K.m;
    for (const Creation& K : P.c[1]) oL += (size_t)K.m;
    auto one = [&](int block, auto& v, size_t gain) {
        ResidentBlock& R = db->blk[block];
        f(block, R.section_of(&v), v.size() + gain);
    };
    if (nP) {
        one(drfe_lmap::ROWS, G.mpBad, nP);
        one(drfe_lmap::ROWS, G.obsOff, nP);
        one(drfe_lmap::ROWS, G.obs, oP);
        one(drfe_lmap::ATTR, A.nObs, nP);
        one(drfe_lmap::ATTR, A.obsIdx, oP);
        one(drfe_lmap::RECENT, Q.mpFound, nP);
        one(drfe_lmap::RECENT, Q.mpVisible, nP);
        one(drfe_lmap::RECENT, Q.mpFirst, nP);
        if (!db->geoDirty) {
            one(drfe_lmap::GEO, E.mpWorld, 3 * nP);
            one(drfe_lmap::GEO, E.mpRef, nP);
            one(drfe_lmap::GEO, E.mpLevel, nP);
            one(drfe_lmap::GEO, E.mpBy, nP);
            one(drfe_lmap::GEO, E.mpByRef, nP);
        }
        if (!db->gbaDirty) {
            one(drfe_lmap::GBA, B.mpPosGBA, 3 * nP);
            one(drfe_lmap::GBA, B.mpStamp, nP);
        }
    }
    if (nL) {
        one(drfe_lmap::ROWS, G.mlBad, nL);
        one(drfe_lmap::RECENT, Q.mlFound, nL);
        one(drfe_lmap::RECENT, Q.mlVisible, nL);
        one(drfe_lmap::RECENT, Q.mlFirst, nL);
        one(drfe_lmap::RECENT, Q.mlNObs, nL);
        one(drfe_lmap::RECENT, Q.mlObsOff, nL);
        one(drfe_lmap::RECENT, Q.mlObs, oL);
        one(drfe_lmap::RECENT, Q.mlObsIdx, oL);
    }
}

/* room in the resident blocks for what the call appends, before it does; the number of blocks whose layout that moved */
int64_t grant_room(drfe_lmap* db, const CreatePlan& P)
{
    bool moved[drfe_lmap::BLOCKS] = {false, false, false, false, false, false};
    appended_sections(db, P, [&](int block, int section, size_t need) {
        if (db->blk[block].grant(section, need)) moved[block] = true;
    });
    int64_t n = 0;
    for (const bool m : moved) n += m ? 1 : 0;
    return n;
}

/* the rows by handle, one creation after another; fills the displaced handles and returns how many row entries held an item */
int64_t commit_rows(drfe_lmap* db, const CreatePlan& P, drfe_lmap_create_call* c)
{
    const Image& G = db->img;
    int64_t nDisplaced = 0;
    for (int kind = 0; kind < 2; kind++) {
        const bool point = kind == FUSE_POINT;
        int32_t* displaced = point ? c->point_displaced : c->line_displaced;
        for (size_t t = 0; t < P.c[kind].size(); t++) {
            const Creation& K = P.c[kind][t];
            std::vector<int32_t> obs, idx(K.oIdx, K.oIdx + K.m);
            for (int32_t o = 0; o < K.m; o++) obs.push_back(G.kfHandle[(size_t)K.oKf[o]]);
            if (point) {
                MpRow& R = db->mp[K.handle];
                R.bad = 0;
                R.obs = obs;
                MpCull& U = db->mpCull[K.handle];
                U.nObs = K.nObs;
                U.obsIdx = idx;
                MpGeo& E = db->mpGeo[K.handle];
                std::memcpy(E.X, c->point_world + 3 * t, sizeof(E.X));
                E.ref = G.kfHandle[(size_t)K.ref];
                E.level = K.level;
                E.by = E.byRef = 0;
                db->mpRec[K.handle] = ItemRecent{1, 1, K.first};
                db->mpGba.erase(K.handle);
                db->mpReplaced.erase(K.handle);
            } else {
                db->ml[K.handle] = 0;
                MlObs& O = db->mlObs[K.handle];
                O.nObs = K.nObs;
                O.obs = obs;
                O.obsIdx = idx;
                db->mlRec[K.handle] = ItemRecent{1, 1, K.first};
                db->mlReplaced.erase(K.handle);
            }
            displaced[2 * t + 1] = -1;
            for (int32_t o = 0; o < K.n; o++) {
                KfRow& R = db->kf.at(G.kfHandle[(size_t)K.kf[o]]);
                int32_t& e = (point ? R.mps : R.mls)[(size_t)K.idx[o]];
                displaced[2 * t + o] = e;
                if (e >= 0) nDisplaced++;
                e = K.handle;
            }
        }
    }
    return nDisplaced;
}

/* the scratch of a device call with at most `chunk` creations a chunk */
struct CreateLayout {
    StageLayout<16> scr;
    Section<int32_t> local, tile, claimP, claimL;
};

CreateLayout create_layout(const drfe_lmap* db, size_t chunk)
{
    CreateLayout Y;
    Y.claimP = Y.scr.add<int32_t>(db->img.kfMp.size());
    Y.claimL = Y.scr.add<int32_t>(db->img.kfMl.size());
    Y.local = Y.scr.add<int32_t>(chunk);
    Y.tile = Y.scr.add<int32_t>((chunk + CREATE_TILE - 1) / CREATE_TILE);
    return Y;
}

/* the most creations a chunk, a whole number of tiles, that fit the configured scratch; 0 when not even one tile does */
int64_t create_chunk(const drfe_lmap* db, size_t longest)
{
    const size_t tiles = (longest + CREATE_TILE - 1) / CREATE_TILE;
    if ((int64_t)create_layout(db, longest).scr.bytes() <= db->scratchBytes) return (int64_t)tiles * CREATE_TILE;
    size_t lo = 0, hi = tiles;         /* lo tiles fit (or 0), hi do not */
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if ((int64_t)create_layout(db, mid * CREATE_TILE).scr.bytes() <= db->scratchBytes) lo = mid;
        else hi = mid;
    }
    return (int64_t)lo * CREATE_TILE;
}

/* The device entry: the blocks brought up to date with the granted room, the call staged, chunk after chunk of each kind.  The
 * records come back in slots. */
int create_device(drfe_lmap* db, const CreatePlan& P, const drfe_lmap_create_call* c, int64_t chunk, std::vector<int32_t> displaced[2],
                  int64_t* chunks, void* stream)
{
    const bool geo = !db->geoDirty;
    LmapCall call{db, "lmap create"};
    if (const int rc = call.begin(geo ? (LMAP_NEED_RECENT | LMAP_NEED_GEO) : LMAP_NEED_RECENT, stream)) return rc;
    const size_t nP = P.c[0].size(), nL = P.c[1].size(), n = nP + nL, rec = P.normals ? nP : 0;
    StageLayout<16> in, out;
    const auto sCnt = in.add<int32_t>(n);
    const auto sKf = in.add<int32_t>(2 * n);
    const auto sIdx = in.add<int32_t>(2 * n);
    const auto sRef = in.add<int32_t>(n);
    const auto sPrev = in.add<int32_t>(2 * n);
    const auto sFirst = in.add<int64_t>(n);
    const auto sWorld = in.add<float>(3 * nP);
    const auto oDisp = out.add<int32_t>(2 * n);
    const auto oNrm = out.add<float>(3 * rec);
    const auto oMax = out.add<float>(rec);
    const auto oMin = out.add<float>(rec);
    const auto oStatus = out.add<uint8_t>(rec);
    const CreateLayout Y = create_layout(db, (size_t)std::min<int64_t>(chunk, (int64_t)std::max(nP, nL)));
    if (const int rc = call.stage(in.bytes(), out.bytes(), Y.scr.bytes())) return rc;
    const auto [h, d, dO, dS, r] = call.at;
    /* the point creations from 0, the line creations behind them */
    for (int kind = 0; kind < 2; kind++)
        for (size_t t = 0; t < P.c[kind].size(); t++) {
            const Creation& K = P.c[kind][t];
            const size_t g = (kind ? nP : 0) + t;
            sCnt.at(h)[g] = K.n;
            sRef.at(h)[g] = K.ref;
            sFirst.at(h)[g] = K.first;
            for (int o = 0; o < 2; o++) {
                sKf.at(h)[2 * g + o] = K.kf[o];
                sIdx.at(h)[2 * g + o] = K.idx[o];
                sPrev.at(h)[2 * g + o] = K.prev[o];
            }
        }
    if (nP) std::memcpy(sWorld.at(h), c->point_world, sizeof(float) * 3 * nP);
    if (const int rc = call.send()) return rc;
    /* from here the resident blocks are not what the host arrays hold */
    ResidentBlock* written[4] = {&db->blk[drfe_lmap::ROWS], &db->blk[drfe_lmap::ATTR], &db->blk[drfe_lmap::RECENT], geo ? &db->blk[drfe_lmap::GEO] : nullptr};
    for (ResidentBlock* B : written)
        if (B) B->stale_all();
    hipError_t e = hipSuccess;
    for (int kind = 0; kind < 2 && e == hipSuccess; kind++) {
        const size_t g0 = kind ? nP : 0, count = P.c[kind].size();
        CreateLaunch L{};
        L.I = db->dView;
        L.A = db->dCull;
        L.R = db->dRec;
        L.G = db->dCorr;
        L.kind = kind;
        L.geo = geo ? 1 : 0;
        L.normals = P.normals ? 1 : 0;
        L.slot0 = (int32_t)(kind ? db->img.mlHandle.size() : db->img.mpHandle.size());
        L.cnt = sCnt.at(d) + g0;
        L.kf = sKf.at(d) + 2 * g0;
        L.idx = sIdx.at(d) + 2 * g0;
        L.ref = sRef.at(d) + g0;
        L.prev = sPrev.at(d) + 2 * g0;
        L.first = sFirst.at(d) + g0;
        L.world = sWorld.at(d);
        L.local = Y.local.at(dS);
        L.tile = Y.tile.at(dS);
        L.claim = kind ? Y.claimL.at(dS) : Y.claimP.at(dS);
        L.displaced = oDisp.at(dO) + 2 * g0;
        L.nrm = oNrm.at(dO);
        L.maxD = oMax.at(dO);
        L.minD = oMin.at(dO);
        L.status = oStatus.at(dO);
        int64_t obs0 = (int64_t)(kind ? db->rec.mlObs.size() : db->img.obs.size());
        for (size_t t0 = 0; t0 < count && e == hipSuccess; t0 += (size_t)chunk) {
            L.t0 = (int32_t)t0;
            L.t1 = (int32_t)std::min(count, t0 + (size_t)chunk);
            L.obs0 = (int32_t)obs0;
            e = drfe_launch_create_chunk(L, call.st);
            for (int32_t t = L.t0; t < L.t1; t++) obs0 += P.c[kind][(size_t)t].m;
            (*chunks)++;
        }
    }
    if (const int rc = call.back(e)) return rc;
    for (ResidentBlock* B : written)
        if (B) B->assume_current();
    const int32_t* disp = oDisp.at(r);
    displaced[0].assign(disp, disp + 2 * nP);
    displaced[1].assign(disp + 2 * nP, disp + 2 * n);
    if (rec) {
        std::memcpy(c->normal, oNrm.at(r), sizeof(float) * 3 * rec);
        std::memcpy(c->max_distance, oMax.at(r), sizeof(float) * rec);
        std::memcpy(c->min_distance, oMin.at(r), sizeof(float) * rec);
        std::memcpy(c->status, oStatus.at(r), rec);
    }
    return DRFE_OK;
}

/* mode: 0 host, 1 device, 2 by the crossover */
int create_entry_point(drfe_lmap* db, drfe_lmap_create_call* c, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_create: a device call on a store without a context");
    if (!call_ok(c)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_create: invalid call or output arrays");
    CreatePlan P;
    int rc = create_plan(db, c, P);
    if (rc) return rc;
    if (c->displaced_capacity[0] < 2 * (int64_t)c->n_points) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_create: the call returns more than displaced_capacity[0]");
    if (c->displaced_capacity[1] < 2 * (int64_t)c->n_lines) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_create: the call returns more than displaced_capacity[1]");
    if (P.normals && c->record_capacity < c->n_points) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_create: the call returns more than record_capacity");
    const int64_t total = (int64_t)c->n_points + c->n_lines;
    bool stale = false;
    for (int kind = 0; kind < 2; kind++)
        if (!P.c[kind].empty() && !P.append[kind]) stale = true;
    /* without slots at the end there is nothing the device could write in place */
    bool dev = total > 0 && !stale && (mode == 1 || (mode == 2 && db->ctx && total >= DRFE_LMAP_CREATE_DEVICE_FROM));
    int64_t chunk = 0;
    if (dev) {
        chunk = create_chunk(db, (size_t)std::max(c->n_points, c->n_lines));
        if (!chunk && mode == 1) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_create: the call does not fit the configured device scratch with one tile of creations a chunk");
        dev = chunk > 0;
    }
    int64_t st[8] = {1, 0, c->n_points, c->n_lines, 0, 0, 0, 0};
    if (stale) {
        if (P.normals) host_records(db, P, c);
        st[4] = commit_rows(db, P, c);
        db->imgDirty = true;
        st[5] = 1;
    } else {
        st[6] = grant_room(db, P);
        std::vector<int32_t> slots[2];
        if (dev) {
            rc = create_device(db, P, c, chunk, slots, &st[7], stream);
            if (rc) return rc;
            st[1] = 1;
        } else if (P.normals) {
            host_records(db, P, c);    /* before the geometry image grows: its arrays move */
        }
        st[4] = commit_rows(db, P, c);
        append_slots(db, P, c, FUSE_POINT, dev);
        append_slots(db, P, c, FUSE_LINE, dev);
        if (dev) {
            /* the device wrote what the host arrays hold now; the adjustment block's tail goes up with its next use */
            appended_sections(db, P, [&](int block, int section, size_t) {
                if (block != drfe_lmap::GBA) db->blk[block].took(section);
            });
            /* its report is in slots, of the stored items or of the call's: the same handles the rows gave up on the host */
            const Image& G = db->img;
            for (int kind = 0; kind < 2; kind++) {
                const int32_t* handle = kind ? G.mlHandle.data() : G.mpHandle.data();
                int32_t* o = kind ? c->line_displaced : c->point_displaced;
                for (size_t i = 0; i < slots[kind].size(); i++) o[i] = slots[kind][i] < 0 ? -1 : handle[(size_t)slots[kind][i]];
            }
        }
    }
    for (int i = 0; i < 8; i++) db->createStats[i] += st[i];
    return DRFE_OK;
}

}  // namespace

extern "C" {

int drfe_lmap_create_host(drfe_lmap* db, drfe_lmap_create_call* call) { return create_entry_point(db, call, 0, nullptr); }
int drfe_lmap_create_device(drfe_lmap* db, drfe_lmap_create_call* call, void* stream) { return create_entry_point(db, call, 1, stream); }
int drfe_lmap_create_batch(drfe_lmap* db, drfe_lmap_create_call* call, void* stream) { return create_entry_point(db, call, 2, stream); }

int drfe_lmap_create_limits(int32_t* out8)
{
    if (!out8) return DRFE_ERR_INVALID;
    out8[0] = CREATE_TILE;
    out8[1] = 64;
    out8[2] = CREATE_CLAIM_BYTES;
    out8[3] = CREATE_ITEM_BYTES;
    out8[4] = LMAP_THREADS;
    out8[5] = 0;
    out8[6] = DRFE_LMAP_CREATE_DEVICE_FROM;
    out8[7] = 0;
    return DRFE_OK;
}

int drfe_lmap_create_scratch(drfe_lmap* db, int32_t n_points, int32_t n_lines, int64_t* out3)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!out3 || n_points < 0 || n_lines < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_create_scratch: invalid argument");
    const int rc = lmap_build_recent(db);
    if (rc) return rc;
    const size_t longest = (size_t)std::max(n_points, n_lines);
    out3[0] = (int64_t)create_layout(db, longest).scr.bytes();
    out3[1] = (int64_t)create_layout(db, std::min<size_t>(longest, CREATE_TILE)).scr.bytes();
    out3[2] = (int64_t)create_layout(db, 0).scr.bytes();
    return DRFE_OK;
}

int drfe_lmap_create_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::createStats, stats); }

}  // extern "C"
