/* lmap_cull.cpp — LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:1226-1285) with KeyFrame::SetBadFlag
 * (src/KeyFrame.cc:574-683) on the local-map store, behind the C-ABI of include/drfe.h: the attribute setter and getter, the
 * attribute image, the checks, the host walk, the device entry (cull_kernels.hip), the effects of a verdict, the commit and the
 * counters.  Both sides evaluate cull_core.h.  The decisions of a call come from the host walk or from the device; what a culled
 * key frame does to points, connections and the spanning tree is applied here, from the culled list, in both cases.  The point
 * part works on the image in place and keeps a log, so that a call that is refused late is undone; the graph part works on copies
 * of the touched rows.  DESIGN.md section 28.  Parity with a build of the reference's LocalMapping.cc and KeyFrame.cc is not
 * pinned: neither can be built here. */
#include "lmap_call.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <set>

using namespace lmap_store;

namespace {

}  // namespace

/* the attributes by slot, after the image */
int lmap_build_cull(drfe_lmap* db)
{
    const int rc = lmap_build_image(db);
    if (rc) return rc;
    if (!db->cullDirty) return DRFE_OK;
    const Image& G = db->img;
    CullAttr& A = db->cull;
    const size_t nK = G.kfHandle.size(), nP = G.mpHandle.size();
    A.kfHas.assign(nK, 0);
    A.kfFlags.assign(nK, 0);
    A.thDepth.assign(nK, 0.0f);
    A.octave.assign(G.kfMp.size(), 0);
    A.depth.assign(G.kfMp.size(), 0.0f);
    A.stereo.assign(G.kfMp.size(), 0);
    A.mpHas.assign(nP, 0);
    A.nObs.assign(nP, 0);
    A.obsIdx.assign(G.obs.size(), 0);
    A.live.assign(G.obs.size(), 1);
    for (size_t s = 0; s < nK; s++) {
        const auto it = db->kfCull.find(G.kfHandle[s]);
        if (it == db->kfCull.end()) continue;
        const KfCull& K = it->second;
        const size_t r0 = (size_t)G.kfMpOff[s], len = (size_t)G.kfMpOff[s + 1] - r0;
        A.kfFlags[s] = K.flags;
        A.thDepth[s] = K.thDepth;
        A.kfHas[s] = 1;
        if (K.octave.size() != len) continue;
        A.kfHas[s] = 2;                        /* its arrays fit the row */
        if (len) {
            std::memcpy(&A.octave[r0], K.octave.data(), sizeof(int32_t) * len);
            std::memcpy(&A.depth[r0], K.depth.data(), sizeof(float) * len);
            std::memcpy(&A.stereo[r0], K.stereo.data(), len);
        }
    }
    for (size_t s = 0; s < nP; s++) {
        const auto it = db->mpCull.find(G.mpHandle[s]);
        if (it == db->mpCull.end()) continue;
        const MpCull& P = it->second;
        const size_t o0 = (size_t)G.obsOff[s], len = (size_t)G.obsOff[s + 1] - o0;
        if (P.obsIdx.size() != len) continue;
        A.mpHas[s] = 1;
        A.nObs[s] = P.nObs;
        if (len) std::memcpy(&A.obsIdx[o0], P.obsIdx.data(), sizeof(int32_t) * len);
    }
    /* whether any call can be refused for its attributes: looked at once per edit, so that a call does not walk its observers on
     * the host before the device walks them (a commit keeps what holds here: it only takes observations away) */
    bool complete = true;
    for (size_t s = 0; s < nK && complete; s++) complete = A.kfHas[s] == 2;
    for (size_t s = 0; s < nP && complete; s++) complete = A.mpHas[s] != 0;
    for (size_t p = 0; p < nP && complete; p++)
        for (int32_t o = G.obsOff[p]; o < G.obsOff[p + 1] && complete; o++) {
            const size_t k = (size_t)G.obs[(size_t)o];
            complete = A.obsIdx[(size_t)o] >= 0 && A.obsIdx[(size_t)o] < G.kfMpOff[k + 1] - G.kfMpOff[k];
        }
    A.complete = complete;
    db->cullDirty = false;
    db->recDirty = true;               /* which points have attributes that fit is part of that image */
    db->blk[drfe_lmap::ATTR].stale_all();
    return DRFE_OK;
}

namespace {

/* the walk's state over the image I and the attributes A, host or device; row, mpBad, nObs and live are the caller's working arrays */
CullState cull_state(const LmapImage& I, const CullImage& A, int32_t* row, uint8_t* mpBad, int32_t* nObs, uint8_t* live)
{
    return CullState{I.kfMpOff, I.obsOff, I.obs, row, mpBad, nObs, live, A.thDepth, A.kfFlags, A.octave, A.depth, A.stereo, A.obsIdx};
}

/* on the host the walk works on the image and the counters themselves, and cull_undo takes it back */
CullState host_state(drfe_lmap* db)
{
    lmap_host_views(db);
    return cull_state(db->hView, db->hCull, db->img.kfMp.data(), db->img.mpBad.data(), db->cull.nObs.data(), db->cull.live.data());
}

/* a checked call, in slots */
struct CullPlan {
    int32_t n = 0, monocular = 0, maxRow = 0;
    int64_t sumRows = 0;
    std::vector<int32_t> called, pos, recOff;
};

bool cull_out_ok(const drfe_lmap_cull_out* o)
{
    if (!o) return false;
    const drfe_lmap_conn_rows& r = o->rows;
    return o->touched_capacity >= 0 && o->children_capacity >= 0 && o->nulled_capacity >= 0 && o->points_capacity >= 0 &&
           o->obs_capacity >= 0 && o->record && o->Tcp && o->has_Tcp && o->n_culled && o->culled && o->n_touched && o->n_points &&
           o->children_offsets && o->nulled_offsets && o->obs_offsets && r.weights_capacity >= 0 && r.ordered_capacity >= 0 &&
           r.weight_offsets && r.ordered_offsets && (o->touched_capacity == 0 || (o->touched && o->flags && r.parent && r.first_connection)) &&
           (r.weights_capacity == 0 || (r.weight_kfs && r.weight_w)) && (r.ordered_capacity == 0 || (r.ordered_kfs && r.ordered_w)) &&
           (o->children_capacity == 0 || o->children) && (o->nulled_capacity == 0 || o->nulled) &&
           (o->points_capacity == 0 || (o->points && o->point_n_obs && o->point_ref && o->point_bad)) &&
           (o->obs_capacity == 0 || (o->obs && o->obs_index));
}

/* the handles of a call into slots; refuses an unknown handle, a duplicate and a key frame that is already bad */
int cull_plan(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t monocular, CullPlan& C)
{
    if (n < 0 || (n > 0 && !handles)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_cull: invalid argument");
    if (n > DRFE_LMAP_MAX_QUERIES) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_cull: more than DRFE_LMAP_MAX_QUERIES key frames in a call");
    const int rc = lmap_build_cull(db);
    if (rc) return rc;
    const Image& G = db->img;
    C.n = n;
    C.monocular = monocular ? 1 : 0;
    C.called.resize((size_t)n);
    C.pos.assign(G.kfHandle.size(), -1);
    C.recOff.assign(1, 0);
    for (int j = 0; j < n; j++) {
        const auto it = G.kfSlot.find(handles[j]);
        if (it == G.kfSlot.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_cull: the call names an unknown key-frame handle");
        const size_t s = (size_t)it->second;
        if (C.pos[s] >= 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_cull: the call names a key frame twice");
        if (G.kfBad[s]) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_cull: the call names a key frame that is already bad");
        C.pos[s] = j;
        C.called[(size_t)j] = it->second;
        const int32_t len = G.kfMpOff[s + 1] - G.kfMpOff[s];
        C.maxRow = std::max(C.maxRow, len);
        C.sumRows += len;
        C.recOff.push_back((int32_t)C.sumRows);
    }
    return DRFE_OK;
}

/* DRFE_ERR_STATE and the name of the item when the walk could read an attribute that is not there */
int cull_check(drfe_lmap* db, const CullPlan& C)
{
    const Image& G = db->img;
    const CullAttr& A = db->cull;
    if (A.complete) return DRFE_OK;
    auto lacks = [&](const char* kind, int32_t h, const std::string& of) {
        return lmap_fail(db, DRFE_ERR_STATE, std::string("lmap_cull: ") + kind + " " + std::to_string(h) + of + " has no culling attributes that fit its row");
    };
    for (int j = 0; j < C.n; j++) {
        const size_t k = (size_t)C.called[(size_t)j];
        if (!A.kfHas[k]) return lacks("key frame", G.kfHandle[k], "");
        if (A.kfFlags[k] & CULL_KF_ORIGIN) continue;
        if (A.kfHas[k] != 2) return lacks("key frame", G.kfHandle[k], "");
        for (int32_t e = G.kfMpOff[k]; e < G.kfMpOff[k + 1]; e++) {
            const int32_t p = G.kfMp[(size_t)e];
            if (p < 0) continue;
            const int32_t h = G.mpHandle[(size_t)p];
            if (!A.mpHas[(size_t)p]) return lacks("map point", h, "");
            for (int32_t o = G.obsOff[(size_t)p]; o < G.obsOff[(size_t)p + 1]; o++) {
                const size_t ok = (size_t)G.obs[(size_t)o];
                if (A.kfHas[ok] != 2) return lacks("observing key frame", G.kfHandle[ok], ", of map point " + std::to_string(h) + ",");
                const int32_t idx = A.obsIdx[(size_t)o];
                if (idx < 0 || idx >= G.kfMpOff[ok + 1] - G.kfMpOff[ok])
                    return lmap_fail(db, DRFE_ERR_STATE, "lmap_cull: obs_index " + std::to_string(idx) + " of map point " + std::to_string(h) +
                                                        " lies outside the match row of key frame " + std::to_string(G.kfHandle[ok]));
            }
        }
    }
    return DRFE_OK;
}

typedef std::pair<int32_t, int32_t> Entry;     /* (slot, weight) */

/* a touched key frame's side of the graph, on a copy */
struct GraphWork {
    std::vector<Entry> w, ord;
    std::vector<int32_t> children;             /* ascending slot */
    int32_t parent = -1;
};

struct PointLog {
    int32_t oldNObs = 0, ref = -1;             /* ref: the current reference key frame as a handle, -1 without geometry */
    uint8_t oldBad = 0, refChanged = 0;
};

/* what a call has done so far */
struct CullWork {
    std::vector<int32_t> record, died;         /* n x 4; points gone bad per position */
    std::vector<float> Tcp;
    std::vector<uint8_t> hasTcp;
    std::vector<int32_t> culled, deferred;     /* positions */
    std::map<int32_t, PointLog> pts;           /* by slot: the points that lost an observation */
    std::vector<Entry> nulledLog;              /* (index into the match rows, what stood there) */
    std::map<int32_t, GraphWork> T;            /* by slot */
    std::set<int32_t> nowBad;                  /* culled by this call */
    int64_t walked = 0, emptyBegin = 0;
    bool onDevice = false;
};

bool by_key(const Entry& a, const Entry& b) { return conn_key(a.second, a.first) > conn_key(b.second, b.first); }

GraphWork& touch(const Image& G, CullWork& W, int32_t s)
{
    const auto it = W.T.find(s);
    if (it != W.T.end()) return it->second;
    GraphWork& K = W.T[s];
    for (int32_t i = G.cwOff[(size_t)s]; i < G.cwOff[(size_t)s + 1]; i++) K.w.emplace_back(G.cwKf[(size_t)i], G.cwW[(size_t)i]);
    for (int32_t i = G.coOff[(size_t)s]; i < G.coOff[(size_t)s + 1]; i++) K.ord.emplace_back(G.coKf[(size_t)i], G.coW[(size_t)i]);
    K.children.assign(G.child.begin() + G.childOff[(size_t)s], G.child.begin() + G.childOff[(size_t)s + 1]);
    K.parent = G.kfParent[(size_t)s];
    return K;
}

void add_child(GraphWork& K, int32_t c)
{
    const auto at = std::lower_bound(K.children.begin(), K.children.end(), c);
    if (at == K.children.end() || *at != c) K.children.insert(at, c);
}

/* the image as the call found it, from the log */
void cull_undo(drfe_lmap* db, CullWork& W)
{
    Image& G = db->img;
    CullAttr& A = db->cull;
    for (size_t i = W.nulledLog.size(); i-- > 0;) G.kfMp[(size_t)W.nulledLog[i].first] = W.nulledLog[i].second;
    for (const auto& e : W.pts) {
        const size_t p = (size_t)e.first;
        A.nObs[p] = e.second.oldNObs;
        G.mpBad[p] = e.second.oldBad;
        std::fill(A.live.begin() + G.obsOff[p], A.live.begin() + G.obsOff[p + 1], (uint8_t)1);
    }
}

/* SetBadFlag of the key frame at position j, past the mbNotErase test.  DRFE_ERR_STATE when it has no parent. */
int cull_effects(drfe_lmap* db, const CullPlan& C, CullWork& W, int j)
{
    Image& G = db->img;
    const CullState S = host_state(db);
    const int32_t c = C.called[(size_t)j];
    GraphWork* Kc = &touch(G, W, c);
    const int32_t parent = Kc->parent;
    if (parent < 0)
        return lmap_fail(db, DRFE_ERR_STATE, "lmap_cull: key frame " + std::to_string(G.kfHandle[(size_t)c]) + " would be culled and has no parent");
    /* EraseConnection on every key frame of its weights row */
    const std::vector<Entry> mine = Kc->w;
    for (const Entry& e : mine) {
        GraphWork& Kj = touch(G, W, e.first);
        const auto at = std::lower_bound(Kj.w.begin(), Kj.w.end(), Entry(c, 0), [](const Entry& a, const Entry& b) { return a.first < b.first; });
        if (at == Kj.w.end() || at->first != c) continue;
        Kj.w.erase(at);
        Kj.ord = Kj.w;                         /* UpdateBestCovisibles: every entry */
        std::sort(Kj.ord.begin(), Kj.ord.end(), by_key);
    }
    /* EraseObservation on every entry of its match row that is not null */
    std::vector<Entry> before;
    int32_t died = 0;
    for (int32_t e = G.kfMpOff[(size_t)c]; e < G.kfMpOff[(size_t)c + 1]; e++) {
        const int32_t q = G.kfMp[(size_t)e];
        if (q < 0) continue;
        bool holds = false;
        before.clear();
        for (int32_t o = S.obsOff[q]; o < S.obsOff[q + 1]; o++) {
            if (!S.live[o]) continue;
            if (S.obs[o] == c) {
                holds = true;
                continue;
            }
            const int32_t at = S.kfMpOff[S.obs[o]] + S.obsIdx[o];
            before.emplace_back(at, S.row[at]);
        }
        if (!holds) continue;
        auto ins = W.pts.emplace(q, PointLog());
        PointLog& P = ins.first->second;
        if (ins.second) {
            P.oldNObs = S.nObs[q];
            P.oldBad = S.mpBad[q];
            const auto g = db->mpGeo.find(G.mpHandle[(size_t)q]);
            P.ref = g != db->mpGeo.end() ? g->second.ref : -1;
        }
        int32_t front;
        const int res = cull_erase(S, c, q, &front);
        if (P.ref >= 0 && P.ref == G.kfHandle[(size_t)c]) {
            if (front >= 0) {
                P.ref = G.kfHandle[(size_t)front];
                P.refChanged = 1;
            } else {
                W.emptyBegin++;
            }
        }
        if (res == 3) {
            died++;
            for (const Entry& b : before)      /* the observers are distinct key frames, so an entry is logged once */
                if (b.second >= 0) W.nulledLog.push_back(b);
        }
    }
    W.died[(size_t)j] = died;
    /* the spanning tree */
    Kc = &touch(G, W, c);
    Kc->w.clear();
    Kc->ord.clear();
    std::vector<int32_t> children = Kc->children;
    std::set<int32_t> candidates;
    candidates.insert(parent);
    while (!children.empty()) {
        int32_t max = -1, pC = -1, pP = -1;
        for (const int32_t ch : children) {
            if (G.kfBad[(size_t)ch] || W.nowBad.count(ch)) continue;
            const GraphWork& Kh = touch(G, W, ch);
            for (const Entry& v : Kh.ord) {
                if (!candidates.count(v.first)) continue;
                const auto at = std::lower_bound(Kh.w.begin(), Kh.w.end(), Entry(v.first, 0), [](const Entry& a, const Entry& b) { return a.first < b.first; });
                const int32_t w = at != Kh.w.end() && at->first == v.first ? at->second : 0;   /* GetWeight */
                if (w > max) {
                    pC = ch;
                    pP = v.first;
                    max = w;
                }
            }
        }
        if (pC < 0) break;
        touch(G, W, pC).parent = pP;
        add_child(touch(G, W, pP), pC);
        candidates.insert(pC);
        children.erase(std::find(children.begin(), children.end(), pC));
    }
    for (const int32_t ch : children) {
        touch(G, W, ch).parent = parent;
        add_child(touch(G, W, parent), ch);
    }
    touch(G, W, c).children = children;
    GraphWork& Kp = touch(G, W, parent);
    const auto at = std::lower_bound(Kp.children.begin(), Kp.children.end(), c);
    if (at != Kp.children.end() && *at == c) Kp.children.erase(at);
    /* mTcp = Tcw * mpParent->GetPoseInverse() */
    const auto pc = db->kfPose.find(G.kfHandle[(size_t)c]), pp = db->kfPose.find(G.kfHandle[(size_t)parent]);
    if (pc != db->kfPose.end() && pp != db->kfPose.end()) {
        float Twc[16];
        pose_inverse_kf(pp->second.data(), Twc);
        corr_gemm4(pc->second.data(), Twc, &W.Tcp[16 * (size_t)j]);
        W.hasTcp[(size_t)j] = 1;
    }
    W.nowBad.insert(c);
    W.culled.push_back(j);
    return DRFE_OK;
}

/* the record of position j from its counts, and what follows from the verdict */
int cull_decided(drfe_lmap* db, const CullPlan& C, CullWork& W, int j, int32_t nMPs, int32_t nRedundant)
{
    const uint8_t flags = db->cull.kfFlags[(size_t)C.called[(size_t)j]];
    const bool verdict = !(flags & CULL_KF_ORIGIN) && cull_verdict(nRedundant, nMPs);
    const int action = cull_action(verdict, flags);
    int32_t* rec = &W.record[4 * (size_t)j];
    rec[0] = nMPs;
    rec[1] = nRedundant;
    rec[2] = verdict ? 1 : 0;
    rec[3] = action;
    if (action == CULL_DEFERRED) W.deferred.push_back(j);
    if (action == CULL_CULLED) return cull_effects(db, C, W, j);
    return DRFE_OK;
}

void cull_start(const CullPlan& C, CullWork& W)
{
    const size_t n = (size_t)C.n;
    W.record.assign(4 * n, 0);
    W.died.assign(n, 0);
    W.Tcp.assign(16 * n, 0.0f);
    W.hasTcp.assign(n, 0);
}

/* the reference's loop: key frame after key frame its row, then its verdict */
int cull_host(drfe_lmap* db, const CullPlan& C, CullWork& W)
{
    const Image& G = db->img;
    const CullState S = host_state(db);
    for (int j = 0; j < C.n; j++) {
        const int32_t k = C.called[(size_t)j];
        int32_t nMPs = 0, nRedundant = 0, walked = 0;
        if (!(S.kfFlags[k] & CULL_KF_ORIGIN)) {
            const int32_t len = G.kfMpOff[(size_t)k + 1] - G.kfMpOff[(size_t)k];
            for (int32_t i = 0; i < len; i++) {
                const int v = cull_entry(S, k, i, C.monocular, &walked);
                nMPs += v > 0;
                nRedundant += v > 1;
            }
        }
        W.walked += walked;
        const int rc = cull_decided(db, C, W, j, nMPs, nRedundant);
        if (rc) return rc;
    }
    return DRFE_OK;
}

/* how a device call divides the scratch: the working state is shared, a chunk adds the records of its rows */
struct CullFit {
    int64_t fixed = 0, whole = 0, least = 0;
    bool fits = false;
};

CullFit cull_fit(const drfe_lmap* db, const CullPlan& C)
{
    const Image& G = db->img;
    CullFit F;
    F.fixed = 4 * (int64_t)G.kfMp.size() + 10 * (int64_t)G.mpHandle.size() + (int64_t)G.obs.size() + (int64_t)sizeof(CullSpec) * C.n + 1024;
    F.whole = F.fixed + CULL_ENTRY_BYTES * C.sumRows;
    F.least = F.fixed + CULL_ENTRY_BYTES * (int64_t)C.maxRow;
    F.fits = F.least <= db->scratchBytes;
    return F;
}

/* The working state copied from the resident image, the chunks one after another on the stream, the counts of every position
 * back in one copy; then the effects of the verdicts here, in order, as the host entry applies them.  The resident image is only
 * read. */
int cull_device(drfe_lmap* db, const CullPlan& C, const CullFit& F, CullWork& W, void* stream)
{
    LmapCall call{db, "lmap cull"};
    if (const int rc = call.begin(LMAP_NEED_ATTR, stream)) return rc;
    const Image& G = db->img;
    const size_t n = (size_t)C.n, nK = G.kfHandle.size(), nP = G.mpHandle.size();
    const int64_t room = (std::min<int64_t>(db->scratchBytes, F.whole) - F.fixed) / CULL_ENTRY_BYTES;
    int64_t chunkRows = 0, rows = 0;
    for (size_t j = 0; j < n; j++) {
        const int64_t len = C.recOff[j + 1] - C.recOff[j];
        if (rows + len > room) rows = 0;
        rows += len;
        chunkRows = std::max(chunkRows, rows);
    }
    StageLayout<16> in, out, scr;
    const auto sCalled = in.add<int32_t>(n);
    const auto sPos = in.add<int32_t>(nK);
    const auto sRecOff = in.add<int32_t>(n + 1);
    const auto oOut = out.add<int32_t>(CULL_OUT_WORDS * n);
    const auto xRow = scr.add<int32_t>(G.kfMp.size());
    const auto xNObs = scr.add<int32_t>(nP);
    const auto xClaim = scr.add<int32_t>(nP);
    const auto xBad = scr.add<uint8_t>(nP);
    const auto xLive = scr.add<uint8_t>(G.obs.size());
    const auto xTouched = scr.add<uint8_t>(nP);
    const auto xSpec = scr.add<CullSpec>(n);
    const auto xRec = scr.add<CullRecord>((size_t)chunkRows);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, ho] = call.at;
    sCalled.put(h, C.called.data());
    sPos.put(h, C.pos.data());
    sRecOff.put(h, C.recOff.data());
    if (const int rc = call.send()) return rc;
    hipError_t e = hipSuccess;
    if (xRow.bytes()) e = hipMemcpyAsync(xRow.at(dS), db->dView.kfMp, xRow.bytes(), hipMemcpyDeviceToDevice, call.st);
    if (e == hipSuccess && nP) e = hipMemcpyAsync(xNObs.at(dS), db->dCull.nObs, xNObs.bytes(), hipMemcpyDeviceToDevice, call.st);
    if (e == hipSuccess && nP) e = hipMemcpyAsync(xBad.at(dS), db->dView.mpBad, xBad.bytes(), hipMemcpyDeviceToDevice, call.st);
    if (e == hipSuccess && nP) e = hipMemsetAsync(xClaim.at(dS), 0xff, xClaim.bytes(), call.st);
    if (e == hipSuccess && xLive.bytes()) e = hipMemsetAsync(xLive.at(dS), 1, xLive.bytes(), call.st);
    if (e == hipSuccess) e = hipMemsetAsync(xSpec.at(dS), 0, xSpec.bytes(), call.st);
    CullLaunch L{};
    L.S = cull_state(db->dView, db->dCull, xRow.at(dS), xBad.at(dS), xNObs.at(dS), xLive.at(dS));
    L.monocular = C.monocular;
    L.called = sCalled.at(d);
    L.pos = sPos.at(d);
    L.recOff = sRecOff.at(d);
    L.rec = xRec.at(dS);
    L.claim = xClaim.at(dS);
    L.touched = xTouched.at(dS);
    L.spec = xSpec.at(dS);
    L.out = oOut.at(dO);
    for (size_t j0 = 0; j0 < n && e == hipSuccess;) {
        size_t j1 = j0;
        rows = 0;
        int32_t maxRow = 0;
        while (j1 < n) {
            const int64_t len = C.recOff[j1 + 1] - C.recOff[j1];
            if (j1 > j0 && rows + len > room) break;
            rows += len;
            maxRow = std::max(maxRow, (int32_t)len);
            j1++;
        }
        L.j0 = (int32_t)j0;
        L.j1 = (int32_t)j1;
        L.maxRow = maxRow;
        if (nP) e = hipMemsetAsync(xTouched.at(dS), 0, xTouched.bytes(), call.st);
        if (e == hipSuccess) e = drfe_launch_cull_chunk(L, call.st);
        j0 = j1;
    }
    if (const int rc = call.back(e)) return rc;
    const int32_t* res = oOut.at(ho);
    W.onDevice = true;
    for (size_t j = 0; j < n; j++) {
        const int32_t* r = res + CULL_OUT_WORDS * j;
        if (const int rc = cull_decided(db, C, W, (int)j, r[0], r[1])) return rc;
        if (W.record[4 * j + 3] != r[2] || W.died[j] != r[3])
            return lmap_fail(db, DRFE_ERR_STATE, "lmap cull device call: the device and the host disagree on key frame " +
                                                std::to_string(G.kfHandle[(size_t)C.called[j]]));
        W.walked += (int64_t)(uint32_t)r[4] | ((int64_t)r[5] << 32);
    }
    return DRFE_OK;
}

/* a CSR array with the rows of `fresh` (by slot) in place of the stored ones */
template <class T, class Rows>
void splice(std::vector<int32_t>& off, std::vector<T>& data, const Rows& fresh)
{
    std::vector<int32_t> nOff(1, 0);
    std::vector<T> nData;
    nData.reserve(data.size());
    const size_t rows = off.size() - 1;
    auto it = fresh.begin();
    for (size_t s = 0; s < rows; s++) {
        if (it != fresh.end() && (size_t)it->first == s) {
            nData.insert(nData.end(), it->second.begin(), it->second.end());
            ++it;
        } else {
            nData.insert(nData.end(), data.begin() + off[s], data.begin() + off[s + 1]);
        }
        nOff.push_back((int32_t)nData.size());
    }
    off.swap(nOff);
    data.swap(nData);
}

/* results into the caller's arrays and the changes into the store, or the image as it was */
int cull_finish(drfe_lmap* db, const CullPlan& C, CullWork& W, drfe_lmap_cull_out* o)
{
    Image& G = db->img;
    CullAttr& A = db->cull;
    auto handle = [&](int32_t s) { return s >= 0 ? G.kfHandle[(size_t)s] : -1; };
    /* the nulled indices per key frame */
    std::map<int32_t, std::vector<int32_t>> nulled;
    for (const Entry& e : W.nulledLog) {
        const size_t k = (size_t)(std::upper_bound(G.kfMpOff.begin(), G.kfMpOff.end(), e.first) - G.kfMpOff.begin()) - 1;
        nulled[(int32_t)k].push_back(e.first - G.kfMpOff[k]);
    }
    for (auto& e : nulled) std::sort(e.second.begin(), e.second.end());
    /* the touched key frames: whatever differs from the stored state */
    struct Touched {
        int32_t s;
        uint8_t flags;
    };
    std::vector<Touched> touched;
    std::set<int32_t> cand;
    for (const auto& e : W.T) cand.insert(e.first);
    for (const auto& e : nulled) cand.insert(e.first);
    int64_t tW = 0, tO = 0, tCh = 0, tNu = 0;
    for (const int32_t s : cand) {
        GraphWork& K = touch(G, W, s);
        const size_t u = (size_t)s;
        auto same = [&](const std::vector<Entry>& row, const std::vector<int32_t>& off, const std::vector<int32_t>& kf, const std::vector<int32_t>& w) {
            if ((int32_t)row.size() != off[u + 1] - off[u]) return false;
            for (size_t i = 0; i < row.size(); i++)
                if (row[i].first != kf[(size_t)off[u] + i] || row[i].second != w[(size_t)off[u] + i]) return false;
            return true;
        };
        uint8_t f = 0;
        if (!same(K.w, G.cwOff, G.cwKf, G.cwW)) f |= 1;
        if (!same(K.ord, G.coOff, G.coKf, G.coW)) f |= 2;
        if (K.parent != G.kfParent[u]) f |= 4;
        if ((int32_t)K.children.size() != G.childOff[u + 1] - G.childOff[u] || !std::equal(K.children.begin(), K.children.end(), G.child.begin() + G.childOff[u]))
            f |= 8;
        if (nulled.count(s)) f |= 16;
        if (W.nowBad.count(s)) f |= 32;
        if (!f) continue;
        touched.push_back({s, f});
        tW += (int64_t)K.w.size();
        tO += (int64_t)K.ord.size();
        tCh += (int64_t)K.children.size();
        if (f & 16) tNu += (int64_t)nulled[s].size();
    }
    int64_t tObs = 0;
    const CullState S = host_state(db);
    for (const auto& e : W.pts)
        for (int32_t q = S.obsOff[e.first]; q < S.obsOff[e.first + 1]; q++) tObs += S.live[q];
    const char* small = nullptr;
    if ((int64_t)touched.size() > o->touched_capacity) small = "touched_capacity";
    else if (tW > o->rows.weights_capacity) small = "weights_capacity";
    else if (tO > o->rows.ordered_capacity) small = "ordered_capacity";
    else if (tCh > o->children_capacity) small = "children_capacity";
    else if (tNu > o->nulled_capacity) small = "nulled_capacity";
    else if ((int64_t)W.pts.size() > o->points_capacity) small = "points_capacity";
    else if (tObs > o->obs_capacity) small = "obs_capacity";
    if (small) {
        cull_undo(db, W);
        return lmap_fail(db, DRFE_ERR_CAPACITY, std::string("lmap_cull: the call returns more than ") + small);
    }
    /* per called key frame */
    const size_t n = (size_t)C.n;
    if (n) {
        std::memcpy(o->record, W.record.data(), sizeof(int32_t) * 4 * n);
        std::memcpy(o->Tcp, W.Tcp.data(), sizeof(float) * 16 * n);
        std::memcpy(o->has_Tcp, W.hasTcp.data(), n);
    }
    *o->n_culled = (int32_t)W.culled.size();
    for (size_t i = 0; i < W.culled.size(); i++) o->culled[i] = handle(C.called[(size_t)W.culled[i]]);
    /* per touched key frame, and its rows into the store */
    *o->n_touched = (int32_t)touched.size();
    o->rows.weight_offsets[0] = o->rows.ordered_offsets[0] = 0;
    o->children_offsets[0] = o->nulled_offsets[0] = 0;
    int32_t aW = 0, aO = 0, aCh = 0, aNu = 0;
    std::map<int32_t, std::vector<int32_t>> fwKf, fwW, foKf, foW, fCh;
    for (size_t t = 0; t < touched.size(); t++) {
        const int32_t s = touched[t].s, h = handle(s);
        const uint8_t f = touched[t].flags;
        const GraphWork& K = W.T.at(s);
        o->touched[t] = h;
        o->flags[t] = f;
        const int32_t w0 = aW, o0 = aO, c0 = aCh;
        for (const Entry& e : K.w) {
            o->rows.weight_kfs[aW] = handle(e.first);
            o->rows.weight_w[aW++] = e.second;
        }
        for (const Entry& e : K.ord) {
            o->rows.ordered_kfs[aO] = handle(e.first);
            o->rows.ordered_w[aO++] = e.second;
        }
        for (const int32_t ch : K.children) o->children[aCh++] = handle(ch);
        if (f & 16)
            for (const int32_t i : nulled[s]) o->nulled[aNu++] = i;
        o->rows.weight_offsets[t + 1] = aW;
        o->rows.ordered_offsets[t + 1] = aO;
        o->children_offsets[t + 1] = aCh;
        o->nulled_offsets[t + 1] = aNu;
        o->rows.parent[t] = handle(K.parent);
        o->rows.first_connection[t] = G.kfFirst[(size_t)s];
        /* the commit of this key frame */
        KfRow& R = db->kf.at(h);
        if (f & 3) {
            ConnRow& Cn = db->conn[h];
            if (f & 1) {
                Cn.wKf.assign(o->rows.weight_kfs + w0, o->rows.weight_kfs + aW);
                Cn.wW.assign(o->rows.weight_w + w0, o->rows.weight_w + aW);
                std::vector<int32_t>& a = fwKf[s];
                std::vector<int32_t>& b = fwW[s];
                for (const Entry& e : K.w) {
                    a.push_back(e.first);
                    b.push_back(e.second);
                }
            }
            if (f & 2) {
                Cn.oKf.assign(o->rows.ordered_kfs + o0, o->rows.ordered_kfs + aO);
                Cn.oW.assign(o->rows.ordered_w + o0, o->rows.ordered_w + aO);
                std::vector<int32_t>& a = foKf[s];
                std::vector<int32_t>& b = foW[s];
                for (const Entry& e : K.ord) {
                    a.push_back(e.first);
                    b.push_back(e.second);
                }
                for (int k = 0; k < LMAP_NEIGHBOURS; k++) {
                    const int32_t v = k < (int)K.ord.size() ? K.ord[(size_t)k].first : -1;
                    G.kfNbr[(size_t)s * LMAP_NEIGHBOURS + (size_t)k] = v;
                    R.nbr[k] = handle(v);
                }
            }
        }
        if (f & 4) {
            R.parent = handle(K.parent);
            G.kfParent[(size_t)s] = K.parent;
        }
        if (f & 8) {
            R.children.assign(o->children + c0, o->children + aCh);
            fCh[s] = K.children;
        }
        if (f & 16)
            for (const int32_t i : nulled[s]) R.mps[(size_t)i] = -1;
        if (f & 32) {
            R.bad = 1;
            G.kfBad[(size_t)s] = 1;
        }
    }
    if (!fwKf.empty()) {
        std::vector<int32_t> off = G.cwOff;
        splice(off, G.cwKf, fwKf);
        splice(G.cwOff, G.cwW, fwW);
    }
    if (!foKf.empty()) {
        std::vector<int32_t> off = G.coOff;
        splice(off, G.coKf, foKf);
        splice(G.coOff, G.coW, foW);
    }
    if (!fCh.empty()) splice(G.childOff, G.child, fCh);
    /* per touched point, and its row into the store */
    *o->n_points = (int32_t)W.pts.size();
    o->obs_offsets[0] = 0;
    int32_t aP = 0, aOb = 0;
    bool refMoved = false;
    std::map<int32_t, std::vector<int32_t>> fObs, fIdx;
    for (const auto& e : W.pts) {
        const int32_t p = e.first, h = G.mpHandle[(size_t)p];
        const PointLog& P = e.second;
        std::vector<int32_t>& keptObs = fObs[p];
        std::vector<int32_t>& keptIdx = fIdx[p];
        MpRow& R = db->mp.at(h);
        MpCull& Q = db->mpCull.at(h);
        std::vector<int32_t> rowObs;
        for (int32_t q = S.obsOff[p]; q < S.obsOff[p + 1]; q++) {
            if (!S.live[q]) continue;
            keptObs.push_back(S.obs[q]);
            keptIdx.push_back(S.obsIdx[q]);
            rowObs.push_back(handle(S.obs[q]));
            o->obs[aOb] = handle(S.obs[q]);
            o->obs_index[aOb++] = S.obsIdx[q];
        }
        o->points[aP] = h;
        o->point_n_obs[aP] = S.nObs[p];
        o->point_ref[aP] = P.ref;
        o->point_bad[aP] = S.mpBad[p];
        o->obs_offsets[++aP] = aOb;
        R.bad = S.mpBad[p];
        R.obs.swap(rowObs);
        Q.nObs = S.nObs[p];
        Q.obsIdx = keptIdx;
        if (P.refChanged) {
            db->mpGeo.at(h).ref = P.ref;
            refMoved = true;
        }
    }
    if (!fObs.empty()) {
        std::vector<int32_t> off = G.obsOff;
        splice(off, G.obs, fObs);
        splice(G.obsOff, A.obsIdx, fIdx);
        A.live.assign(G.obs.size(), 1);
    }
    for (const int32_t j : W.deferred) {
        const size_t s = (size_t)C.called[(size_t)j];
        db->kfCull.at(G.kfHandle[s]).flags |= CULL_KF_TO_BE_ERASED;
        A.kfFlags[s] |= CULL_KF_TO_BE_ERASED;
    }
    /* what the device copy now lacks, piece by piece: the bad flags and the graph block after a cull, the nulled entries one by
     * one, the observations and their offsets when a row got shorter, with the counters and indices parallel to them; a deferred
     * key frame's flag is the one change in front of those */
    ResidentBlock &rows = db->blk[drfe_lmap::ROWS], &attr = db->blk[drfe_lmap::ATTR];
    if (!W.culled.empty()) {
        rows.stale(0, db->secMlBad);
        db->blk[drfe_lmap::GRAPH].stale_all();
    }
    for (const Entry& e : W.nulledLog) rows.stale_at(db->secKfMp, (size_t)e.first);
    if (!W.pts.empty()) {
        rows.stale(db->secObsOff);
        attr.stale(db->secNObs);
    }
    if (!W.deferred.empty()) attr.stale_all();
    if (refMoved) db->geoDirty = true;
    int64_t died = 0;
    for (const int32_t d : W.died) died += d;
    int64_t* st = db->cullStats;
    if (C.n) st[0]++;
    st[1] += C.n;
    if (W.onDevice) st[2]++;
    st[3] += (int64_t)W.culled.size();
    st[4] += (int64_t)W.deferred.size();
    st[5] += died;
    st[6] += W.walked;
    st[7] += W.emptyBegin;
    return DRFE_OK;
}

/* mode: 0 host, 1 device, 2 by the crossover */
int cull_entry_point(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t monocular, drfe_lmap_cull_out* o, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_cull: a device call on a store without a context");
    if (!cull_out_ok(o)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_cull: invalid output arrays");
    CullPlan C;
    int rc = cull_plan(db, n, handles, monocular, C);
    if (rc) return rc;
    rc = cull_check(db, C);
    if (rc) return rc;
    bool dev = n > 0 && (mode == 1 || (mode == 2 && db->ctx && n >= DRFE_LMAP_CULL_DEVICE_FROM));
    CullFit F;
    if (dev) {
        F = cull_fit(db, C);
        if (!F.fits && mode == 1)
            return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_cull: the working state and the longest called row do not fit the configured device scratch");
        dev = F.fits;
    }
    CullWork W;
    cull_start(C, W);
    rc = dev ? cull_device(db, C, F, W, stream) : cull_host(db, C, W);
    if (rc) {
        cull_undo(db, W);
        return rc;
    }
    return cull_finish(db, C, W, o);
}

}  // namespace

extern "C" {

int drfe_lmap_set_cull_attributes(drfe_lmap* db, const drfe_lmap_cull_attributes* r)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!r || r->n_kfs < 0 || r->n_points < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_cull_attributes: invalid argument");
    const int nk = r->n_kfs, np = r->n_points;
    if (nk > 0 && (!r->kf_handle || !r->th_depth || !r->kf_flags || !lmap_offsets_ok(r->row_offsets, nk) ||
                   (r->row_offsets[nk] > 0 && (!r->octave || !r->depth || !r->stereo))))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_cull_attributes: invalid key-frame arrays");
    if (np > 0 && (!r->point_handle || !r->n_obs || !lmap_offsets_ok(r->obs_offsets, np) || (r->obs_offsets[np] > 0 && !r->obs_index)))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_cull_attributes: invalid map-point arrays");
    for (int i = 0; i < nk; i++)
        if (r->kf_handle[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_cull_attributes: a negative handle");
    for (int i = 0; i < np; i++)
        if (r->point_handle[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_cull_attributes: a negative handle");
    for (int i = 0; i < nk; i++) {
        KfCull& K = db->kfCull[r->kf_handle[i]];
        const int32_t a = r->row_offsets[i], b = r->row_offsets[i + 1];
        K.thDepth = r->th_depth[i];
        K.flags = r->kf_flags[i];
        K.octave.assign(r->octave + a, r->octave + b);
        K.depth.assign(r->depth + a, r->depth + b);
        K.stereo.resize((size_t)(b - a));
        for (int32_t e = a; e < b; e++) K.stereo[(size_t)(e - a)] = r->stereo[e] ? 1 : 0;
    }
    for (int i = 0; i < np; i++) {
        MpCull& P = db->mpCull[r->point_handle[i]];
        P.nObs = r->n_obs[i];
        P.obsIdx.assign(r->obs_index + r->obs_offsets[i], r->obs_index + r->obs_offsets[i + 1]);
    }
    if (nk || np) db->cullDirty = true;
    return DRFE_OK;
}

int drfe_lmap_get_cull_attributes(drfe_lmap* db, drfe_lmap_cull_attributes_out* o)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!o || o->n_kfs < 0 || o->n_points < 0 || o->row_capacity < 0 || o->obs_capacity < 0 ||
        (o->n_kfs > 0 && (!o->kf_handle || !o->th_depth || !o->kf_flags || !o->row_offsets)) ||
        (o->row_capacity > 0 && (!o->octave || !o->depth || !o->stereo)) ||
        (o->n_points > 0 && (!o->point_handle || !o->n_obs || !o->obs_offsets)) || (o->obs_capacity > 0 && !o->obs_index))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_cull_attributes: invalid argument");
    int64_t tR = 0, tO = 0;
    for (int i = 0; i < o->n_kfs; i++) {
        const auto it = db->kfCull.find(o->kf_handle[i]);
        if (it == db->kfCull.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_cull_attributes: a key frame without attributes");
        tR += (int64_t)it->second.octave.size();
    }
    for (int i = 0; i < o->n_points; i++) {
        const auto it = db->mpCull.find(o->point_handle[i]);
        if (it == db->mpCull.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_cull_attributes: a map point without attributes");
        tO += (int64_t)it->second.obsIdx.size();
    }
    if (tR > o->row_capacity || tO > o->obs_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_get_cull_attributes: an output array is too small");
    int32_t a = 0;
    if (o->n_kfs) o->row_offsets[0] = 0;
    for (int i = 0; i < o->n_kfs; i++) {
        const KfCull& K = db->kfCull.at(o->kf_handle[i]);
        o->th_depth[i] = K.thDepth;
        o->kf_flags[i] = K.flags;
        for (size_t e = 0; e < K.octave.size(); e++, a++) {
            o->octave[a] = K.octave[e];
            o->depth[a] = K.depth[e];
            o->stereo[a] = K.stereo[e];
        }
        o->row_offsets[i + 1] = a;
    }
    a = 0;
    if (o->n_points) o->obs_offsets[0] = 0;
    for (int i = 0; i < o->n_points; i++) {
        const MpCull& P = db->mpCull.at(o->point_handle[i]);
        o->n_obs[i] = P.nObs;
        for (const int32_t v : P.obsIdx) o->obs_index[a++] = v;
        o->obs_offsets[i + 1] = a;
    }
    return DRFE_OK;
}

int drfe_lmap_cull_host(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t monocular, drfe_lmap_cull_out* o)
{
    return cull_entry_point(db, n, handles, monocular, o, 0, nullptr);
}
int drfe_lmap_cull_device(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t monocular, drfe_lmap_cull_out* o, void* stream)
{
    return cull_entry_point(db, n, handles, monocular, o, 1, stream);
}
int drfe_lmap_cull_batch(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t monocular, drfe_lmap_cull_out* o, void* stream)
{
    return cull_entry_point(db, n, handles, monocular, o, 2, stream);
}

int drfe_lmap_cull_limits(int32_t* out4)
{
    if (!out4) return DRFE_ERR_INVALID;
    out4[0] = CULL_TILE;
    out4[1] = DRFE_LMAP_CULL_DEVICE_FROM;
    out4[2] = CULL_ENTRY_BYTES;
    out4[3] = CULL_WALK_THREADS;
    return DRFE_OK;
}

int drfe_lmap_cull_scratch(drfe_lmap* db, int32_t n, const int32_t* handles, int64_t* out3)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!out3) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_cull_scratch: invalid argument");
    CullPlan C;
    const int rc = cull_plan(db, n, handles, 0, C);
    if (rc) return rc;
    const CullFit F = cull_fit(db, C);
    out3[0] = F.whole;
    out3[1] = F.least;
    out3[2] = F.fixed;
    return DRFE_OK;
}

int drfe_lmap_cull_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::cullStats, stats); }

}  // extern "C"
