/* lmap_insert.cpp — the item loops of LocalMapping::ProcessNewKeyFrame (reference src/LocalMapping.cc:113-173) with
 * MapPoint::AddObservation and UpdateNormalAndDepth (src/MapPoint.cc:124-138, :370-417) and MapLine::AddObservation
 * (src/MapLine.cpp:91-100) on the local-map store, behind the C-ABI of include/drfe.h: the checks, the host walk, the device entry
 * (insert_kernels.hip), the commit and the counters.  Both sides evaluate insert_core.h.  The walk of either entry only decides:
 * it returns the actions, the lists and the records, and one commit applies them to the rows by handle and to the image - marking
 * for upload what the host entry changed, and only the spliced observation arrays after the device entry, which added to nObs in
 * the resident blocks itself.  DESIGN.md section 33.  Parity with a build of the reference's LocalMapping.cc, MapPoint.cc and
 * MapLine.cpp is not pinned: they cannot be built here. */
#include "lmap_call.h"

#include <algorithm>
#include <cstring>
#include <unordered_set>

using namespace lmap_store;

namespace {

/* a checked call, in slots */
struct InsPlan {
    int32_t n = 0, words = 0;
    bool normals = false;
    std::vector<int32_t> called, segOff, byRank, rankOf;
    int32_t entries(int kind) const { return segOff[(size_t)(kind + 1) * n] - segOff[(size_t)kind * n]; }
    int32_t total() const { return segOff[2 * (size_t)n]; }
};

/* what a walk decided: per entry of the flat space its action; the ADDED entries and the RECENT items (slots) of each kind in
 * walk order; per ADDED point entry its record */
struct InsWork {
    std::vector<uint8_t> action, status;
    std::vector<int32_t> addEntry[2], recent[2];
    std::vector<float> nrm, maxD, minD;
};

bool call_ok(const drfe_lmap_insert_call* c)
{
    if (!c || c->n < 0 || (c->n > 0 && !c->handles) || !c->point_offsets || !c->line_offsets || !c->n_added || !c->n_recent) return false;
    for (int k = 0; k < 2; k++)
        if (c->action_capacity[k] < 0 || c->added_capacity[k] < 0 || c->recent_capacity[k] < 0) return false;
    if (c->action_capacity[0] > 0 && !c->point_action) return false;
    if (c->action_capacity[1] > 0 && !c->line_action) return false;
    if (c->added_capacity[0] > 0 && (!c->added_points || !c->added_point_kf || !c->added_point_index)) return false;
    if (c->added_capacity[0] > 0 && c->normal && (!c->max_distance || !c->min_distance || !c->status)) return false;
    if (c->added_capacity[1] > 0 && (!c->added_lines || !c->added_line_kf || !c->added_line_index)) return false;
    if (c->recent_capacity[0] > 0 && !c->recent_points) return false;
    if (c->recent_capacity[1] > 0 && !c->recent_lines) return false;
    return true;
}

int insert_plan(drfe_lmap* db, int32_t n, const int32_t* handles, bool normals, InsPlan& P)
{
    if (n > DRFE_LMAP_MAX_QUERIES) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_insert: more than DRFE_LMAP_MAX_QUERIES key frames in a call");
    int rc = lmap_build_recent(db);
    if (!rc && normals) rc = lmap_build_geo(db);
    if (rc) return rc;
    lmap_host_views(db);
    const Image& G = db->img;
    P.n = n;
    P.normals = normals;
    P.words = (n + 31) / 32;
    std::unordered_set<int32_t> seen;
    for (int j = 0; j < n; j++) {
        const auto it = G.kfSlot.find(handles[j]);
        if (it == G.kfSlot.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_insert: unknown key frame " + std::to_string(handles[j]));
        if (!seen.insert(handles[j]).second) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_insert: key frame " + std::to_string(handles[j]) + " is named twice");
        P.called.push_back(it->second);
    }
    P.segOff.assign(1, 0);
    int64_t total = 0;
    for (int kind = 0; kind < 2; kind++)
        for (int j = 0; j < n; j++) {
            const std::vector<int32_t>& off = kind == FUSE_POINT ? G.kfMpOff : G.kfMlOff;
            total += off[(size_t)P.called[(size_t)j] + 1] - off[(size_t)P.called[(size_t)j]];
            if (total > 0x7fffffff) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_insert: the called rows are too long for one call");
            P.segOff.push_back((int32_t)total);
        }
    P.byRank.resize((size_t)n);
    for (int j = 0; j < n; j++) P.byRank[(size_t)j] = j;
    std::sort(P.byRank.begin(), P.byRank.end(), [&](int32_t a, int32_t b) { return P.called[(size_t)a] < P.called[(size_t)b]; });
    P.rankOf.resize((size_t)n);
    for (int r = 0; r < n; r++) P.rankOf[(size_t)P.byRank[(size_t)r]] = r;
    return DRFE_OK;
}

/* no call of this store can be refused for a missing piece: a device call need not walk on the host first */
bool nothing_missing(const drfe_lmap* db, const InsPlan& P)
{
    return db->cull.complete && db->rec.complete && (!P.normals || db->geo.complete);
}

/* The reference's loops, key frame after key frame, on the image; nothing is written.  Returns DRFE_OK or the refusal. */
int host_walk(drfe_lmap* db, const InsPlan& P, InsWork& W)
{
    const Image& G = db->img;
    const CullAttr& A = db->cull;
    const RecentAttr& Q = db->rec;
    const GeoImage& E = db->geo;
    const CorrImage& C = db->hCorr;
    const LmapImage& I = db->hView;
    W.action.assign((size_t)P.total(), INS_NULL);
    /* the row index at which the key frame at hand first named the item: stamped by position */
    std::vector<int32_t> stamp[2];
    stamp[0].assign(G.mpHandle.size(), -1);
    stamp[1].assign(G.mlHandle.size(), -1);
    std::unordered_map<int32_t, std::vector<uint32_t>> adders;
    const std::string who = "lmap_insert: ";
    for (int kind = 0; kind < 2; kind++) {
        const bool point = kind == FUSE_POINT;
        const std::vector<int32_t>&rowOff = point ? G.kfMpOff : G.kfMlOff, &row = point ? G.kfMp : G.kfMl;
        const std::vector<int32_t>&obsOff = point ? G.obsOff : Q.mlObsOff, &obs = point ? G.obs : Q.mlObs;
        const std::vector<uint8_t>&bad = point ? G.mpBad : G.mlBad, &has = point ? A.mpHas : Q.mlHas;
        for (int32_t j = 0; j < P.n; j++) {
            const int32_t kf = P.called[(size_t)j], e0 = P.segOff[(size_t)kind * P.n + j];
            const int32_t r0 = rowOff[(size_t)kf], len = rowOff[(size_t)kf + 1] - r0;
            for (int32_t i = 0; i < len; i++) {
                const int32_t s = row[(size_t)(r0 + i)];
                if (s < 0) continue;
                if (bad[(size_t)s]) {
                    W.action[(size_t)(e0 + i)] = INS_BAD;
                    continue;
                }
                if (!has[(size_t)s])
                    return lmap_fail(db, DRFE_ERR_STATE, who + (point ? "map point " + std::to_string(G.mpHandle[(size_t)s]) + " has no culling attributes that fit its observations"
                                                                       : "map line " + std::to_string(G.mlHandle[(size_t)s]) + " has no recent-list state"));
                const bool first = stamp[kind][(size_t)s] != j;
                stamp[kind][(size_t)s] = j;
                const int a = ins_verdict(s, 0, ins_observes(obs.data(), obsOff[(size_t)s], obsOff[(size_t)s + 1], kf), first);
                W.action[(size_t)(e0 + i)] = (uint8_t)a;
                if (a == INS_RECENT) {
                    W.recent[kind].push_back(s);
                    continue;
                }
                W.addEntry[kind].push_back(e0 + i);
                if (!point) continue;
                if (A.kfHas[(size_t)kf] != 2)
                    return lmap_fail(db, DRFE_ERR_STATE, who + "key frame " + std::to_string(G.kfHandle[(size_t)kf]) + " has no culling attributes that fit its row");
                if (!P.normals) continue;
                const std::string pt = who + "map point " + std::to_string(G.mpHandle[(size_t)s]);
                if (C.nLevels <= 0) return lmap_fail(db, DRFE_ERR_STATE, who + "the store has no scales");
                if (!E.mpHas[(size_t)s]) return lmap_fail(db, DRFE_ERR_STATE, pt + " has no geometry");
                if (E.mpRef[(size_t)s] < 0) return lmap_fail(db, DRFE_ERR_STATE, pt + " has no reference key frame in the store");
                if (!E.kfHas[(size_t)E.mpRef[(size_t)s]]) return lmap_fail(db, DRFE_ERR_STATE, pt + ": its reference key frame has no pose");
                if (E.mpLevel[(size_t)s] < 0 || E.mpLevel[(size_t)s] >= C.nLevels) return lmap_fail(db, DRFE_ERR_STATE, pt + ": ref_level is out of range");
                if (!E.kfHas[(size_t)kf]) return lmap_fail(db, DRFE_ERR_STATE, pt + ": observer " + std::to_string(G.kfHandle[(size_t)kf]) + " has no pose");
                for (int32_t o = obsOff[(size_t)s]; o < obsOff[(size_t)s + 1]; o++)
                    if (!E.kfHas[(size_t)obs[(size_t)o]])
                        return lmap_fail(db, DRFE_ERR_STATE, pt + ": observer " + std::to_string(G.kfHandle[(size_t)obs[(size_t)o]]) + " has no pose");
                std::vector<uint32_t>& bits = adders[s];
                bits.resize((size_t)P.words, 0u);
                const int32_t r = P.rankOf[(size_t)j];
                bits[(size_t)(r >> 5)] |= 1u << (r & 31);
                const InsAdders Ad{bits.data(), P.words, P.byRank.data(), P.called.data(), j};
                float nrm[3], maxD, minD;
                W.status.push_back(ins_point_normal(C, I.obsOff, I.obs, Ad, s, nrm, &maxD, &minD));
                W.nrm.insert(W.nrm.end(), nrm, nrm + 3);
                W.maxD.push_back(maxD);
                W.minD.push_back(minD);
            }
        }
    }
    return DRFE_OK;
}

/* the name of the capacity that is too small for what a walk decided, or nullptr */
const char* insert_capacity(const InsWork& W, const drfe_lmap_insert_call* c)
{
    for (int k = 0; k < 2; k++) {
        if ((int64_t)W.addEntry[k].size() > c->added_capacity[k]) return k ? "added_capacity[1]" : "added_capacity[0]";
        if ((int64_t)W.recent[k].size() > c->recent_capacity[k]) return k ? "recent_capacity[1]" : "recent_capacity[0]";
    }
    return nullptr;
}

/* the place of a new observer in a stored list: in front of the first stored observer of greater rank (slot) */
template <class SlotOf>
size_t rank_place(const std::vector<int32_t>& l, int32_t kf, SlotOf slot_of)
{
    size_t at = 0;
    while (at < l.size() && slot_of(l[at]) <= kf) at++;
    return at;
}

/* Applies the ADDED entries in walk order to the lists by handle and to the image.  onDevice: the device already holds nObs, so
 * only the spliced observations travel. */
void commit(drfe_lmap* db, const InsPlan& P, const InsWork& W, bool onDevice)
{
    Image& G = db->img;
    CullAttr& A = db->cull;
    RecentAttr& Q = db->rec;
    auto slot_of = [&](int32_t kfHandle) { return G.kfSlot.at(kfHandle); };
    for (int kind = 0; kind < 2; kind++) {
        if (W.addEntry[kind].empty()) continue;
        const bool point = kind == FUSE_POINT;
        std::unordered_set<int32_t> changed;
        for (const int32_t e : W.addEntry[kind]) {
            const int32_t q = ins_segment(P.segOff.data(), 2 * P.n, e), j = q - kind * P.n, i = e - P.segOff[(size_t)q];
            const int32_t kf = P.called[(size_t)j];
            const int32_t s = point ? G.kfMp[(size_t)(G.kfMpOff[(size_t)kf] + i)] : G.kfMl[(size_t)(G.kfMlOff[(size_t)kf] + i)];
            const int32_t h = point ? G.mpHandle[(size_t)s] : G.mlHandle[(size_t)s];
            std::vector<int32_t>*obs, *idx;
            int32_t* nObs;
            if (point) {
                MpCull& C = db->mpCull.at(h);
                obs = &db->mp.at(h).obs;
                idx = &C.obsIdx;
                nObs = &C.nObs;
            } else {
                MlObs& O = db->mlObs.at(h);
                obs = &O.obs;
                idx = &O.obsIdx;
                nObs = &O.nObs;
            }
            const size_t at = rank_place(*obs, kf, slot_of);
            obs->insert(obs->begin() + (ptrdiff_t)at, G.kfHandle[(size_t)kf]);
            idx->insert(idx->begin() + (ptrdiff_t)at, i);
            *nObs += fuse_obs_weight(kind, point ? A.stereo[(size_t)(G.kfMpOff[(size_t)kf] + i)] : 0);
            (point ? A.nObs : Q.mlNObs)[(size_t)s] = *nObs;
            changed.insert(s);
        }
        /* the observation arrays of the image with the changed rows spliced in, from the lists by handle */
        std::vector<int32_t>&off = point ? G.obsOff : Q.mlObsOff, &a = point ? G.obs : Q.mlObs, &b = point ? A.obsIdx : Q.mlObsIdx;
        std::vector<int32_t> nOff(1, 0), nObsA, nIdx;
        nObsA.reserve(a.size() + W.addEntry[kind].size());
        nIdx.reserve(a.size() + W.addEntry[kind].size());
        for (size_t s = 0; s + 1 < off.size(); s++) {
            if (changed.count((int32_t)s)) {
                const int32_t h = point ? G.mpHandle[s] : G.mlHandle[s];
                const std::vector<int32_t>&ho = point ? db->mp.at(h).obs : db->mlObs.at(h).obs, &hi = point ? db->mpCull.at(h).obsIdx : db->mlObs.at(h).obsIdx;
                for (size_t t = 0; t < ho.size(); t++) {
                    nObsA.push_back(slot_of(ho[t]));
                    nIdx.push_back(hi[t]);
                }
            } else {
                nObsA.insert(nObsA.end(), a.begin() + off[s], a.begin() + off[s + 1]);
                nIdx.insert(nIdx.end(), b.begin() + off[s], b.begin() + off[s + 1]);
            }
            nOff.push_back((int32_t)nObsA.size());
        }
        off.swap(nOff);
        a.swap(nObsA);
        b.swap(nIdx);
        ResidentBlock &rows = db->blk[drfe_lmap::ROWS], &attr = db->blk[drfe_lmap::ATTR], &recent = db->blk[drfe_lmap::RECENT];
        if (point) {
            A.live.assign(G.obs.size(), 1);
            rows.stale(db->secObsOff);
            attr.stale(db->secObsIdx);
            if (!onDevice) attr.stale(db->secNObs, db->secNObs);
        } else {
            recent.stale(db->secRecObsOff);
            if (!onDevice) recent.stale(db->secRecObsOff - 1, db->secRecObsOff - 1);   /* the lines' nObs: bound right before the offsets */
        }
    }
}

/* the scratch of a device call with `chunk` key frames a chunk */
struct InsLayout {
    StageLayout<16> scr;
    Section<uint32_t> adders;
    Section<InsertGroup> group;
    Section<int32_t> addP, addL, recP, recL, claimP, claimL;
    Section<float> nrm, maxD, minD;
    Section<uint8_t> status;
};

InsLayout insert_layout(const drfe_lmap* db, const InsPlan& P, int32_t chunk)
{
    const size_t nP = db->img.mpHandle.size(), nL = db->img.mlHandle.size();
    const size_t eP = (size_t)P.entries(0), eL = (size_t)P.entries(1), rec = P.normals ? eP : 0;
    InsLayout Y;
    Y.adders = Y.scr.add<uint32_t>(P.normals ? nP * (size_t)P.words : 0);
    Y.group = Y.scr.add<InsertGroup>(((size_t)P.total() + INSERT_TILE - 1) / INSERT_TILE);
    Y.addP = Y.scr.add<int32_t>(eP);
    Y.addL = Y.scr.add<int32_t>(eL);
    Y.recP = Y.scr.add<int32_t>(eP);
    Y.recL = Y.scr.add<int32_t>(eL);
    Y.nrm = Y.scr.add<float>(3 * rec);
    Y.maxD = Y.scr.add<float>(rec);
    Y.minD = Y.scr.add<float>(rec);
    Y.status = Y.scr.add<uint8_t>(rec);
    Y.claimP = Y.scr.add<int32_t>((size_t)chunk * nP);
    Y.claimL = Y.scr.add<int32_t>((size_t)chunk * nL);
    return Y;
}

/* the most key frames a chunk that fits the configured scratch, 0 when not even one does */
int32_t insert_chunk(const drfe_lmap* db, const InsPlan& P)
{
    int32_t lo = 0, hi = P.n;          /* lo fits (or is 0), everything above hi does not */
    if ((int64_t)insert_layout(db, P, P.n).scr.bytes() <= db->scratchBytes) return P.n;
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if ((int64_t)insert_layout(db, P, mid).scr.bytes() <= db->scratchBytes) lo = mid;
        else hi = mid;
    }
    return lo;
}

int insert_device(drfe_lmap* db, const InsPlan& P, int32_t chunk, InsWork& W, int64_t* chunks, void* stream)
{
    LmapCall call{db, "lmap insert"};
    if (const int rc = call.begin(P.normals ? (LMAP_NEED_RECENT | LMAP_NEED_GEO) : LMAP_NEED_RECENT, stream)) return rc;
    const size_t n = (size_t)P.n, total = (size_t)P.total(), eP = (size_t)P.entries(0), eL = (size_t)P.entries(1);
    StageLayout<16> in, out;
    const auto sCalled = in.add<int32_t>(n);
    const auto sSeg = in.add<int32_t>(2 * n + 1);
    const auto sByRank = in.add<int32_t>(n);
    const auto sRankOf = in.add<int32_t>(n);
    const auto oHead = out.add<int32_t>(INSERT_HEAD_WORDS);
    const auto oAction = out.add<uint8_t>(total);
    const InsLayout Y = insert_layout(db, P, chunk);
    if (const int rc = call.stage(in.bytes(), out.bytes(), Y.scr.bytes())) return rc;
    const auto [h, d, dO, dS, r] = call.at;
    sCalled.put(h, P.called.data());
    sSeg.put(h, P.segOff.data());
    sByRank.put(h, P.byRank.data());
    sRankOf.put(h, P.rankOf.data());
    InsertLaunch L{};
    L.I = db->dView;
    L.A = db->dCull;
    L.R = db->dRec;
    L.G = db->dCorr;
    L.n = P.n;
    L.normals = P.normals ? 1 : 0;
    L.words = P.words;
    L.called = sCalled.at(d);
    L.segOff = sSeg.at(d);
    L.byRank = sByRank.at(d);
    L.rankOf = sRankOf.at(d);
    L.claim[0] = Y.claimP.at(dS);
    L.claim[1] = Y.claimL.at(dS);
    L.adders = Y.adders.at(dS);
    L.group = Y.group.at(dS);
    L.addEntry[0] = Y.addP.at(dS);
    L.addEntry[1] = Y.addL.at(dS);
    L.recent[0] = Y.recP.at(dS);
    L.recent[1] = Y.recL.at(dS);
    L.nrm = Y.nrm.at(dS);
    L.maxD = Y.maxD.at(dS);
    L.minD = Y.minD.at(dS);
    L.status = Y.status.at(dS);
    L.head = oHead.at(dO);
    L.action = oAction.at(dO);
    if (const int rc = call.send()) return rc;
    hipError_t e = hipMemsetAsync(dO, 0, out.bytes(), call.st);
    if (e == hipSuccess && Y.adders.bytes()) e = hipMemsetAsync(L.adders, 0, Y.adders.bytes(), call.st);
    /* the verdict launches add to nObs in the attribute and the recent-list block */
    LmapWrites writes(db->blk[drfe_lmap::ATTR], &db->blk[drfe_lmap::RECENT]);
    for (int32_t j0 = 0; j0 < P.n && e == hipSuccess; j0 += chunk) {
        L.j0 = j0;
        L.j1 = std::min(P.n, j0 + chunk);
        /* the claim words of the chunk: cleared by the stream, one behind the other */
        const size_t claimBytes = Y.claimL.off + Y.claimL.bytes() - Y.claimP.off;
        if (claimBytes) e = hipMemsetAsync(L.claim[0], LMAP_NO_CLAIM & 0xff, claimBytes, call.st);
        if (e == hipSuccess) e = drfe_launch_insert_chunk(L, P.segOff.data(), call.st);
        (*chunks)++;
    }
    if (e == hipSuccess) e = drfe_launch_insert_finish(L, P.segOff.data(), call.st);
    if (const int rc = call.back(e)) return rc;
    const int32_t* head = oHead.at(r);
    const int32_t nAddP = head[INSERT_HEAD_ADDED_P], nRecP = head[INSERT_HEAD_RECENT_P], nAddL = head[INSERT_HEAD_ADDED_L], nRecL = head[INSERT_HEAD_RECENT_L];
    if (nAddP < 0 || nRecP < 0 || (size_t)nAddP + (size_t)nRecP > eP || nAddL < 0 || nRecL < 0 || (size_t)nAddL + (size_t)nRecL > eL)
        return lmap_fail(db, DRFE_ERR_STATE, "lmap insert device call: the device's totals do not fit the call");
    const size_t nRec = P.normals ? (size_t)nAddP : 0;
    LmapFetch F;
    const auto fAddP = F.add(L.addEntry[0], (size_t)nAddP);
    const auto fAddL = F.add(L.addEntry[1], (size_t)nAddL);
    const auto fRecP = F.add(L.recent[0], (size_t)nRecP);
    const auto fRecL = F.add(L.recent[1], (size_t)nRecL);
    const auto fNrm = F.add(L.nrm, 3 * nRec);
    const auto fMax = F.add(L.maxD, nRec);
    const auto fMin = F.add(L.minD, nRec);
    const auto fStatus = F.add(L.status, nRec);
    if (const int rc = call.fetch(F)) return rc;
    writes.done();
    W.action.assign(oAction.at(r), oAction.at(r) + total);
    W.addEntry[0].assign(F.at(fAddP), F.at(fAddP) + nAddP);
    W.addEntry[1].assign(F.at(fAddL), F.at(fAddL) + nAddL);
    W.recent[0].assign(F.at(fRecP), F.at(fRecP) + nRecP);
    W.recent[1].assign(F.at(fRecL), F.at(fRecL) + nRecL);
    W.nrm.assign(F.at(fNrm), F.at(fNrm) + 3 * nRec);
    W.maxD.assign(F.at(fMax), F.at(fMax) + nRec);
    W.minD.assign(F.at(fMin), F.at(fMin) + nRec);
    W.status.assign(F.at(fStatus), F.at(fStatus) + nRec);
    return DRFE_OK;
}

void insert_fill(const drfe_lmap* db, const InsPlan& P, const InsWork& W, drfe_lmap_insert_call* c)
{
    const Image& G = db->img;
    for (int j = 0; j <= P.n; j++) {
        c->point_offsets[j] = P.segOff[(size_t)j];
        c->line_offsets[j] = P.segOff[(size_t)(P.n + j)] - P.segOff[(size_t)P.n];
    }
    if (P.entries(0)) std::memcpy(c->point_action, W.action.data(), (size_t)P.entries(0));
    if (P.entries(1)) std::memcpy(c->line_action, W.action.data() + P.segOff[(size_t)P.n], (size_t)P.entries(1));
    for (int kind = 0; kind < 2; kind++) {
        const bool point = kind == FUSE_POINT;
        const std::vector<int32_t>& handle = point ? G.mpHandle : G.mlHandle;
        int32_t *oItem = point ? c->added_points : c->added_lines, *oKf = point ? c->added_point_kf : c->added_line_kf,
                *oIdx = point ? c->added_point_index : c->added_line_index, *oRecent = point ? c->recent_points : c->recent_lines;
        c->n_added[kind] = (int32_t)W.addEntry[kind].size();
        c->n_recent[kind] = (int32_t)W.recent[kind].size();
        for (size_t t = 0; t < W.addEntry[kind].size(); t++) {
            const int32_t e = W.addEntry[kind][t], q = ins_segment(P.segOff.data(), 2 * P.n, e), j = q - kind * P.n, i = e - P.segOff[(size_t)q];
            const int32_t kf = P.called[(size_t)j];
            const int32_t s = point ? G.kfMp[(size_t)(G.kfMpOff[(size_t)kf] + i)] : G.kfMl[(size_t)(G.kfMlOff[(size_t)kf] + i)];
            oItem[t] = handle[(size_t)s];
            oKf[t] = G.kfHandle[(size_t)kf];
            oIdx[t] = i;
        }
        for (size_t t = 0; t < W.recent[kind].size(); t++) oRecent[t] = handle[(size_t)W.recent[kind][t]];
    }
    if (P.normals && !W.status.empty()) {
        std::memcpy(c->normal, W.nrm.data(), sizeof(float) * W.nrm.size());
        std::memcpy(c->max_distance, W.maxD.data(), sizeof(float) * W.maxD.size());
        std::memcpy(c->min_distance, W.minD.data(), sizeof(float) * W.minD.size());
        std::memcpy(c->status, W.status.data(), W.status.size());
    }
}

/* mode: 0 host, 1 device, 2 by the crossover */
int insert_entry_point(drfe_lmap* db, drfe_lmap_insert_call* c, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_insert: a device call on a store without a context");
    if (!call_ok(c)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_insert: invalid call or output arrays");
    InsPlan P;
    int rc = insert_plan(db, c->n, c->handles, c->normal != nullptr, P);
    if (rc) return rc;
    for (int k = 0; k < 2; k++)
        if (c->action_capacity[k] < P.entries(k))
            return lmap_fail(db, DRFE_ERR_CAPACITY, std::string("lmap_insert: the call returns more than action_capacity[") + (k ? "1]" : "0]"));
    const int64_t total = P.total();
    bool dev = total > 0 && (mode == 1 || (mode == 2 && db->ctx && total >= DRFE_LMAP_INSERT_DEVICE_FROM));
    int32_t chunk = 0;
    if (dev) {
        chunk = insert_chunk(db, P);
        if (!chunk && mode == 1) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_insert: the call does not fit the configured device scratch with one key frame a chunk");
        dev = chunk > 0;
    }
    InsWork W;
    int64_t st[8] = {1, P.n, 0, 0, 0, 0, 0, 0};
    if (dev) {
        /* the device commits as it goes, so the refusals and the capacities are settled first: by the image's flags and the
         * bounds, or by a walk of the host */
        bool sure = nothing_missing(db, P);
        for (int k = 0; k < 2; k++) sure = sure && c->added_capacity[k] >= P.entries(k) && c->recent_capacity[k] >= P.entries(k);
        if (!sure) {
            InsWork H;
            rc = host_walk(db, P, H);
            if (rc) return rc;
            if (const char* small = insert_capacity(H, c)) return lmap_fail(db, DRFE_ERR_CAPACITY, std::string("lmap_insert: the call returns more than ") + small);
        }
        rc = insert_device(db, P, chunk, W, &st[7], stream);
        if (rc) return rc;
        st[2] = 1;
        commit(db, P, W, true);
    } else {
        rc = host_walk(db, P, W);
        if (rc) return rc;
        if (const char* small = insert_capacity(W, c)) return lmap_fail(db, DRFE_ERR_CAPACITY, std::string("lmap_insert: the call returns more than ") + small);
        commit(db, P, W, false);
    }
    insert_fill(db, P, W, c);
    st[3] = (int64_t)W.addEntry[0].size();
    st[4] = (int64_t)W.addEntry[1].size();
    st[5] = (int64_t)W.recent[0].size();
    st[6] = (int64_t)W.recent[1].size();
    for (int i = 0; i < 8; i++) db->insStats[i] += st[i];
    return DRFE_OK;
}

}  // namespace

extern "C" {

int drfe_lmap_insert_host(drfe_lmap* db, drfe_lmap_insert_call* call) { return insert_entry_point(db, call, 0, nullptr); }
int drfe_lmap_insert_device(drfe_lmap* db, drfe_lmap_insert_call* call, void* stream) { return insert_entry_point(db, call, 1, stream); }
int drfe_lmap_insert_batch(drfe_lmap* db, drfe_lmap_insert_call* call, void* stream) { return insert_entry_point(db, call, 2, stream); }

int drfe_lmap_insert_limits(int32_t* out8)
{
    if (!out8) return DRFE_ERR_INVALID;
    out8[0] = INSERT_TILE;
    out8[1] = 64;
    out8[2] = (int32_t)sizeof(int32_t);
    out8[3] = INSERT_NORMAL_GROUPS;
    out8[4] = LMAP_THREADS;
    out8[5] = DRFE_LMAP_MAX_QUERIES;
    out8[6] = DRFE_LMAP_INSERT_DEVICE_FROM;
    out8[7] = 0;
    return DRFE_OK;
}

int drfe_lmap_insert_scratch(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t normals, int64_t* out3)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!out3 || n < 0 || (n > 0 && !handles)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_insert_scratch: invalid argument");
    InsPlan P;
    const int rc = insert_plan(db, n, handles, normals != 0, P);
    if (rc) return rc;
    out3[0] = (int64_t)insert_layout(db, P, n).scr.bytes();
    out3[1] = (int64_t)insert_layout(db, P, n ? 1 : 0).scr.bytes();
    out3[2] = (int64_t)insert_layout(db, P, 0).scr.bytes();
    return DRFE_OK;
}

int drfe_lmap_insert_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::insStats, stats); }

}  // extern "C"
