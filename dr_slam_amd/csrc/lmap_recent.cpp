/* lmap_recent.cpp — LocalMapping::MapPointCulling and MapLineCulling (reference src/LocalMapping.cc:175-231) with
 * MapPoint::SetBadFlag and MapLine::SetBadFlag on the local-map store, behind the C-ABI of include/drfe.h: the setter, getter and
 * cheap edit of the recent-list attributes, their image, the checks, the host walk, the device entry (recent_kernels.hip), the
 * commit and the counters.  Both sides evaluate recent_core.h.  The walk of either entry only decides: it returns the actions, the
 * surviving lists and the erased observations, and one commit applies them to the rows and the image - marking for upload what the
 * host entry changed, and nothing of what the device entry already stored in the resident image.  DESIGN.md section 31.  Parity
 * with a build of the reference's LocalMapping.cc is not pinned: it cannot be built here. */
#include "lmap_call.h"

#include <algorithm>
#include <cstring>
#include <unordered_set>

using namespace lmap_store;

/* the attributes by slot, after the image and the culling attributes */
int lmap_build_recent(drfe_lmap* db)
{
    const int rc = lmap_build_cull(db);
    if (rc) return rc;
    if (!db->recDirty) return DRFE_OK;
    const Image& G = db->img;
    const CullAttr& A = db->cull;
    RecentAttr& Q = db->rec;
    const size_t nP = G.mpHandle.size(), nL = G.mlHandle.size();
    Q.mpHas.assign(nP, 0);
    Q.mpFound.assign(nP, 0);
    Q.mpVisible.assign(nP, 0);
    Q.mpFirst.assign(nP, 0);
    Q.mlHas.assign(nL, 0);
    Q.mlFound.assign(nL, 0);
    Q.mlVisible.assign(nL, 0);
    Q.mlFirst.assign(nL, 0);
    Q.mlNObs.assign(nL, 0);
    Q.mlObsOff.assign(1, 0);
    Q.mlObs.clear();
    Q.mlObsIdx.clear();
    bool complete = true;
    for (size_t s = 0; s < nP; s++) {
        const auto it = db->mpRec.find(G.mpHandle[s]);
        if (it != db->mpRec.end()) {
            Q.mpFound[s] = it->second.found;
            Q.mpVisible[s] = it->second.visible;
            Q.mpFirst[s] = it->second.first;
            Q.mpHas[s] = A.mpHas[s] ? 1 : 0;   /* nObs and mit->second are the culling attributes */
        }
        if (!Q.mpHas[s]) complete = false;
        for (int32_t o = G.obsOff[s]; o < G.obsOff[s + 1] && complete; o++) {
            const size_t k = (size_t)G.obs[(size_t)o];
            complete = A.obsIdx[(size_t)o] >= 0 && A.obsIdx[(size_t)o] < G.kfMpOff[k + 1] - G.kfMpOff[k];
        }
    }
    for (size_t s = 0; s < nL; s++) {
        const int32_t h = G.mlHandle[s];
        const auto it = db->mlRec.find(h);
        const auto ob = db->mlObs.find(h);
        if (it != db->mlRec.end() && ob != db->mlObs.end()) {
            Q.mlFound[s] = it->second.found;
            Q.mlVisible[s] = it->second.visible;
            Q.mlFirst[s] = it->second.first;
            Q.mlNObs[s] = ob->second.nObs;
            Q.mlHas[s] = 1;
            for (size_t i = 0; i < ob->second.obs.size(); i++) {
                const auto k = G.kfSlot.find(ob->second.obs[i]);
                if (k == G.kfSlot.end())
                    return lmap_fail(db, DRFE_ERR_STATE, "lmap: an observation of map line " + std::to_string(h) + " names unknown handle " + std::to_string(ob->second.obs[i]));
                const int32_t idx = ob->second.obsIdx[i];
                if (idx < 0 || idx >= G.kfMlOff[(size_t)k->second + 1] - G.kfMlOff[(size_t)k->second]) complete = false;
                Q.mlObs.push_back(k->second);
                Q.mlObsIdx.push_back(idx);
            }
        } else {
            complete = false;
        }
        Q.mlObsOff.push_back((int32_t)Q.mlObs.size());
    }
    Q.complete = complete;
    db->recDirty = false;
    db->blk[drfe_lmap::RECENT].stale_all();
    return DRFE_OK;
}

namespace {

struct KindView {
    const std::vector<uint8_t>*bad, *has;
    const std::vector<int32_t>*handle, *found, *visible, *nObs, *obsOff, *obs, *obsIdx, *rowOff;
    const std::vector<int64_t>* first;
    const char* name;
};

KindView kind_view(const drfe_lmap* db, int kind)
{
    const Image& G = db->img;
    const RecentAttr& Q = db->rec;
    if (kind == RECENT_POINT)
        return KindView{&G.mpBad, &Q.mpHas, &G.mpHandle, &Q.mpFound, &Q.mpVisible, &db->cull.nObs, &G.obsOff, &G.obs, &db->cull.obsIdx, &G.kfMpOff, &Q.mpFirst, "map point"};
    return KindView{&G.mlBad, &Q.mlHas, &G.mlHandle, &Q.mlFound, &Q.mlVisible, &Q.mlNObs, &Q.mlObsOff, &Q.mlObs, &Q.mlObsIdx, &G.kfMlOff, &Q.mlFirst, "map line"};
}

/* a checked call, in slots: the flat entry space is the point list, then the line list */
struct RecentPlan {
    int64_t current = 0;
    int32_t monocular = 0, nPts = 0, n = 0;
    std::vector<int32_t> item, handle;
    std::vector<int64_t> bound;                /* n + 1: the observations of the listed items that are not bad, before each entry */
};

/* what a walk decided */
struct RecentWork {
    std::vector<uint8_t> action;
    std::vector<int32_t> kept[2], culledEntry, erOff, erKf, erIdx;     /* erKf in slots */
    bool onDevice = false;
};

bool list_ok(const drfe_lmap_recent_list* l)
{
    return l && l->n >= 0 && l->erased_capacity >= 0 && l->n_kept && l->n_culled && l->erased_offsets &&
           (l->n == 0 || (l->handles && l->action && l->kept && l->culled)) && (l->erased_capacity == 0 || (l->erased_kf && l->erased_index));
}

int recent_plan(drfe_lmap* db, int64_t current, int32_t monocular, const drfe_lmap_recent_list* const lists[2], RecentPlan& P)
{
    for (int k = 0; k < 2; k++)
        if (lists[k]->n > DRFE_LMAP_RECENT_MAX_ENTRIES)
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap_recent_cull: more than DRFE_LMAP_RECENT_MAX_ENTRIES entries in a list");
    const int rc = lmap_build_recent(db);
    if (rc) return rc;
    const Image& G = db->img;
    P.current = current;
    P.monocular = monocular ? 1 : 0;
    P.nPts = lists[0]->n;
    P.n = lists[0]->n + lists[1]->n;
    P.item.reserve((size_t)P.n);
    P.handle.reserve((size_t)P.n);
    for (int k = 0; k < 2; k++) {
        const std::unordered_map<int32_t, int32_t>& slot = k == RECENT_POINT ? G.mpSlot : G.mlSlot;
        for (int i = 0; i < lists[k]->n; i++) {
            const auto it = slot.find(lists[k]->handles[i]);
            if (it == slot.end())
                return lmap_fail(db, DRFE_ERR_INVALID, std::string("lmap_recent_cull: the ") + (k ? "line" : "point") + " list names an unknown handle");
            P.item.push_back(it->second);
            P.handle.push_back(it->first);
        }
    }
    /* what the walk reads of every listed item that is not bad */
    P.bound.assign(1, 0);
    for (int e = 0; e < P.n; e++) {
        const int kind = e < P.nPts ? RECENT_POINT : RECENT_LINE;
        const KindView V = kind_view(db, kind);
        const size_t s = (size_t)P.item[(size_t)e];
        int64_t obs = 0;
        if (!(*V.bad)[s]) {
            const std::string who = std::string("lmap_recent_cull: ") + V.name + " " + std::to_string((*V.handle)[s]);
            if (!db->rec.complete) {
                if (!(*V.has)[s])
                    return lmap_fail(db, DRFE_ERR_STATE, who + (kind == RECENT_POINT ? " has no recent-list attributes, or no culling attributes that fit its observations"
                                                                                     : " has no recent-list attributes"));
                for (int32_t o = (*V.obsOff)[s]; o < (*V.obsOff)[s + 1]; o++) {
                    const size_t k = (size_t)(*V.obs)[(size_t)o];
                    const int32_t idx = (*V.obsIdx)[(size_t)o];
                    if (idx < 0 || idx >= (*V.rowOff)[k + 1] - (*V.rowOff)[k])
                        return lmap_fail(db, DRFE_ERR_STATE, who + ": obs_index " + std::to_string(idx) + " lies outside the row of key frame " + std::to_string(G.kfHandle[k]));
                }
            }
            if (kind == RECENT_LINE && recent_line_undefined((*V.found)[s], (*V.visible)[s]))
                return lmap_fail(db, DRFE_ERR_STATE, who + ": mnFound / mnVisible is not defined (" + std::to_string((*V.found)[s]) + " / " + std::to_string((*V.visible)[s]) + ")");
            obs = (*V.obsOff)[s + 1] - (*V.obsOff)[s];
        }
        P.bound.push_back(P.bound.back() + obs);
    }
    return DRFE_OK;
}

/* the reference's two walks, entry after entry; the state is only read, the items culled so far are a set */
void recent_host(const drfe_lmap* db, const RecentPlan& P, RecentWork& W)
{
    W.action.assign((size_t)P.n, 0);
    std::unordered_set<int32_t> gone[2];
    for (int e = 0; e < P.n; e++) {
        const int kind = e < P.nPts ? RECENT_POINT : RECENT_LINE;
        const KindView V = kind_view(db, kind);
        const int32_t s = P.item[(size_t)e];
        int action = RECENT_WAS_BAD;
        if (!(*V.bad)[(size_t)s] && !gone[kind].count(s))
            action = recent_verdict(kind, (*V.found)[(size_t)s], (*V.visible)[(size_t)s], (*V.first)[(size_t)s], (*V.nObs)[(size_t)s], P.current, P.monocular);
        W.action[(size_t)e] = (uint8_t)action;
        if (action == RECENT_KEPT) W.kept[kind].push_back(P.handle[(size_t)e]);
        if (!recent_culls(action)) continue;
        gone[kind].insert(s);
        W.culledEntry.push_back(e);
        W.erOff.push_back((int32_t)W.erKf.size());
        for (int32_t o = (*V.obsOff)[(size_t)s]; o < (*V.obsOff)[(size_t)s + 1]; o++) {
            W.erKf.push_back((*V.obs)[(size_t)o]);
            W.erIdx.push_back((*V.obsIdx)[(size_t)o]);
        }
    }
    W.erOff.push_back((int32_t)W.erKf.size());
}

/* how a device call divides the scratch: the claim words are shared, a chunk adds its entries */
struct RecentFit {
    int64_t fixed = 0, whole = 0, least = 0;
    bool fits = false;
};

RecentFit recent_fit(const drfe_lmap* db, int64_t n)
{
    RecentFit F;
    F.fixed = 4 * ((int64_t)db->img.mpHandle.size() + (int64_t)db->img.mlHandle.size()) + RECENT_FIXED_BYTES;
    F.whole = F.fixed + RECENT_ENTRY_BYTES * n;
    F.least = F.fixed + RECENT_ENTRY_BYTES;
    F.fits = F.least <= db->scratchBytes;
    return F;
}

/* The chunks one after another on the stream, everything back in one copy.  The kernels store the bad flags and the nulled
 * entries into the resident image; the commit mirrors them on the host. */
int recent_device(drfe_lmap* db, const RecentPlan& P, const RecentFit& F, RecentWork& W, void* stream)
{
    LmapCall call{db, "lmap recent cull"};
    if (const int rc = call.begin(LMAP_NEED_RECENT, stream)) return rc;
    const Image& G = db->img;
    const size_t n = (size_t)P.n, nP = G.mpHandle.size(), nL = G.mlHandle.size(), bound = (size_t)P.bound[n];
    const size_t room = (size_t)std::min<int64_t>((int64_t)n, (std::min<int64_t>(db->scratchBytes, F.whole) - F.fixed) / RECENT_ENTRY_BYTES);
    const size_t groups = (room + RECENT_TILE - 1) / RECENT_TILE;
    StageLayout<16> in, out, scr;
    const auto sItem = in.add<int32_t>(n);
    const auto sHandle = in.add<int32_t>(n);
    const auto oHead = out.add<int32_t>(RECENT_HEAD_WORDS);
    const auto oAction = out.add<uint8_t>(n);
    const auto oKeptP = out.add<int32_t>((size_t)P.nPts);
    const auto oKeptL = out.add<int32_t>(n - (size_t)P.nPts);
    const auto oCulled = out.add<int32_t>(n);
    const auto oErOff = out.add<int32_t>(n + 1);
    const auto oErKf = out.add<int32_t>(bound);
    const auto oErIdx = out.add<int32_t>(bound);
    const auto xClaimP = scr.add<int32_t>(nP);
    const auto xClaimL = scr.add<int32_t>(nL);
    const auto xCnt = scr.add<int32_t>(room);
    const auto xGroup = scr.add<RecentGroup>(groups);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, r] = call.at;
    sItem.put(h, P.item.data());
    sHandle.put(h, P.handle.data());
    RecentLaunch L{};
    L.I = db->dView;
    L.A = db->dCull;
    L.R = db->dRec;
    L.current = P.current;
    L.monocular = P.monocular;
    L.nPts = P.nPts;
    L.n = P.n;
    L.item = sItem.at(d);
    L.handle = sHandle.at(d);
    L.claim[0] = xClaimP.at(dS);
    L.claim[1] = xClaimL.at(dS);
    L.cnt = xCnt.at(dS);
    L.group = xGroup.at(dS);
    L.action = oAction.at(dO);
    L.kept[0] = oKeptP.at(dO);
    L.kept[1] = oKeptL.at(dO);
    L.culledEntry = oCulled.at(dO);
    L.erOff = oErOff.at(dO);
    L.erKf = oErKf.at(dO);
    L.erIdx = oErIdx.at(dO);
    L.head = oHead.at(dO);
    if (const int rc = call.send()) return rc;
    hipError_t e = nP + nL ? hipMemsetAsync(xClaimP.at(dS), 0x7f, xClaimL.off + xClaimL.bytes() - xClaimP.off, call.st) : hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync(oHead.at(dO), 0, oHead.bytes(), call.st);
    LmapWrites writes(db->blk[drfe_lmap::ROWS]);   /* a chunk stores into the resident image */
    for (size_t e0 = 0; e0 < n && e == hipSuccess; e0 += room) {
        L.e0 = (int32_t)e0;
        L.e1 = (int32_t)std::min(n, e0 + room);
        e = drfe_launch_recent_chunk(L, P.bound[(size_t)L.e1] - P.bound[e0], call.st);
    }
    if (const int rc = call.back(e)) return rc;
    const int32_t* head = oHead.at(r);
    const size_t keptP = (size_t)head[RECENT_HEAD_KEPT_P], keptL = (size_t)head[RECENT_HEAD_KEPT_L], culled = (size_t)head[RECENT_HEAD_CULLED],
                 erased = (size_t)head[RECENT_HEAD_ERASED];
    if (head[RECENT_HEAD_KEPT_P] < 0 || head[RECENT_HEAD_KEPT_L] < 0 || head[RECENT_HEAD_CULLED] < 0 || head[RECENT_HEAD_ERASED] < 0 ||
        keptP > (size_t)P.nPts || keptL > n - (size_t)P.nPts || culled > n || erased > bound)
        return lmap_fail(db, DRFE_ERR_STATE, "lmap recent cull device call: the device's totals do not fit the call");
    writes.done();
    W.onDevice = true;
    W.action.assign(oAction.at(r), oAction.at(r) + n);
    W.kept[0].assign(oKeptP.at(r), oKeptP.at(r) + keptP);
    W.kept[1].assign(oKeptL.at(r), oKeptL.at(r) + keptL);
    W.culledEntry.assign(oCulled.at(r), oCulled.at(r) + culled);
    W.erOff.assign(oErOff.at(r), oErOff.at(r) + culled);
    W.erOff.push_back((int32_t)erased);
    W.erKf.assign(oErKf.at(r), oErKf.at(r) + erased);
    W.erIdx.assign(oErIdx.at(r), oErIdx.at(r) + erased);
    return DRFE_OK;
}

/* a CSR array without the rows of `gone` (ascending slots) */
void drop_rows(std::vector<int32_t>& off, std::vector<int32_t>& a, std::vector<int32_t>& b, const std::vector<int32_t>& gone)
{
    std::vector<int32_t> nOff(1, 0), nA, nB;
    nA.reserve(a.size());
    nB.reserve(b.size());
    size_t g = 0;
    for (size_t s = 0; s + 1 < off.size(); s++) {
        if (g < gone.size() && (size_t)gone[g] == s) {
            g++;
        } else {
            nA.insert(nA.end(), a.begin() + off[s], a.begin() + off[s + 1]);
            nB.insert(nB.end(), b.begin() + off[s], b.begin() + off[s + 1]);
        }
        nOff.push_back((int32_t)nA.size());
    }
    off.swap(nOff);
    a.swap(nA);
    b.swap(nB);
}

/* more nulled entries than this go up as the whole section rather than one by one */
const size_t kNulledOneByOne = 1024;

/* the erased observations of both kinds against the caller's capacities, or the name of the one that is too small */
const char* recent_capacity(const RecentPlan& P, const RecentWork& W, drfe_lmap_recent_list* const lists[2], size_t* culledPts)
{
    size_t cP = 0;
    while (cP < W.culledEntry.size() && W.culledEntry[cP] < P.nPts) cP++;
    *culledPts = cP;
    if (W.erOff[cP] > lists[0]->erased_capacity) return "points";
    if (W.erOff.back() - W.erOff[cP] > lists[1]->erased_capacity) return "lines";
    return nullptr;
}

/* results into the caller's arrays and the changes into the store */
void recent_finish(drfe_lmap* db, const RecentPlan& P, const RecentWork& W, drfe_lmap_recent_list* const lists[2], size_t cP)
{
    Image& G = db->img;
    CullAttr& A = db->cull;
    RecentAttr& Q = db->rec;
    ResidentBlock &rows = db->blk[drfe_lmap::ROWS], &attr = db->blk[drfe_lmap::ATTR], &recent = db->blk[drfe_lmap::RECENT];
    const size_t nCulled = W.culledEntry.size();
    /* the caller's arrays */
    for (int k = 0; k < 2; k++) {
        drfe_lmap_recent_list* o = lists[k];
        const size_t e0 = k ? (size_t)P.nPts : 0, c0 = k ? cP : 0, c1 = k ? nCulled : cP;
        if (o->n) std::memcpy(o->action, W.action.data() + e0, (size_t)o->n);
        *o->n_kept = (int32_t)W.kept[k].size();
        if (!W.kept[k].empty()) std::memcpy(o->kept, W.kept[k].data(), sizeof(int32_t) * W.kept[k].size());
        *o->n_culled = (int32_t)(c1 - c0);
        const int32_t t0 = W.erOff[c0];
        for (size_t r = c0; r < c1; r++) {
            o->culled[r - c0] = P.handle[(size_t)W.culledEntry[r]];
            o->erased_offsets[r - c0] = W.erOff[r] - t0;
        }
        o->erased_offsets[c1 - c0] = W.erOff[c1] - t0;
        for (int32_t t = t0; t < W.erOff[c1]; t++) {
            o->erased_kf[t - t0] = G.kfHandle[(size_t)W.erKf[(size_t)t]];
            o->erased_index[t - t0] = W.erIdx[(size_t)t];
        }
    }
    /* SetBadFlag of every culled item, in list order: the flag, the nulled entries, the cleared observations */
    std::vector<int32_t> goneObs[2];
    std::vector<size_t> nulledAt[2];
    int64_t st[8] = {P.n ? 1 : 0, P.n, W.onDevice ? 1 : 0, 0, 0, 0, 0, 0};
    for (size_t e = 0; e < (size_t)P.n; e++) st[3 + (W.action[e] == RECENT_RATIO ? 0 : W.action[e] == RECENT_OBS ? 1 : W.action[e] == RECENT_AGED ? 2 : 3)] += W.action[e] != RECENT_KEPT;
    for (size_t r = 0; r < nCulled; r++) {
        const int kind = r < cP ? RECENT_POINT : RECENT_LINE;
        const size_t s = (size_t)P.item[(size_t)W.culledEntry[r]];
        const int32_t h = P.handle[(size_t)W.culledEntry[r]];
        if (kind == RECENT_POINT) {
            MpRow& R = db->mp.at(h);
            R.bad = 1;
            R.obs.clear();
            db->mpCull.at(h).obsIdx.clear();
            G.mpBad[s] = 1;
        } else {
            db->ml.at(h) = 1;
            MlObs& R = db->mlObs.at(h);
            R.obs.clear();
            R.obsIdx.clear();
            G.mlBad[s] = 1;
        }
        if (W.erOff[r + 1] > W.erOff[r]) goneObs[kind].push_back((int32_t)s);
        const std::vector<int32_t>& rowOff = kind == RECENT_POINT ? G.kfMpOff : G.kfMlOff;
        std::vector<int32_t>& row = kind == RECENT_POINT ? G.kfMp : G.kfMl;
        for (int32_t t = W.erOff[r]; t < W.erOff[r + 1]; t++) {
            const size_t k = (size_t)W.erKf[(size_t)t], at = (size_t)rowOff[k] + (size_t)W.erIdx[(size_t)t];
            if (row[at] < 0) continue;
            row[at] = -1;
            KfRow& K = db->kf.at(G.kfHandle[k]);
            (kind == RECENT_POINT ? K.mps : K.mls)[(size_t)W.erIdx[(size_t)t]] = -1;
            nulledAt[kind].push_back(at);
            st[7]++;
        }
    }
    /* what the device copy now lacks.  The device entry stored the flags and the nulled entries itself; after the host entry
     * they travel: the bad flags in front of the rows block, the entries one by one or, when they are many, as their section. */
    if (!W.onDevice) {
        if (nCulled) rows.stale(0, db->secMlBad);
        for (int k = 0; k < 2; k++) {
            const int sec = k == RECENT_POINT ? db->secKfMp : db->secKfMl;
            if (nulledAt[k].size() > kNulledOneByOne) rows.stale(sec, sec);
            else
                for (const size_t at : nulledAt[k]) rows.stale_at(sec, at);
        }
    }
    /* the cleared observation rows: spliced on the host, the tail of their block sent before the next device call */
    for (int k = 0; k < 2; k++) std::sort(goneObs[k].begin(), goneObs[k].end());
    if (!goneObs[RECENT_POINT].empty()) {
        drop_rows(G.obsOff, G.obs, A.obsIdx, goneObs[RECENT_POINT]);
        A.live.assign(G.obs.size(), 1);
        rows.stale(db->secObsOff);
        attr.stale(db->secObsIdx);
    }
    if (!goneObs[RECENT_LINE].empty()) {
        drop_rows(Q.mlObsOff, Q.mlObs, Q.mlObsIdx, goneObs[RECENT_LINE]);
        recent.stale(db->secRecObsOff);
    }
    for (int i = 0; i < 8; i++) db->recStats[i] += st[i];
}

/* mode: 0 host, 1 device, 2 by the crossover */
int recent_entry_point(drfe_lmap* db, int64_t current, int32_t monocular, drfe_lmap_recent_list* points, drfe_lmap_recent_list* lines, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_recent_cull: a device call on a store without a context");
    if (!list_ok(points) || !list_ok(lines)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_recent_cull: invalid list or output arrays");
    drfe_lmap_recent_list* const lists[2] = {points, lines};
    const drfe_lmap_recent_list* const clists[2] = {points, lines};
    RecentPlan P;
    int rc = recent_plan(db, current, monocular, clists, P);
    if (rc) return rc;
    bool dev = P.n > 0 && (mode == 1 || (mode == 2 && db->ctx && P.n >= DRFE_LMAP_RECENT_DEVICE_FROM));
    RecentFit F;
    if (dev) {
        F = recent_fit(db, P.n);
        const bool fits = F.fits && P.bound[(size_t)P.n] <= INT32_MAX;
        if (!fits && mode == 1)
            return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_recent_cull: the claim words and one list entry do not fit the configured device scratch");
        dev = fits;
    }
    RecentWork W;
    size_t cP = 0;
    const char* small = nullptr;
    if (dev) {
        /* the device commits as it goes, so the capacities are settled first: by the bound, or by the host's walk when the bound
         * does not settle it */
        const int64_t bP = P.bound[(size_t)P.nPts], bL = P.bound[(size_t)P.n] - bP;
        if (bP > points->erased_capacity || bL > lines->erased_capacity) {
            RecentWork H;
            recent_host(db, P, H);
            small = recent_capacity(P, H, lists, &cP);
        }
        if (!small) {
            rc = recent_device(db, P, F, W, stream);
            if (rc) return rc;
            small = recent_capacity(P, W, lists, &cP);   /* cannot be: the same verdicts */
        }
    } else {
        recent_host(db, P, W);
        small = recent_capacity(P, W, lists, &cP);
    }
    if (small) return lmap_fail(db, DRFE_ERR_CAPACITY, std::string("lmap_recent_cull: the call erases more observations of ") + small + " than erased_capacity");
    recent_finish(db, P, W, lists, cP);
    return DRFE_OK;
}

template <class Map>
bool known_all(const Map& m, int32_t n, const int32_t* handles)
{
    for (int i = 0; i < n; i++)
        if (m.find(handles[i]) == m.end()) return false;
    return true;
}

}  // namespace

extern "C" {

int drfe_lmap_set_recent_attributes(drfe_lmap* db, const drfe_lmap_recent_attributes* r)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!r || r->n_points < 0 || r->n_lines < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_recent_attributes: invalid argument");
    const int np = r->n_points, nl = r->n_lines;
    if (np > 0 && (!r->point_handle || !r->point_found || !r->point_visible || !r->point_first_kf))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_recent_attributes: invalid map-point arrays");
    if (nl > 0 && (!r->line_handle || !r->line_found || !r->line_visible || !r->line_first_kf || !r->line_n_obs || !lmap_offsets_ok(r->line_obs_offsets, nl) ||
                   (r->line_obs_offsets[nl] > 0 && (!r->line_obs || !r->line_obs_index))))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_recent_attributes: invalid map-line arrays");
    for (int i = 0; i < np; i++)
        if (r->point_handle[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_recent_attributes: a negative handle");
    std::vector<int32_t> row;
    for (int i = 0; i < nl; i++) {
        if (r->line_handle[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_recent_attributes: a negative handle");
        row.assign(r->line_obs + r->line_obs_offsets[i], r->line_obs + r->line_obs_offsets[i + 1]);
        std::sort(row.begin(), row.end());
        if (!row.empty() && row[0] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_recent_attributes: a negative observation");
        if (std::adjacent_find(row.begin(), row.end()) != row.end())
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_recent_attributes: a key frame observes a line twice");
    }
    for (int i = 0; i < np; i++) {
        ItemRecent& P = db->mpRec[r->point_handle[i]];
        P.found = r->point_found[i];
        P.visible = r->point_visible[i];
        P.first = r->point_first_kf[i];
    }
    for (int i = 0; i < nl; i++) {
        ItemRecent& P = db->mlRec[r->line_handle[i]];
        P.found = r->line_found[i];
        P.visible = r->line_visible[i];
        P.first = r->line_first_kf[i];
        MlObs& O = db->mlObs[r->line_handle[i]];
        O.nObs = r->line_n_obs[i];
        O.obs.assign(r->line_obs + r->line_obs_offsets[i], r->line_obs + r->line_obs_offsets[i + 1]);
        O.obsIdx.assign(r->line_obs_index + r->line_obs_offsets[i], r->line_obs_index + r->line_obs_offsets[i + 1]);
    }
    if (np || nl) db->recDirty = true;
    if (nl) db->recCheck = true;
    return DRFE_OK;
}

int drfe_lmap_get_recent_attributes(drfe_lmap* db, drfe_lmap_recent_attributes_out* o)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!o || o->n_points < 0 || o->n_lines < 0 || o->line_obs_capacity < 0 ||
        (o->n_points > 0 && (!o->point_handle || !o->point_found || !o->point_visible || !o->point_first_kf)) ||
        (o->n_lines > 0 && (!o->line_handle || !o->line_found || !o->line_visible || !o->line_first_kf || !o->line_n_obs || !o->line_obs_offsets)) ||
        (o->line_obs_capacity > 0 && (!o->line_obs || !o->line_obs_index)))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_recent_attributes: invalid argument");
    if (!known_all(db->mpRec, o->n_points, o->point_handle)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_recent_attributes: a map point without attributes");
    if (!known_all(db->mlRec, o->n_lines, o->line_handle)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_recent_attributes: a map line without attributes");
    int64_t total = 0;
    for (int i = 0; i < o->n_lines; i++) total += (int64_t)db->mlObs.at(o->line_handle[i]).obs.size();
    if (total > o->line_obs_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_get_recent_attributes: an output array is too small");
    for (int i = 0; i < o->n_points; i++) {
        const ItemRecent& P = db->mpRec.at(o->point_handle[i]);
        o->point_found[i] = P.found;
        o->point_visible[i] = P.visible;
        o->point_first_kf[i] = P.first;
    }
    int32_t a = 0;
    if (o->n_lines) o->line_obs_offsets[0] = 0;
    for (int i = 0; i < o->n_lines; i++) {
        const ItemRecent& P = db->mlRec.at(o->line_handle[i]);
        const MlObs& O = db->mlObs.at(o->line_handle[i]);
        o->line_found[i] = P.found;
        o->line_visible[i] = P.visible;
        o->line_first_kf[i] = P.first;
        o->line_n_obs[i] = O.nObs;
        for (size_t k = 0; k < O.obs.size(); k++, a++) {
            o->line_obs[a] = O.obs[k];
            o->line_obs_index[a] = O.obsIdx[k];
        }
        o->line_obs_offsets[i + 1] = a;
    }
    return DRFE_OK;
}

int drfe_lmap_recent_increase(drfe_lmap* db, int kind, int32_t count, const int32_t* handles, const int32_t* d_found, const int32_t* d_visible)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !d_found || !d_visible))) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_recent_increase: invalid argument");
    if (kind != DRFE_LMAP_POINT && kind != DRFE_LMAP_LINE) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_recent_increase: unknown kind");
    std::unordered_map<int32_t, ItemRecent>& rows = kind == DRFE_LMAP_POINT ? db->mpRec : db->mlRec;
    if (!known_all(rows, count, handles)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_recent_increase: a handle without recent-list attributes");
    /* the image follows in place while it is current; the slots of an item that is not stored yet come with the next build */
    const bool inPlace = !db->imgDirty && !db->cullDirty && !db->recDirty;
    const std::unordered_map<int32_t, int32_t>& slot = kind == DRFE_LMAP_POINT ? db->img.mpSlot : db->img.mlSlot;
    std::vector<int32_t>& found = kind == DRFE_LMAP_POINT ? db->rec.mpFound : db->rec.mlFound;
    std::vector<int32_t>& visible = kind == DRFE_LMAP_POINT ? db->rec.mpVisible : db->rec.mlVisible;
    for (int i = 0; i < count; i++) {
        ItemRecent& P = rows.at(handles[i]);
        P.found = (int32_t)((uint32_t)P.found + (uint32_t)d_found[i]);
        P.visible = (int32_t)((uint32_t)P.visible + (uint32_t)d_visible[i]);
        if (!inPlace) continue;
        const auto it = slot.find(handles[i]);
        if (it == slot.end()) continue;
        found[(size_t)it->second] = P.found;
        visible[(size_t)it->second] = P.visible;
    }
    if (count && inPlace) db->blk[drfe_lmap::RECENT].stale(0, db->secRecCounters);
    return DRFE_OK;
}

int drfe_lmap_recent_cull_host(drfe_lmap* db, int64_t current_kf_id, int32_t monocular, drfe_lmap_recent_list* points, drfe_lmap_recent_list* lines)
{
    return recent_entry_point(db, current_kf_id, monocular, points, lines, 0, nullptr);
}
int drfe_lmap_recent_cull_device(drfe_lmap* db, int64_t current_kf_id, int32_t monocular, drfe_lmap_recent_list* points, drfe_lmap_recent_list* lines,
                                 void* stream)
{
    return recent_entry_point(db, current_kf_id, monocular, points, lines, 1, stream);
}
int drfe_lmap_recent_cull_batch(drfe_lmap* db, int64_t current_kf_id, int32_t monocular, drfe_lmap_recent_list* points, drfe_lmap_recent_list* lines,
                                void* stream)
{
    return recent_entry_point(db, current_kf_id, monocular, points, lines, 2, stream);
}

int drfe_lmap_recent_cull_limits(int32_t* out6)
{
    if (!out6) return DRFE_ERR_INVALID;
    out6[0] = RECENT_TILE;
    out6[1] = RECENT_ERASE_TILE;
    out6[2] = RECENT_ENTRY_BYTES;
    out6[3] = 64;
    out6[4] = DRFE_LMAP_RECENT_MAX_ENTRIES;
    out6[5] = DRFE_LMAP_RECENT_DEVICE_FROM;
    return DRFE_OK;
}

int drfe_lmap_recent_cull_scratch(drfe_lmap* db, int64_t n_entries, int64_t* out3)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!out3 || n_entries < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_recent_cull_scratch: invalid argument");
    const int rc = lmap_build_image(db);
    if (rc) return rc;
    const RecentFit F = recent_fit(db, n_entries);
    out3[0] = F.whole;
    out3[1] = F.least;
    out3[2] = F.fixed;
    return DRFE_OK;
}

int drfe_lmap_recent_cull_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::recStats, stats); }

int drfe_lmap_recent_upload_bytes(drfe_lmap* db, int64_t* out1)
{
    if (!db || !out1) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    *out1 = db->sentBytes[drfe_lmap::RECENT];
    return DRFE_OK;
}

}  // extern "C"
