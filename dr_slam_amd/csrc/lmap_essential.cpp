/* lmap_essential.cpp — what surrounds the solver of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2910-3131) on the
 * local-map store, behind the C-ABI of include/drfe.h: the loop edges as store state, by handle and by slot; the edge builder with
 * its checks, its host entry and its device entry; the commit of the solver's estimates with its checks, its host entry, its
 * device entry and the write into the rows; the counters.  Both sides evaluate essential_core.h (essential_kernels.hip on the
 * device).  A call is checked as a whole before anything is written.  DESIGN.md section 35. */
#include "lmap_call.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <unordered_set>

using namespace lmap_store;

namespace {

/* the loop edges by slot, after the image and the geometry */
int build_ess(drfe_lmap* db)
{
    const int rc = lmap_build_geo(db);
    if (rc) return rc;
    if (!db->essDirty) return DRFE_OK;
    const Image& G = db->img;
    EssAttr& A = db->ess;
    const size_t nK = G.kfHandle.size();
    A.leOff.assign(1, 0);
    A.le.clear();
    A.unknown.clear();
    std::vector<int32_t> row;
    for (size_t s = 0; s < nK; s++) {
        const auto it = db->loopEdges.empty() ? db->loopEdges.end() : db->loopEdges.find(G.kfHandle[s]);
        if (it != db->loopEdges.end()) {
            row.clear();
            for (const int32_t m : it->second) {
                const auto k = G.kfSlot.find(m);
                if (k == G.kfSlot.end()) A.unknown.emplace_back((int32_t)s, m);
                else row.push_back(k->second);
            }
            std::sort(row.begin(), row.end());   /* ascending slot = rank order: set<KeyFrame*> */
            A.le.insert(A.le.end(), row.begin(), row.end());
        }
        A.leOff.push_back((int32_t)A.le.size());
    }
    db->essDirty = false;
    db->blk[drfe_lmap::LOOPS].stale_all();
    return DRFE_OK;
}

/* ---------------------------------------------------------------- the edge builder ---------------------------------------------- */

/* a checked call in slots */
struct EdgePlan {
    int32_t loop = -1, cur = -1;
    std::vector<int32_t> vert, tab;                    /* the vertices; per slot the row of the tables or -1 */
    std::vector<int32_t> lcKey, lcOff, lcKf;           /* keys in rank order, members in rank order */
    std::vector<uint64_t> pairKey;
    std::vector<int32_t> pairI, pairJ;
    std::vector<int32_t> capOff;                       /* per unit: where its descriptors start in the bound */
    int64_t bound = 0;
};

struct EdgeResult {
    std::vector<double> scw, meas;                     /* 8 per vertex, 8 per edge */
    std::vector<int32_t> from, to;                     /* slots */
    std::vector<uint8_t> kind;
    int64_t emptied = 0;
};

bool edges_call_ok(const drfe_lmap_essential_edges_call* c)
{
    return c && c->n_sim3 >= 0 && c->n_lc >= 0 && (c->n_sim3 == 0 || (c->sim3_handles && c->corrected && c->non_corrected)) &&
           (c->n_lc == 0 || (c->lc_handles && lmap_offsets_ok(c->lc_offsets, c->n_lc) && (c->lc_offsets[c->n_lc] == 0 || c->lc_kfs))) &&
           c->vertices_capacity >= 0 && c->edges_capacity >= 0 && c->n_vertices && c->n_edges &&
           (c->vertices_capacity == 0 || (c->vertices && c->Scw && c->fixed)) &&
           (c->edges_capacity == 0 || (c->from && c->to && c->measurement && c->kind));
}

int edges_plan(drfe_lmap* db, const drfe_lmap_essential_edges_call* c, EdgePlan& P)
{
    const Image& G = db->img;
    const GeoImage& E = db->geo;
    const EssAttr& A = db->ess;
    const size_t nK = G.kfHandle.size();
    auto fail = [&](int rc, const std::string& why) { return lmap_fail(db, rc, "lmap_essential_edges: " + why); };
    auto name = [&](int32_t s) { return std::to_string(G.kfHandle[(size_t)s]); };
    /* what is wrong with the arguments themselves, first */
    std::unordered_set<int32_t> seen;
    for (int a = 0; a < c->n_sim3; a++)
        if (!seen.insert(c->sim3_handles[a]).second) return fail(DRFE_ERR_INVALID, "the Sim3 table names key frame " + std::to_string(c->sim3_handles[a]) + " twice");
    seen.clear();
    for (int a = 0; a < c->n_lc; a++)
        if (!seen.insert(c->lc_handles[a]).second) return fail(DRFE_ERR_INVALID, "the loop connections name the key " + std::to_string(c->lc_handles[a]) + " twice");
    for (int a = 0; a < c->n_lc; a++) {
        seen.clear();
        for (int32_t e = c->lc_offsets[a]; e < c->lc_offsets[a + 1]; e++)
            if (!seen.insert(c->lc_kfs[e]).second)
                return fail(DRFE_ERR_INVALID, "the loop connections of key " + std::to_string(c->lc_handles[a]) + " name key frame " + std::to_string(c->lc_kfs[e]) + " twice");
    }
    const auto lp = G.kfSlot.find(c->loop_kf), cu = G.kfSlot.find(c->cur_kf);
    if (lp == G.kfSlot.end()) return fail(DRFE_ERR_STATE, "the loop key frame " + std::to_string(c->loop_kf) + " is unknown");
    if (cu == G.kfSlot.end()) return fail(DRFE_ERR_STATE, "the current key frame " + std::to_string(c->cur_kf) + " is unknown");
    P.loop = lp->second;
    P.cur = cu->second;
    P.tab.assign(nK, -1);
    for (int a = 0; a < c->n_sim3; a++) {
        const auto it = G.kfSlot.find(c->sim3_handles[a]);
        if (it != G.kfSlot.end()) P.tab[(size_t)it->second] = a;
    }
    for (size_t s = 0; s < nK; s++) {
        if (G.kfBad[s]) continue;
        if (P.tab[s] < 0 && !E.kfHas[s]) return fail(DRFE_ERR_STATE, "key frame " + name((int32_t)s) + " has no pose and the corrected table does not name it");
        P.vert.push_back((int32_t)s);
    }
    /* LoopConnections: map<KeyFrame*, set<KeyFrame*>> */
    std::vector<std::pair<int32_t, int32_t>> keys;     /* (slot, index in the call) */
    for (int a = 0; a < c->n_lc; a++) {
        const auto it = G.kfSlot.find(c->lc_handles[a]);
        if (it == G.kfSlot.end()) return fail(DRFE_ERR_STATE, "the loop-connection key " + std::to_string(c->lc_handles[a]) + " is unknown");
        keys.emplace_back(it->second, a);
    }
    std::sort(keys.begin(), keys.end());
    P.lcOff.assign(1, 0);
    std::vector<int32_t> row;
    for (const auto& k : keys) {
        row.clear();
        for (int32_t e = c->lc_offsets[k.second]; e < c->lc_offsets[k.second + 1]; e++) {
            const auto it = G.kfSlot.find(c->lc_kfs[e]);
            if (it == G.kfSlot.end())
                return fail(DRFE_ERR_STATE, "the loop-connection member " + std::to_string(c->lc_kfs[e]) + " of key " + name(k.first) + " is unknown");
            row.push_back(it->second);
        }
        std::sort(row.begin(), row.end());
        P.lcKey.push_back(k.first);
        P.lcKf.insert(P.lcKf.end(), row.begin(), row.end());
        P.lcOff.push_back((int32_t)P.lcKf.size());
    }
    /* every edge that would go to a null vertex */
    const int32_t *wOff = G.cwOff.data(), *wKf = G.cwKf.data(), *wW = G.cwW.data();
    for (size_t u = 0; u < P.lcKey.size(); u++) {
        const int32_t i = P.lcKey[u];
        for (int32_t e = P.lcOff[u]; e < P.lcOff[u + 1]; e++) {
            const int32_t j = P.lcKf[(size_t)e];
            if (!ess_lc_kept(wOff, wKf, wW, i, j, P.cur, P.loop)) continue;
            if (G.kfBad[(size_t)i] || G.kfBad[(size_t)j])
                return fail(DRFE_ERR_STATE, "the loop-connection edge " + name(i) + " -> " + name(j) + " has an end without a vertex: key frame " +
                                                name(G.kfBad[(size_t)i] ? i : j) + " is bad");
        }
    }
    for (const int32_t i : P.vert) {
        const int32_t pa = G.kfParent[(size_t)i];
        if (pa >= 0 && G.kfBad[(size_t)pa])
            return fail(DRFE_ERR_STATE, "the spanning-tree edge " + name(i) + " -> " + name(pa) + " has an end without a vertex: the parent " + name(pa) + " is bad");
        for (int32_t e = A.leOff[(size_t)i]; e < A.leOff[(size_t)i + 1]; e++) {
            const int32_t m = A.le[(size_t)e];
            if (G.kfHandle[(size_t)m] < G.kfHandle[(size_t)i] && G.kfBad[(size_t)m])
                return fail(DRFE_ERR_STATE, "the loop edge " + name(i) + " -> " + name(m) + " has an end without a vertex: key frame " + name(m) + " is bad");
        }
    }
    for (const auto& d : A.unknown)
        if (!G.kfBad[(size_t)d.first] && d.second < G.kfHandle[(size_t)d.first])
            return fail(DRFE_ERR_STATE, "the loop edge " + name(d.first) + " -> " + std::to_string(d.second) + " has an end without a vertex: key frame " +
                                            std::to_string(d.second) + " is unknown");
    /* the bound of each unit, from the row lengths */
    P.capOff.assign(1, 0);
    for (size_t u = 0; u < P.lcKey.size(); u++) {
        P.bound += P.lcOff[u + 1] - P.lcOff[u];
        P.capOff.push_back((int32_t)std::min<int64_t>(P.bound, INT32_MAX));
    }
    for (const int32_t i : P.vert) {
        P.bound += (G.kfParent[(size_t)i] >= 0) + (A.leOff[(size_t)i + 1] - A.leOff[(size_t)i]) + (G.coOff[(size_t)i + 1] - G.coOff[(size_t)i]);
        P.capOff.push_back((int32_t)std::min<int64_t>(P.bound, INT32_MAX));
    }
    if (P.bound >= INT32_MAX) return fail(DRFE_ERR_CAPACITY, "more possible edges than an int32 counts");
    /* every entry as a pair, for sInsertedEdges.count() */
    std::vector<std::pair<uint64_t, std::pair<int32_t, int32_t>>> pairs;
    for (size_t u = 0; u < P.lcKey.size(); u++)
        for (int32_t e = P.lcOff[u]; e < P.lcOff[u + 1]; e++)
            pairs.push_back({ess_pair(P.lcKey[u], P.lcKf[(size_t)e]), {P.lcKey[u], P.lcKf[(size_t)e]}});
    std::sort(pairs.begin(), pairs.end());
    for (const auto& p : pairs) {
        P.pairKey.push_back(p.first);
        P.pairI.push_back(p.second.first);
        P.pairJ.push_back(p.second.second);
    }
    return DRFE_OK;
}

void table_rows(const drfe_lmap_essential_edges_call* c, int32_t row, const double*& co, const double*& nc)
{
    co = row < 0 ? nullptr : c->corrected + 8 * (size_t)row;
    nc = row < 0 ? nullptr : c->non_corrected + 8 * (size_t)row;
}

/* the reference's loops */
void edges_host(drfe_lmap* db, const drfe_lmap_essential_edges_call* c, const EdgePlan& P, EdgeResult& R)
{
    const Image& G = db->img;
    const GeoImage& E = db->geo;
    const EssAttr& A = db->ess;
    const size_t nK = G.kfHandle.size();
    const int32_t *wOff = G.cwOff.data(), *wKf = G.cwKf.data(), *wW = G.cwW.data();
    std::vector<EssKf> kf(nK);
    R.scw.resize(8 * P.vert.size());
    for (size_t v = 0; v < P.vert.size(); v++) {
        const size_t s = (size_t)P.vert[v];
        const double *co, *nc;
        table_rows(c, P.tab[s], co, nc);
        ess_vertex(co, nc, &E.kfTcw[16 * s], kf[s]);
        corr_sim3_to8(kf[s].scw, &R.scw[8 * v]);
    }
    auto add = [&](int32_t i, int32_t j, int kind) {
        R.from.push_back(i);
        R.to.push_back(j);
        R.kind.push_back((uint8_t)kind);
    };
    for (size_t u = 0; u < P.lcKey.size(); u++)
        for (int32_t e = P.lcOff[u]; e < P.lcOff[u + 1]; e++)
            if (ess_lc_kept(wOff, wKf, wW, P.lcKey[u], P.lcKf[(size_t)e], P.cur, P.loop)) add(P.lcKey[u], P.lcKf[(size_t)e], ESS_KIND_LOOP_CONNECTION);
    for (const int32_t i : P.vert) {
        const int32_t pa = G.kfParent[(size_t)i];
        if (pa >= 0) add(i, pa, ESS_KIND_SPANNING_TREE);
        const int32_t l0 = A.leOff[(size_t)i], nLe = A.leOff[(size_t)i + 1] - l0;
        for (int32_t e = 0; e < nLe; e++)
            if (G.kfHandle[(size_t)A.le[(size_t)(l0 + e)]] < G.kfHandle[(size_t)i]) add(i, A.le[(size_t)(l0 + e)], ESS_KIND_LOOP_EDGE);
        const int32_t o0 = G.coOff[(size_t)i], len = G.coOff[(size_t)i + 1] - o0;
        int32_t first = 0;
        while (first < len && G.coW[(size_t)(o0 + first)] >= ESS_MIN_FEAT) first++;
        const int32_t n = ess_prefix(first, len);
        R.emptied += len > 0 && first == len;
        const int32_t c0 = G.childOff[(size_t)i];
        for (int32_t e = 0; e < n; e++) {
            const int32_t other = G.coKf[(size_t)(o0 + e)];
            if (ess_covis_kept(G.child.data() + c0, G.childOff[(size_t)i + 1] - c0, A.le.data() + l0, nLe, G.kfBad.data(), G.kfHandle.data(), pa, i, other) &&
                !ess_inserted(P.pairKey.data(), P.pairI.data(), P.pairJ.data(), (int32_t)P.pairKey.size(), wOff, wKf, wW, i, other, P.cur, P.loop))
                add(i, other, ESS_KIND_COVISIBILITY);
        }
    }
    R.meas.resize(8 * R.from.size());
    for (size_t e = 0; e < R.from.size(); e++) ess_measure(kf[(size_t)R.from[e]], kf[(size_t)R.to[e]], R.kind[e], &R.meas[8 * e]);
}

int64_t edges_scratch(const drfe_lmap* db, int64_t bound, int64_t* fixed)
{
    *fixed = ESS_FIXED_BYTES + (int64_t)ESS_VERTEX_BYTES * (int64_t)db->img.kfHandle.size();
    return *fixed + (int64_t)ESS_EDGE_BYTES * bound;
}

/* the plan launches and the total back, the capacity test, then the write launch and the edges back.  Nothing resident is written. */
int edges_device(drfe_lmap* db, const drfe_lmap_essential_edges_call* c, const EdgePlan& P, EdgeResult& R, void* stream)
{
    LmapCall call{db, "lmap essential edges"};
    if (const int rc = call.begin(LMAP_NEED_LOOPS, stream)) return rc;
    const Image& G = db->img;
    const size_t nK = G.kfHandle.size(), nV = P.vert.size(), nLc = P.lcKey.size(), nU = nLc + nV, nPairs = P.pairKey.size();
    const size_t nT = (size_t)c->n_sim3, bound = (size_t)P.bound;
    StageLayout<16> in, out, scr;
    const auto sHandle = in.add<int32_t>(nK);
    const auto sVert = in.add<int32_t>(nV);
    const auto sTab = in.add<int32_t>(nK);
    const auto sCo = in.add<double>(8 * nT);
    const auto sNc = in.add<double>(8 * nT);
    const auto sKey = in.add<int32_t>(nLc);
    const auto sOff = in.add<int32_t>(nLc + 1);
    const auto sKf = in.add<int32_t>(P.lcKf.size());
    const auto sPair = in.add<uint64_t>(nPairs);
    const auto sPairI = in.add<int32_t>(nPairs);
    const auto sPairJ = in.add<int32_t>(nPairs);
    const auto sCap = in.add<int32_t>(nU + 1);
    const auto oScw = out.add<double>(8 * nV);
    const auto oCnt = out.add<int32_t>(nU + 2);
    const auto oEmp = out.add<uint8_t>(nU);
    const auto xKf = scr.add<EssKf>(nK);
    const auto xTo = scr.add<int32_t>(bound);
    const auto xKind = scr.add<uint8_t>(bound);
    const auto xFrom = scr.add<int32_t>(bound);
    const auto xETo = scr.add<int32_t>(bound);
    const auto xMeas = scr.add<double>(8 * bound);
    const auto xEKind = scr.add<uint8_t>(bound);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, ho] = call.at;
    sHandle.put(h, G.kfHandle.data());
    sVert.put(h, P.vert.data());
    sTab.put(h, P.tab.data());
    sCo.put(h, c->corrected);
    sNc.put(h, c->non_corrected);
    sKey.put(h, P.lcKey.data());
    sOff.put(h, P.lcOff.data());
    sKf.put(h, P.lcKf.data());
    sPair.put(h, P.pairKey.data());
    sPairI.put(h, P.pairI.data());
    sPairJ.put(h, P.pairJ.data());
    sCap.put(h, P.capOff.data());
    if (const int rc = call.send()) return rc;
    EssEdgesLaunch L{};
    L.I = db->dView;
    L.C = db->dConn;
    L.G = db->dCorr;
    L.E = db->dEss;
    L.nV = (int32_t)nV;
    L.nLc = (int32_t)nLc;
    L.nU = (int32_t)nU;
    L.nPairs = (int32_t)nPairs;
    L.cur = P.cur;
    L.loop = P.loop;
    L.bound = (int32_t)bound;
    L.kfHandle = sHandle.at(d);
    L.vert = sVert.at(d);
    L.tab = sTab.at(d);
    L.corrected = sCo.at(d);
    L.nonCorrected = sNc.at(d);
    L.lcKey = sKey.at(d);
    L.lcOff = sOff.at(d);
    L.lcKf = sKf.at(d);
    L.pairKey = sPair.at(d);
    L.pairI = sPairI.at(d);
    L.pairJ = sPairJ.at(d);
    L.capOff = sCap.at(d);
    L.kf = xKf.at(dS);
    L.cnt = oCnt.at(dO);
    L.emptied = oEmp.at(dO);
    L.dTo = xTo.at(dS);
    L.dKind = xKind.at(dS);
    L.outScw = oScw.at(dO);
    L.eFrom = xFrom.at(dS);
    L.eTo = xETo.at(dS);
    L.eMeas = xMeas.at(dS);
    L.eKind = xEKind.at(dS);
    if (const int rc = call.back(drfe_launch_essential_plan(L, call.st))) return rc;
    R.scw.assign(oScw.at(ho), oScw.at(ho) + 8 * nV);
    const int64_t total = oCnt.at(ho)[nU];
    R.emptied = oCnt.at(ho)[nU + 1];
    if (total < 0 || total > P.bound) return lmap_fail(db, DRFE_ERR_STATE, "lmap essential edges device call: the total is past its bound");
    if (total > c->edges_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_essential_edges: more edges than edges_capacity");
    LmapFetch f;
    const auto lFrom = f.add(xFrom.at(dS), (size_t)total);
    const auto lTo = f.add(xETo.at(dS), (size_t)total);
    const auto lMeas = f.add(xMeas.at(dS), 8 * (size_t)total);
    const auto lKind = f.add(xEKind.at(dS), (size_t)total);
    if (const int rc = call.fetch(f, drfe_launch_essential_write(L, (int32_t)total, call.st))) return rc;
    R.from.resize((size_t)total);
    R.to.resize((size_t)total);
    R.meas.resize(8 * (size_t)total);
    R.kind.resize((size_t)total);
    f.get(lFrom, R.from.data());
    f.get(lTo, R.to.data());
    f.get(lMeas, R.meas.data());
    f.get(lKind, R.kind.data());
    return DRFE_OK;
}

/* mode: 0 host, 1 device, 2 by the crossover */
int edges_entry(drfe_lmap* db, drfe_lmap_essential_edges_call* c, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_essential_edges: a device call on a store without a context");
    if (!edges_call_ok(c)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_essential_edges: invalid argument");
    int rc = build_ess(db);
    if (rc) return rc;
    EdgePlan P;
    rc = edges_plan(db, c, P);
    if (rc) return rc;
    const Image& G = db->img;
    if ((int64_t)P.vert.size() > c->vertices_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_essential_edges: more vertices than vertices_capacity");
    bool dev = mode == 1 || (mode == 2 && db->ctx && (int64_t)G.kfHandle.size() >= (int64_t)DRFE_LMAP_ESSENTIAL_EDGES_DEVICE_FROM);
    if (dev) {
        int64_t fixed;
        const bool fits = edges_scratch(db, P.bound, &fixed) <= db->scratchBytes;
        if (!fits && mode == 1) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_essential_edges: the call does not fit the configured device scratch");
        dev = fits;
    }
    EdgeResult R;
    if (dev) {
        rc = edges_device(db, c, P, R, stream);
        if (rc) return rc;
    } else {
        edges_host(db, c, P, R);
        if ((int64_t)R.from.size() > c->edges_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_essential_edges: more edges than edges_capacity");
    }
    const size_t nV = P.vert.size(), nE = R.from.size();
    *c->n_vertices = (int32_t)nV;
    *c->n_edges = (int32_t)nE;
    for (size_t v = 0; v < nV; v++) {
        c->vertices[v] = G.kfHandle[(size_t)P.vert[v]];
        c->fixed[v] = P.vert[v] == P.loop;
    }
    if (nV) std::memcpy(c->Scw, R.scw.data(), 64 * nV);
    for (size_t e = 0; e < nE; e++) {
        c->from[e] = G.kfHandle[(size_t)R.from[e]];
        c->to[e] = G.kfHandle[(size_t)R.to[e]];
    }
    if (nE) {
        std::memcpy(c->measurement, R.meas.data(), 64 * nE);
        std::memcpy(c->kind, R.kind.data(), nE);
    }
    int64_t* st = db->essStats;
    st[0]++;
    if (dev) st[2]++;
    st[3] += (int64_t)nV;
    st[4] += (int64_t)nE;
    st[7] += R.emptied;
    return DRFE_OK;
}

/* ---------------------------------------------------------------- the commit ---------------------------------------------------- */

struct CommitPlan {
    std::vector<int32_t> named, posOf;                 /* slots in the caller's order; per slot the index in the call or -1 */
    int64_t moved = 0, identity = 0, chunkPts = 0;
    std::vector<int32_t> chunkMoved, grpStart, grpOff; /* per chunk its moved points and where its workgroups' offsets start */
};

struct CommitResult {
    std::vector<float> Tiw;                            /* 16 per named key frame */
    std::vector<double> swc;                           /* 8 */
    std::vector<int32_t> item, ref;                    /* point slots, nIDr as a handle */
    std::vector<float> world, normal, maxD, minD;
    std::vector<uint8_t> status;
};

bool commit_call_ok(const drfe_lmap_essential_commit_call* c)
{
    return c && c->n >= 0 && (c->n == 0 || (c->handles && c->Scw && c->optimised && c->Tiw && c->Swc)) && c->points_capacity >= 0 && c->n_points &&
           (c->points_capacity == 0 || (c->points && c->ref && c->world && c->normal && c->max_distance && c->min_distance && c->status));
}

struct CommitFit {
    int64_t fixed = 0, whole = 0, least = 0, chunkPts = 0;
    bool fits = false;
};

CommitFit commit_fit(const drfe_lmap* db)
{
    CommitFit F;
    const int64_t nP = (int64_t)db->img.mpHandle.size();
    F.fixed = ESS_FIXED_BYTES + (int64_t)ESS_KF_BYTES * (int64_t)db->img.kfHandle.size();
    F.whole = F.fixed + ESS_POINT_BYTES * nP;
    F.least = F.fixed + ESS_POINT_BYTES * std::min<int64_t>(nP, 1);
    F.fits = F.least <= db->scratchBytes;
    F.chunkPts = F.fits ? std::min<int64_t>(nP, (db->scratchBytes - F.fixed) / ESS_POINT_BYTES) : 0;
    return F;
}

/* everything the call can be refused for, and its counts; with chunkPts the moved points of every chunk and workgroup */
int commit_check(drfe_lmap* db, const drfe_lmap_essential_commit_call* c, CommitPlan& P)
{
    const Image& G = db->img;
    const GeoImage& E = db->geo;
    const size_t nK = G.kfHandle.size(), nP = G.mpHandle.size();
    const int32_t nLevels = (int32_t)db->scales.size();
    auto fail = [&](int rc, const std::string& why) { return lmap_fail(db, rc, "lmap_essential_commit: " + why); };
    auto kfName = [&](int32_t s) { return "key frame " + std::to_string(G.kfHandle[(size_t)s]); };
    P.posOf.assign(nK, -1);
    for (int a = 0; a < c->n; a++) {
        const auto it = G.kfSlot.find(c->handles[a]);
        if (it == G.kfSlot.end()) return fail(DRFE_ERR_INVALID, "the call names the unknown key-frame handle " + std::to_string(c->handles[a]));
        if (P.posOf[(size_t)it->second] >= 0) return fail(DRFE_ERR_INVALID, "the call names " + kfName(it->second) + " twice");
        P.posOf[(size_t)it->second] = a;
        P.named.push_back(it->second);
    }
    for (size_t s = 0; s < nK; s++) {
        if (G.kfBad[s] && P.posOf[s] >= 0) return fail(DRFE_ERR_STATE, "the named " + kfName((int32_t)s) + " is bad and has no vertex");
        if (!G.kfBad[s] && P.posOf[s] < 0) return fail(DRFE_ERR_STATE, "the call does not name " + kfName((int32_t)s));
    }
    auto centre_ok = [&](int32_t s) { return P.posOf[(size_t)s] >= 0 || E.kfHas[(size_t)s]; };
    for (size_t p = 0; p < nP; p++) {
        if (G.mpBad[p]) continue;
        const int32_t h = G.mpHandle[p];
        const std::string mp = "map point " + std::to_string(h);
        if (!E.mpHas[p]) return fail(DRFE_ERR_STATE, mp + " has no geometry");
        if (nLevels <= 0) return fail(DRFE_ERR_STATE, "the store has no scale factors");
        const int32_t r = E.mpRef[p];
        if (r < 0) return fail(DRFE_ERR_STATE, "the reference key frame " + std::to_string(db->mpGeo.at(h).ref) + " of " + mp + " is unknown");
        if (E.mpLevel[p] < 0 || E.mpLevel[p] >= nLevels) return fail(DRFE_ERR_STATE, "ref_level of " + mp + " is not a level of the store");
        const int32_t idr = ess_ref_handle(E.mpBy[p], E.mpByRef[p], G.kfHandle[(size_t)r], c->cur_kf);
        const auto it = G.kfSlot.find(idr);
        if (it == G.kfSlot.end()) return fail(DRFE_ERR_STATE, "nIDr " + std::to_string(idr) + " of " + mp + " is not a stored key frame");
        if (G.obsOff[p + 1] > G.obsOff[p]) {
            for (int32_t o = G.obsOff[p]; o < G.obsOff[p + 1]; o++)
                if (!centre_ok(G.obs[(size_t)o])) return fail(DRFE_ERR_STATE, "the observing " + kfName(G.obs[(size_t)o]) + " of " + mp + " is not named and has no pose");
            if (!centre_ok(r)) return fail(DRFE_ERR_STATE, "the reference " + kfName(r) + " of " + mp + " is not named and has no pose");
        }
        P.moved++;
        P.identity += P.posOf[(size_t)it->second] < 0;
    }
    if (P.moved > c->points_capacity) return fail(DRFE_ERR_CAPACITY, "more moved points than points_capacity");
    if (P.chunkPts > 0)
        for (size_t p0 = 0; p0 < nP; p0 += (size_t)P.chunkPts) {
            const size_t p1 = std::min(nP, p0 + (size_t)P.chunkPts);
            P.grpStart.push_back((int32_t)P.grpOff.size());
            int32_t m = 0;
            for (size_t g0 = p0; g0 < p1; g0 += ESS_TILE) {
                P.grpOff.push_back(m);
                for (size_t p = g0; p < std::min(p1, g0 + ESS_TILE); p++) m += !G.mpBad[p];
            }
            P.chunkMoved.push_back(m);
        }
    return DRFE_OK;
}

void commit_host(drfe_lmap* db, const drfe_lmap_essential_commit_call* c, const CommitPlan& P, CommitResult& R)
{
    lmap_host_views(db);
    const LmapImage I = db->hView;
    const CorrImage V = db->hCorr;
    const Image& G = db->img;
    const size_t nK = G.kfHandle.size(), n = P.named.size();
    std::vector<EssMove> mv(nK);
    for (EssMove& m : mv) {
        ess_identity(m.scw);
        ess_identity(m.swc);
    }
    std::vector<float> ow(db->geo.kfOw);
    R.Tiw.resize(16 * n);
    R.swc.resize(8 * n);
    for (size_t a = 0; a < n; a++) {
        const size_t s = (size_t)P.named[a];
        corr_sim3_from8(c->Scw + 8 * a, mv[s].scw);
        ess_pose(c->optimised + 8 * a, mv[s].swc, &R.Tiw[16 * a], &ow[3 * s]);
        corr_sim3_to8(mv[s].swc, &R.swc[8 * a]);
    }
    for (int32_t p = 0; p < I.nP; p++) {
        if (I.mpBad[p]) continue;
        const int32_t idr = ess_ref_handle(V.mpBy[p], V.mpByRef[p], G.kfHandle[(size_t)V.mpRef[p]], c->cur_kf);
        const EssMove& m = mv[(size_t)G.kfSlot.at(idr)];
        float Xn[3], nrm[3], maxD, minD;
        corr_point(m.scw, m.swc, V.mpWorld + 3 * (size_t)p, Xn);
        const uint8_t st = ess_normal(V, ow.data(), I.obsOff, I.obs, p, Xn, nrm, &maxD, &minD);
        R.item.push_back(p);
        R.ref.push_back(idr);
        R.world.insert(R.world.end(), Xn, Xn + 3);
        R.normal.insert(R.normal.end(), nrm, nrm + 3);
        R.maxD.push_back(maxD);
        R.minD.push_back(minD);
        R.status.push_back(st);
    }
}

/* The key-frame launch and its records back, then chunk after chunk of point slots its records back.  Everything the call could
 * be refused for has been checked, so the resident geometry is written from the first launch on; a HIP failure in between leaves
 * it to be sent again. */
int commit_device(drfe_lmap* db, const drfe_lmap_essential_commit_call* c, const CommitPlan& P, CommitResult& R, void* stream)
{
    LmapCall call{db, "lmap essential commit"};
    if (const int rc = call.begin(LMAP_NEED_GEO, stream)) return rc;
    const Image& G = db->img;
    const size_t nK = G.kfHandle.size(), nP = G.mpHandle.size(), n = P.named.size(), chunk = (size_t)P.chunkPts;
    size_t most = 0;
    for (const int32_t m : P.chunkMoved) most = std::max(most, (size_t)m);
    std::vector<std::pair<int32_t, int32_t>> byHandle;
    for (size_t s = 0; s < nK; s++) byHandle.emplace_back(G.kfHandle[s], (int32_t)s);
    std::sort(byHandle.begin(), byHandle.end());
    StageLayout<16> in, out, scr;
    const auto sNamed = in.add<int32_t>(n);
    const auto sPos = in.add<int32_t>(nK);
    const auto sScw = in.add<double>(8 * n);
    const auto sOpt = in.add<double>(8 * n);
    const auto sHandle = in.add<int32_t>(nK);
    const auto sSorted = in.add<int32_t>(nK);
    const auto sSlot = in.add<int32_t>(nK);
    const auto sGrp = in.add<int32_t>(P.grpOff.size());
    const auto oTiw = out.add<float>(16 * n);
    const auto oSwc = out.add<double>(8 * n);
    const auto xMv = scr.add<EssMove>(nK);
    const auto xItem = scr.add<int32_t>(most);
    const auto xRef = scr.add<int32_t>(most);
    const auto xWorld = scr.add<float>(3 * most);
    const auto xNormal = scr.add<float>(3 * most);
    const auto xMax = scr.add<float>(most);
    const auto xMin = scr.add<float>(most);
    const auto xStatus = scr.add<uint8_t>(most);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, ho] = call.at;
    LmapFetch f;
    const auto lItem = f.add(xItem.at(dS), most);
    const auto lRef = f.add(xRef.at(dS), most);
    const auto lWorld = f.add(xWorld.at(dS), 3 * most);
    const auto lNormal = f.add(xNormal.at(dS), 3 * most);
    const auto lMax = f.add(xMax.at(dS), most);
    const auto lMin = f.add(xMin.at(dS), most);
    const auto lStatus = f.add(xStatus.at(dS), most);
    if (const int rc = call.room(f)) return rc;
    sNamed.put(h, P.named.data());
    sPos.put(h, P.posOf.data());
    sScw.put(h, c->Scw);
    sOpt.put(h, c->optimised);
    sHandle.put(h, G.kfHandle.data());
    for (size_t k = 0; k < nK; k++) {
        sSorted.at(h)[k] = byHandle[k].first;
        sSlot.at(h)[k] = byHandle[k].second;
    }
    sGrp.put(h, P.grpOff.data());
    if (const int rc = call.send()) return rc;
    EssCommitLaunch L{};
    L.I = db->dView;
    L.G = db->dCorr;
    L.n = (int32_t)n;
    L.cur = c->cur_kf;
    L.pkCap = (int32_t)most;
    L.named = sNamed.at(d);
    L.posOf = sPos.at(d);
    L.scw = sScw.at(d);
    L.optimised = sOpt.at(d);
    L.kfHandle = sHandle.at(d);
    L.hSorted = sSorted.at(d);
    L.hSlot = sSlot.at(d);
    L.mv = xMv.at(dS);
    L.pkItem = xItem.at(dS);
    L.pkRef = xRef.at(dS);
    L.pkWorld = xWorld.at(dS);
    L.pkNormal = xNormal.at(dS);
    L.pkMax = xMax.at(dS);
    L.pkMin = xMin.at(dS);
    L.pkStatus = xStatus.at(dS);
    L.outTiw = oTiw.at(dO);
    L.outSwc = oSwc.at(dO);
    LmapWrites writes(db->blk[drfe_lmap::GEO]);
    if (const int rc = call.back(drfe_launch_essential_poses(L, call.st))) return rc;
    R.Tiw.assign(oTiw.at(ho), oTiw.at(ho) + 16 * n);
    R.swc.assign(oSwc.at(ho), oSwc.at(ho) + 8 * n);
    const size_t total = (size_t)P.moved;
    R.item.resize(total);
    R.ref.resize(total);
    R.world.resize(3 * total);
    R.normal.resize(3 * total);
    R.maxD.resize(total);
    R.minD.resize(total);
    R.status.resize(total);
    size_t b = 0;
    for (size_t p0 = 0, k = 0; p0 < nP; p0 += chunk, k++) {
        const size_t p1 = std::min(nP, p0 + chunk), cnt = (size_t)P.chunkMoved[k];
        L.p0 = (int32_t)p0;
        L.p1 = (int32_t)p1;
        L.grpOff = sGrp.at(d) + P.grpStart[k];
        f.set(cnt, lItem, lRef, lMax, lMin, lStatus);
        f.set(3 * cnt, lWorld, lNormal);
        if (const int rc = call.fetch(f, drfe_launch_essential_points(L, call.st))) return rc;
        f.get(lItem, R.item.data() + b);
        f.get(lRef, R.ref.data() + b);
        f.get(lWorld, R.world.data() + 3 * b);
        f.get(lNormal, R.normal.data() + 3 * b);
        f.get(lMax, R.maxD.data() + b);
        f.get(lMin, R.minD.data() + b);
        f.get(lStatus, R.status.data() + b);
        b += cnt;
    }
    writes.done();
    return DRFE_OK;
}

/* results into the caller's arrays, and poses and positions into the store */
void commit_finish(drfe_lmap* db, drfe_lmap_essential_commit_call* c, const CommitPlan& P, const CommitResult& R, bool onDevice)
{
    const Image& G = db->img;
    GeoImage& E = db->geo;
    const size_t n = P.named.size(), total = R.item.size();
    if (n) {
        std::memcpy(c->Tiw, R.Tiw.data(), 64 * n);
        std::memcpy(c->Swc, R.swc.data(), 64 * n);
    }
    for (size_t a = 0; a < n; a++) {
        const size_t s = (size_t)P.named[a];
        const float* T = &R.Tiw[16 * a];
        std::memcpy(db->kfPose[G.kfHandle[s]].data(), T, sizeof(float) * 16);
        std::memcpy(&E.kfTcw[16 * s], T, sizeof(float) * 16);
        camera_centre_kf(T, &E.kfOw[3 * s]);
        E.kfHas[s] = 1;
    }
    *c->n_points = (int32_t)total;
    for (size_t t = 0; t < total; t++) {
        const size_t p = (size_t)R.item[t];
        c->points[t] = G.mpHandle[p];
        c->ref[t] = R.ref[t];
        std::memcpy(db->mpGeo.at(c->points[t]).X, &R.world[3 * t], sizeof(float) * 3);
        std::memcpy(&E.mpWorld[3 * p], &R.world[3 * t], sizeof(float) * 3);
    }
    if (total) {
        std::memcpy(c->world, R.world.data(), 12 * total);
        std::memcpy(c->normal, R.normal.data(), 12 * total);
        std::memcpy(c->max_distance, R.maxD.data(), 4 * total);
        std::memcpy(c->min_distance, R.minD.data(), 4 * total);
        std::memcpy(c->status, R.status.data(), total);
    }
    if (!onDevice) db->blk[drfe_lmap::GEO].stale_all();
    int64_t* st = db->essStats;
    st[1]++;
    if (onDevice) st[2]++;
    st[5] += (int64_t)total;
    st[6] += P.identity;
}

int commit_entry(drfe_lmap* db, drfe_lmap_essential_commit_call* c, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_essential_commit: a device call on a store without a context");
    if (!commit_call_ok(c)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_essential_commit: invalid argument");
    int rc = lmap_build_geo(db);
    if (rc) return rc;
    bool dev = mode == 1 || (mode == 2 && db->ctx && (int64_t)db->img.mpHandle.size() >= (int64_t)DRFE_LMAP_ESSENTIAL_COMMIT_DEVICE_FROM);
    CommitPlan P;
    if (dev) {
        const CommitFit F = commit_fit(db);
        if (!F.fits && mode == 1)
            return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_essential_commit: the configured device scratch does not hold the key frames and one point slot");
        dev = F.fits;
        P.chunkPts = F.chunkPts;
    }
    rc = commit_check(db, c, P);
    if (rc) return rc;
    CommitResult R;
    if (dev) {
        rc = commit_device(db, c, P, R, stream);
        if (rc) return rc;
    } else {
        commit_host(db, c, P, R);
    }
    commit_finish(db, c, P, R, dev);
    return DRFE_OK;
}

}  // namespace

extern "C" {

int drfe_lmap_set_loop_edges(drfe_lmap* db, int32_t count, const int32_t* handles, const int32_t* offsets, const int32_t* edges)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_loop_edges: invalid argument");
    if (count == 0) return DRFE_OK;
    if (!handles || !lmap_offsets_ok(offsets, count) || (offsets[count] > 0 && !edges))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_loop_edges: invalid argument");
    std::vector<int32_t> row;
    for (int i = 0; i < count; i++) {
        if (handles[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_loop_edges: a negative handle");
        row.assign(edges + offsets[i], edges + offsets[i + 1]);
        std::sort(row.begin(), row.end());
        if (!row.empty() && row[0] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_loop_edges: a negative loop edge");
        if (std::adjacent_find(row.begin(), row.end()) != row.end())
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_loop_edges: a row names a key frame twice");
    }
    for (int i = 0; i < count; i++) db->loopEdges[handles[i]].assign(edges + offsets[i], edges + offsets[i + 1]);
    db->essDirty = true;
    return DRFE_OK;
}

int drfe_lmap_get_loop_edges(drfe_lmap* db, int32_t count, const int32_t* handles, int32_t capacity, int32_t* offsets, int32_t* edges)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || capacity < 0 || !offsets || (count > 0 && !handles) || (capacity > 0 && !edges))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_loop_edges: invalid argument");
    int64_t total = 0;
    for (int i = 0; i < count; i++) {
        if (db->kf.find(handles[i]) == db->kf.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_loop_edges: unknown handle");
        const auto it = db->loopEdges.find(handles[i]);
        if (it != db->loopEdges.end()) total += (int64_t)it->second.size();
    }
    offsets[0] = 0;
    if (total > capacity) {
        for (int i = 0; i < count; i++) offsets[i + 1] = 0;
        offsets[count] = (int32_t)std::min<int64_t>(total, INT32_MAX);
        return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_get_loop_edges: more loop edges than capacity");
    }
    std::vector<std::pair<std::pair<int, uint64_t>, int32_t>> row;   /* ((not stored, rank or handle), handle) */
    int32_t at = 0;
    for (int i = 0; i < count; i++) {
        const auto it = db->loopEdges.find(handles[i]);
        if (it != db->loopEdges.end()) {
            row.clear();
            for (const int32_t m : it->second) {
                const auto k = db->kf.find(m);
                if (k == db->kf.end()) row.push_back({{1, (uint64_t)m}, m});
                else row.push_back({{0, k->second.rank}, m});
            }
            std::sort(row.begin(), row.end());
            for (const auto& e : row) edges[at++] = e.second;
        }
        offsets[i + 1] = at;
    }
    return DRFE_OK;
}

int drfe_lmap_essential_upload_bytes(drfe_lmap* db, int64_t* out1)
{
    if (!db || !out1) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    *out1 = db->sentBytes[drfe_lmap::LOOPS];
    return DRFE_OK;
}

int drfe_lmap_essential_edges_host(drfe_lmap* db, drfe_lmap_essential_edges_call* call) { return edges_entry(db, call, 0, nullptr); }
int drfe_lmap_essential_edges_device(drfe_lmap* db, drfe_lmap_essential_edges_call* call, void* stream) { return edges_entry(db, call, 1, stream); }
int drfe_lmap_essential_edges_batch(drfe_lmap* db, drfe_lmap_essential_edges_call* call, void* stream) { return edges_entry(db, call, 2, stream); }
int drfe_lmap_essential_commit_host(drfe_lmap* db, drfe_lmap_essential_commit_call* call) { return commit_entry(db, call, 0, nullptr); }
int drfe_lmap_essential_commit_device(drfe_lmap* db, drfe_lmap_essential_commit_call* call, void* stream) { return commit_entry(db, call, 1, stream); }
int drfe_lmap_essential_commit_batch(drfe_lmap* db, drfe_lmap_essential_commit_call* call, void* stream) { return commit_entry(db, call, 2, stream); }

int drfe_lmap_essential_limits(int32_t* out8)
{
    if (!out8) return DRFE_ERR_INVALID;
    out8[0] = ESS_TILE;
    out8[1] = ESS_WAVE;
    out8[2] = DRFE_LMAP_ESSENTIAL_EDGES_DEVICE_FROM;
    out8[3] = DRFE_LMAP_ESSENTIAL_COMMIT_DEVICE_FROM;
    out8[4] = ESS_POINT_BYTES;
    out8[5] = ESS_KF_BYTES;
    out8[6] = ESS_EDGE_BYTES;
    out8[7] = ESS_VERTEX_BYTES;
    return DRFE_OK;
}

int drfe_lmap_essential_scratch(drfe_lmap* db, int32_t lc_entries, int64_t* out6)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!out6 || lc_entries < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_essential_scratch: invalid argument");
    const int rc = build_ess(db);
    if (rc) return rc;
    const Image& G = db->img;
    int64_t bound = lc_entries;
    for (size_t s = 0; s < G.kfHandle.size(); s++)
        if (!G.kfBad[s]) bound += (G.kfParent[s] >= 0) + (db->ess.leOff[s + 1] - db->ess.leOff[s]) + (G.coOff[s + 1] - G.coOff[s]);
    out6[0] = edges_scratch(db, bound, &out6[1]);
    const CommitFit F = commit_fit(db);
    out6[2] = F.whole;
    out6[3] = F.least;
    out6[4] = F.fixed;
    out6[5] = bound;
    return DRFE_OK;
}

int drfe_lmap_essential_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::essStats, stats); }

}  // extern "C"
