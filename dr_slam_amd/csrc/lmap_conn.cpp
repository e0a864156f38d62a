/* lmap_conn.cpp — KeyFrame::UpdateConnections (reference src/KeyFrame.cc:366-500) on the local-map store (lmap_store.h), behind
 * the C-ABI of include/drfe.h: the setter and getter of the connection rows, the checks, the host walk, the device entry
 * (conn_kernels.hip), the commit into rows and image and the counters.  Both sides evaluate conn_core.h.  DESIGN.md section 26. */
#include "lmap_call.h"

static_assert(CONN_TH == DRFE_LMAP_CONNECT_TH, "the vote threshold of conn_core.h is the header's");

#include <algorithm>
#include <cstring>
#include <map>

using namespace lmap_store;

namespace {

/* what a call leaves, in slots: per called key frame and per touched one (ascending slot) */
struct ConnResult {
    std::vector<int32_t> cntOff, cntKf, cntW, record, newParent;
    std::vector<int32_t> touched, wOff, wKf, wW, oOff, oKf, oW, parent;
    std::vector<uint8_t> first;
};

bool conn_rows_ok(const drfe_lmap_conn_rows& r)
{
    return r.weights_capacity >= 0 && r.ordered_capacity >= 0 && r.weight_offsets && r.ordered_offsets && r.parent && r.first_connection &&
           (r.weights_capacity == 0 || (r.weight_kfs && r.weight_w)) && (r.ordered_capacity == 0 || (r.ordered_kfs && r.ordered_w));
}

int conn_plan(drfe_lmap* db, int32_t n, const int32_t* handles, const drfe_lmap_connect_out* o, std::vector<int32_t>& called,
              std::vector<int32_t>& pos)
{
    if (n < 0 || (n > 0 && !handles) || !o) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_connect: invalid argument");
    if (n > DRFE_LMAP_MAX_QUERIES) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_connect: more than DRFE_LMAP_MAX_QUERIES key frames in a call");
    if (o->counter_capacity < 0 || o->touched_capacity < 0 || !o->counter_offsets || !o->record || !o->new_parent || !o->n_touched ||
        (o->counter_capacity > 0 && (!o->counter_kfs || !o->counter_votes)) || (o->touched_capacity > 0 && (!o->touched || !o->flags)) ||
        !conn_rows_ok(o->rows))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_connect: invalid output arrays");
    if (n == 0) return DRFE_OK;
    int rc = lmap_build_image(db);
    if (rc) return rc;
    const Image& G = db->img;
    called.resize((size_t)n);
    pos.assign(G.kfHandle.size(), -1);
    for (int p = 0; p < n; p++) {
        const auto it = G.kfSlot.find(handles[p]);
        if (it == G.kfSlot.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_connect: the call names an unknown key-frame handle");
        if (pos[(size_t)it->second] >= 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_connect: the call names a key frame twice");
        pos[(size_t)it->second] = p;
        called[(size_t)p] = it->second;
    }
    return DRFE_OK;
}

/* the reference's calls, one after another, on working copies of the touched key frames' rows */
void conn_host(drfe_lmap* db, const std::vector<int32_t>& called, ConnResult& R)
{
    typedef std::pair<int32_t, int32_t> Entry;   /* (slot, weight) */
    struct Work {
        std::vector<Entry> w, ord;
        int32_t parent = -1;
        uint8_t first = 0;
    };
    const Image& G = db->img;
    lmap_host_views(db);
    const LmapImage I = db->hView;
    const int n = (int)called.size();
    std::map<int32_t, Work> T;                   /* by slot: references stay valid */
    auto touch = [&](int32_t s) -> Work& {
        const auto it = T.find(s);
        if (it != T.end()) return it->second;
        Work& W = T[s];
        for (int32_t i = G.cwOff[(size_t)s]; i < G.cwOff[(size_t)s + 1]; i++) W.w.emplace_back(G.cwKf[(size_t)i], G.cwW[(size_t)i]);
        for (int32_t i = G.coOff[(size_t)s]; i < G.coOff[(size_t)s + 1]; i++) W.ord.emplace_back(G.coKf[(size_t)i], G.coW[(size_t)i]);
        W.parent = G.kfParent[(size_t)s];
        W.first = G.kfFirst[(size_t)s];
        return W;
    };
    auto by_key = [](const Entry& a, const Entry& b) { return conn_key(a.second, a.first) > conn_key(b.second, b.first); };
    std::vector<int32_t> votes((size_t)I.nK);
    std::vector<Entry> counter, listed;
    R.cntOff.assign(1, 0);
    R.record.assign((size_t)n * 4, 0);
    R.newParent.assign((size_t)n, -1);
    for (int p = 0; p < n; p++) {
        const int32_t k = called[(size_t)p];
        Work& Wk = touch(k);
        std::fill(votes.begin(), votes.end(), 0);
        for (int32_t i = I.kfMpOff[k]; i < I.kfMpOff[k + 1]; i++) {
            const int32_t pt = I.kfMp[i];
            if (!conn_point_votes(pt, I.mpBad)) continue;
            for (int32_t o = I.obsOff[pt]; o < I.obsOff[pt + 1]; o++)
                if (conn_obs_votes(I.obs[o], k)) votes[(size_t)I.obs[o]]++;
        }
        counter.clear();
        listed.clear();
        int32_t nmax = 0, best = 0x7fffffff;
        for (int32_t s = 0; s < I.nK; s++) {
            const int32_t v = votes[(size_t)s];
            if (v <= 0) continue;
            counter.emplace_back(s, v);
            if (conn_better(v, s, nmax, best)) {
                nmax = v;
                best = s;
            }
            if (conn_listed(v)) listed.emplace_back(s, v);
        }
        for (const Entry& e : counter) {
            R.cntKf.push_back(e.first);
            R.cntW.push_back(e.second);
        }
        R.cntOff.push_back((int32_t)R.cntKf.size());
        int32_t* rec = &R.record[4 * (size_t)p];
        rec[0] = (int32_t)counter.size();
        rec[3] = -1;
        if (counter.empty()) continue;           /* the early return (:403) */
        if (listed.empty()) listed.emplace_back(best, nmax);
        rec[1] = (int32_t)listed.size();
        rec[2] = nmax;
        rec[3] = best;
        for (const Entry& e : listed) {          /* AddConnection (:200-213) */
            Work& Wj = touch(e.first);
            const auto at = std::lower_bound(Wj.w.begin(), Wj.w.end(), Entry(k, 0));
            const bool present = at != Wj.w.end() && at->first == k;
            if (!conn_changes(present, present ? at->second : 0, e.second)) continue;
            if (present)
                at->second = e.second;
            else
                Wj.w.insert(at, Entry(k, e.second));
            Wj.ord = Wj.w;                       /* UpdateBestCovisibles (:215-234): every entry */
            std::sort(Wj.ord.begin(), Wj.ord.end(), by_key);
        }
        Wk.w = counter;
        std::sort(listed.begin(), listed.end(), by_key);
        Wk.ord = listed;
        if (Wk.first) {
            Wk.parent = Wk.ord.front().first;
            Wk.first = 0;
            R.newParent[(size_t)p] = Wk.parent;
        }
    }
    R.wOff.assign(1, 0);
    R.oOff.assign(1, 0);
    for (const auto& t : T) {
        const Work& W = t.second;
        R.touched.push_back(t.first);
        for (const Entry& e : W.w) {
            R.wKf.push_back(e.first);
            R.wW.push_back(e.second);
        }
        for (const Entry& e : W.ord) {
            R.oKf.push_back(e.first);
            R.oW.push_back(e.second);
        }
        R.wOff.push_back((int32_t)R.wKf.size());
        R.oOff.push_back((int32_t)R.oKf.size());
        R.parent.push_back(W.parent);
        R.first.push_back(W.first);
    }
}

/* how the device call divides its scratch; fits = the whole call's counters, the packed rows and one vote row are within budget */
struct ConnFit {
    std::vector<int32_t> capOff;       /* n + 1 */
    int64_t rowBound = 0;              /* entries of all final weights rows, and of all final lists */
    int64_t perVote = 0, fixed = 0;
    int chunk = 0;
    bool fits = false;
};

ConnFit conn_fit(const drfe_lmap* db, const std::vector<int32_t>& called)
{
    const Image& G = db->img;
    const int64_t nK = (int64_t)G.kfHandle.size();
    const size_t n = called.size();
    ConnFit F;
    F.capOff.assign(n + 1, 0);
    int64_t cap = 0;
    for (size_t p = 0; p < n; p++) {
        const int32_t k = called[p];
        int64_t entries = 0;
        for (int32_t i = G.kfMpOff[(size_t)k]; i < G.kfMpOff[(size_t)k + 1] && entries < nK; i++) {
            const int32_t pt = G.kfMp[(size_t)i];
            if (conn_point_votes(pt, G.mpBad.data())) entries += G.obsOff[(size_t)pt + 1] - G.obsOff[(size_t)pt];
        }
        cap += std::min<int64_t>(entries, nK - 1);
        if (cap > 0x7fffffff) return F;
        F.capOff[p + 1] = (int32_t)cap;
    }
    /* a final weights row is a stored row or a counter, and one entry per edge at most; a final list is no longer than the
     * stored list or the final weights */
    F.rowBound = (int64_t)G.cwKf.size() + (int64_t)G.coKf.size() + 2 * cap;
    const bool global = nK > LMAP_LDS_KFS;
    F.perVote = global ? 4 * nK : 0;
    F.fixed = cap * (4 + 4 + 8 + 1 + 8) + 16 * F.rowBound + 32 * nK + (global ? 4 * nK * std::min<int64_t>(nK, CONN_ROW_GROUPS) : 0) + 1024;
    if (F.rowBound > 0x7fffffff || F.fixed + F.perVote > db->scratchBytes) return F;
    F.chunk = F.perVote ? (int)std::min<int64_t>((int64_t)n, (db->scratchBytes - F.fixed) / F.perVote) : (int)n;
    F.fits = true;
    return F;
}

int conn_device(drfe_lmap* db, const std::vector<int32_t>& called, const std::vector<int32_t>& pos, const ConnFit& F, ConnResult& R,
                void* stream)
{
    LmapCall call{db, "lmap connect"};
    if (const int rc = call.begin(LMAP_NEED_IMAGE, stream)) return rc;
    const Image& G = db->img;
    const size_t n = called.size(), nK = G.kfHandle.size(), cap = (size_t)F.capOff[n], rows = (size_t)F.rowBound;
    const bool global = nK > LMAP_LDS_KFS;
    StageLayout<16> in, out, scr;
    const auto sCalled = in.add<int32_t>(n);
    const auto sPos = in.add<int32_t>(nK);
    const auto sCapOff = in.add<int32_t>(n + 1);
    const auto oRec = out.add<ConnRec>(n);
    const auto oNewParent = out.add<int32_t>(n);
    const auto oCntOff = out.add<int32_t>(n + 1);
    const auto oHead = out.add<int32_t>(CONN_HEAD_WORDS);
    const auto oTouched = out.add<int32_t>(nK);
    const auto oWOff = out.add<int32_t>(nK + 1);
    const auto oOOff = out.add<int32_t>(nK + 1);
    const auto oParent = out.add<int32_t>(nK);
    const auto oFirst = out.add<uint8_t>(nK);
    const auto xHist = scr.add<int32_t>(global ? (size_t)F.chunk * nK : 0);
    const auto xDense = scr.add<int32_t>(global ? std::min<size_t>(nK, CONN_ROW_GROUPS) * nK : 0);
    const auto xCntKf = scr.add<int32_t>(cap);
    const auto xCntW = scr.add<int32_t>(cap);
    const auto xLst = scr.add<uint64_t>(cap);
    const auto xChg = scr.add<uint8_t>(cap);
    const auto xMark = scr.add<uint8_t>(nK);
    const auto xMode = scr.add<int32_t>(nK);
    const auto xPkCntKf = scr.add<int32_t>(cap);
    const auto xPkCntW = scr.add<int32_t>(cap);
    const auto xPkWKf = scr.add<int32_t>(rows);
    const auto xPkWW = scr.add<int32_t>(rows);
    const auto xPkOKf = scr.add<int32_t>(rows);
    const auto xPkOW = scr.add<int32_t>(rows);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, ho] = call.at;
    sCalled.put(h, called.data());
    sPos.put(h, pos.data());
    sCapOff.put(h, F.capOff.data());
    if (const int rc = call.send()) return rc;
    ConnLaunch L{};
    L.I = db->dView;
    L.G = db->dConn;
    L.n = (int32_t)n;
    L.chunk = F.chunk;
    L.called = sCalled.at(d);
    L.pos = sPos.at(d);
    L.capOff = sCapOff.at(d);
    L.hist = xHist.at(dS);
    L.dense = xDense.at(dS);
    L.cntKf = xCntKf.at(dS);
    L.cntW = xCntW.at(dS);
    L.lst = xLst.at(dS);
    L.chg = xChg.at(dS);
    L.mark = xMark.at(dS);
    L.tMode = xMode.at(dS);
    L.rec = oRec.at(dO);
    L.newParent = oNewParent.at(dO);
    L.cntOff = oCntOff.at(dO);
    L.head = oHead.at(dO);
    L.touched = oTouched.at(dO);
    L.wOff = oWOff.at(dO);
    L.oOff = oOOff.at(dO);
    L.tParent = oParent.at(dO);
    L.tFirst = oFirst.at(dO);
    L.pkCntKf = xPkCntKf.at(dS);
    L.pkCntW = xPkCntW.at(dS);
    L.pkWKf = xPkWKf.at(dS);
    L.pkWW = xPkWW.at(dS);
    L.pkOKf = xPkOKf.at(dS);
    L.pkOW = xPkOW.at(dS);
    if (const int rc = call.back(drfe_launch_conn(L, call.st))) return rc;
    const ConnRec* rec = oRec.at(ho);
    const int32_t* head = oHead.at(ho);
    const size_t nT = (size_t)head[CONN_HEAD_TOUCHED], tW = (size_t)head[CONN_HEAD_WEIGHTS], tO = (size_t)head[CONN_HEAD_ORDERED],
                 tC = (size_t)head[CONN_HEAD_COUNTER];
    if (nT > nK || tW > rows || tO > rows || tC > cap) return lmap_fail(db, DRFE_ERR_STATE, "lmap connect device call: totals past their bounds");
    LmapFetch f;
    const auto lCntKf = f.add(xPkCntKf.at(dS), tC);
    const auto lCntW = f.add(xPkCntW.at(dS), tC);
    const auto lWKf = f.add(xPkWKf.at(dS), tW);
    const auto lWW = f.add(xPkWW.at(dS), tW);
    const auto lOKf = f.add(xPkOKf.at(dS), tO);
    const auto lOW = f.add(xPkOW.at(dS), tO);
    if (const int rc = call.fetch(f)) return rc;
    R.cntOff.assign(oCntOff.at(ho), oCntOff.at(ho) + n + 1);
    R.cntKf.assign(f.at(lCntKf), f.at(lCntKf) + tC);
    R.cntW.assign(f.at(lCntW), f.at(lCntW) + tC);
    R.record.resize(4 * n);
    for (size_t p = 0; p < n; p++) {
        R.record[4 * p + 0] = rec[p].nC;
        R.record[4 * p + 1] = rec[p].nL;
        R.record[4 * p + 2] = rec[p].nC > 0 ? rec[p].nmax : 0;
        R.record[4 * p + 3] = rec[p].nC > 0 ? rec[p].best : -1;
    }
    R.newParent.assign(oNewParent.at(ho), oNewParent.at(ho) + n);
    R.touched.assign(oTouched.at(ho), oTouched.at(ho) + nT);
    R.wOff.assign(oWOff.at(ho), oWOff.at(ho) + nT + 1);
    R.oOff.assign(oOOff.at(ho), oOOff.at(ho) + nT + 1);
    R.parent.assign(oParent.at(ho), oParent.at(ho) + nT);
    R.first.assign(oFirst.at(ho), oFirst.at(ho) + nT);
    R.wKf.assign(f.at(lWKf), f.at(lWKf) + tW);
    R.wW.assign(f.at(lWW), f.at(lWW) + tW);
    R.oKf.assign(f.at(lOKf), f.at(lOKf) + tO);
    R.oW.assign(f.at(lOW), f.at(lOW) + tO);
    return DRFE_OK;
}

/* The commit into the image, in place: the call read the image, so it is current, and the results are in its slots.  Parents,
 * first_connection, the neighbours of a changed list, the connection rows and the new parents' children; the match rows and
 * observations stay, so only the graph block goes to the device again. */
void conn_patch_image(drfe_lmap* db, const std::vector<int32_t>& called, const ConnResult& R)
{
    Image& G = db->img;
    const size_t nK = G.kfHandle.size(), nT = R.touched.size();
    std::vector<int32_t> wOff(1, 0), wKf, wW, oOff(1, 0), oKf, oW;
    wKf.reserve(G.cwKf.size() + R.wKf.size());
    oKf.reserve(G.coKf.size() + R.oKf.size());
    size_t t = 0;
    for (size_t s = 0; s < nK; s++) {
        if (t < nT && (size_t)R.touched[t] == s) {
            const int32_t o0 = R.oOff[t], o1 = R.oOff[t + 1], q0 = G.coOff[s], q1 = G.coOff[s + 1];
            const bool oSame = o1 - o0 == q1 - q0 && std::equal(R.oKf.begin() + o0, R.oKf.begin() + o1, G.coKf.begin() + q0) &&
                               std::equal(R.oW.begin() + o0, R.oW.begin() + o1, G.coW.begin() + q0);
            if (!oSame)
                for (int k = 0; k < LMAP_NEIGHBOURS; k++) G.kfNbr[s * LMAP_NEIGHBOURS + (size_t)k] = k < o1 - o0 ? R.oKf[(size_t)(o0 + k)] : -1;
            G.kfParent[s] = R.parent[t];
            G.kfFirst[s] = R.first[t];
            wKf.insert(wKf.end(), R.wKf.begin() + R.wOff[t], R.wKf.begin() + R.wOff[t + 1]);
            wW.insert(wW.end(), R.wW.begin() + R.wOff[t], R.wW.begin() + R.wOff[t + 1]);
            oKf.insert(oKf.end(), R.oKf.begin() + o0, R.oKf.begin() + o1);
            oW.insert(oW.end(), R.oW.begin() + o0, R.oW.begin() + o1);
            t++;
        } else {
            wKf.insert(wKf.end(), G.cwKf.begin() + G.cwOff[s], G.cwKf.begin() + G.cwOff[s + 1]);
            wW.insert(wW.end(), G.cwW.begin() + G.cwOff[s], G.cwW.begin() + G.cwOff[s + 1]);
            oKf.insert(oKf.end(), G.coKf.begin() + G.coOff[s], G.coKf.begin() + G.coOff[s + 1]);
            oW.insert(oW.end(), G.coW.begin() + G.coOff[s], G.coW.begin() + G.coOff[s + 1]);
        }
        wOff.push_back((int32_t)wKf.size());
        oOff.push_back((int32_t)oKf.size());
    }
    G.cwOff.swap(wOff);
    G.cwKf.swap(wKf);
    G.cwW.swap(wW);
    G.coOff.swap(oOff);
    G.coKf.swap(oKf);
    G.coW.swap(oW);
    std::vector<std::pair<int32_t, int32_t>> gained;   /* (parent, child) */
    for (size_t p = 0; p < called.size(); p++) {
        const int32_t pa = R.newParent[p];
        if (pa < 0) continue;
        const auto b = G.child.begin() + G.childOff[(size_t)pa], e = G.child.begin() + G.childOff[(size_t)pa + 1];
        if (!std::binary_search(b, e, called[p])) gained.emplace_back(pa, called[p]);
    }
    if (!gained.empty()) {
        std::sort(gained.begin(), gained.end());
        std::vector<int32_t> cOff(1, 0), ch;
        size_t g = 0;
        for (size_t s = 0; s < nK; s++) {
            const size_t at = ch.size();
            ch.insert(ch.end(), G.child.begin() + G.childOff[s], G.child.begin() + G.childOff[s + 1]);
            for (; g < gained.size() && (size_t)gained[g].first == s; g++) ch.push_back(gained[g].second);
            std::sort(ch.begin() + (std::ptrdiff_t)at, ch.end());
            cOff.push_back((int32_t)ch.size());
        }
        G.childOff.swap(cOff);
        G.child.swap(ch);
    }
    db->blk[drfe_lmap::GRAPH].stale_all();
}

/* results into the caller's arrays and the touched rows into the store, or neither */
int conn_finish(drfe_lmap* db, const std::vector<int32_t>& called, const ConnResult& R, drfe_lmap_connect_out* o, bool onDevice)
{
    const size_t n = called.size();
    o->counter_offsets[0] = 0;
    o->rows.weight_offsets[0] = o->rows.ordered_offsets[0] = 0;
    *o->n_touched = 0;
    if (n == 0) return DRFE_OK;
    const Image& G = db->img;
    const size_t nT = R.touched.size();
    const int32_t tC = R.cntOff[n], tW = R.wOff[nT], tO = R.oOff[nT];
    if (tC > o->counter_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_connect: more counter entries than counter_capacity");
    if ((int64_t)nT > o->touched_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_connect: more touched key frames than touched_capacity");
    if (tW > o->rows.weights_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_connect: more weights than weights_capacity");
    if (tO > o->rows.ordered_capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_connect: more list entries than ordered_capacity");
    auto handle = [&](int32_t s) { return s >= 0 ? G.kfHandle[(size_t)s] : -1; };
    int64_t listed = 0, firsts = 0, empties = 0;
    for (size_t p = 0; p < n; p++) {
        o->counter_offsets[p + 1] = R.cntOff[p + 1];
        o->record[4 * p + 0] = R.record[4 * p + 0];
        o->record[4 * p + 1] = R.record[4 * p + 1];
        o->record[4 * p + 2] = R.record[4 * p + 2];
        o->record[4 * p + 3] = handle(R.record[4 * p + 3]);
        o->new_parent[p] = handle(R.newParent[p]);
        listed += R.record[4 * p + 1];
        firsts += R.newParent[p] >= 0;
        empties += R.record[4 * p + 0] == 0;
    }
    for (int32_t i = 0; i < tC; i++) {
        o->counter_kfs[i] = handle(R.cntKf[(size_t)i]);
        o->counter_votes[i] = R.cntW[(size_t)i];
    }
    *o->n_touched = (int32_t)nT;
    for (int32_t i = 0; i < tW; i++) {
        o->rows.weight_kfs[i] = handle(R.wKf[(size_t)i]);
        o->rows.weight_w[i] = R.wW[(size_t)i];
    }
    for (int32_t i = 0; i < tO; i++) {
        o->rows.ordered_kfs[i] = handle(R.oKf[(size_t)i]);
        o->rows.ordered_w[i] = R.oW[(size_t)i];
    }
    /* the commit, against the image the call read */
    for (size_t t = 0; t < nT; t++) {
        const int32_t s = R.touched[t], h = handle(s);
        const int32_t w0 = R.wOff[t], w1 = R.wOff[t + 1], o0 = R.oOff[t], o1 = R.oOff[t + 1];
        const int32_t g0 = G.cwOff[(size_t)s], g1 = G.cwOff[(size_t)s + 1], q0 = G.coOff[(size_t)s], q1 = G.coOff[(size_t)s + 1];
        const bool wSame = w1 - w0 == g1 - g0 && std::equal(R.wKf.begin() + w0, R.wKf.begin() + w1, G.cwKf.begin() + g0) &&
                           std::equal(R.wW.begin() + w0, R.wW.begin() + w1, G.cwW.begin() + g0);
        const bool oSame = o1 - o0 == q1 - q0 && std::equal(R.oKf.begin() + o0, R.oKf.begin() + o1, G.coKf.begin() + q0) &&
                           std::equal(R.oW.begin() + o0, R.oW.begin() + o1, G.coW.begin() + q0);
        const bool pSame = R.parent[t] == G.kfParent[(size_t)s];
        o->touched[t] = h;
        o->rows.weight_offsets[t + 1] = w1;
        o->rows.ordered_offsets[t + 1] = o1;
        o->rows.parent[t] = handle(R.parent[t]);
        o->rows.first_connection[t] = R.first[t];
        o->flags[t] = (uint8_t)((wSame ? 0 : 1) | (oSame ? 0 : 2) | (pSame ? 0 : 4));
        KfRow& K = db->kf.at(h);
        ConnRow& C = db->conn[h];
        C.first = R.first[t];
        if (!wSame) {
            C.wKf.assign(o->rows.weight_kfs + w0, o->rows.weight_kfs + w1);
            C.wW.assign(o->rows.weight_w + w0, o->rows.weight_w + w1);
        }
        if (!oSame) {
            C.oKf.assign(o->rows.ordered_kfs + o0, o->rows.ordered_kfs + o1);
            C.oW.assign(o->rows.ordered_w + o0, o->rows.ordered_w + o1);
            for (int k = 0; k < LMAP_NEIGHBOURS; k++) K.nbr[k] = k < o1 - o0 ? o->rows.ordered_kfs[o0 + k] : -1;
        }
        K.parent = handle(R.parent[t]);
    }
    for (size_t p = 0; p < n; p++) {
        if (R.newParent[p] < 0) continue;
        std::vector<int32_t>& ch = db->kf.at(handle(R.newParent[p])).children;
        const int32_t k = handle(called[p]);
        if (std::find(ch.begin(), ch.end(), k) == ch.end()) ch.push_back(k);
    }
    conn_patch_image(db, called, R);
    int64_t* st = db->connStats;
    st[0]++;
    st[1] += (int64_t)n;
    if (onDevice) st[2]++;
    st[3] += tC;
    st[4] += listed;
    st[5] += (int64_t)nT;
    st[6] += firsts;
    st[7] += empties;
    return DRFE_OK;
}

/* mode: 0 host, 1 device, 2 by the crossover */
int conn_entry(drfe_lmap* db, int32_t n, const int32_t* handles, drfe_lmap_connect_out* o, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_connect: a device call on a store without a context");
    std::vector<int32_t> called, pos;
    int rc = conn_plan(db, n, handles, o, called, pos);
    if (rc) return rc;
    bool dev = mode == 1 || (mode == 2 && db->ctx && n >= DRFE_LMAP_CONNECT_DEVICE_FROM);
    if (n == 0) dev = false;
    ConnFit F;
    if (dev) {
        F = conn_fit(db, called);
        if (!F.fits && mode == 1)
            return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_connect: the call's counters and rows do not fit the configured device scratch");
        dev = F.fits;
    }
    ConnResult R;
    if (dev) {
        rc = conn_device(db, called, pos, F, R, stream);
        if (rc) return rc;
    } else if (n > 0) {
        conn_host(db, called, R);
    }
    return conn_finish(db, called, R, o, dev);
}

}  // namespace

extern "C" {

int drfe_lmap_set_connections(drfe_lmap* db, const drfe_lmap_connections* r)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!r || r->count < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_connections: invalid argument");
    const int n = r->count;
    if (n == 0) return DRFE_OK;
    if (!r->handle || !r->first_connection || !lmap_offsets_ok(r->weight_offsets, n) || !lmap_offsets_ok(r->ordered_offsets, n) ||
        (r->weight_offsets[n] > 0 && (!r->weight_kfs || !r->weight_w)) || (r->ordered_offsets[n] > 0 && (!r->ordered_kfs || !r->ordered_w)))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_connections: invalid argument");
    std::vector<int32_t> row;
    for (int i = 0; i < n; i++) {
        if (r->handle[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_connections: a negative handle");
        for (int side = 0; side < 2; side++) {
            const int32_t* off = side ? r->ordered_offsets : r->weight_offsets;
            const int32_t* kfs = side ? r->ordered_kfs : r->weight_kfs;
            const int32_t* w = side ? r->ordered_w : r->weight_w;
            row.assign(kfs + off[i], kfs + off[i + 1]);
            std::sort(row.begin(), row.end());
            if ((!row.empty() && row[0] < 0) || std::adjacent_find(row.begin(), row.end()) != row.end())
                return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_connections: a key frame is negative or named twice in a row");
            for (int32_t k = off[i]; k < off[i + 1]; k++)
                if (w[k] <= 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_connections: a weight that is not positive");
        }
    }
    for (int i = 0; i < n; i++) {
        ConnRow& C = db->conn[r->handle[i]];
        C.first = r->first_connection[i] ? 1 : 0;
        C.wKf.assign(r->weight_kfs + r->weight_offsets[i], r->weight_kfs + r->weight_offsets[i + 1]);
        C.wW.assign(r->weight_w + r->weight_offsets[i], r->weight_w + r->weight_offsets[i + 1]);
        C.oKf.assign(r->ordered_kfs + r->ordered_offsets[i], r->ordered_kfs + r->ordered_offsets[i + 1]);
        C.oW.assign(r->ordered_w + r->ordered_offsets[i], r->ordered_w + r->ordered_offsets[i + 1]);
    }
    db->imgDirty = true;
    return DRFE_OK;
}

int drfe_lmap_get_connections(drfe_lmap* db, int32_t count, const int32_t* handles, drfe_lmap_conn_rows* o, int32_t children_capacity,
                              int32_t* children_offsets, int32_t* children)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && !handles) || !o || !conn_rows_ok(*o) || children_capacity < 0 ||
        (children_offsets && children_capacity > 0 && !children))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_connections: invalid argument");
    const int rc = lmap_build_image(db);
    if (rc) return rc;
    const Image& G = db->img;
    std::vector<int32_t> slots;
    int64_t tW = 0, tO = 0, tCh = 0;
    for (int i = 0; i < count; i++) {
        const auto it = G.kfSlot.find(handles[i]);
        if (it == G.kfSlot.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_connections: unknown handle");
        const size_t s = (size_t)it->second;
        slots.push_back(it->second);
        tW += G.cwOff[s + 1] - G.cwOff[s];
        tO += G.coOff[s + 1] - G.coOff[s];
        tCh += G.childOff[s + 1] - G.childOff[s];
    }
    if (tW > o->weights_capacity || tO > o->ordered_capacity || (children_offsets && tCh > children_capacity))
        return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_get_connections: an output array is too small");
    int32_t aW = 0, aO = 0, aCh = 0;
    o->weight_offsets[0] = o->ordered_offsets[0] = 0;
    if (children_offsets) children_offsets[0] = 0;
    for (int i = 0; i < count; i++) {
        const size_t s = (size_t)slots[(size_t)i];
        for (int32_t k = G.cwOff[s]; k < G.cwOff[s + 1]; k++, aW++) {
            o->weight_kfs[aW] = G.kfHandle[(size_t)G.cwKf[(size_t)k]];
            o->weight_w[aW] = G.cwW[(size_t)k];
        }
        for (int32_t k = G.coOff[s]; k < G.coOff[s + 1]; k++, aO++) {
            o->ordered_kfs[aO] = G.kfHandle[(size_t)G.coKf[(size_t)k]];
            o->ordered_w[aO] = G.coW[(size_t)k];
        }
        o->weight_offsets[i + 1] = aW;
        o->ordered_offsets[i + 1] = aO;
        o->parent[i] = G.kfParent[s] >= 0 ? G.kfHandle[(size_t)G.kfParent[s]] : -1;
        o->first_connection[i] = G.kfFirst[s];
        if (children_offsets) {
            for (int32_t k = G.childOff[s]; k < G.childOff[s + 1]; k++) children[aCh++] = G.kfHandle[(size_t)G.child[(size_t)k]];
            children_offsets[i + 1] = aCh;
        }
    }
    return DRFE_OK;
}

int drfe_lmap_connect_host(drfe_lmap* db, int32_t n, const int32_t* handles, drfe_lmap_connect_out* o)
{
    return conn_entry(db, n, handles, o, 0, nullptr);
}
int drfe_lmap_connect_device(drfe_lmap* db, int32_t n, const int32_t* handles, drfe_lmap_connect_out* o, void* stream)
{
    return conn_entry(db, n, handles, o, 1, stream);
}
int drfe_lmap_connect_batch(drfe_lmap* db, int32_t n, const int32_t* handles, drfe_lmap_connect_out* o, void* stream)
{
    return conn_entry(db, n, handles, o, 2, stream);
}

int drfe_lmap_connect_limits(int32_t* out4)
{
    if (!out4) return DRFE_ERR_INVALID;
    out4[0] = DRFE_LMAP_CONNECT_TH;
    out4[1] = DRFE_LMAP_CONNECT_DEVICE_FROM;
    out4[2] = CONN_SORT_TILE;
    out4[3] = CONN_ROW_GROUPS;
    return DRFE_OK;
}

int drfe_lmap_connect_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::connStats, stats); }
}  // extern "C"
