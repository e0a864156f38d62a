/* lmap.cpp — Tracking::UpdateLocalMap (reference src/Tracking.cc:3383-3541) behind the C-ABI of include/drfe.h: the store of the
 * graph the three functions read, its flat image, the argument checks, the host walk, the device entry (lmap_kernels.hip) and the
 * counters.  Both sides read the same image and evaluate lmap_core.h.  A call is checked as a whole and committed only when its
 * results fit the caller's arrays.  DESIGN.md section 25.  On the same store: KeyFrame::UpdateConnections (section 26) here, and
 * the Sim3 propagation of LoopClosing::CorrectLoop with the geometry it reads in lmap_correct.cpp (section 27); lmap_store.h is
 * the store they share. */
#include "lmap_store.h"
#include "stage_layout.h"

static_assert(CONN_TH == DRFE_LMAP_CONNECT_TH, "the vote threshold of conn_core.h is the header's");

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

int fail(drfe_lmap* db, int rc, const std::string& why)
{
    db->err = why;
    return rc;
}

bool offsets_ok(const int32_t* off, int n)
{
    if (!off || off[0] != 0) return false;
    for (int k = 0; k < n; k++)
        if (off[k + 1] < off[k]) return false;
    return true;
}

bool handles_ok(const int32_t* h, int n)
{
    for (int i = 0; i < n; i++)
        if (h[i] < -1) return false;
    return true;
}

/* the flat image of the rows; DRFE_ERR_STATE and the name of the reference when one dangles */
int build_image(drfe_lmap* db)
{
    if (!db->imgDirty) return DRFE_OK;
    Image G;
    std::vector<std::pair<uint64_t, int32_t>> order;
    order.reserve(db->kf.size());
    for (const auto& e : db->kf) order.emplace_back(e.second.rank, e.first);
    std::sort(order.begin(), order.end());
    for (const auto& e : order) {
        G.kfSlot[e.second] = (int32_t)G.kfHandle.size();
        G.kfHandle.push_back(e.second);
    }
    for (const auto& e : db->mp) G.mpHandle.push_back(e.first);
    std::sort(G.mpHandle.begin(), G.mpHandle.end());
    for (size_t s = 0; s < G.mpHandle.size(); s++) G.mpSlot[G.mpHandle[s]] = (int32_t)s;
    for (const auto& e : db->ml) G.mlHandle.push_back(e.first);
    std::sort(G.mlHandle.begin(), G.mlHandle.end());
    for (size_t s = 0; s < G.mlHandle.size(); s++) G.mlSlot[G.mlHandle[s]] = (int32_t)s;
    const size_t nK = G.kfHandle.size(), nP = G.mpHandle.size(), nL = G.mlHandle.size();
    auto dangling = [&](const char* what, int32_t of, const char* kind, int32_t h) {
        return fail(db, DRFE_ERR_STATE, std::string("lmap: ") + what + " of " + kind + " " + std::to_string(of) + " names unknown handle " + std::to_string(h));
    };
    G.kfBad.resize(nK);
    G.kfParent.assign(nK, -1);
    G.kfNbr.assign(nK * LMAP_NEIGHBOURS, -1);
    G.childOff.assign(1, 0);
    G.kfMpOff.assign(1, 0);
    G.kfMlOff.assign(1, 0);
    std::vector<int32_t> ch;
    for (size_t s = 0; s < nK; s++) {
        const int32_t h = G.kfHandle[s];
        const KfRow& K = db->kf.at(h);
        G.kfBad[s] = K.bad;
        if (K.parent >= 0) {
            const auto it = G.kfSlot.find(K.parent);
            if (it == G.kfSlot.end()) return dangling("the parent", h, "key frame", K.parent);
            G.kfParent[s] = it->second;
        }
        for (int k = 0; k < LMAP_NEIGHBOURS; k++)
            if (K.nbr[k] >= 0) {
                const auto it = G.kfSlot.find(K.nbr[k]);
                if (it == G.kfSlot.end()) return dangling("a neighbour", h, "key frame", K.nbr[k]);
                G.kfNbr[s * LMAP_NEIGHBOURS + k] = it->second;
            }
        ch.clear();
        for (const int32_t c : K.children) {
            const auto it = G.kfSlot.find(c);
            if (it == G.kfSlot.end()) return dangling("a child", h, "key frame", c);
            ch.push_back(it->second);
        }
        std::sort(ch.begin(), ch.end());   /* ascending slot = rank order: set<KeyFrame*> */
        G.child.insert(G.child.end(), ch.begin(), ch.end());
        G.childOff.push_back((int32_t)G.child.size());
        for (const int32_t p : K.mps) {
            int32_t sl = -1;
            if (p >= 0) {
                const auto it = G.mpSlot.find(p);
                if (it == G.mpSlot.end()) return dangling("a map-point match", h, "key frame", p);
                sl = it->second;
            }
            G.kfMp.push_back(sl);
        }
        G.kfMpOff.push_back((int32_t)G.kfMp.size());
        for (const int32_t l : K.mls) {
            int32_t sl = -1;
            if (l >= 0) {
                const auto it = G.mlSlot.find(l);
                if (it == G.mlSlot.end()) return dangling("a map-line match", h, "key frame", l);
                sl = it->second;
            }
            G.kfMl.push_back(sl);
        }
        G.kfMlOff.push_back((int32_t)G.kfMl.size());
        G.maxRow[0] = std::max(G.maxRow[0], (int32_t)K.mps.size());
        G.maxRow[1] = std::max(G.maxRow[1], (int32_t)K.mls.size());
    }
    G.kfFirst.assign(nK, 0);
    G.cwOff.assign(1, 0);
    G.coOff.assign(1, 0);
    std::vector<std::pair<int32_t, int32_t>> wrow;
    for (size_t s = 0; s < nK; s++) {
        const int32_t h = G.kfHandle[s];
        const auto cr = db->conn.find(h);
        if (cr != db->conn.end()) {
            const ConnRow& R = cr->second;
            G.kfFirst[s] = R.first;
            wrow.clear();
            for (size_t i = 0; i < R.wKf.size(); i++) {
                const auto it = G.kfSlot.find(R.wKf[i]);
                if (it == G.kfSlot.end()) return dangling("a connection weight", h, "key frame", R.wKf[i]);
                wrow.emplace_back(it->second, R.wW[i]);
            }
            std::sort(wrow.begin(), wrow.end());
            for (const auto& e : wrow) {
                G.cwKf.push_back(e.first);
                G.cwW.push_back(e.second);
            }
            for (size_t i = 0; i < R.oKf.size(); i++) {
                const auto it = G.kfSlot.find(R.oKf[i]);
                if (it == G.kfSlot.end()) return dangling("an ordered connection", h, "key frame", R.oKf[i]);
                G.coKf.push_back(it->second);
                G.coW.push_back(R.oW[i]);
            }
        }
        G.cwOff.push_back((int32_t)G.cwKf.size());
        G.coOff.push_back((int32_t)G.coKf.size());
    }
    G.mpBad.resize(nP);
    G.obsOff.assign(1, 0);
    for (size_t s = 0; s < nP; s++) {
        const MpRow& P = db->mp.at(G.mpHandle[s]);
        G.mpBad[s] = P.bad;
        for (const int32_t o : P.obs) {
            const auto it = G.kfSlot.find(o);
            if (it == G.kfSlot.end()) return dangling("an observation", G.mpHandle[s], "map point", o);
            G.obs.push_back(it->second);
        }
        G.obsOff.push_back((int32_t)G.obs.size());
    }
    G.mlBad.resize(nL);
    for (size_t s = 0; s < nL; s++) G.mlBad[s] = db->ml.at(G.mlHandle[s]);
    db->img = std::move(G);
    db->imgDirty = false;
    db->devDirty = true;
    db->geoDirty = true;               /* the slots may have moved */
    db->cullDirty = true;
    db->gbaDirty = true;
    return DRFE_OK;
}

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
        if (it == map.end()) return fail(db, DRFE_ERR_INVALID, std::string("lmap: a query names an unknown ") + what + " handle");
        out[(size_t)i] = it->second;
    }
    return DRFE_OK;
}

int plan(drfe_lmap* db, const drfe_lmap_queries* q, const drfe_lmap_out* o, Call& C)
{
    if (!q || q->n < 0 || !o) return fail(db, DRFE_ERR_INVALID, "lmap: invalid argument");
    if (q->n > DRFE_LMAP_MAX_QUERIES) return fail(db, DRFE_ERR_INVALID, "lmap: more than DRFE_LMAP_MAX_QUERIES queries in a call");
    if (o->kf_capacity < 0 || o->mp_capacity < 0 || o->ml_capacity < 0 || o->nulled_capacity < 0 || !o->kf_offsets || !o->ref_kf ||
        !o->mp_offsets || !o->ml_offsets || !o->nulled_offsets || !o->record || (o->kf_capacity > 0 && !o->kfs) ||
        (o->mp_capacity > 0 && (!o->mps || !o->mp_in_frame)) || (o->ml_capacity > 0 && (!o->mls || !o->ml_in_frame)) ||
        (o->nulled_capacity > 0 && !o->nulled))
        return fail(db, DRFE_ERR_INVALID, "lmap: invalid output arrays");
    const int n = q->n;
    C.n = n;
    if (n == 0) return DRFE_OK;
    if (!q->frame_id) return fail(db, DRFE_ERR_INVALID, "lmap: invalid argument");
    int64_t last = db->lastId;
    for (int k = 0; k < n; k++) {
        if (q->frame_id[k] == 0 || q->frame_id[k] <= last)
            return fail(db, DRFE_ERR_INVALID, "lmap: a frame id is 0 or does not exceed the last id used on this store");
        last = q->frame_id[k];
    }
    C.lastId = last;
    if (!offsets_ok(q->point_offsets, n) || (q->point_offsets[n] > 0 && !q->points))
        return fail(db, DRFE_ERR_INVALID, "lmap: point_offsets do not start at 0 or decrease");
    if (q->line_offsets && (!offsets_ok(q->line_offsets, n) || (q->line_offsets[n] > 0 && !q->lines)))
        return fail(db, DRFE_ERR_INVALID, "lmap: line_offsets do not start at 0 or decrease");
    if (q->prev_kf_offsets && (!offsets_ok(q->prev_kf_offsets, n) || (q->prev_kf_offsets[n] > 0 && !q->prev_kfs)))
        return fail(db, DRFE_ERR_INVALID, "lmap: prev_kf_offsets do not start at 0 or decrease");
    int rc = build_image(db);
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
    const LmapImage I = db->img.view();
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

/* The image on the device is two blocks.  The rows block - the bad flags in front, then match rows and observations - goes up
 * whole after an edit of the rows, or its bad flags alone after drfe_lmap_set_bad.  The graph block - parents, neighbours,
 * children and the connection rows, what a connect call commits - goes up with it, or alone after such a commit. */
int upload_image(drfe_lmap* db, hipStream_t st)
{
    const Image& G = db->img;
    if (!db->devDirty && !db->devBadDirty && !db->devGraphDirty && !db->devObsDirty && db->devNulls.empty()) return DRFE_OK;
    const bool all = db->devDirty, graph = all || db->devGraphDirty;
    StageLayout<16> up, gr;
    const auto uKfBad = up.add<uint8_t>(G.kfBad.size());
    const auto uMpBad = up.add<uint8_t>(G.mpBad.size());
    const auto uMlBad = up.add<uint8_t>(G.mlBad.size());
    const size_t badBytes = up.bytes();
    const auto uKfMpOff = up.add<int32_t>(G.kfMpOff.size());
    const auto uKfMp = up.add<int32_t>(G.kfMp.size());
    const auto uKfMlOff = up.add<int32_t>(G.kfMlOff.size());
    const auto uKfMl = up.add<int32_t>(G.kfMl.size());
    const auto uObsOff = up.add<int32_t>(G.obsOff.size());
    const auto uObs = up.add<int32_t>(G.obs.size());
    const auto uParent = gr.add<int32_t>(G.kfParent.size());
    const auto uNbr = gr.add<int32_t>(G.kfNbr.size());
    const auto uChildOff = gr.add<int32_t>(G.childOff.size());
    const auto uChild = gr.add<int32_t>(G.child.size());
    const auto uFirst = gr.add<uint8_t>(G.kfFirst.size());
    const auto uCwOff = gr.add<int32_t>(G.cwOff.size());
    const auto uCwKf = gr.add<int32_t>(G.cwKf.size());
    const auto uCwW = gr.add<int32_t>(G.cwW.size());
    const auto uCoOff = gr.add<int32_t>(G.coOff.size());
    const auto uCoKf = gr.add<int32_t>(G.coKf.size());
    const auto uCoW = gr.add<int32_t>(G.coW.size());
    const size_t bytes = all ? up.bytes() : (db->devBadDirty ? badBytes : 0);
    if (bytes) {
        HIPCHK_TO(db->err, db->hup.grow(db->hup.capacity() >= bytes ? bytes : 2 * bytes));
        char* h = db->hup;
        uKfBad.put(h, G.kfBad.data());
        uMpBad.put(h, G.mpBad.data());
        uMlBad.put(h, G.mlBad.data());
        if (all) {
            uKfMpOff.put(h, G.kfMpOff.data());
            uKfMp.put(h, G.kfMp.data());
            uKfMlOff.put(h, G.kfMlOff.data());
            uKfMl.put(h, G.kfMl.data());
            uObsOff.put(h, G.obsOff.data());
            uObs.put(h, G.obs.data());
            /* an image that no longer fits is allocated at twice the size */
            HIPCHK_TO(db->err, db->dImg.grow(db->dImg.capacity() >= bytes ? bytes : 2 * bytes));
        }
        HIPCHK_TO(db->err, hipMemcpyAsync(db->dImg, h, bytes, hipMemcpyHostToDevice, st));
        db->sentBytes[0] += (int64_t)bytes;
    }
    if (!all) {
        /* what a cull call committed, piece by piece: the nulled match-row entries, and the observations with their offsets,
         * which are the end of the block (a shortened row moves the rows behind it, never the sections in front) */
        static const int32_t kNull = -1;
        char* d = db->dImg;
        for (const int32_t e : db->devNulls)
            HIPCHK_TO(db->err, hipMemcpyAsync(uKfMp.at(d) + e, &kNull, sizeof(kNull), hipMemcpyHostToDevice, st));
        db->sentBytes[0] += (int64_t)(sizeof(kNull) * db->devNulls.size());
        if (db->devObsDirty) {
            const size_t total = up.bytes(), tail = total - uObsOff.off;
            HIPCHK_TO(db->err, db->hup.grow(db->hup.capacity() >= total ? total : 2 * total));
            char* h = db->hup;
            uObsOff.put(h, G.obsOff.data());
            uObs.put(h, G.obs.data());
            HIPCHK_TO(db->err, hipMemcpyAsync(d + uObsOff.off, h + uObsOff.off, tail, hipMemcpyHostToDevice, st));
            db->sentBytes[0] += (int64_t)tail;
        }
    }
    db->devNulls.clear();
    db->devObsDirty = false;
    if (graph) {
        const size_t gb = gr.bytes();
        HIPCHK_TO(db->err, db->hgraph.grow(db->hgraph.capacity() >= gb ? gb : 2 * gb));
        char* h = db->hgraph;
        uParent.put(h, G.kfParent.data());
        uNbr.put(h, G.kfNbr.data());
        uChildOff.put(h, G.childOff.data());
        uChild.put(h, G.child.data());
        uFirst.put(h, G.kfFirst.data());
        uCwOff.put(h, G.cwOff.data());
        uCwKf.put(h, G.cwKf.data());
        uCwW.put(h, G.cwW.data());
        uCoOff.put(h, G.coOff.data());
        uCoKf.put(h, G.coKf.data());
        uCoW.put(h, G.coW.data());
        HIPCHK_TO(db->err, db->dGraph.grow(db->dGraph.capacity() >= gb ? gb : 2 * gb));
        if (gb) HIPCHK_TO(db->err, hipMemcpyAsync(db->dGraph, h, gb, hipMemcpyHostToDevice, st));
        db->sentBytes[1] += (int64_t)gb;
    }
    if (graph) {
        /* either block may have moved or changed its layout */
        const char* d = db->dImg;
        const char* g = db->dGraph;
        LmapImage& V = db->dView;
        V = G.view();
        V.kfBad = uKfBad.at(d);
        V.mpBad = uMpBad.at(d);
        V.mlBad = uMlBad.at(d);
        V.kfMpOff = uKfMpOff.at(d);
        V.kfMp = uKfMp.at(d);
        V.kfMlOff = uKfMlOff.at(d);
        V.kfMl = uKfMl.at(d);
        V.obsOff = uObsOff.at(d);
        V.obs = uObs.at(d);
        V.kfParent = uParent.at(g);
        V.kfNbr = uNbr.at(g);
        V.childOff = uChildOff.at(g);
        V.child = uChild.at(g);
        ConnImage& W = db->dConn;
        W.first = uFirst.at(g);
        W.wOff = uCwOff.at(g);
        W.wKf = uCwKf.at(g);
        W.wW = uCwW.at(g);
        W.oOff = uCoOff.at(g);
        W.oKf = uCoKf.at(g);
        W.oW = uCoW.at(g);
    }
    /* the staging blocks are written again by the next upload */
    HIPCHK_TO(db->err, hipStreamSynchronize(st));
    db->devDirty = db->devBadDirty = db->devGraphDirty = false;
    db->stats[3]++;
    return DRFE_OK;
}

/* queries [k0, k1) of the call: one staging block up, the launches, the offsets and records back, then exactly the lists */
int run_chunk(drfe_lmap* db, const Call& C, int k0, int k1, int32_t rowK, Result& R, hipStream_t st)
{
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
    HIPCHK_TO(db->err, db->io.grow(in.bytes(), out.bytes()));
    HIPCHK_TO(db->err, db->scratch.grow(scr.bytes()));
    char* h = db->io.hin;
    for (size_t k = 0; k <= nQ; k++) {
        sPtOff.at(h)[k] = C.ptOff[(size_t)k0 + k] - pt0;
        sLnOff.at(h)[k] = C.lnOff[(size_t)k0 + k] - ln0;
        sPrevOff.at(h)[k] = C.prevOff[(size_t)k0 + k] - pv0;
    }
    sPts.put(h, C.pts.data() + pt0);
    sLns.put(h, C.lns.data() + ln0);
    sPrev.put(h, C.prev.data() + pv0);
    const char* d = db->io.din;
    char* dO = db->io.dout;
    char* dS = db->scratch;
    HIPCHK_TO(db->err, hipMemcpyAsync(db->io.din, h, in.bytes(), hipMemcpyHostToDevice, st));
    if (zeroEnd) HIPCHK_TO(db->err, hipMemsetAsync(dS, 0, zeroEnd, st));
    if (claimEnd > zeroEnd) HIPCHK_TO(db->err, hipMemsetAsync(dS + zeroEnd, LMAP_NO_CLAIM & 0xff, claimEnd - zeroEnd, st));
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
    hipError_t e = drfe_launch_lmap(L, st);
    if (e == hipSuccess) e = hipMemcpyAsync(db->io.hout, dO, out.bytes(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(db, DRFE_ERR_HIP, std::string("lmap device call: ") + hipGetErrorString(e));
    const char* ho = db->io.hout;
    const LmapQueryRec* rec = oRec.at(ho);
    const int32_t* off = oOff.at(ho);
    const size_t tKf = (size_t)off[nQ], tMp = (size_t)off[2 * nQ + 1], tMl = (size_t)off[3 * nQ + 2], tNu = (size_t)off[4 * nQ + 3];
    StageLayout<16> li;
    const auto lKf = li.add<int32_t>(tKf);
    const auto lMp = li.add<int32_t>(tMp);
    const auto lMl = li.add<int32_t>(tMl);
    const auto lNu = li.add<int32_t>(tNu);
    const auto lMpIn = li.add<uint8_t>(tMp);
    const auto lMlIn = li.add<uint8_t>(tMl);
    HIPCHK_TO(db->err, db->hlist.grow(li.bytes()));
    char* hl = db->hlist;
    if (tKf) HIPCHK_TO(db->err, hipMemcpyAsync(lKf.at(hl), xKf.at(dS), lKf.bytes(), hipMemcpyDeviceToHost, st));
    if (tMp) HIPCHK_TO(db->err, hipMemcpyAsync(lMp.at(hl), xMp.at(dS), lMp.bytes(), hipMemcpyDeviceToHost, st));
    if (tMl) HIPCHK_TO(db->err, hipMemcpyAsync(lMl.at(hl), xMl.at(dS), lMl.bytes(), hipMemcpyDeviceToHost, st));
    if (tNu) HIPCHK_TO(db->err, hipMemcpyAsync(lNu.at(hl), xNulled.at(dS), lNu.bytes(), hipMemcpyDeviceToHost, st));
    if (tMp) HIPCHK_TO(db->err, hipMemcpyAsync(lMpIn.at(hl), xMpIn.at(dS), lMpIn.bytes(), hipMemcpyDeviceToHost, st));
    if (tMl) HIPCHK_TO(db->err, hipMemcpyAsync(lMlIn.at(hl), xMlIn.at(dS), lMlIn.bytes(), hipMemcpyDeviceToHost, st));
    HIPCHK_TO(db->err, hipStreamSynchronize(st));
    const int32_t bKf = R.kfOff.back(), bMp = R.mpOff.back(), bMl = R.mlOff.back(), bNu = R.nuOff.back();
    for (size_t k = 0; k < nQ; k++) {
        R.kfOff.push_back(bKf + off[k + 1]);
        R.mpOff.push_back(bMp + off[(nQ + 1) + k + 1]);
        R.mlOff.push_back(bMl + off[2 * (nQ + 1) + k + 1]);
        R.nuOff.push_back(bNu + off[3 * (nQ + 1) + k + 1]);
        R.ref.push_back(rec[k].refKf);
        for (int f = 0; f < 4; f++) R.record.push_back(rec[k].rec[f]);
    }
    R.kfs.insert(R.kfs.end(), lKf.at(hl), lKf.at(hl) + tKf);
    R.mps.insert(R.mps.end(), lMp.at(hl), lMp.at(hl) + tMp);
    R.mls.insert(R.mls.end(), lMl.at(hl), lMl.at(hl) + tMl);
    R.nulled.insert(R.nulled.end(), lNu.at(hl), lNu.at(hl) + tNu);
    R.mpIn.insert(R.mpIn.end(), lMpIn.at(hl), lMpIn.at(hl) + tMp);
    R.mlIn.insert(R.mlIn.end(), lMlIn.at(hl), lMlIn.at(hl) + tMl);
    return DRFE_OK;
}

int run_device(drfe_lmap* db, const Call& C, Result& R, void* stream)
{
    drfe_ctx* c = db->ctx;
    HIPCHK_TO(db->err, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    int rc = upload_image(db, st);
    if (rc) return rc;
    const int32_t rowK = row_k(db, C);
    const int64_t perQuery = query_scratch(db, C, rowK);
    const int chunk = (int)std::min<int64_t>(C.n, std::max<int64_t>(1, db->scratchBytes / perQuery));
    R.start();
    for (int k0 = 0; k0 < C.n; k0 += chunk) {
        rc = run_chunk(db, C, k0, std::min(C.n, k0 + chunk), rowK, R, st);
        if (rc) return rc;
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
    if (tKf > o->kf_capacity) return fail(db, DRFE_ERR_CAPACITY, "lmap: more local key frames than kf_capacity");
    if (tMp > o->mp_capacity) return fail(db, DRFE_ERR_CAPACITY, "lmap: more local points than mp_capacity");
    if (tMl > o->ml_capacity) return fail(db, DRFE_ERR_CAPACITY, "lmap: more local lines than ml_capacity");
    if (tNu > o->nulled_capacity) return fail(db, DRFE_ERR_CAPACITY, "lmap: more nulled points than nulled_capacity");
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
    if (mode == 1 && !db->ctx) return fail(db, DRFE_ERR_STATE, "lmap: a device call on a store without a context");
    Call C;
    int rc = plan(db, q, o, C);
    if (rc) return rc;
    bool dev = mode == 1;
    if (mode == 2) dev = db->ctx && C.n >= DRFE_LMAP_DEVICE_FROM && device_fits(db, C);
    if (C.n == 0) dev = false;
    if (dev && !device_fits(db, C))
        return fail(db, DRFE_ERR_CAPACITY, "lmap: one query does not fit the configured device scratch (or its walk ranks an int32)");
    Result R;
    if (dev) {
        rc = run_device(db, C, R, stream);
        if (rc) return rc;
    } else if (C.n > 0) {
        run_host(db, C, R);
    }
    return finish(db, C, R, o, dev);
}

template <class Map>
int set_bad(drfe_lmap* db, Map& rows, const std::unordered_map<int32_t, int32_t>& slot, std::vector<uint8_t>& bad, int32_t count,
            const int32_t* handles, const uint8_t* flags, uint8_t& (*field)(typename Map::mapped_type&))
{
    for (int i = 0; i < count; i++)
        if (rows.find(handles[i]) == rows.end()) return fail(db, DRFE_ERR_INVALID, "lmap_set_bad: unknown handle");
    for (int i = 0; i < count; i++) {
        field(rows.at(handles[i])) = flags[i] ? 1 : 0;
        if (!db->imgDirty) bad[(size_t)slot.at(handles[i])] = flags[i] ? 1 : 0;
    }
    if (count) db->devBadDirty = true;
    return DRFE_OK;
}

uint8_t& kf_bad(KfRow& r) { return r.bad; }
uint8_t& mp_bad(MpRow& r) { return r.bad; }
uint8_t& ml_bad(uint8_t& r) { return r; }

/* ---- KeyFrame::UpdateConnections ---- */

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
    if (n < 0 || (n > 0 && !handles) || !o) return fail(db, DRFE_ERR_INVALID, "lmap_connect: invalid argument");
    if (n > DRFE_LMAP_MAX_QUERIES) return fail(db, DRFE_ERR_INVALID, "lmap_connect: more than DRFE_LMAP_MAX_QUERIES key frames in a call");
    if (o->counter_capacity < 0 || o->touched_capacity < 0 || !o->counter_offsets || !o->record || !o->new_parent || !o->n_touched ||
        (o->counter_capacity > 0 && (!o->counter_kfs || !o->counter_votes)) || (o->touched_capacity > 0 && (!o->touched || !o->flags)) ||
        !conn_rows_ok(o->rows))
        return fail(db, DRFE_ERR_INVALID, "lmap_connect: invalid output arrays");
    if (n == 0) return DRFE_OK;
    int rc = build_image(db);
    if (rc) return rc;
    const Image& G = db->img;
    called.resize((size_t)n);
    pos.assign(G.kfHandle.size(), -1);
    for (int p = 0; p < n; p++) {
        const auto it = G.kfSlot.find(handles[p]);
        if (it == G.kfSlot.end()) return fail(db, DRFE_ERR_INVALID, "lmap_connect: the call names an unknown key-frame handle");
        if (pos[(size_t)it->second] >= 0) return fail(db, DRFE_ERR_INVALID, "lmap_connect: the call names a key frame twice");
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
    const LmapImage I = G.view();
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
    drfe_ctx* c = db->ctx;
    HIPCHK_TO(db->err, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    int rc = upload_image(db, st);
    if (rc) return rc;
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
    HIPCHK_TO(db->err, db->io.grow(in.bytes(), out.bytes()));
    HIPCHK_TO(db->err, db->scratch.grow(scr.bytes()));
    char* h = db->io.hin;
    sCalled.put(h, called.data());
    sPos.put(h, pos.data());
    sCapOff.put(h, F.capOff.data());
    const char* d = db->io.din;
    char* dO = db->io.dout;
    char* dS = db->scratch;
    HIPCHK_TO(db->err, hipMemcpyAsync(db->io.din, h, in.bytes(), hipMemcpyHostToDevice, st));
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
    hipError_t e = drfe_launch_conn(L, st);
    if (e == hipSuccess) e = hipMemcpyAsync(db->io.hout, dO, out.bytes(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(db, DRFE_ERR_HIP, std::string("lmap connect device call: ") + hipGetErrorString(e));
    const char* ho = db->io.hout;
    const ConnRec* rec = oRec.at(ho);
    const int32_t* head = oHead.at(ho);
    const size_t nT = (size_t)head[CONN_HEAD_TOUCHED], tW = (size_t)head[CONN_HEAD_WEIGHTS], tO = (size_t)head[CONN_HEAD_ORDERED],
                 tC = (size_t)head[CONN_HEAD_COUNTER];
    if (nT > nK || tW > rows || tO > rows || tC > cap) return fail(db, DRFE_ERR_STATE, "lmap connect device call: totals past their bounds");
    StageLayout<16> li;
    const auto lCntKf = li.add<int32_t>(tC);
    const auto lCntW = li.add<int32_t>(tC);
    const auto lWKf = li.add<int32_t>(tW);
    const auto lWW = li.add<int32_t>(tW);
    const auto lOKf = li.add<int32_t>(tO);
    const auto lOW = li.add<int32_t>(tO);
    HIPCHK_TO(db->err, db->hlist.grow(li.bytes()));
    char* hl = db->hlist;
    if (tC) HIPCHK_TO(db->err, hipMemcpyAsync(lCntKf.at(hl), xPkCntKf.at(dS), lCntKf.bytes(), hipMemcpyDeviceToHost, st));
    if (tC) HIPCHK_TO(db->err, hipMemcpyAsync(lCntW.at(hl), xPkCntW.at(dS), lCntW.bytes(), hipMemcpyDeviceToHost, st));
    if (tW) HIPCHK_TO(db->err, hipMemcpyAsync(lWKf.at(hl), xPkWKf.at(dS), lWKf.bytes(), hipMemcpyDeviceToHost, st));
    if (tW) HIPCHK_TO(db->err, hipMemcpyAsync(lWW.at(hl), xPkWW.at(dS), lWW.bytes(), hipMemcpyDeviceToHost, st));
    if (tO) HIPCHK_TO(db->err, hipMemcpyAsync(lOKf.at(hl), xPkOKf.at(dS), lOKf.bytes(), hipMemcpyDeviceToHost, st));
    if (tO) HIPCHK_TO(db->err, hipMemcpyAsync(lOW.at(hl), xPkOW.at(dS), lOW.bytes(), hipMemcpyDeviceToHost, st));
    HIPCHK_TO(db->err, hipStreamSynchronize(st));
    R.cntOff.assign(oCntOff.at(ho), oCntOff.at(ho) + n + 1);
    R.cntKf.assign(lCntKf.at(hl), lCntKf.at(hl) + tC);
    R.cntW.assign(lCntW.at(hl), lCntW.at(hl) + tC);
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
    R.wKf.assign(lWKf.at(hl), lWKf.at(hl) + tW);
    R.wW.assign(lWW.at(hl), lWW.at(hl) + tW);
    R.oKf.assign(lOKf.at(hl), lOKf.at(hl) + tO);
    R.oW.assign(lOW.at(hl), lOW.at(hl) + tO);
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
    db->devGraphDirty = true;
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
    if (tC > o->counter_capacity) return fail(db, DRFE_ERR_CAPACITY, "lmap_connect: more counter entries than counter_capacity");
    if ((int64_t)nT > o->touched_capacity) return fail(db, DRFE_ERR_CAPACITY, "lmap_connect: more touched key frames than touched_capacity");
    if (tW > o->rows.weights_capacity) return fail(db, DRFE_ERR_CAPACITY, "lmap_connect: more weights than weights_capacity");
    if (tO > o->rows.ordered_capacity) return fail(db, DRFE_ERR_CAPACITY, "lmap_connect: more list entries than ordered_capacity");
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
    if (mode == 1 && !db->ctx) return fail(db, DRFE_ERR_STATE, "lmap_connect: a device call on a store without a context");
    std::vector<int32_t> called, pos;
    int rc = conn_plan(db, n, handles, o, called, pos);
    if (rc) return rc;
    bool dev = mode == 1 || (mode == 2 && db->ctx && n >= DRFE_LMAP_CONNECT_DEVICE_FROM);
    if (n == 0) dev = false;
    ConnFit F;
    if (dev) {
        F = conn_fit(db, called);
        if (!F.fits && mode == 1)
            return fail(db, DRFE_ERR_CAPACITY, "lmap_connect: the call's counters and rows do not fit the configured device scratch");
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

/* what lmap_correct.cpp shares (lmap_store.h) */
int lmap_fail(drfe_lmap* db, int rc, const std::string& why) { return fail(db, rc, why); }
int lmap_build_image(drfe_lmap* db) { return build_image(db); }
int lmap_upload_image(drfe_lmap* db, hipStream_t st) { return upload_image(db, st); }

extern "C" {

int drfe_lmap_create(drfe_ctx* ctx, drfe_lmap** out)
{
    if (!out) return DRFE_ERR_INVALID;
    drfe_lmap* db = new drfe_lmap();
    db->ctx = ctx;
    if (ctx) db->device = ctx->device;
    db->dView = LmapImage{};
    db->dConn = ConnImage{};
    db->dCorr = CorrImage{};
    db->dCull = CullImage{};
    *out = db;
    return DRFE_OK;
}

void drfe_lmap_destroy(drfe_lmap* db)
{
    if (!db) return;
    if (db->ctx) (void)hipSetDevice(db->device);
    delete db;
}

const char* drfe_lmap_last_error(const drfe_lmap* db) { return db ? db->err.c_str() : "lmap: no store"; }

int drfe_lmap_configure(drfe_lmap* db, int64_t scratch_bytes)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (scratch_bytes <= 0) return fail(db, DRFE_ERR_INVALID, "lmap_configure: scratch_bytes must be positive");
    db->scratchBytes = scratch_bytes;
    return DRFE_OK;
}

int drfe_lmap_limits(int32_t* out4)
{
    if (!out4) return DRFE_ERR_INVALID;
    out4[0] = LMAP_LDS_KFS;
    out4[1] = LMAP_THREADS;
    out4[2] = LMAP_GATHER_ENTRIES;
    out4[3] = DRFE_LMAP_DEVICE_FROM;
    return DRFE_OK;
}

int drfe_lmap_set_keyframes(drfe_lmap* db, const drfe_lmap_keyframes* r)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!r || r->count < 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: invalid argument");
    const int n = r->count;
    if (n == 0) return DRFE_OK;
    if (!r->handle || !r->rank || !r->bad || !r->parent || !r->neighbours || !offsets_ok(r->child_offsets, n) ||
        !offsets_ok(r->point_offsets, n) || !offsets_ok(r->line_offsets, n) || (r->child_offsets[n] > 0 && !r->children) ||
        (r->point_offsets[n] > 0 && !r->points) || (r->line_offsets[n] > 0 && !r->lines))
        return fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: invalid argument");
    if (!handles_ok(r->parent, n) || !handles_ok(r->neighbours, n * LMAP_NEIGHBOURS) || !handles_ok(r->points, r->point_offsets[n]) ||
        !handles_ok(r->lines, r->line_offsets[n]))
        return fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: a handle below -1");
    /* the last row of a handle wins; ranks stay distinct within the store */
    std::unordered_map<int32_t, int> lastRow;
    for (int i = 0; i < n; i++) {
        if (r->handle[i] < 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: a negative handle");
        lastRow[r->handle[i]] = i;
    }
    std::unordered_map<uint64_t, int32_t> ranks;
    std::vector<int32_t> ch;
    for (const auto& e : lastRow) {
        const int i = e.second;
        const auto own = db->rankOwner.find(r->rank[i]);
        if ((own != db->rankOwner.end() && lastRow.find(own->second) == lastRow.end()) || !ranks.emplace(r->rank[i], e.first).second)
            return fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: two key frames of the store would have the same rank");
        ch.assign(r->children + r->child_offsets[i], r->children + r->child_offsets[i + 1]);
        std::sort(ch.begin(), ch.end());
        if ((!ch.empty() && ch[0] < 0) || std::adjacent_find(ch.begin(), ch.end()) != ch.end())
            return fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: a child is negative or named twice");
    }
    for (const auto& e : lastRow) {
        const auto old = db->kf.find(e.first);
        if (old != db->kf.end()) db->rankOwner.erase(old->second.rank);
    }
    for (const auto& e : lastRow) {
        const int i = e.second;
        KfRow& K = db->kf[e.first];
        K.rank = r->rank[i];
        K.bad = r->bad[i] ? 1 : 0;
        K.parent = r->parent[i];
        std::memcpy(K.nbr, r->neighbours + (size_t)i * LMAP_NEIGHBOURS, sizeof(K.nbr));
        K.children.assign(r->children + r->child_offsets[i], r->children + r->child_offsets[i + 1]);
        K.mps.assign(r->points + r->point_offsets[i], r->points + r->point_offsets[i + 1]);
        K.mls.assign(r->lines + r->line_offsets[i], r->lines + r->line_offsets[i + 1]);
        db->rankOwner[K.rank] = e.first;
    }
    db->imgDirty = true;
    return DRFE_OK;
}

int drfe_lmap_set_points(drfe_lmap* db, int32_t count, const int32_t* handles, const uint8_t* bad, const int32_t* obs_offsets, const int32_t* obs)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_points: invalid argument");
    if (count == 0) return DRFE_OK;
    if (!handles || !bad || !offsets_ok(obs_offsets, count) || (obs_offsets[count] > 0 && !obs))
        return fail(db, DRFE_ERR_INVALID, "lmap_set_points: invalid argument");
    std::vector<int32_t> row;
    for (int i = 0; i < count; i++) {
        if (handles[i] < 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_points: a negative handle");
        row.assign(obs + obs_offsets[i], obs + obs_offsets[i + 1]);
        std::sort(row.begin(), row.end());
        if (!row.empty() && row[0] < 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_points: a negative observation");
        if (std::adjacent_find(row.begin(), row.end()) != row.end())
            return fail(db, DRFE_ERR_INVALID, "lmap_set_points: a key frame observes a point twice");
    }
    for (int i = 0; i < count; i++) {
        MpRow& P = db->mp[handles[i]];
        P.bad = bad[i] ? 1 : 0;
        P.obs.assign(obs + obs_offsets[i], obs + obs_offsets[i + 1]);
    }
    db->imgDirty = true;
    return DRFE_OK;
}

int drfe_lmap_set_lines(drfe_lmap* db, int32_t count, const int32_t* handles, const uint8_t* bad)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !bad))) return fail(db, DRFE_ERR_INVALID, "lmap_set_lines: invalid argument");
    for (int i = 0; i < count; i++)
        if (handles[i] < 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_lines: a negative handle");
    for (int i = 0; i < count; i++) db->ml[handles[i]] = bad[i] ? 1 : 0;
    if (count) db->imgDirty = true;
    return DRFE_OK;
}

int drfe_lmap_set_bad(drfe_lmap* db, int kind, int32_t count, const int32_t* handles, const uint8_t* flags)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !flags))) return fail(db, DRFE_ERR_INVALID, "lmap_set_bad: invalid argument");
    Image& G = db->img;
    if (kind == DRFE_LMAP_KEYFRAME) return set_bad(db, db->kf, G.kfSlot, G.kfBad, count, handles, flags, kf_bad);
    if (kind == DRFE_LMAP_POINT) return set_bad(db, db->mp, G.mpSlot, G.mpBad, count, handles, flags, mp_bad);
    if (kind == DRFE_LMAP_LINE) return set_bad(db, db->ml, G.mlSlot, G.mlBad, count, handles, flags, ml_bad);
    return fail(db, DRFE_ERR_INVALID, "lmap_set_bad: unknown kind");
}

int drfe_lmap_remove(drfe_lmap* db, int kind, int32_t handle)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    size_t gone = 0;
    if (kind == DRFE_LMAP_KEYFRAME) {
        const auto it = db->kf.find(handle);
        if (it != db->kf.end()) {
            db->rankOwner.erase(it->second.rank);
            db->kf.erase(it);
            db->conn.erase(handle);
            db->kfPose.erase(handle);
            db->kfCull.erase(handle);
            db->kfGba.erase(handle);
            gone = 1;
        }
    } else if (kind == DRFE_LMAP_POINT) {
        gone = db->mp.erase(handle);
        if (gone) {
            db->mpGeo.erase(handle);
            db->mpCull.erase(handle);
            db->mpGba.erase(handle);
        }
    } else if (kind == DRFE_LMAP_LINE) {
        gone = db->ml.erase(handle);
    } else {
        return fail(db, DRFE_ERR_INVALID, "lmap_remove: unknown kind");
    }
    if (!gone) return fail(db, DRFE_ERR_INVALID, "lmap_remove: unknown handle");
    db->imgDirty = true;
    return DRFE_OK;
}

int drfe_lmap_size(drfe_lmap* db, int32_t* out3)
{
    if (!db || !out3) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    out3[0] = (int32_t)db->kf.size();
    out3[1] = (int32_t)db->mp.size();
    out3[2] = (int32_t)db->ml.size();
    return DRFE_OK;
}

int drfe_lmap_update_host(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* o) { return entry(db, q, o, 0, nullptr); }
int drfe_lmap_update_device(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* o, void* stream) { return entry(db, q, o, 1, stream); }
int drfe_lmap_update_batch(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* o, void* stream) { return entry(db, q, o, 2, stream); }

int drfe_lmap_stats(drfe_lmap* db, int64_t* stats)
{
    if (!db || !stats) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    std::memcpy(stats, db->stats, sizeof(db->stats));
    return DRFE_OK;
}

int drfe_lmap_set_connections(drfe_lmap* db, const drfe_lmap_connections* r)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!r || r->count < 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_connections: invalid argument");
    const int n = r->count;
    if (n == 0) return DRFE_OK;
    if (!r->handle || !r->first_connection || !offsets_ok(r->weight_offsets, n) || !offsets_ok(r->ordered_offsets, n) ||
        (r->weight_offsets[n] > 0 && (!r->weight_kfs || !r->weight_w)) || (r->ordered_offsets[n] > 0 && (!r->ordered_kfs || !r->ordered_w)))
        return fail(db, DRFE_ERR_INVALID, "lmap_set_connections: invalid argument");
    std::vector<int32_t> row;
    for (int i = 0; i < n; i++) {
        if (r->handle[i] < 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_connections: a negative handle");
        for (int side = 0; side < 2; side++) {
            const int32_t* off = side ? r->ordered_offsets : r->weight_offsets;
            const int32_t* kfs = side ? r->ordered_kfs : r->weight_kfs;
            const int32_t* w = side ? r->ordered_w : r->weight_w;
            row.assign(kfs + off[i], kfs + off[i + 1]);
            std::sort(row.begin(), row.end());
            if ((!row.empty() && row[0] < 0) || std::adjacent_find(row.begin(), row.end()) != row.end())
                return fail(db, DRFE_ERR_INVALID, "lmap_set_connections: a key frame is negative or named twice in a row");
            for (int32_t k = off[i]; k < off[i + 1]; k++)
                if (w[k] <= 0) return fail(db, DRFE_ERR_INVALID, "lmap_set_connections: a weight that is not positive");
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
        return fail(db, DRFE_ERR_INVALID, "lmap_get_connections: invalid argument");
    const int rc = build_image(db);
    if (rc) return rc;
    const Image& G = db->img;
    std::vector<int32_t> slots;
    int64_t tW = 0, tO = 0, tCh = 0;
    for (int i = 0; i < count; i++) {
        const auto it = G.kfSlot.find(handles[i]);
        if (it == G.kfSlot.end()) return fail(db, DRFE_ERR_INVALID, "lmap_get_connections: unknown handle");
        const size_t s = (size_t)it->second;
        slots.push_back(it->second);
        tW += G.cwOff[s + 1] - G.cwOff[s];
        tO += G.coOff[s + 1] - G.coOff[s];
        tCh += G.childOff[s + 1] - G.childOff[s];
    }
    if (tW > o->weights_capacity || tO > o->ordered_capacity || (children_offsets && tCh > children_capacity))
        return fail(db, DRFE_ERR_CAPACITY, "lmap_get_connections: an output array is too small");
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

int drfe_lmap_upload_bytes(drfe_lmap* db, int64_t* out5)
{
    if (!db || !out5) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    std::memcpy(out5, db->sentBytes, sizeof(db->sentBytes));
    return DRFE_OK;
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

int drfe_lmap_connect_stats(drfe_lmap* db, int64_t* stats)
{
    if (!db || !stats) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    std::memcpy(stats, db->connStats, sizeof(db->connStats));
    return DRFE_OK;
}
}  // extern "C"
