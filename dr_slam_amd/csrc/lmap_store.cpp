/* lmap_store.cpp — the local-map store behind the C-ABI of include/drfe.h (lmap_store.h): its lifecycle, the setters of its rows,
 * the flat image of them, the bindings of the seven resident blocks and the one function that brings them up to date on the device.
 * DESIGN.md section 25, "The resident blocks". */
#include "lmap_store.h"

#include <algorithm>
#include <cstring>

using namespace lmap_store;

int lmap_fail(drfe_lmap* db, int rc, const std::string& why)
{
    db->err = why;
    return rc;
}

bool lmap_offsets_ok(const int32_t* off, int n)
{
    if (!off || off[0] != 0) return false;
    for (int k = 0; k < n; k++)
        if (off[k + 1] < off[k]) return false;
    return true;
}

static bool handles_ok(const int32_t* h, int n)
{
    for (int i = 0; i < n; i++)
        if (h[i] < -1) return false;
    return true;
}

/* the flat image of the rows; DRFE_ERR_STATE and the name of the reference when one dangles */
int lmap_build_image(drfe_lmap* db)
{
    /* the observations of the stored map lines are looked at like those of the points, after an edit of
     * either side; they are not part of this image, so an edit of them does not rebuild it */
    if (db->imgDirty || db->recCheck) {
        for (const auto& e : db->mlObs) {
            if (db->ml.find(e.first) == db->ml.end()) continue;
            for (const int32_t o : e.second.obs)
                if (db->kf.find(o) == db->kf.end())
                    return lmap_fail(db, DRFE_ERR_STATE, "lmap: an observation of map line " + std::to_string(e.first) + " names unknown handle " + std::to_string(o));
        }
        db->recCheck = false;
    }
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
        return lmap_fail(db, DRFE_ERR_STATE, std::string("lmap: ") + what + " of " + kind + " " + std::to_string(of) + " names unknown handle " + std::to_string(h));
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
    db->geoDirty = true;               /* the slots may have moved: everything by slot is built and sent again */
    db->cullDirty = true;
    db->gbaDirty = true;
    db->recDirty = true;
    db->essDirty = true;
    for (ResidentBlock& B : db->blk) B.stale_all();
    return DRFE_OK;
}

/* Every resident array, once: the vector, the device view's field, the host view's.  The rows block has the bad flags in front
 * and the observations at its end, the attribute block the counters and observation indices at its end, so that drfe_lmap_set_bad
 * and a cull that shortened rows each send one short run.  The graph block is what a connect call commits. */
static void bind_blocks(drfe_lmap* db)
{
    Image& G = db->img;
    LmapImage &D = db->dView, &H = db->hView;
    ResidentBlock& R = db->blk[drfe_lmap::ROWS];
    R.bind(G.kfBad, &D.kfBad, &H.kfBad);
    R.bind(G.mpBad, &D.mpBad, &H.mpBad);
    db->secMlBad = R.bind(G.mlBad, &D.mlBad, &H.mlBad);
    R.bind(G.kfMpOff, &D.kfMpOff, &H.kfMpOff);
    db->secKfMp = R.bind(G.kfMp, &D.kfMp, &H.kfMp);
    R.bind(G.kfMlOff, &D.kfMlOff, &H.kfMlOff);
    db->secKfMl = R.bind(G.kfMl, &D.kfMl, &H.kfMl);
    db->secObsOff = R.bind(G.obsOff, &D.obsOff, &H.obsOff);
    R.bind(G.obs, &D.obs, &H.obs);
    ResidentBlock& Gr = db->blk[drfe_lmap::GRAPH];
    Gr.bind(G.kfParent, &D.kfParent, &H.kfParent);
    Gr.bind(G.kfNbr, &D.kfNbr, &H.kfNbr);
    Gr.bind(G.childOff, &D.childOff, &H.childOff);
    Gr.bind(G.child, &D.child, &H.child);
    Gr.bind(G.kfFirst, &db->dConn.first);
    Gr.bind(G.cwOff, &db->dConn.wOff);
    Gr.bind(G.cwKf, &db->dConn.wKf);
    Gr.bind(G.cwW, &db->dConn.wW);
    Gr.bind(G.coOff, &db->dConn.oOff);
    Gr.bind(G.coKf, &db->dConn.oKf);
    Gr.bind(G.coW, &db->dConn.oW);
    GeoImage& E = db->geo;
    ResidentBlock& Ge = db->blk[drfe_lmap::GEO];
    Ge.bind(db->scales, &db->dCorr.scale, &db->hCorr.scale);
    Ge.bind(E.kfTcw, &db->dCorr.kfTcw, &db->hCorr.kfTcw);
    Ge.bind(E.kfOw, &db->dCorr.kfOw, &db->hCorr.kfOw);
    Ge.bind(E.mpWorld, &db->dCorr.mpWorld, &db->hCorr.mpWorld);
    Ge.bind(E.mpRef, &db->dCorr.mpRef, &db->hCorr.mpRef);
    Ge.bind(E.mpLevel, &db->dCorr.mpLevel, &db->hCorr.mpLevel);
    Ge.bind(E.mpBy, &db->dCorr.mpBy, &db->hCorr.mpBy);
    Ge.bind(E.mpByRef, &db->dCorr.mpByRef, &db->hCorr.mpByRef);
    CullAttr& A = db->cull;
    ResidentBlock& At = db->blk[drfe_lmap::ATTR];
    At.bind(A.thDepth, &db->dCull.thDepth, &db->hCull.thDepth);
    At.bind(A.kfFlags, &db->dCull.kfFlags, &db->hCull.kfFlags);
    At.bind(A.octave, &db->dCull.octave, &db->hCull.octave);
    At.bind(A.depth, &db->dCull.depth, &db->hCull.depth);
    At.bind(A.stereo, &db->dCull.stereo, &db->hCull.stereo);
    db->secNObs = At.bind(A.nObs, &db->dCull.nObs, &db->hCull.nObs);
    db->secObsIdx = At.bind(A.obsIdx, &db->dCull.obsIdx, &db->hCull.obsIdx);
    GbaAttr& B = db->gba;
    ResidentBlock& Gb = db->blk[drfe_lmap::GBA];
    Gb.bind(B.kfTcwGBA, &db->dGba.kfTcwGBA);
    Gb.bind(B.kfBef, &db->dGba.kfBef);
    Gb.bind(B.mpPosGBA, &db->dGba.mpPosGBA);
    Gb.bind(B.kfStamp, &db->dGba.kfStamp);
    Gb.bind(B.mpStamp, &db->dGba.mpStamp);
    Gb.bind(B.kfHasBef, &db->dGba.kfHasBef);
    /* the counters that Tracking raises every frame in front, the line observations at the end */
    RecentAttr& Q = db->rec;
    ResidentBlock& Rc = db->blk[drfe_lmap::RECENT];
    Rc.bind(Q.mpFound, &db->dRec.found[0], &db->hRec.found[0]);
    Rc.bind(Q.mpVisible, &db->dRec.visible[0], &db->hRec.visible[0]);
    Rc.bind(Q.mlFound, &db->dRec.found[1], &db->hRec.found[1]);
    db->secRecCounters = Rc.bind(Q.mlVisible, &db->dRec.visible[1], &db->hRec.visible[1]);
    Rc.bind(Q.mpFirst, &db->dRec.first[0], &db->hRec.first[0]);
    Rc.bind(Q.mlFirst, &db->dRec.first[1], &db->hRec.first[1]);
    Rc.bind(Q.mlNObs, &db->dRec.mlNObs, &db->hRec.mlNObs);
    db->secRecObsOff = Rc.bind(Q.mlObsOff, &db->dRec.mlObsOff, &db->hRec.mlObsOff);
    Rc.bind(Q.mlObs, &db->dRec.mlObs, &db->hRec.mlObs);
    Rc.bind(Q.mlObsIdx, &db->dRec.mlObsIdx, &db->hRec.mlObsIdx);
    ResidentBlock& Lp = db->blk[drfe_lmap::LOOPS];
    Lp.bind(db->ess.leOff, &db->dEss.leOff, &db->hEss.leOff);
    Lp.bind(db->ess.le, &db->dEss.le, &db->hEss.le);
}

void lmap_host_views(drfe_lmap* db)
{
    for (ResidentBlock& B : db->blk) B.point_host();
    for (LmapImage* V : {&db->dView, &db->hView}) {
        V->nK = (int32_t)db->img.kfHandle.size();
        V->nP = (int32_t)db->img.mpHandle.size();
        V->nL = (int32_t)db->img.mlHandle.size();
    }
    db->dCorr.nLevels = db->hCorr.nLevels = (int32_t)db->scales.size();
}

int lmap_upload(drfe_lmap* db, unsigned need, hipStream_t st)
{
    lmap_host_views(db);
    size_t staged = 0, all = 0, sent[drfe_lmap::BLOCKS] = {0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < drfe_lmap::BLOCKS; b++) {
        if (!(need >> b & 1)) continue;
        /* a block that no longer fits is allocated at twice the size */
        const size_t want = db->blk[b].plan(db->dev[b].capacity());
        if (want != db->dev[b].capacity()) HIPCHK_TO(db->err, db->dev[b].alloc(want));
        staged += db->blk[b].staged();
    }
    hipError_t e = db->hup.grow(db->hup.capacity() >= staged ? staged : 2 * staged);
    char* h = db->hup;
    for (int b = 0; b < drfe_lmap::BLOCKS && e == hipSuccess; b++) {
        if (!(need >> b & 1)) continue;
        char* d = db->dev[b];
        sent[b] = db->blk[b].send(d, h, [&](size_t off, const void* src, size_t n) {
            if (e == hipSuccess) e = hipMemcpyAsync(d + off, src, n, hipMemcpyHostToDevice, st);
        }, &db->sentBytes[b]);
        h += db->blk[b].staged();
        all += sent[b];
    }
    /* the staging block is written again by the next upload */
    if (e == hipSuccess && all) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        for (int b = 0; b < drfe_lmap::BLOCKS; b++)
            if (need >> b & 1) db->blk[b].stale_all();
        return lmap_fail(db, DRFE_ERR_HIP, std::string("lmap upload: ") + hipGetErrorString(e));
    }
    if (sent[drfe_lmap::ROWS] + sent[drfe_lmap::GRAPH]) db->stats[3]++;
    if (sent[drfe_lmap::GEO]) db->corrStats[7]++;
    return DRFE_OK;
}

namespace {

template <class Map>
int set_bad(drfe_lmap* db, Map& rows, const std::unordered_map<int32_t, int32_t>& slot, std::vector<uint8_t>& bad, int32_t count,
            const int32_t* handles, const uint8_t* flags, uint8_t& (*field)(typename Map::mapped_type&))
{
    for (int i = 0; i < count; i++)
        if (rows.find(handles[i]) == rows.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_bad: unknown handle");
    for (int i = 0; i < count; i++) {
        field(rows.at(handles[i])) = flags[i] ? 1 : 0;
        if (!db->imgDirty) bad[(size_t)slot.at(handles[i])] = flags[i] ? 1 : 0;
    }
    if (count) db->blk[drfe_lmap::ROWS].stale(0, db->secMlBad);
    return DRFE_OK;
}

uint8_t& kf_bad(KfRow& r) { return r.bad; }
uint8_t& mp_bad(MpRow& r) { return r.bad; }
uint8_t& ml_bad(uint8_t& r) { return r; }

}  // namespace

extern "C" {

int drfe_lmap_create(drfe_ctx* ctx, drfe_lmap** out)
{
    if (!out) return DRFE_ERR_INVALID;
    drfe_lmap* db = new drfe_lmap();
    db->ctx = ctx;
    if (ctx) db->device = ctx->device;
    bind_blocks(db);
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
    if (scratch_bytes <= 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_configure: scratch_bytes must be positive");
    db->scratchBytes = scratch_bytes;
    return DRFE_OK;
}

int drfe_lmap_set_keyframes(drfe_lmap* db, const drfe_lmap_keyframes* r)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!r || r->count < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: invalid argument");
    const int n = r->count;
    if (n == 0) return DRFE_OK;
    if (!r->handle || !r->rank || !r->bad || !r->parent || !r->neighbours || !lmap_offsets_ok(r->child_offsets, n) ||
        !lmap_offsets_ok(r->point_offsets, n) || !lmap_offsets_ok(r->line_offsets, n) || (r->child_offsets[n] > 0 && !r->children) ||
        (r->point_offsets[n] > 0 && !r->points) || (r->line_offsets[n] > 0 && !r->lines))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: invalid argument");
    if (!handles_ok(r->parent, n) || !handles_ok(r->neighbours, n * LMAP_NEIGHBOURS) || !handles_ok(r->points, r->point_offsets[n]) ||
        !handles_ok(r->lines, r->line_offsets[n]))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: a handle below -1");
    /* the last row of a handle wins; ranks stay distinct within the store */
    std::unordered_map<int32_t, int> lastRow;
    for (int i = 0; i < n; i++) {
        if (r->handle[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: a negative handle");
        lastRow[r->handle[i]] = i;
    }
    std::unordered_map<uint64_t, int32_t> ranks;
    std::vector<int32_t> ch;
    for (const auto& e : lastRow) {
        const int i = e.second;
        const auto own = db->rankOwner.find(r->rank[i]);
        if ((own != db->rankOwner.end() && lastRow.find(own->second) == lastRow.end()) || !ranks.emplace(r->rank[i], e.first).second)
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: two key frames of the store would have the same rank");
        ch.assign(r->children + r->child_offsets[i], r->children + r->child_offsets[i + 1]);
        std::sort(ch.begin(), ch.end());
        if ((!ch.empty() && ch[0] < 0) || std::adjacent_find(ch.begin(), ch.end()) != ch.end())
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_keyframes: a child is negative or named twice");
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
    if (count < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_points: invalid argument");
    if (count == 0) return DRFE_OK;
    if (!handles || !bad || !lmap_offsets_ok(obs_offsets, count) || (obs_offsets[count] > 0 && !obs))
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_points: invalid argument");
    std::vector<int32_t> row;
    for (int i = 0; i < count; i++) {
        if (handles[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_points: a negative handle");
        row.assign(obs + obs_offsets[i], obs + obs_offsets[i + 1]);
        std::sort(row.begin(), row.end());
        if (!row.empty() && row[0] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_points: a negative observation");
        if (std::adjacent_find(row.begin(), row.end()) != row.end())
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_points: a key frame observes a point twice");
    }
    for (int i = 0; i < count; i++) {
        MpRow& P = db->mp[handles[i]];
        P.bad = bad[i] ? 1 : 0;
        P.obs.assign(obs + obs_offsets[i], obs + obs_offsets[i + 1]);
        db->mpReplaced.erase(handles[i]);
    }
    db->imgDirty = true;
    return DRFE_OK;
}

int drfe_lmap_set_lines(drfe_lmap* db, int32_t count, const int32_t* handles, const uint8_t* bad)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !bad))) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_lines: invalid argument");
    for (int i = 0; i < count; i++)
        if (handles[i] < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_lines: a negative handle");
    for (int i = 0; i < count; i++) {
        db->ml[handles[i]] = bad[i] ? 1 : 0;
        db->mlReplaced.erase(handles[i]);
    }
    if (count) db->imgDirty = true;
    return DRFE_OK;
}

int drfe_lmap_set_bad(drfe_lmap* db, int kind, int32_t count, const int32_t* handles, const uint8_t* flags)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !flags))) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_bad: invalid argument");
    Image& G = db->img;
    if (kind == DRFE_LMAP_KEYFRAME) return set_bad(db, db->kf, G.kfSlot, G.kfBad, count, handles, flags, kf_bad);
    if (kind == DRFE_LMAP_POINT) return set_bad(db, db->mp, G.mpSlot, G.mpBad, count, handles, flags, mp_bad);
    if (kind == DRFE_LMAP_LINE) return set_bad(db, db->ml, G.mlSlot, G.mlBad, count, handles, flags, ml_bad);
    return lmap_fail(db, DRFE_ERR_INVALID, "lmap_set_bad: unknown kind");
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
            db->loopEdges.erase(handle);
            gone = 1;
        }
    } else if (kind == DRFE_LMAP_POINT) {
        gone = db->mp.erase(handle);
        if (gone) {
            db->mpGeo.erase(handle);
            db->mpCull.erase(handle);
            db->mpGba.erase(handle);
            db->mpRec.erase(handle);
            db->mpReplaced.erase(handle);
        }
    } else if (kind == DRFE_LMAP_LINE) {
        gone = db->ml.erase(handle);
        if (gone) {
            db->mlRec.erase(handle);
            db->mlObs.erase(handle);
            db->mlReplaced.erase(handle);
        }
    } else {
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_remove: unknown kind");
    }
    if (!gone) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_remove: unknown handle");
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

int drfe_lmap_upload_bytes(drfe_lmap* db, int64_t* out5)
{
    if (!db || !out5) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    std::memcpy(out5, db->sentBytes, 5 * sizeof(int64_t));
    return DRFE_OK;
}

}  // extern "C"
