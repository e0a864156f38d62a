/* fuse_caller.cpp — Planar_SLAM::LocalMapTracker::Fuse (points and lines), FuseLoop and FuseMatched of include/drfe_adaptor.hpp
 * over stand-in classes with the reference's members: a real std::map<KeyFrame*, size_t> of observations in pointer order, the
 * nObs counter, mnFound, mnVisible and mpReplaced per map point and per map line.  Their Replace and AddObservation restate what the
 * reference's do (src/MapPoint.cc:91-107 and :223-261, src/MapLine.cpp:91-100 and :178-214).
 *
 *   fuse_caller [host | device]
 *
 * Two equal worlds are built.  On the first the adaptor's methods run: the store call, then the reference's loop on the objects.
 * On the second the reference's loops (src/ORBmatcher.cc:845-976 and :1001-1101, src/LSDmatcher.cpp:897-1012,
 * src/LoopClosing.cc:566-581 and :650-657) run on the objects alone.  The answers of the search are seeded.  After each of four
 * SearchInNeighbors-shaped rounds (the neighbours' points and lines into the key frame, then its own into every neighbour) and
 * one CorrectLoop-shaped round (the matched points, then SearchAndFuse over three key frames) the two worlds must be equal (bad
 * flags, rows, observations, counters, mpReplaced), and the store must equal the objects of the first: counters, nObs, observers and
 * indices, mpReplaced and the rows through the getters, and - through an UpdateLocalMap of every key frame's row next to a store
 * synced afresh from the objects - the bad flags and the match rows again. */
#include "drfe_adaptor.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <list>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace fuse_world {

struct KeyFrame;

struct Item {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    long int mnFirstKFid = 0;
    bool mbBad = false;
    int nObs = 0, mnFound = 1, mnVisible = 1;
    std::map<KeyFrame*, size_t> mObservations;
    bool isBad() const { return mbBad; }
    int Observations() const { return nObs; }
    int GetFound() const { return mnFound; }
    int GetVisible() const { return mnVisible; }          /* the getter the integrator adds */
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
    bool IsInKeyFrame(KeyFrame* pKF) const { return mObservations.count(pKF) != 0; }
    void IncreaseFound(int n) { mnFound += n; }
    void IncreaseVisible(int n) { mnVisible += n; }
};

struct MapPoint : Item {
    float GetFoundRatio() const { return static_cast<float>(mnFound) / mnVisible; }
    MapPoint* mpReplaced = nullptr;
    void SetBadFlag();
    void AddObservation(KeyFrame* pKF, size_t idx);
    void Replace(MapPoint* pMP);
};

struct MapLine : Item {
    float GetFoundRatio() const { return static_cast<float>(mnFound / mnVisible); }
    MapLine* mpReplaced = nullptr;
    void SetBadFlag();
    void AddObservation(KeyFrame* pKF, size_t idx);
    void Replace(MapLine* pML);
};

struct Frame {
    long unsigned int mnId = 0;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    void* mpReferenceKF = nullptr;
};

struct KeyFrame {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    bool mbBad = false;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    bool isBad() const { return mbBad; }
    KeyFrame* GetParent() const { return mpParent; }
    std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int&) const { return std::vector<KeyFrame*>(); }
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    std::vector<MapLine*> GetMapLineMatches() const { return mvpMapLines; }
    void EraseMapPointMatch(size_t idx) { mvpMapPoints[idx] = nullptr; }
    void EraseMapLineMatch(size_t idx) { mvpMapLines[idx] = nullptr; }
    /* what SyncCulling reads, and the fuse commit of it the stereo flags */
    struct Key { int octave = 0; };
    std::vector<Key> mvKeysUn;
    std::vector<float> mvDepth, mvuRight;
    float mThDepth = 40.0f;
    bool GetNotErase() const { return false; }
    bool GetToBeErased() const { return false; }
    MapPoint* GetMapPoint(size_t idx) const { return mvpMapPoints[idx]; }
    MapLine* GetMapLine(size_t idx) const { return mvpMapLines[idx]; }
    void AddMapPoint(MapPoint* p, size_t idx) { mvpMapPoints[idx] = p; }
    void AddMapLine(MapLine* l, size_t idx) { mvpMapLines[idx] = l; }
    void ReplaceMapPointMatch(size_t idx, MapPoint* p) { mvpMapPoints[idx] = p; }
    void ReplaceMapLineMatch(size_t idx, MapLine* l) { mvpMapLines[idx] = l; }
    std::set<MapPoint*> GetMapPoints() const
    {
        std::set<MapPoint*> s;
        for (MapPoint* p : mvpMapPoints)
            if (p) s.insert(p);
        return s;
    }
};

/* src/MapPoint.cc:91-107: a stereo keypoint counts twice */
void MapPoint::AddObservation(KeyFrame* pKF, size_t idx)
{
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs += pKF->mvuRight[idx] >= 0 ? 2 : 1;
}

void MapLine::AddObservation(KeyFrame* pKF, size_t idx)
{
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs++;
}

/* src/MapPoint.cc:223-261 */
void MapPoint::Replace(MapPoint* pMP)
{
    if (pMP->mnId == mnId) return;
    std::map<KeyFrame*, size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    const int nvisible = mnVisible, nfound = mnFound;
    mpReplaced = pMP;
    for (auto& o : obs) {
        if (!pMP->IsInKeyFrame(o.first)) {
            o.first->ReplaceMapPointMatch(o.second, pMP);
            pMP->AddObservation(o.first, o.second);
        } else {
            o.first->EraseMapPointMatch(o.second);
        }
    }
    pMP->IncreaseFound(nfound);
    pMP->IncreaseVisible(nvisible);
}

/* src/MapLine.cpp:178-214 */
void MapLine::Replace(MapLine* pML)
{
    if (pML->mnId == mnId) return;
    std::map<KeyFrame*, size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    const int nvisible = mnVisible, nfound = mnFound;
    mpReplaced = pML;
    for (auto& o : obs) {
        if (!pML->IsInKeyFrame(o.first)) {
            o.first->ReplaceMapLineMatch(o.second, pML);
            pML->AddObservation(o.first, o.second);
        } else {
            o.first->EraseMapLineMatch(o.second);
        }
    }
    pML->IncreaseFound(nfound);
    pML->IncreaseVisible(nvisible);
}

void MapPoint::SetBadFlag()
{
    std::map<KeyFrame*, size_t> obs = mObservations;
    mbBad = true;
    mObservations.clear();
    for (auto& o : obs) o.first->EraseMapPointMatch(o.second);
}

void MapLine::SetBadFlag()
{
    std::map<KeyFrame*, size_t> obs = mObservations;
    mbBad = true;
    mObservations.clear();
    for (auto& o : obs) o.first->EraseMapLineMatch(o.second);
}

typedef Planar_SLAM::LocalMapTracker<KeyFrame, MapPoint, MapLine, Frame> Tracker;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2654435761u + 12345) {}
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

/* nKf key frames under key frame 0, points and lines seen by 0 .. 5 of them; a tenth bad, a few with stale indices */
struct World {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
    std::vector<MapLine> mls;
    std::list<MapPoint*> recentPoints;
    std::list<MapLine*> recentLines;

    template <class ItemT, class Row> void fill(std::vector<ItemT>& items, Row row, Rng& R, long int newest)
    {
        for (size_t i = 0; i < items.size(); i++) {
            ItemT& p = items[i];
            p.mnId = (long unsigned int)i;
            p.mnFound = R.below(12);
            p.mnVisible = 1 + R.below(11);
            p.mnFirstKFid = newest - R.below(5);
            const int nSeen = R.below(6);
            for (int k = 0; k < nSeen; k++) {
                KeyFrame* pKF = &kfs[(size_t)R.below((int)kfs.size())];
                if (p.mObservations.count(pKF)) continue;
                (pKF->*row).push_back(&p);
                p.mObservations[pKF] = (pKF->*row).size() - 1;
                p.nObs++;
            }
            if (R.below(10) == 0) p.mbBad = true;
        }
        /* a stale index: an observation that names a place where another item stands */
        for (size_t i = 0; i + 1 < items.size(); i += 9) {
            KeyFrame* pKF = &kfs[(size_t)R.below((int)kfs.size())];
            if (items[i].mObservations.count(pKF) || (pKF->*row).empty()) continue;
            items[i].mObservations[pKF] = (size_t)R.below((int)(pKF->*row).size());
        }
    }

    World(int nKf, int nMp, int nMl, uint64_t seed) : kfs((size_t)nKf), mps((size_t)nMp), mls((size_t)nMl)
    {
        Rng R(seed);
        for (int k = 0; k < nKf; k++) {
            kfs[(size_t)k].mnId = (long unsigned int)k;
            if (k) {
                kfs[(size_t)k].mpParent = &kfs[0];
                kfs[0].mspChildrens.insert(&kfs[(size_t)k]);
            }
        }
        kfs[(size_t)nKf - 1].mbBad = true;
        fill(mps, &KeyFrame::mvpMapPoints, R, (long int)nKf);
        fill(mls, &KeyFrame::mvpMapLines, R, (long int)nKf);
        /* ProcessNewKeyFrame pushes once per row index: some items stand in the list more than once */
        for (MapPoint& p : mps) {
            recentPoints.push_back(&p);
            if (p.mnId % 7 == 3) recentPoints.push_back(&p);
        }
        for (MapLine& l : mls) {
            recentLines.push_back(&l);
            if (l.mnId % 5 == 2) recentLines.push_back(&l);
        }
        for (size_t i = 0; i + 20 < mps.size(); i += 11) recentPoints.push_back(&mps[i]);
        /* empty entries to add into, the keypoints' attributes, and nObs with the stereo observations counted twice */
        for (KeyFrame& k : kfs) {
            for (int e = 0; e < 8; e++) {
                k.mvpMapPoints.insert(k.mvpMapPoints.begin() + R.below((int)k.mvpMapPoints.size() + 1), nullptr);
                k.mvpMapLines.insert(k.mvpMapLines.begin() + R.below((int)k.mvpMapLines.size() + 1), nullptr);
            }
            const size_t n = k.mvpMapPoints.size();
            k.mvKeysUn.resize(n);
            k.mvDepth.assign(n, 1.0f);
            k.mvuRight.resize(n);
            for (size_t i = 0; i < n; i++) k.mvuRight[i] = R.below(2) ? 5.0f : -1.0f;
        }
        /* the inserted entries moved the rows: the observations name the places again, but for the stale ones of fill() */
        for (KeyFrame& k : kfs) {
            for (size_t i = 0; i < k.mvpMapPoints.size(); i++)
                if (k.mvpMapPoints[i] && k.mvpMapPoints[i]->mObservations.count(&k) && (i % 17) != 3) k.mvpMapPoints[i]->mObservations[&k] = i;
            for (size_t i = 0; i < k.mvpMapLines.size(); i++)
                if (k.mvpMapLines[i] && k.mvpMapLines[i]->mObservations.count(&k) && (i % 17) != 3) k.mvpMapLines[i]->mObservations[&k] = i;
        }
        for (MapPoint& p : mps) {
            p.nObs = 0;
            for (auto& o : p.mObservations) {
                if (o.second >= o.first->mvpMapPoints.size()) o.second = 0;
                p.nObs += o.first->mvuRight[o.second] >= 0 ? 2 : 1;
            }
        }
        for (MapLine& l : mls)
            for (auto& o : l.mObservations)
                if (o.second >= o.first->mvpMapLines.size()) o.second = 0;
    }

    void sync(Tracker& T)
    {
        for (KeyFrame& k : kfs) {
            T.Sync(&k);
            T.SyncCulling(&k);
        }
        for (MapPoint& p : mps) {
            T.Sync(&p);
            T.SyncCulling(&p);
            T.SyncRecent(&p);
        }
        for (MapLine& l : mls) {
            T.Sync(&l);
            T.SyncRecent(&l);
        }
    }
};

/* the reference's loops on the objects alone */
template <class ItemT, class Get, class Add> int reference_fuse(KeyFrame* pKF, const std::vector<ItemT*>& v, const std::vector<int32_t>& best, bool asksInKF, Get get, Add add)
{
    int nFused = 0;
    for (size_t i = 0; i < v.size(); i++) {
        ItemT* p = v[i];
        if (!p) continue;
        if (p->isBad() || (asksInKF && p->IsInKeyFrame(pKF))) continue;
        if (best[i] < 0) continue;
        ItemT* inKF = get(pKF, (size_t)best[i]);
        if (inKF) {
            if (!inKF->isBad()) {
                if (inKF->Observations() > p->Observations()) p->Replace(inKF);
                else inKF->Replace(p);
            }
        } else {
            p->AddObservation(pKF, (size_t)best[i]);
            add(pKF, p, (size_t)best[i]);
        }
        nFused++;
    }
    return nFused;
}

int reference_loop(KeyFrame* pKF, const std::vector<MapPoint*>& v, const std::vector<int32_t>& best)
{
    const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();
    std::vector<MapPoint*> vpReplacePoint(v.size(), nullptr);
    std::vector<uint8_t> skip(v.size());
    for (size_t i = 0; i < v.size(); i++) skip[i] = v[i]->isBad() || spAlreadyFound.count(v[i]);
    int nFused = 0;
    for (size_t i = 0; i < v.size(); i++) {
        if (skip[i] || best[i] < 0) continue;
        MapPoint* inKF = pKF->GetMapPoint((size_t)best[i]);
        if (inKF) {
            if (!inKF->isBad()) vpReplacePoint[i] = inKF;
        } else {
            v[i]->AddObservation(pKF, (size_t)best[i]);
            pKF->AddMapPoint(v[i], (size_t)best[i]);
        }
        nFused++;
    }
    for (size_t i = 0; i < v.size(); i++)
        if (vpReplacePoint[i]) vpReplacePoint[i]->Replace(v[i]);
    return nFused;
}

int reference_matched(KeyFrame* pKF, const std::vector<MapPoint*>& v)
{
    int n = 0;
    for (size_t i = 0; i < v.size(); i++) {
        if (!v[i]) continue;
        MapPoint* cur = pKF->GetMapPoint(i);
        if (cur) cur->Replace(v[i]);
        else {
            pKF->AddMapPoint(v[i], i);
            v[i]->AddObservation(pKF, i);
        }
        n++;
    }
    return n;
}

int fail(const char* what, long a = -1, long b = -1)
{
    std::fprintf(stderr, "fuse_caller: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

template <class ItemT> std::vector<long> ids(const std::list<ItemT*>& l)
{
    std::vector<long> v;
    for (ItemT* p : l) v.push_back((long)p->mnId);
    return v;
}

template <class ItemT> std::vector<long> row_ids(const std::vector<ItemT*>& r)
{
    std::vector<long> v;
    for (ItemT* p : r) v.push_back(p ? (long)p->mnId : -1);
    return v;
}

template <class ItemT> bool same_items(const std::vector<ItemT>& a, const std::vector<ItemT>& b)
{
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].mbBad != b[i].mbBad || a[i].nObs != b[i].nObs || a[i].mObservations.size() != b[i].mObservations.size()) return false;
        if (a[i].mnFound != b[i].mnFound || a[i].mnVisible != b[i].mnVisible) return false;
        if ((a[i].mpReplaced ? (long)a[i].mpReplaced->mnId : -1) != (b[i].mpReplaced ? (long)b[i].mpReplaced->mnId : -1)) return false;
        auto x = a[i].mObservations.begin();
        auto y = b[i].mObservations.begin();
        for (; x != a[i].mObservations.end(); ++x, ++y)
            if (x->first->mnId != y->first->mnId || x->second != y->second) return false;
    }
    return true;
}

int same_worlds(const World& A, const World& B)
{
    if (ids(A.recentPoints) != ids(B.recentPoints)) return fail("the point lists differ");
    if (ids(A.recentLines) != ids(B.recentLines)) return fail("the line lists differ");
    if (!same_items(A.mps, B.mps)) return fail("the map points differ");
    if (!same_items(A.mls, B.mls)) return fail("the map lines differ");
    for (size_t k = 0; k < A.kfs.size(); k++) {
        if (row_ids(A.kfs[k].mvpMapPoints) != row_ids(B.kfs[k].mvpMapPoints)) return fail("a point row differs", (long)k);
        if (row_ids(A.kfs[k].mvpMapLines) != row_ids(B.kfs[k].mvpMapLines)) return fail("a line row differs", (long)k);
    }
    return 0;
}

/* UpdateLocalMap of every key frame's row, as one flat vector of everything it returned */
int local_maps(drfe_lmap* db, const World& W, int64_t* nextFrame, bool device, std::vector<int32_t>& out)
{
    const int32_t n = (int32_t)W.kfs.size();
    std::vector<int64_t> frame((size_t)n);
    std::vector<int32_t> pOff(1, 0), pts, lOff(1, 0), lns;
    for (int32_t k = 0; k < n; k++) {
        frame[(size_t)k] = (*nextFrame)++;
        for (MapPoint* p : W.kfs[(size_t)k].mvpMapPoints) pts.push_back(p ? (int32_t)p->mnId : -1);
        for (MapLine* l : W.kfs[(size_t)k].mvpMapLines) lns.push_back(l ? (int32_t)l->mnId : -1);
        pOff.push_back((int32_t)pts.size());
        lOff.push_back((int32_t)lns.size());
    }
    drfe_lmap_queries q = {};
    q.n = n; q.frame_id = frame.data(); q.point_offsets = pOff.data(); q.points = pts.data(); q.line_offsets = lOff.data(); q.lines = lns.data();
    const size_t nK = (size_t)n * W.kfs.size(), nP = (size_t)n * W.mps.size(), nL = (size_t)n * W.mls.size();
    std::vector<int32_t> kOff((size_t)n + 1), kf(nK + 1), ref((size_t)n), mOff((size_t)n + 1), mp(nP + 1), lOut((size_t)n + 1), ml(nL + 1),
        nuOff((size_t)n + 1), nu(pts.size() + 1), rec(4 * (size_t)n);
    std::vector<uint8_t> mpIn(nP + 1), mlIn(nL + 1);
    drfe_lmap_out o = {};
    o.kf_capacity = (int32_t)nK; o.mp_capacity = (int32_t)nP; o.ml_capacity = (int32_t)nL; o.nulled_capacity = (int32_t)pts.size();
    o.kf_offsets = kOff.data(); o.kfs = kf.data(); o.ref_kf = ref.data(); o.mp_offsets = mOff.data(); o.mps = mp.data();
    o.mp_in_frame = mpIn.data(); o.ml_offsets = lOut.data(); o.mls = ml.data(); o.ml_in_frame = mlIn.data();
    o.nulled_offsets = nuOff.data(); o.nulled = nu.data(); o.record = rec.data();
    const int rc = device ? drfe_lmap_update_device(db, &q, &o, nullptr) : drfe_lmap_update_host(db, &q, &o);
    if (rc != DRFE_OK) return fail(drfe_lmap_last_error(db), rc);
    out.clear();
    out.insert(out.end(), kOff.begin(), kOff.end());
    out.insert(out.end(), kf.begin(), kf.begin() + kOff[(size_t)n]);
    out.insert(out.end(), ref.begin(), ref.end());
    out.insert(out.end(), mOff.begin(), mOff.end());
    out.insert(out.end(), mp.begin(), mp.begin() + mOff[(size_t)n]);
    out.insert(out.end(), mpIn.begin(), mpIn.begin() + mOff[(size_t)n]);
    out.insert(out.end(), lOut.begin(), lOut.end());
    out.insert(out.end(), ml.begin(), ml.begin() + lOut[(size_t)n]);
    out.insert(out.end(), mlIn.begin(), mlIn.begin() + lOut[(size_t)n]);
    out.insert(out.end(), nuOff.begin(), nuOff.end());
    out.insert(out.end(), nu.begin(), nu.begin() + nuOff[(size_t)n]);
    out.insert(out.end(), rec.begin(), rec.end());
    return 0;
}

/* the store of T against the objects of W */
int same_store(Tracker& T, World& W, int64_t* nextFrame, bool device)
{
    drfe_lmap* db = T.db();
    /* the getters */
    for (MapPoint& p : W.mps) {
        const int32_t h = (int32_t)p.mnId;
        int32_t found = 0, visible = 0, nObs = 0, off[2] = {0, 0};
        int64_t first = 0;
        std::vector<int32_t> idx(p.mObservations.size() + 1);
        drfe_lmap_recent_attributes_out r = {};
        r.n_points = 1; r.point_handle = &h; r.point_found = &found; r.point_visible = &visible; r.point_first_kf = &first;
        if (drfe_lmap_get_recent_attributes(db, &r) != DRFE_OK) return fail(drfe_lmap_last_error(db), h);
        if (found != p.mnFound || visible != p.mnVisible || first != (int64_t)p.mnFirstKFid) return fail("a point's counters differ", h);
        drfe_lmap_cull_attributes_out c = {};
        c.n_points = 1; c.obs_capacity = (int32_t)idx.size(); c.point_handle = &h; c.n_obs = &nObs; c.obs_offsets = off; c.obs_index = idx.data();
        if (drfe_lmap_get_cull_attributes(db, &c) != DRFE_OK) return fail(drfe_lmap_last_error(db), h);
        if (nObs != p.nObs || off[1] != (int32_t)p.mObservations.size()) return fail("a point's observations differ", h, off[1]);
        size_t i = 0;
        for (const auto& o : p.mObservations)
            if (idx[i++] != (int32_t)o.second) return fail("a point's observation index differs", h);
    }
    for (MapLine& l : W.mls) {
        const int32_t h = (int32_t)l.mnId;
        int32_t found = 0, visible = 0, nObs = 0, off[2] = {0, 0};
        int64_t first = 0;
        std::vector<int32_t> obs(l.mObservations.size() + 1), idx(l.mObservations.size() + 1);
        drfe_lmap_recent_attributes_out r = {};
        r.n_lines = 1; r.line_obs_capacity = (int32_t)obs.size(); r.line_handle = &h; r.line_found = &found; r.line_visible = &visible;
        r.line_first_kf = &first; r.line_n_obs = &nObs; r.line_obs_offsets = off; r.line_obs = obs.data(); r.line_obs_index = idx.data();
        if (drfe_lmap_get_recent_attributes(db, &r) != DRFE_OK) return fail(drfe_lmap_last_error(db), h);
        if (found != l.mnFound || visible != l.mnVisible || first != (int64_t)l.mnFirstKFid || nObs != l.nObs) return fail("a line's counters differ", h);
        if (off[1] != (int32_t)l.mObservations.size()) return fail("a line's observations differ", h, off[1]);
        size_t i = 0;
        for (const auto& o : l.mObservations) {
            if (obs[i] != (int32_t)o.first->mnId || idx[i] != (int32_t)o.second) return fail("a line's observation differs", h);
            i++;
        }
    }
    /* mpReplaced, the observers and the rows through the getters of the fuse commit */
    for (int kind = DRFE_LMAP_POINT; kind <= DRFE_LMAP_LINE; kind++) {
        const size_t n = kind == DRFE_LMAP_POINT ? W.mps.size() : W.mls.size();
        for (size_t i = 0; i < n; i++) {
            const Item& it = kind == DRFE_LMAP_POINT ? static_cast<const Item&>(W.mps[i]) : static_cast<const Item&>(W.mls[i]);
            const long want = kind == DRFE_LMAP_POINT ? (W.mps[i].mpReplaced ? (long)W.mps[i].mpReplaced->mnId : -1) : (W.mls[i].mpReplaced ? (long)W.mls[i].mpReplaced->mnId : -1);
            const int32_t h = (int32_t)it.mnId;
            int32_t rep = -2, nObs = 0;
            uint8_t bad = 9;
            std::vector<int32_t> obs(it.mObservations.size() + 1);
            if (drfe_lmap_get_replaced(db, kind, 1, &h, &rep) != DRFE_OK || rep != want) return fail("mpReplaced differs", h, rep);
            if (drfe_lmap_get_observers(db, kind, h, (int32_t)obs.size(), &bad, &nObs, obs.data()) != DRFE_OK) return fail(drfe_lmap_last_error(db), h);
            if (bad != (it.mbBad ? 1 : 0) || nObs != (int32_t)it.mObservations.size()) return fail("the bad flag or the observers differ", h, nObs);
            size_t o = 0;
            for (const auto& e : it.mObservations)
                if (obs[o++] != (int32_t)e.first->mnId) return fail("an observer differs", h);
        }
    }
    for (const KeyFrame& k : W.kfs) {
        std::vector<int32_t> row(k.mvpMapPoints.size() + k.mvpMapLines.size() + 1);
        int32_t n = 0;
        if (drfe_lmap_get_match_row(db, DRFE_LMAP_POINT, (int32_t)k.mnId, (int32_t)row.size(), &n, row.data()) != DRFE_OK) return fail(drfe_lmap_last_error(db));
        if (std::vector<long>(row.begin(), row.begin() + n) != row_ids(k.mvpMapPoints)) return fail("a point row of the store differs", (long)k.mnId);
        if (drfe_lmap_get_match_row(db, DRFE_LMAP_LINE, (int32_t)k.mnId, (int32_t)row.size(), &n, row.data()) != DRFE_OK) return fail(drfe_lmap_last_error(db));
        if (std::vector<long>(row.begin(), row.begin() + n) != row_ids(k.mvpMapLines)) return fail("a line row of the store differs", (long)k.mnId);
    }
    /* the bad flags and the rows, next to a store synced afresh */
    Tracker fresh(-1);
    W.sync(fresh);
    std::vector<int32_t> a, b;
    int64_t f2 = *nextFrame;
    if (local_maps(db, W, nextFrame, device, a) || local_maps(fresh.db(), W, &f2, false, b)) return 1;
    if (a != b) return fail("UpdateLocalMap on the store and on a fresh one differ", (long)a.size(), (long)b.size());
    return 0;
}

/* the seeded answer of a search: half the candidates get an entry of the row */
std::vector<int32_t> answers(Rng& R, size_t n, size_t width)
{
    std::vector<int32_t> b(n);
    for (size_t i = 0; i < n; i++) b[i] = R.below(2) && width ? R.below((int)width) : -1;
    return b;
}

int run(bool device)
{
    World A(24, 400, 160, 5), B(24, 400, 160, 5);
    Tracker T(device ? 0 : -1);
    T.UseDevice(device);
    A.sync(T);
    int64_t nextFrame = 1000;
    int calls = 0;
    Rng R(99);
    auto getP = [](KeyFrame* k, size_t i) { return k->GetMapPoint(i); };
    auto addP = [](KeyFrame* k, MapPoint* p, size_t i) { k->AddMapPoint(p, i); };
    auto getL = [](KeyFrame* k, size_t i) { return k->GetMapLine(i); };
    auto addL = [](KeyFrame* k, MapLine* l, size_t i) { k->AddMapLine(l, i); };
    /* one Fuse call on both worlds; the candidates are taken from the rows of key frame `from` (with their nulls) */
    auto fuse_points = [&](size_t kf, size_t from) {
        const std::vector<int32_t> best = answers(R, A.kfs[from].mvpMapPoints.size(), A.kfs[kf].mvpMapPoints.size());
        const std::vector<MapPoint*> va = A.kfs[from].mvpMapPoints, vb = B.kfs[from].mvpMapPoints;
        const int a = T.Fuse(&A.kfs[kf], va, best), b = reference_fuse(&B.kfs[kf], vb, best, true, getP, addP);
        calls++;
        return a == b ? 0 : fail("nFused of a point Fuse differs", a, b);
    };
    auto fuse_lines = [&](size_t kf, size_t from) {
        const std::vector<int32_t> best = answers(R, A.kfs[from].mvpMapLines.size(), A.kfs[kf].mvpMapLines.size());
        const std::vector<MapLine*> va = A.kfs[from].mvpMapLines, vb = B.kfs[from].mvpMapLines;
        const int a = T.Fuse(&A.kfs[kf], va, best), b = reference_fuse(&B.kfs[kf], vb, best, false, getL, addL);
        calls++;
        return a == b ? 0 : fail("nFused of a line Fuse differs", a, b);
    };
    for (int round = 0; round < 4; round++) {
        const size_t cur = (size_t)(1 + 5 * round);
        for (size_t nb = cur + 1; nb < cur + 5; nb++)
            if (fuse_points(cur, nb) || fuse_lines(cur, nb)) return 1;
        for (size_t nb = cur + 1; nb < cur + 5; nb++)
            if (fuse_points(nb, cur) || fuse_lines(nb, cur)) return 1;
        if (same_worlds(A, B)) return 1;
        if (same_store(T, A, &nextFrame, device)) return 1;
    }
    /* CorrectLoop: the matched points into the current key frame, then SearchAndFuse of the loop points into three key frames */
    {
        const size_t cur = 22, n = A.kfs[cur].mvpMapPoints.size();
        std::vector<MapPoint*> va(n, nullptr), vb(n, nullptr);
        for (size_t i = 0; i < n; i++)
            if (R.below(3) == 0) {
                const size_t p = (size_t)R.below((int)A.mps.size());
                va[i] = &A.mps[p];
                vb[i] = &B.mps[p];
            }
        if (T.FuseMatched(&A.kfs[cur], va) != reference_matched(&B.kfs[cur], vb)) return fail("FuseMatched counts differ");
        calls++;
        std::vector<MapPoint*> la, lb;
        for (int i = 0; i < 150; i++) {
            const size_t p = (size_t)R.below((int)A.mps.size());
            la.push_back(&A.mps[p]);
            lb.push_back(&B.mps[p]);
        }
        for (size_t kf : {(size_t)22, (size_t)3, (size_t)9}) {
            const std::vector<int32_t> best = answers(R, la.size(), A.kfs[kf].mvpMapPoints.size());
            std::vector<MapPoint*> vpReplace;
            if (T.FuseLoop(&A.kfs[kf], la, best, vpReplace) != reference_loop(&B.kfs[kf], lb, best)) return fail("FuseLoop counts differ", (long)kf);
            calls++;
        }
        if (same_worlds(A, B)) return 1;
        if (same_store(T, A, &nextFrame, device)) return 1;
    }
    int64_t st[8];
    drfe_lmap_fuse_stats(T.db(), st);
    if (st[0] != calls || st[2] != (device ? st[0] : 0)) return fail("the calls ran on the wrong entry", (long)st[2], (long)st[0]);
    std::printf("fuse_caller ok (%s, %d calls, %ld added, %ld replaced, %ld moved, %ld erased)\n", device ? "device" : "host", calls, (long)st[3], (long)st[4],
                (long)st[5], (long)st[6]);
    return st[3] > 50 && st[4] > 50 && st[6] > 0 ? 0 : fail("too little happened", (long)st[3], (long)st[4]);
}

}  // namespace fuse_world

#ifndef FUSE_CALLER_NO_MAIN
int main(int argc, char** argv)
{
    const bool device = argc > 1 && std::string(argv[1]) == "device";
    try {
        return fuse_world::run(device);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "fuse_caller: %s\n", e.what());
        return 1;
    }
}
#endif
