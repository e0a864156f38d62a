/* recent_cull_caller.cpp — Planar_SLAM::LocalMapTracker::SyncRecent / MapPointCulling / MapLineCulling of
 * include/drfe_adaptor.hpp over stand-in classes with the reference's members: a real std::map<KeyFrame*, size_t> of observations,
 * the nObs counter, mnFound, mnVisible and mnFirstKFid per map point and per map line.  Their SetBadFlag restates what the
 * reference's do (src/MapPoint.cc:175-202 and MapLine's): the observations are taken, cleared, and every former observer's
 * EraseMapPointMatch / EraseMapLineMatch is called with the stored index.
 *
 *   recent_cull_caller [host | device]
 *
 * Two equal worlds are built.  On the first the adaptor's methods run: the store decides and changes itself, then the list is
 * walked and the objects' own SetBadFlag() called.  On the second the rules of the reference's two loops
 * (src/LocalMapping.cc:175-231) run on the objects alone.  After every call the two worlds must be equal (lists, bad flags, rows, observations), and the
 * store must equal the objects of the first: the recent-list attributes and observation indices through the getters, and - through
 * an UpdateLocalMap of every key frame's row next to a store synced afresh from the objects - the bad flags and the match rows. */
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

namespace recent_world {

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
};

struct MapPoint : Item {
    float GetFoundRatio() const { return static_cast<float>(mnFound) / mnVisible; }
    void SetBadFlag();
};

struct MapLine : Item {
    float GetFoundRatio() const { return static_cast<float>(mnFound / mnVisible); }
    void SetBadFlag();
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
};

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
    }

    void sync(Tracker& T)
    {
        for (KeyFrame& k : kfs) T.Sync(&k);
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

/* the rules of LocalMapping::MapPointCulling / MapLineCulling (src/LocalMapping.cc:175-231) on the objects alone, one entry after
 * another with the list erased as it goes */
template <class ItemT> void reference_culling(std::list<ItemT*>& recent, unsigned long int currentId, bool monocular)
{
    const int fewObservations = monocular ? 2 : 3;
    for (auto it = recent.begin(); it != recent.end();) {
        ItemT* p = *it;
        const int age = (int)currentId - (int)p->mnFirstKFid;
        bool drop = true;
        if (p->isBad()) {
        } else if (p->GetFoundRatio() < 0.25f || (age >= 2 && p->Observations() <= fewObservations)) {
            p->SetBadFlag();
        } else if (age < 3) {
            drop = false;
        }
        it = drop ? recent.erase(it) : std::next(it);
    }
}

int fail(const char* what, long a = -1, long b = -1)
{
    std::fprintf(stderr, "recent_cull_caller: %s (%ld, %ld)\n", what, a, b);
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
    /* the bad flags and the rows, next to a store synced afresh */
    Tracker fresh(-1);
    W.sync(fresh);
    std::vector<int32_t> a, b;
    int64_t f2 = *nextFrame;
    if (local_maps(db, W, nextFrame, device, a) || local_maps(fresh.db(), W, &f2, false, b)) return 1;
    if (a != b) return fail("UpdateLocalMap on the store and on a fresh one differ", (long)a.size(), (long)b.size());
    return 0;
}

int run(bool device)
{
    World A(24, 400, 160, 5), B(24, 400, 160, 5);
    Tracker T(device ? 0 : -1);
    T.UseDevice(device);
    A.sync(T);
    int64_t nextFrame = 1000;
    int calls = 0;
    long culled = 0;
    for (int round = 0; round < 4; round++) {
        const unsigned long cur = 24 + (unsigned long)round;
        const bool mono = round == 2;
        KeyFrame current;
        current.mnId = cur;
        long before = 0;
        for (MapPoint& p : A.mps) before += p.mbBad;
        for (MapLine& l : A.mls) before += l.mbBad;
        T.MapPointCulling(A.recentPoints, &current, mono);
        T.MapLineCulling(A.recentLines, &current, mono);
        reference_culling(B.recentPoints, cur, mono);
        reference_culling(B.recentLines, cur, mono);
        calls += 2;
        for (MapPoint& p : A.mps) culled += p.mbBad;
        for (MapLine& l : A.mls) culled += l.mbBad;
        culled -= before;
        if (same_worlds(A, B)) return 1;
        if (same_store(T, A, &nextFrame, device)) return 1;
        /* tracking goes on: counters rise on both sides, and a few items come back into the lists */
        for (World* W : {&A, &B})
            for (MapPoint& p : W->mps) {
                if (p.mbBad || p.mnId % 3 != (unsigned long)round % 3) continue;
                p.mnVisible += 9;
                p.mnFound += (int)(p.mnId % 2);
                if (W == &A) T.Increased(&p, (int)(p.mnId % 2), 9);
            }
        for (World* W : {&A, &B})
            for (MapLine& l : W->mls) {
                if (l.mbBad || l.mnId % 4 != (unsigned long)round % 4) continue;
                l.mnFound += 5;
                if (W == &A) T.Increased(&l, 5, 0);
            }
        for (World* W : {&A, &B})
            for (size_t k = (size_t)round; k < W->mps.size(); k += 13) W->recentPoints.push_back(&W->mps[k]);
    }
    int64_t st[8];
    drfe_lmap_recent_cull_stats(T.db(), st);
    if (st[2] != (device ? st[0] : 0)) return fail("the calls ran on the wrong entry", (long)st[2], (long)st[0]);
    std::printf("recent_cull_caller ok (%s, %d calls, %ld culled, %ld entries nulled)\n", device ? "device" : "host", calls, culled, (long)st[7]);
    return culled > 50 && st[7] > 50 ? 0 : fail("too little happened", culled, (long)st[7]);
}

}  // namespace recent_world

#ifndef RECENT_CULL_CALLER_NO_MAIN
int main(int argc, char** argv)
{
    const bool device = argc > 1 && std::string(argv[1]) == "device";
    try {
        return recent_world::run(device);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "recent_cull_caller: %s\n", e.what());
        return 1;
    }
}
#endif
