/* lmap_caller.cpp — Planar_SLAM::LocalMapTracker of include/drfe_adaptor.hpp next to a literal copy of the three loops of
 * Tracking::UpdateLocalMap (UpdateLocalKeyFrames, UpdateLocalPoints, UpdateLocalLines), written here over stand-in classes with
 * the reference's accessors: a std::map<KeyFrame*, int> counter and a std::set<KeyFrame*> of children walked in pointer order,
 * mnTrackReferenceForFrame stamps compared with the frame's id.
 *
 *   lmap_caller [host | device]
 *
 * Two worlds are built from the same description, so that pointer order is the same in both: the loops run on one, the adaptor
 * on the other, and the lists (by mnId), the reference key frame, the frame's nulled points and every stamp must come out equal.
 * Worlds: a seeded random graph with 40 frames one after another and then 8 frames in one batch call, and two hand-built ones
 * (a vote tie that the lowest address wins; the parent's break that ends the whole expansion). */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace {

struct MapPoint;
struct MapLine;

struct KeyFrame {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    bool mbBad = false;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    bool isBad() const { return mbBad; }
    KeyFrame* GetParent() const { return mpParent; }
    std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) const
    {
        return (int)mvpOrderedConnectedKeyFrames.size() < N
                   ? mvpOrderedConnectedKeyFrames
                   : std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    std::vector<MapLine*> GetMapLineMatches() const { return mvpMapLines; }
};

struct MapPoint {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    bool isBad() const { return mbBad; }
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
};

struct MapLine {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    bool mbBad = false;
    bool isBad() const { return mbBad; }
};

struct Frame {
    long unsigned int mnId = 0;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    KeyFrame* mpReferenceKF = nullptr;
};

/* Tracking's members that UpdateLocalMap touches, and its three loops */
struct Tracking {
    Frame mCurrentFrame;
    std::vector<KeyFrame*> mvpLocalKeyFrames;
    std::vector<MapPoint*> mvpLocalMapPoints;
    std::vector<MapLine*> mvpLocalMapLines;
    KeyFrame* mpReferenceKF = nullptr;

    void UpdateLocalMap()
    {
        UpdateLocalKeyFrames();
        UpdateLocalPoints();
        UpdateLocalLines();
    }
    void UpdateLocalKeyFrames()
    {
        std::map<KeyFrame*, int> keyframeCounter;
        for (size_t i = 0; i < mCurrentFrame.mvpMapPoints.size(); i++) {
            MapPoint* pMP = mCurrentFrame.mvpMapPoints[i];
            if (!pMP) continue;
            if (!pMP->isBad()) {
                const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
                for (const auto& o : observations) keyframeCounter[o.first]++;
            } else {
                mCurrentFrame.mvpMapPoints[i] = nullptr;
            }
        }
        if (keyframeCounter.empty()) return;
        int max = 0;
        KeyFrame* pKFmax = nullptr;
        mvpLocalKeyFrames.clear();
        mvpLocalKeyFrames.reserve(3 * keyframeCounter.size());
        for (const auto& c : keyframeCounter) {
            KeyFrame* pKF = c.first;
            if (pKF->isBad()) continue;
            if (c.second > max) {
                max = c.second;
                pKFmax = pKF;
            }
            mvpLocalKeyFrames.push_back(pKF);
            pKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
        }
        const size_t listed = mvpLocalKeyFrames.size();      /* itEndKF, taken before any push */
        for (size_t it = 0; it < listed; it++) {
            if (mvpLocalKeyFrames.size() > 80) break;
            KeyFrame* pKF = mvpLocalKeyFrames[it];
            const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
            for (KeyFrame* pNeighKF : vNeighs) {
                if (!pNeighKF->isBad()) {
                    if (pNeighKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                        mvpLocalKeyFrames.push_back(pNeighKF);
                        pNeighKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                        break;
                    }
                }
            }
            const std::set<KeyFrame*> spChilds = pKF->GetChilds();
            for (KeyFrame* pChildKF : spChilds) {
                if (!pChildKF->isBad()) {
                    if (pChildKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                        mvpLocalKeyFrames.push_back(pChildKF);
                        pChildKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                        break;
                    }
                }
            }
            KeyFrame* pParent = pKF->GetParent();
            if (pParent) {
                if (pParent->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pParent);
                    pParent->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;
                }
            }
        }
        if (pKFmax) {
            mpReferenceKF = pKFmax;
            mCurrentFrame.mpReferenceKF = mpReferenceKF;
        }
    }
    void UpdateLocalPoints()
    {
        mvpLocalMapPoints.clear();
        for (KeyFrame* pKF : mvpLocalKeyFrames) {
            const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
            for (MapPoint* pMP : vpMPs) {
                if (!pMP) continue;
                if (pMP->mnTrackReferenceForFrame == mCurrentFrame.mnId) continue;
                if (!pMP->isBad()) {
                    mvpLocalMapPoints.push_back(pMP);
                    pMP->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                }
            }
        }
    }
    void UpdateLocalLines()
    {
        mvpLocalMapLines.clear();
        for (KeyFrame* pKF : mvpLocalKeyFrames) {
            const std::vector<MapLine*> vpMLs = pKF->GetMapLineMatches();
            for (MapLine* pML : vpMLs) {
                if (!pML) continue;
                if (pML->mnTrackReferenceForFrame == mCurrentFrame.mnId) continue;
                if (!pML->isBad()) {
                    mvpLocalMapLines.push_back(pML);
                    pML->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                }
            }
        }
    }
};

using Tracker = Planar_SLAM::LocalMapTracker<KeyFrame, MapPoint, MapLine, Frame>;

/* a graph by index; a world is its objects.  Key frame i has mnId kfId[i], so address order and id order differ. */
struct Description {
    std::vector<long unsigned int> kfId;
    std::vector<int> kfBad, parent;
    std::vector<std::vector<int>> nbr, children, kfPoints, kfLines, obs;
    std::vector<int> mpBad, mlBad;
    std::vector<std::vector<int>> framePoints, frameLines;
};

struct World {
    std::vector<KeyFrame> kf;
    std::vector<MapPoint> mp;
    std::vector<MapLine> ml;
    explicit World(const Description& D) : kf(D.kfId.size()), mp(D.mpBad.size()), ml(D.mlBad.size())
    {
        for (size_t i = 0; i < mp.size(); i++) {
            mp[i].mnId = 100 + i;
            mp[i].mbBad = D.mpBad[i] != 0;
            for (int k : D.obs[i]) mp[i].mObservations[&kf[(size_t)k]] = 0;
        }
        for (size_t i = 0; i < ml.size(); i++) {
            ml[i].mnId = 500 + i;
            ml[i].mbBad = D.mlBad[i] != 0;
        }
        for (size_t i = 0; i < kf.size(); i++) {
            kf[i].mnId = D.kfId[i];
            kf[i].mbBad = D.kfBad[i] != 0;
            kf[i].mpParent = D.parent[i] >= 0 ? &kf[(size_t)D.parent[i]] : nullptr;
            for (int k : D.nbr[i]) kf[i].mvpOrderedConnectedKeyFrames.push_back(&kf[(size_t)k]);
            for (int k : D.children[i]) kf[i].mspChildrens.insert(&kf[(size_t)k]);
            for (int p : D.kfPoints[i]) kf[i].mvpMapPoints.push_back(p >= 0 ? &mp[(size_t)p] : nullptr);
            for (int l : D.kfLines[i]) kf[i].mvpMapLines.push_back(l >= 0 ? &ml[(size_t)l] : nullptr);
        }
    }
    Frame frame(const Description& D, size_t f, long unsigned int id)
    {
        Frame F;
        F.mnId = id;
        for (int p : D.framePoints[f]) F.mvpMapPoints.push_back(p >= 0 ? &mp[(size_t)p] : nullptr);
        for (int l : D.frameLines[f]) F.mvpMapLines.push_back(l >= 0 ? &ml[(size_t)l] : nullptr);
        return F;
    }
};

struct Rng {
    uint64_t s;
    int below(int n)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((s >> 33) % (uint64_t)n);
    }
};

Description seeded(uint64_t seed, int nKf, int nMp, int nMl, int nFrames)
{
    Rng r{seed};
    Description D;
    std::vector<int> ids(nKf);
    for (int i = 0; i < nKf; i++) ids[i] = i + 1;
    for (int i = nKf - 1; i > 0; i--) std::swap(ids[i], ids[r.below(i + 1)]);
    auto some = [&](int n, int range, int nullOneIn) {
        std::vector<int> v;
        for (int i = 0; i < n; i++) v.push_back(nullOneIn && r.below(nullOneIn) == 0 ? -1 : r.below(range));
        return v;
    };
    auto distinct = [&](int n, int range, int skip) {
        std::set<int> seen;
        std::vector<int> v;
        for (int i = 0; i < n; i++) {
            const int k = r.below(range);
            if (k != skip && seen.insert(k).second) v.push_back(k);
        }
        return v;
    };
    for (int i = 0; i < nKf; i++) {
        D.kfId.push_back((long unsigned int)ids[i]);
        D.kfBad.push_back(r.below(7) == 0);
        D.parent.push_back(r.below(3) ? r.below(nKf) : -1);
        if (D.parent.back() == i) D.parent.back() = -1;
        D.nbr.push_back(distinct(r.below(12), nKf, i));
        D.children.push_back(distinct(r.below(4), nKf, i));
        D.kfPoints.push_back(some(r.below(40), nMp, 5));
        D.kfLines.push_back(some(r.below(12), nMl, 5));
    }
    for (int i = 0; i < nMp; i++) {
        D.mpBad.push_back(r.below(10) == 0);
        D.obs.push_back(distinct(r.below(7), nKf, -1));
    }
    for (int i = 0; i < nMl; i++) D.mlBad.push_back(r.below(10) == 0);
    for (int f = 0; f < nFrames; f++) {
        D.framePoints.push_back(some(r.below(8) ? r.below(60) : 0, nMp, 4));
        D.frameLines.push_back(some(r.below(10), nMl, 4));
    }
    return D;
}

/* key frames 0 and 1 tie at two votes: the lower address (index 0, mnId 30) is pKFmax; the list is in address order */
Description vote_tie()
{
    Description D;
    D.kfId = {30, 10, 20};
    D.kfBad = {0, 0, 0};
    D.parent = {-1, -1, -1};
    D.nbr = D.children = {{}, {}, {}};
    D.kfPoints = {{1, 3}, {0, -1, 1}, {2, 0}};
    D.kfLines = {{}, {}, {}};
    D.mpBad = {0, 0, 0, 0};
    D.obs = {{0, 1}, {1, 0}, {2}, {}};
    D.framePoints = {{0, 1, 2}};
    D.frameLines = {{}};
    return D;
}

/* key frame 0 contributes its neighbour 2, child 3 and parent 4; the parent's break ends the expansion before key frame 1's
 * neighbour 5 is looked at; the bad parent's point 1 is listed */
Description parent_break()
{
    Description D;
    D.kfId = {1, 2, 3, 4, 5, 6};
    D.kfBad = {0, 0, 0, 0, 1, 0};
    D.parent = {4, -1, -1, -1, -1, -1};
    D.nbr = {{2}, {5}, {}, {}, {}, {}};
    D.children = {{3}, {}, {}, {}, {}, {}};
    D.kfPoints = {{0}, {}, {}, {}, {1}, {2}};
    D.kfLines = {{0}, {}, {}, {}, {0, 1}, {}};
    D.mpBad = {0, 0, 0};
    D.mlBad = {0, 0};
    D.obs = {{0, 1}, {}, {}};
    D.framePoints = {{0, -1}};
    D.frameLines = {{1}};
    return D;
}

int failures = 0;

template <class T> std::vector<long unsigned int> ids(const std::vector<T*>& v)
{
    std::vector<long unsigned int> o;
    for (T* p : v) o.push_back(p ? p->mnId : 0);
    return o;
}

void same(const char* world, size_t f, const char* what, const std::vector<long unsigned int>& a, const std::vector<long unsigned int>& b)
{
    if (a == b) return;
    failures++;
    fprintf(stderr, "lmap_caller: %s, frame %zu: %s differ (%zu / %zu entries)\n", world, f, what, a.size(), b.size());
}

template <class T> std::vector<long unsigned int> stamps(const std::vector<T>& v)
{
    std::vector<long unsigned int> o;
    for (const T& x : v) o.push_back(x.mnTrackReferenceForFrame);
    return o;
}

void compare(const char* world, size_t f, const Tracking& T, const World& A, const Frame& FB, const std::vector<KeyFrame*>& kfs,
             const std::vector<MapPoint*>& mps, const std::vector<MapLine*>& mls, KeyFrame* ref, const World& B)
{
    same(world, f, "mvpLocalKeyFrames", ids(T.mvpLocalKeyFrames), ids(kfs));
    same(world, f, "mvpLocalMapPoints", ids(T.mvpLocalMapPoints), ids(mps));
    same(world, f, "mvpLocalMapLines", ids(T.mvpLocalMapLines), ids(mls));
    same(world, f, "the frame's map points", ids(T.mCurrentFrame.mvpMapPoints), ids(FB.mvpMapPoints));
    same(world, f, "mpReferenceKF", {T.mpReferenceKF ? T.mpReferenceKF->mnId : 0, T.mCurrentFrame.mpReferenceKF ? T.mCurrentFrame.mpReferenceKF->mnId : 0},
         {ref ? ref->mnId : 0, FB.mpReferenceKF ? FB.mpReferenceKF->mnId : 0});
    same(world, f, "key-frame stamps", stamps(A.kf), stamps(B.kf));
    same(world, f, "map-point stamps", stamps(A.mp), stamps(B.mp));
    same(world, f, "map-line stamps", stamps(A.ml), stamps(B.ml));
}

/* frames [0, single) one call each, the rest in one batch call; returns the number of frames */
size_t run(const char* name, const Description& D, size_t single, const std::string& mode, int64_t* deviceCalls)
{
    World A(D), B(D);
    Tracker tracker(mode == "device" ? 0 : -1);
    tracker.UseDevice(mode == "device");
    for (KeyFrame& k : B.kf) tracker.Sync(&k);
    for (MapPoint& p : B.mp) tracker.Sync(&p);
    for (MapLine& l : B.ml) tracker.Sync(&l);
    Tracking T;
    std::vector<KeyFrame*> kfs;
    std::vector<MapPoint*> mps;
    std::vector<MapLine*> mls;
    KeyFrame* ref = nullptr;
    const size_t n = D.framePoints.size();
    for (size_t f = 0; f < single && f < n; f++) {
        T.mCurrentFrame = A.frame(D, f, 1 + f);
        T.UpdateLocalMap();
        Frame FB = B.frame(D, f, 1 + f);
        tracker.UpdateLocalMap(FB, kfs, mps, mls, ref);
        compare(name, f, T, A, FB, kfs, mps, mls, ref, B);
        if (f == 3 && n > 8) {
            /* an edit in both worlds, synced: a key frame turns bad, a point loses its observations */
            A.kf[2].mbBad = B.kf[2].mbBad = true;
            A.mp[5].mObservations.clear();
            B.mp[5].mObservations.clear();
            tracker.Sync(&B.kf[2]);
            tracker.Sync(&B.mp[5]);
        }
    }
    if (single < n) {
        /* a batched tracker: every frame with the list the frame before it left, as one tracker would see them in turn */
        std::vector<Frame> FB;
        for (size_t f = single; f < n; f++) FB.push_back(B.frame(D, f, 1 + f));
        std::vector<Frame*> frames;
        for (Frame& F : FB) frames.push_back(&F);
        std::vector<Tracker::Local> locals(frames.size());
        tracker.UpdateLocalMap(frames, locals);
        for (size_t f = single; f < n; f++) {
            /* the literal loops with an empty previous list each, as the batch's Locals had */
            T.mvpLocalKeyFrames.clear();
            T.mpReferenceKF = nullptr;
            T.mCurrentFrame = A.frame(D, f, 1 + f);
            T.UpdateLocalMap();
            const Tracker::Local& L = locals[f - single];
            same(name, f, "batch mvpLocalKeyFrames", ids(T.mvpLocalKeyFrames), ids(L.kfs));
            same(name, f, "batch mvpLocalMapPoints", ids(T.mvpLocalMapPoints), ids(L.mps));
            same(name, f, "batch mvpLocalMapLines", ids(T.mvpLocalMapLines), ids(L.mls));
            same(name, f, "batch frame points", ids(T.mCurrentFrame.mvpMapPoints), ids(FB[f - single].mvpMapPoints));
            same(name, f, "batch mpReferenceKF", {T.mpReferenceKF ? T.mpReferenceKF->mnId : 0}, {L.ref ? L.ref->mnId : 0});
        }
        same(name, n, "batch key-frame stamps", stamps(A.kf), stamps(B.kf));
        same(name, n, "batch map-point stamps", stamps(A.mp), stamps(B.mp));
        same(name, n, "batch map-line stamps", stamps(A.ml), stamps(B.ml));
    }
    int64_t st[8];
    if (drfe_lmap_stats(tracker.db(), st) != DRFE_OK) throw std::runtime_error("drfe_lmap_stats failed");
    *deviceCalls += st[2];
    return n;
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    try {
        int64_t deviceCalls = 0;
        size_t frames = run("seeded", seeded(2024, 30, 200, 40, 48), 40, mode, &deviceCalls);
        frames += run("vote_tie", vote_tie(), 1, mode, &deviceCalls);
        frames += run("parent_break", parent_break(), 1, mode, &deviceCalls);
        if (failures) return 1;
        printf("lmap_caller ok (%s, %zu frames, device calls %lld)\n", mode.c_str(), frames, (long long)deviceCalls);
    } catch (const std::exception& e) {
        fprintf(stderr, "lmap_caller: %s\n", e.what());
        return 2;
    }
    return 0;
}
