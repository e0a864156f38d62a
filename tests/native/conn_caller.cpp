/* conn_caller.cpp — Planar_SLAM::LocalMapTracker::UpdateConnections of include/drfe_adaptor.hpp next to a restatement of
 * KeyFrame::UpdateConnections, AddConnection and UpdateBestCovisibles, written here over stand-in classes with the reference's
 * members: a real std::map<KeyFrame*, int> of weights and a std::set<KeyFrame*> of children, both walked in pointer order.
 *
 *   conn_caller [host | device]
 *
 * Two worlds are built from the same description, so that pointer order is the same in both: the restatement runs on one, the
 * adaptor on the other, and the weights, ordered lists with their weights, parents, children and first-connection flags of every
 * key frame must come out equal (by mnId) after 40 single calls, an edit of rows and points, and one call of 30 key frames. */
#include "drfe_adaptor.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace {

struct KeyFrame;

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
    bool isBad() const { return false; }
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
    bool mbFirstConnection = true;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    std::vector<MapPoint*> mvpMapPoints;

    bool isBad() const { return mbBad; }
    KeyFrame* GetParent() const { return mpParent; }
    std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
    void AddChild(KeyFrame* pKF) { mspChildrens.insert(pKF); }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) const
    {
        return (int)mvpOrderedConnectedKeyFrames.size() < N
                   ? mvpOrderedConnectedKeyFrames
                   : std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    std::vector<MapLine*> GetMapLineMatches() const { return std::vector<MapLine*>(); }
    std::set<KeyFrame*> GetConnectedKeyFrames() const
    {
        std::set<KeyFrame*> s;
        for (const auto& e : mConnectedKeyFrameWeights) s.insert(e.first);
        return s;
    }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return mvpOrderedConnectedKeyFrames; }
    int GetWeight(KeyFrame* pKF) const
    {
        const auto it = mConnectedKeyFrameWeights.find(pKF);
        return it == mConnectedKeyFrameWeights.end() ? 0 : it->second;
    }
    /* the setter the integrator adds */
    void SetConnections(const std::map<KeyFrame*, int>& weights, const std::vector<KeyFrame*>& ordered, const std::vector<int>& orderedWeights,
                        KeyFrame* parent, bool firstConnection)
    {
        mConnectedKeyFrameWeights = weights; mvpOrderedConnectedKeyFrames = ordered; mvOrderedWeights = orderedWeights;
        mpParent = parent; mbFirstConnection = firstConnection;
    }

    /* ---- the restatement ---- */
    void UpdateBestCovisibles()
    {
        std::vector<std::pair<int, KeyFrame*>> byWeight;
        for (const auto& e : mConnectedKeyFrameWeights) byWeight.push_back(std::make_pair(e.second, e.first));
        std::sort(byWeight.begin(), byWeight.end());
        mvpOrderedConnectedKeyFrames.clear();
        mvOrderedWeights.clear();
        for (size_t i = byWeight.size(); i-- > 0;) {
            mvpOrderedConnectedKeyFrames.push_back(byWeight[i].second);
            mvOrderedWeights.push_back(byWeight[i].first);
        }
    }
    void AddConnection(KeyFrame* pKF, int weight)
    {
        const auto it = mConnectedKeyFrameWeights.find(pKF);
        if (it == mConnectedKeyFrameWeights.end())
            mConnectedKeyFrameWeights[pKF] = weight;
        else if (it->second != weight)
            it->second = weight;
        else
            return;
        UpdateBestCovisibles();
    }
    void UpdateConnections()
    {
        std::map<KeyFrame*, int> counter;
        for (MapPoint* pMP : mvpMapPoints) {
            if (!pMP || pMP->isBad()) continue;
            for (const auto& o : pMP->mObservations) {
                if (o.first->mnId == mnId) continue;
                counter[o.first]++;
            }
        }
        if (counter.empty()) return;
        int nmax = 0;
        KeyFrame* pKFmax = nullptr;
        std::vector<std::pair<int, KeyFrame*>> listed;
        for (const auto& c : counter) {
            if (c.second > nmax) {
                nmax = c.second;
                pKFmax = c.first;
            }
            if (c.second >= DRFE_LMAP_CONNECT_TH) {
                listed.push_back(std::make_pair(c.second, c.first));
                c.first->AddConnection(this, c.second);
            }
        }
        if (listed.empty()) {
            listed.push_back(std::make_pair(nmax, pKFmax));
            pKFmax->AddConnection(this, nmax);
        }
        std::sort(listed.begin(), listed.end());
        mConnectedKeyFrameWeights = counter;
        mvpOrderedConnectedKeyFrames.clear();
        mvOrderedWeights.clear();
        for (size_t i = listed.size(); i-- > 0;) {
            mvpOrderedConnectedKeyFrames.push_back(listed[i].second);
            mvOrderedWeights.push_back(listed[i].first);
        }
        if (mbFirstConnection && mnId != 0) {
            mpParent = mvpOrderedConnectedKeyFrames.front();
            mpParent->AddChild(this);
            mbFirstConnection = false;
        }
    }
};

using Tracker = Planar_SLAM::LocalMapTracker<KeyFrame, MapPoint, MapLine, Frame>;

struct Rng {
    uint64_t s;
    int below(int n)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((s >> 33) % (uint64_t)n);
    }
};

/* key frames share points with their neighbours in index order, so pairs pass, meet and miss the threshold */
struct Description {
    std::vector<long unsigned int> kfId;
    std::vector<int> kfBad, mpBad;
    std::vector<std::vector<int>> kfPoints, obs;
};

Description seeded(uint64_t seed, int nKf, int row)
{
    Rng r{seed};
    Description D;
    std::vector<int> ids(nKf);
    for (int i = 0; i < nKf; i++) ids[i] = i;
    for (int i = nKf - 1; i > 0; i--) std::swap(ids[i], ids[r.below(i + 1)]);
    D.kfPoints.resize(nKf);
    for (int i = 0; i < nKf; i++) {
        D.kfId.push_back((long unsigned int)ids[i]);
        D.kfBad.push_back(r.below(8) == 0);
    }
    for (int i = 0; i < nKf; i++)
        for (int k = 0; k < row; k++) {
            std::set<int> o;
            o.insert(i);
            for (int j = r.below(5); j > 0; j--) o.insert(std::min(nKf - 1, std::max(0, i - 4 + r.below(9))));
            const int p = (int)D.obs.size();
            D.obs.push_back(std::vector<int>(o.begin(), o.end()));
            D.mpBad.push_back(r.below(20) == 0);
            for (int kf : o)
                if ((int)D.kfPoints[kf].size() < (kf % 7 == 3 ? 12 : row)) D.kfPoints[kf].push_back(r.below(20) ? p : -1);   /* some short rows: the fallback */
        }
    return D;
}

struct World {
    std::vector<KeyFrame> kf;
    std::vector<MapPoint> mp;
    explicit World(const Description& D) : kf(D.kfId.size()), mp(D.mpBad.size())
    {
        for (size_t i = 0; i < mp.size(); i++) {
            mp[i].mnId = 100 + i;
            mp[i].mbBad = D.mpBad[i] != 0;
            for (int k : D.obs[i]) mp[i].mObservations[&kf[(size_t)k]] = 0;
        }
        for (size_t i = 0; i < kf.size(); i++) {
            kf[i].mnId = D.kfId[i];
            kf[i].mbBad = D.kfBad[i] != 0;
            for (int p : D.kfPoints[i]) kf[i].mvpMapPoints.push_back(p >= 0 ? &mp[(size_t)p] : nullptr);
        }
    }
};

int failures = 0;

typedef std::vector<long> Flat;

/* everything UpdateConnections writes, of every key frame, by mnId */
Flat state(const World& W)
{
    Flat f;
    for (const KeyFrame& k : W.kf) {
        f.push_back(-1000 - (long)k.mnId);
        for (const auto& e : k.mConnectedKeyFrameWeights) {
            f.push_back((long)e.first->mnId);
            f.push_back(e.second);
        }
        f.push_back(-2);
        for (size_t i = 0; i < k.mvpOrderedConnectedKeyFrames.size(); i++) {
            f.push_back((long)k.mvpOrderedConnectedKeyFrames[i]->mnId);
            f.push_back(i < k.mvOrderedWeights.size() ? k.mvOrderedWeights[i] : -7);
        }
        f.push_back(-3);
        f.push_back(k.mpParent ? (long)k.mpParent->mnId : -1);
        for (KeyFrame* c : k.mspChildrens) f.push_back((long)c->mnId);
        f.push_back(k.mbFirstConnection && k.mnId != 0 ? 1 : 0);
    }
    return f;
}

void same(const char* when, int step, const World& A, const World& B)
{
    if (state(A) == state(B)) return;
    failures++;
    fprintf(stderr, "conn_caller: %s %d: the two worlds differ\n", when, step);
}

void run(const std::string& mode, int64_t* deviceCalls, int* listedMany, int* fallbacks)
{
    const Description D = seeded(77, 60, 70);
    World A(D), B(D);
    Tracker tracker(mode == "device" ? 0 : -1);
    tracker.UseDevice(mode == "device");
    for (KeyFrame& k : B.kf) {
        tracker.Sync(&k);
        tracker.SyncConnections(&k);
    }
    for (MapPoint& p : B.mp) tracker.Sync(&p);
    Rng r{5};
    const int nKf = (int)A.kf.size();
    for (int s = 0; s < 40; s++) {
        const int i = r.below(nKf);
        A.kf[(size_t)i].UpdateConnections();
        tracker.UpdateConnections(&B.kf[(size_t)i]);
        same("single call", s, A, B);
        const size_t listed = A.kf[(size_t)i].mvpOrderedConnectedKeyFrames.size();
        if (listed > 1) ++*listedMany;
        if (listed == 1 && A.kf[(size_t)i].mvOrderedWeights[0] < DRFE_LMAP_CONNECT_TH) ++*fallbacks;
    }
    /* an edit in both worlds: rows lose entries, points turn bad or lose an observation; the points are synced, the rows are
     * synced by the call that names their key frame */
    for (int e = 0; e < 12; e++) {
        const size_t i = (size_t)r.below(nKf);
        if (A.kf[i].mvpMapPoints.size() > 10) {
            A.kf[i].mvpMapPoints.resize(A.kf[i].mvpMapPoints.size() - 9);
            B.kf[i].mvpMapPoints.resize(B.kf[i].mvpMapPoints.size() - 9);
        }
        const size_t p = (size_t)r.below((int)A.mp.size());
        A.mp[p].mbBad = B.mp[p].mbBad = true;
        tracker.Sync(&B.mp[p]);
        const size_t q = (size_t)r.below((int)A.mp.size());
        if (A.mp[q].mObservations.size() > 1) {
            A.mp[q].mObservations.erase(A.mp[q].mObservations.begin());
            B.mp[q].mObservations.erase(B.mp[q].mObservations.begin());
            tracker.Sync(&B.mp[q]);
        }
    }
    std::vector<int> order(nKf);
    for (int i = 0; i < nKf; i++) order[(size_t)i] = i;
    for (int i = nKf - 1; i > 0; i--) std::swap(order[(size_t)i], order[(size_t)r.below(i + 1)]);
    std::vector<KeyFrame*> batch;
    for (int k = 0; k < 30; k++) {
        A.kf[(size_t)order[(size_t)k]].UpdateConnections();
        batch.push_back(&B.kf[(size_t)order[(size_t)k]]);
    }
    const std::vector<std::set<KeyFrame*>> connected = tracker.UpdateConnections(batch);
    same("the call of", 30, A, B);
    if (connected.size() != 30) failures++;
    int64_t st[8];
    if (drfe_lmap_connect_stats(tracker.db(), st) != DRFE_OK) throw std::runtime_error("drfe_lmap_connect_stats failed");
    if (st[0] != 41 || st[1] != 70) failures++;
    *deviceCalls += st[2];
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    try {
        int64_t deviceCalls = 0;
        int listedMany = 0, fallbacks = 0;
        run(mode, &deviceCalls, &listedMany, &fallbacks);
        if (!listedMany || !fallbacks) {
            fprintf(stderr, "conn_caller: the seeded world took only one branch (%d listed, %d fallbacks)\n", listedMany, fallbacks);
            return 1;
        }
        if (failures) return 1;
        printf("conn_caller ok (%s, 40 single calls, 1 call of 30, device calls %lld)\n", mode.c_str(), (long long)deviceCalls);
    } catch (const std::exception& e) {
        fprintf(stderr, "conn_caller: %s\n", e.what());
        return 2;
    }
    return 0;
}
