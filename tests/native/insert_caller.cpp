/* insert_caller.cpp — Planar_SLAM::LocalMapTracker::ProcessNewKeyFrame of include/drfe_adaptor.hpp (one key frame, and a queue of
 * them) over stand-in classes with the reference's members: a real std::map<KeyFrame*, size_t> of observations with the nObs
 * counter per map point and map line, AddObservation as the reference has it (src/MapPoint.cc:124-138, src/MapLine.cpp:91-100),
 * key frames with a pose, key points with octaves and the stereo coordinate.
 *
 *   insert_caller [host | device]
 *
 * Two equal worlds are built.  On the first the adaptor's methods run: the store decides and commits, then the rows are walked
 * and the objects' own AddObservation called.  On the second the reference's loop (src/LocalMapping.cc:124-157) runs on the
 * objects alone, with UpdateNormalAndDepth (src/MapPoint.cc:370-417) written out in its float and double steps.  After every
 * call the two worlds must be equal (observations, nObs, the recent lists), the returned records must be the second world's
 * normals and distances bit for bit, and the store must hold the observers of the first world's items in their map order.  A
 * second call of the same key frames then finds nothing to add. */
#include "drfe_adaptor.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace insert_world {

#define REQUIRE(c)                                                                \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::printf("insert_caller: %s failed at line %d\n", #c, __LINE__);   \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

/* what the adaptor reads of a cv::Mat */
struct Mat {
    int cols = 1;
    std::vector<float> v;
    template <class T> const T* ptr(int r) const { return &v[(size_t)(r * cols)]; }
};

struct KeyPoint {
    int octave = 0;
};

struct MapPoint;
struct MapLine;

struct KeyFrame {
    long unsigned int mnId = 0;
    bool mbBad = false;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    float mThDepth = 40.0f;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvDepth, mvuRight, mvScaleFactors;
    int mnScaleLevels = 3;
    float Ow[3] = {0, 0, 0};
    bool isBad() const { return mbBad; }
    KeyFrame* GetParent() const { return mpParent; }
    std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int&) const { return std::vector<KeyFrame*>(); }
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    std::vector<MapLine*> GetMapLineMatches() const { return mvpMapLines; }
    bool GetNotErase() const { return false; }
    bool GetToBeErased() const { return false; }
    /* the identity rotation and tcw = -Ow */
    Mat GetPose() const
    {
        Mat T;
        T.cols = 4;
        T.v = {1, 0, 0, -Ow[0], 0, 1, 0, -Ow[1], 0, 0, 1, -Ow[2], 0, 0, 0, 1};
        return T;
    }
};

struct Item {
    long unsigned int mnId = 0;
    long int mnFirstKFid = 0;
    bool mbBad = false;
    int nObs = 0, mnFound = 1, mnVisible = 1;
    std::map<KeyFrame*, size_t> mObservations;
    bool isBad() const { return mbBad; }
    int Observations() const { return nObs; }
    int GetFound() const { return mnFound; }
    int GetVisible() const { return mnVisible; }
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
    bool IsInKeyFrame(KeyFrame* pKF) const { return mObservations.count(pKF) != 0; }
};

struct MapPoint : Item {
    float X[3] = {0, 0, 0};
    KeyFrame* mpRefKF = nullptr;
    int refLevel = 0;                  /* the octave of the reference key frame's key point when the geometry was synced */
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    float normal[3] = {0, 0, 0}, maxD = 0, minD = 0;
    Mat GetWorldPos() const
    {
        Mat P;
        P.v = {X[0], X[1], X[2]};
        return P;
    }
    KeyFrame* GetReferenceKeyFrame() const { return mpRefKF; }
    void AddObservation(KeyFrame* pKF, size_t idx)
    {
        if (mObservations.count(pKF)) return;
        mObservations[pKF] = idx;
        nObs += pKF->mvuRight[idx] >= 0 ? 2 : 1;
    }
    /* src/MapPoint.cc:370-417: cv::norm is the double sum of squares in order, the MatExpr scales are floats */
    void UpdateNormalAndDepth()
    {
        float nrm[3] = {0, 0, 0};
        int n = 0;
        for (const auto& o : mObservations) {
            const float v[3] = {X[0] - o.first->Ow[0], X[1] - o.first->Ow[1], X[2] - o.first->Ow[2]};
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
            const float a = (float)(1.0 / std::sqrt(s));
            for (int k = 0; k < 3; k++) nrm[k] = v[k] * a + nrm[k];
            n++;
        }
        const float c[3] = {X[0] - mpRefKF->Ow[0], X[1] - mpRefKF->Ow[1], X[2] - mpRefKF->Ow[2]};
        double s = 0.0;
        for (int k = 0; k < 3; k++) s += (double)c[k] * (double)c[k];
        const float dist = (float)std::sqrt(s);
        maxD = dist * mpRefKF->mvScaleFactors[(size_t)refLevel];
        minD = maxD / mpRefKF->mvScaleFactors[(size_t)mpRefKF->mnScaleLevels - 1];
        const float a = (float)(1.0 / (double)n);
        for (int k = 0; k < 3; k++) normal[k] = nrm[k] * a;
    }
};

struct MapLine : Item {
    void AddObservation(KeyFrame* pKF, size_t idx)
    {
        if (mObservations.count(pKF)) return;
        mObservations[pKF] = idx;
        nObs++;
    }
};

struct Frame {
    long unsigned int mnId = 0;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    void* mpReferenceKF = nullptr;
};

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

const int ROW = 16, LROW = 6;

/* key frames under key frame 0 with rows of ROW points and LROW lines; items seen by 0 .. 4 of them; then what tracking leaves:
 * row entries that name items which do not observe the key frame, now and then one twice, one that observes it elsewhere */
struct World {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
    std::vector<MapLine> mls;
    std::list<MapPoint*> recentPoints;
    std::list<MapLine*> recentLines;

    template <class ItemT, class Row> void fill(std::vector<ItemT>& items, Row row, Rng& R)
    {
        for (size_t i = 0; i < items.size(); i++) {
            ItemT& p = items[i];
            p.mnId = (long unsigned int)i;
            const int nSeen = R.below(5);
            for (int k = 0; k < nSeen; k++) {
                KeyFrame* pKF = &kfs[(size_t)R.below((int)kfs.size())];
                const size_t idx = (size_t)R.below((int)(pKF->*row).size());
                if (p.mObservations.count(pKF) || (pKF->*row)[idx]) continue;
                (pKF->*row)[idx] = &p;
                p.AddObservation(pKF, idx);
            }
            if (R.below(10) == 0) p.mbBad = true;
        }
        for (KeyFrame& k : kfs)
            for (size_t i = 0; i < (k.*row).size(); i++)
                if (!(k.*row)[i] && R.below(2)) (k.*row)[i] = &items[(size_t)R.below((int)items.size())];
    }

    World(int nKf, int nMp, int nMl, uint64_t seed) : kfs((size_t)nKf), mps((size_t)nMp), mls((size_t)nMl)
    {
        Rng R(seed);
        for (int k = 0; k < nKf; k++) {
            KeyFrame& K = kfs[(size_t)k];
            K.mnId = (long unsigned int)k;
            if (k) {
                K.mpParent = &kfs[0];
                kfs[0].mspChildrens.insert(&K);
            }
            K.mvpMapPoints.assign((size_t)ROW, nullptr);
            K.mvpMapLines.assign((size_t)LROW, nullptr);
            K.mvKeysUn.resize((size_t)ROW);
            for (int i = 0; i < ROW; i++) {
                K.mvKeysUn[(size_t)i].octave = R.below(3);
                K.mvDepth.push_back(1.0f);
                K.mvuRight.push_back(R.below(2) ? 1.0f : -1.0f);
            }
            K.mvScaleFactors = {1.0f, 1.2f, 1.44f};
            K.Ow[0] = 0.25f * (float)R.below(9);
            K.Ow[1] = 0.5f * (float)R.below(5);
            K.Ow[2] = -0.125f * (float)R.below(4);
        }
        fill(mps, &KeyFrame::mvpMapPoints, R);
        fill(mls, &KeyFrame::mvpMapLines, R);
        for (MapPoint& p : mps) {
            for (int k = 0; k < 3; k++) p.X[k] = 0.5f * (float)R.below(17) + 0.125f;
            p.X[2] += 3.0f;
            p.mpRefKF = p.mObservations.empty() ? &kfs[(size_t)R.below(nKf)] : p.mObservations.begin()->first;
            const auto f = p.mObservations.find(p.mpRefKF);
            p.refLevel = p.mpRefKF->mvKeysUn[f == p.mObservations.end() ? (size_t)0 : f->second].octave;
        }
    }

    void sync(Tracker& T)
    {
        for (KeyFrame& k : kfs) {
            T.Sync(&k);
            T.SyncCulling(&k);
            T.SyncGeometry(&k);
        }
        for (MapPoint& p : mps) {
            T.Sync(&p);
            T.SyncCulling(&p);
            T.SyncRecent(&p);
            T.SyncGeometry(&p);
        }
        for (MapLine& l : mls) {
            T.Sync(&l);
            T.SyncRecent(&l);
        }
    }

    /* src/LocalMapping.cc:124-157 on the objects alone; returns the added points with their normals, in walk order */
    std::vector<MapPoint> reference(KeyFrame* pKF, bool normals)
    {
        std::vector<MapPoint> out;
        const std::vector<MapPoint*> vpMapPointMatches = pKF->GetMapPointMatches();
        for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
            MapPoint* pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            if (!pMP->IsInKeyFrame(pKF)) {
                pMP->AddObservation(pKF, i);
                if (normals) pMP->UpdateNormalAndDepth();
                out.push_back(*pMP);
            } else {
                recentPoints.push_back(pMP);
            }
        }
        const std::vector<MapLine*> vpMapLineMatches = pKF->GetMapLineMatches();
        for (size_t i = 0; i < vpMapLineMatches.size(); i++) {
            MapLine* pML = vpMapLineMatches[i];
            if (!pML || pML->isBad()) continue;
            if (!pML->IsInKeyFrame(pKF)) pML->AddObservation(pKF, i);
            else recentLines.push_back(pML);
        }
        return out;
    }
};

template <class ItemT> std::vector<std::pair<long unsigned int, size_t>> obs_of(const ItemT& p)
{
    std::vector<std::pair<long unsigned int, size_t>> o;
    for (const auto& e : p.mObservations) o.emplace_back(e.first->mnId, e.second);
    return o;
}

template <class ItemT> std::vector<long unsigned int> ids_of(const std::list<ItemT*>& l)
{
    std::vector<long unsigned int> o;
    for (ItemT* p : l) o.push_back(p->mnId);
    return o;
}

void same_worlds(const World& A, const World& B)
{
    for (size_t i = 0; i < A.mps.size(); i++) REQUIRE(obs_of(A.mps[i]) == obs_of(B.mps[i]) && A.mps[i].nObs == B.mps[i].nObs);
    for (size_t i = 0; i < A.mls.size(); i++) REQUIRE(obs_of(A.mls[i]) == obs_of(B.mls[i]) && A.mls[i].nObs == B.mls[i].nObs);
    REQUIRE(ids_of(A.recentPoints) == ids_of(B.recentPoints) && ids_of(A.recentLines) == ids_of(B.recentLines));
}

/* the store's observers of every item of A, in the map's order */
void store_holds(Tracker& T, const World& A)
{
    std::vector<int32_t> out(64);
    for (int kind = 0; kind < 2; kind++)
        for (size_t i = 0; i < (kind ? A.mls.size() : A.mps.size()); i++) {
            const Item& p = kind ? static_cast<const Item&>(A.mls[i]) : static_cast<const Item&>(A.mps[i]);
            uint8_t bad = 0;
            int32_t n = 0;
            REQUIRE(drfe_lmap_get_observers(T.db(), kind ? DRFE_LMAP_LINE : DRFE_LMAP_POINT, (int32_t)p.mnId, (int32_t)out.size(), &bad, &n, out.data()) == DRFE_OK);
            REQUIRE((bad != 0) == p.mbBad && (size_t)n == p.mObservations.size());
            size_t t = 0;
            for (const auto& e : p.mObservations) REQUIRE(out[t++] == (int32_t)e.first->mnId);
        }
}

int run(bool device, uint64_t seed, bool queue, bool normals)
{
    World A(10, 60, 20, seed), B(10, 60, 20, seed);
    Tracker T(device ? 0 : -1);
    T.UseDevice(device);
    A.sync(T);
    Rng R(seed + 99);
    std::vector<size_t> order;
    for (size_t k = 0; k < A.kfs.size(); k++) order.push_back(k);
    for (size_t k = order.size(); k > 1; k--) std::swap(order[k - 1], order[(size_t)R.below((int)k)]);
    order.resize(6);
    int added = 0;
    std::vector<drfe::MapPointUpkeep> got;
    std::vector<MapPoint> want;
    std::vector<MapPoint*> addedPoints;
    if (queue) {
        std::vector<KeyFrame*> called;
        for (const size_t k : order) called.push_back(&A.kfs[k]);
        got = T.ProcessNewKeyFrame(called, A.recentPoints, A.recentLines, normals, &addedPoints);
        for (const size_t k : order) {
            const std::vector<MapPoint> w = B.reference(&B.kfs[k], normals);
            want.insert(want.end(), w.begin(), w.end());
        }
    } else {
        for (const size_t k : order) {
            std::vector<MapPoint*> some;
            const std::vector<drfe::MapPointUpkeep> g = T.ProcessNewKeyFrame(&A.kfs[k], A.recentPoints, A.recentLines, normals, &some);
            got.insert(got.end(), g.begin(), g.end());
            addedPoints.insert(addedPoints.end(), some.begin(), some.end());
            const std::vector<MapPoint> w = B.reference(&B.kfs[k], normals);
            want.insert(want.end(), w.begin(), w.end());
        }
    }
    REQUIRE(got.size() == want.size() && addedPoints.size() == want.size());
    for (size_t t = 0; t < got.size(); t++) {
        REQUIRE(addedPoints[t]->mnId == want[t].mnId);
        REQUIRE(got[t].status == (normals ? DRFE_UPKEEP_NORMAL : 0));
        if (!normals) continue;
        REQUIRE(std::memcmp(got[t].normal, want[t].normal, sizeof(want[t].normal)) == 0);
        REQUIRE(std::memcmp(&got[t].max_distance, &want[t].maxD, sizeof(float)) == 0);
        REQUIRE(std::memcmp(&got[t].min_distance, &want[t].minD, sizeof(float)) == 0);
        added++;
    }
    same_worlds(A, B);
    store_holds(T, A);
    /* again: everything that was added is recent now */
    const size_t before = A.recentPoints.size();
    std::vector<KeyFrame*> called;
    for (const size_t k : order) called.push_back(&A.kfs[k]);
    REQUIRE(T.ProcessNewKeyFrame(called, A.recentPoints, A.recentLines, normals).empty());
    REQUIRE(A.recentPoints.size() >= before + want.size());
    store_holds(T, A);
    int64_t st[8];
    REQUIRE(drfe_lmap_insert_stats(T.db(), st) == DRFE_OK);
    REQUIRE(st[3] == (int64_t)want.size() && st[2] == (device ? st[0] : 0));
    return (int)want.size();
}

}  // namespace insert_world

int main(int argc, char** argv)
{
    const bool device = argc > 1 && std::string(argv[1]) == "device";
    int added = 0;
    try {
        for (uint64_t seed = 1; seed <= 6; seed++)
            for (int queue = 0; queue < 2; queue++) added += insert_world::run(device, seed, queue != 0, seed % 3 != 0);
    } catch (const std::exception& e) {
        std::printf("insert_caller: %s\n", e.what());
        return 1;
    }
    if (added < 100) {
        std::printf("insert_caller: only %d points added\n", added);
        return 1;
    }
    std::printf("insert_caller %s: ok, %d points added\n", device ? "device" : "host", added);
    return 0;
}
