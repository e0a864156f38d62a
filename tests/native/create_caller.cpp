/* create_caller.cpp — Planar_SLAM::LocalMapTracker::CreateMapPoints / CreateMapLines of include/drfe_adaptor.hpp (the two-observer
 * form of CreateNewMapPoints and CreateNewMapLines2 and the single-observer form of CreateNewKeyFrame) over stand-in classes with
 * the reference's members: a real std::map<KeyFrame*, size_t> of observations with the nObs counter per map point and map line,
 * AddObservation as the reference has it (src/MapPoint.cc:124-138, src/MapLine.cpp:91-100), AddMapPoint / AddMapLine
 * (src/KeyFrame.cc:287-291, :849-853), key frames with a pose, key points with octaves and the stereo coordinate.
 *
 *   create_caller [host | device]
 *
 * Two equal worlds are built.  On the first the adaptor's methods run: the store creates and commits, then the objects get their
 * own AddObservation and AddMapPoint.  On the second the tail of CreateNewMapPoints (src/LocalMapping.cc:522-535) runs on the
 * objects alone, with UpdateNormalAndDepth (src/MapPoint.cc:376-417) written out in its float and double steps.  After every call
 * the two worlds must be equal (rows, observations, nObs), the returned records must be the second world's normals and distances
 * bit for bit, and the store must hold the rows and the observers of the first world in their map order.  Every call appends:
 * none leaves the store's image stale. */
#include "drfe_adaptor.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace create_world {

#define REQUIRE(c)                                                                \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::printf("create_caller: %s failed at line %d\n", #c, __LINE__);   \
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
    void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }
    void AddMapLine(MapLine* pML, const size_t& idx) { mvpMapLines[idx] = pML; }
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
    /* src/MapPoint.cc:376-417: cv::norm is the double sum of squares in order, the MatExpr scales are floats */
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
        const int level = mpRefKF->mvKeysUn[mObservations[mpRefKF]].octave;
        maxD = dist * mpRefKF->mvScaleFactors[(size_t)level];
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

const int ROW = 24, LROW = 8;

/* key frames under key frame 0 with rows of ROW points and LROW lines, a few stored items in them; created items live in deques,
 * whose elements do not move */
struct World {
    std::vector<KeyFrame> kfs;
    std::deque<MapPoint> mps;
    std::deque<MapLine> mls;

    World(int nKf, uint64_t seed) : kfs((size_t)nKf)
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
        for (int i = 0; i < 12; i++) {
            MapPoint& p = add_point(R);
            KeyFrame* pKF = &kfs[(size_t)R.below(nKf)];
            const size_t idx = (size_t)R.below(ROW);
            p.mpRefKF = pKF;
            p.AddObservation(pKF, idx);
            pKF->AddMapPoint(&p, idx);
        }
        for (int i = 0; i < 4; i++) {
            MapLine& l = add_line();
            KeyFrame* pKF = &kfs[(size_t)R.below(nKf)];
            const size_t idx = (size_t)R.below(LROW);
            l.AddObservation(pKF, idx);
            pKF->AddMapLine(&l, idx);
        }
    }

    MapPoint& add_point(Rng& R)
    {
        mps.emplace_back();
        MapPoint& p = mps.back();
        p.mnId = (long unsigned int)mps.size() - 1;
        for (int k = 0; k < 3; k++) p.X[k] = 0.5f * (float)R.below(17) + 0.125f;
        p.X[2] += 3.0f;
        return p;
    }
    MapLine& add_line()
    {
        mls.emplace_back();
        mls.back().mnId = (long unsigned int)mls.size() - 1;
        return mls.back();
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
};

template <class ItemT> std::vector<std::pair<long unsigned int, size_t>> obs_of(const ItemT& p)
{
    std::vector<std::pair<long unsigned int, size_t>> o;
    for (const auto& e : p.mObservations) o.emplace_back(e.first->mnId, e.second);
    return o;
}

void same_worlds(const World& A, const World& B)
{
    REQUIRE(A.mps.size() == B.mps.size() && A.mls.size() == B.mls.size());
    for (size_t i = 0; i < A.mps.size(); i++) REQUIRE(obs_of(A.mps[i]) == obs_of(B.mps[i]) && A.mps[i].nObs == B.mps[i].nObs);
    for (size_t i = 0; i < A.mls.size(); i++) REQUIRE(obs_of(A.mls[i]) == obs_of(B.mls[i]) && A.mls[i].nObs == B.mls[i].nObs);
    for (size_t k = 0; k < A.kfs.size(); k++) {
        for (int i = 0; i < ROW; i++) {
            const MapPoint *a = A.kfs[k].mvpMapPoints[(size_t)i], *b = B.kfs[k].mvpMapPoints[(size_t)i];
            REQUIRE((a == nullptr) == (b == nullptr) && (!a || a->mnId == b->mnId));
        }
        for (int i = 0; i < LROW; i++) {
            const MapLine *a = A.kfs[k].mvpMapLines[(size_t)i], *b = B.kfs[k].mvpMapLines[(size_t)i];
            REQUIRE((a == nullptr) == (b == nullptr) && (!a || a->mnId == b->mnId));
        }
    }
}

/* the store's rows, and its observers of every item of A in the map's order */
void store_holds(Tracker& T, const World& A)
{
    std::vector<int32_t> out(64);
    for (int kind = 0; kind < 2; kind++)
        for (size_t i = 0; i < (kind ? A.mls.size() : A.mps.size()); i++) {
            const Item& p = kind ? static_cast<const Item&>(A.mls[i]) : static_cast<const Item&>(A.mps[i]);
            uint8_t bad = 0;
            int32_t n = 0;
            REQUIRE(drfe_lmap_get_observers(T.db(), kind ? DRFE_LMAP_LINE : DRFE_LMAP_POINT, (int32_t)p.mnId, (int32_t)out.size(), &bad, &n, out.data()) == DRFE_OK);
            REQUIRE(bad == 0 && (size_t)n == p.mObservations.size());
            size_t t = 0;
            for (const auto& e : p.mObservations) REQUIRE(out[t++] == (int32_t)e.first->mnId);
        }
    for (const KeyFrame& k : A.kfs) {
        int32_t n = 0;
        REQUIRE(drfe_lmap_get_match_row(T.db(), DRFE_LMAP_POINT, (int32_t)k.mnId, (int32_t)out.size(), &n, out.data()) == DRFE_OK && n == ROW);
        for (int i = 0; i < ROW; i++) REQUIRE(out[(size_t)i] == (k.mvpMapPoints[(size_t)i] ? (int32_t)k.mvpMapPoints[(size_t)i]->mnId : -1));
        REQUIRE(drfe_lmap_get_match_row(T.db(), DRFE_LMAP_LINE, (int32_t)k.mnId, (int32_t)out.size(), &n, out.data()) == DRFE_OK && n == LROW);
        for (int i = 0; i < LROW; i++) REQUIRE(out[(size_t)i] == (k.mvpMapLines[(size_t)i] ? (int32_t)k.mvpMapLines[(size_t)i]->mnId : -1));
    }
}

int run(bool device, uint64_t seed, bool normals)
{
    const int nKf = 8;
    World A(nKf, seed), B(nKf, seed);
    Tracker T(device ? 0 : -1);
    T.UseDevice(device);
    A.sync(T);
    Rng R(seed + 77);
    int created = 0;
    for (int round = 0; round < 4; round++) {
        const bool single = round == 2;                        /* CreateNewKeyFrame's form */
        const int cur = R.below(nKf), n = 5 + R.below(20), nl = 2 + R.below(4);
        std::vector<MapPoint*> pa, pb;
        std::vector<MapLine*> la, lb;
        std::vector<KeyFrame*> k1a, k2a, k1b, k2b, l1a, l2a, l1b, l2b;
        std::vector<size_t> i1, i2, j1, j2;
        std::vector<float> world;
        for (int t = 0; t < n; t++) {
            Rng P(seed * 1000 + (uint64_t)created + (uint64_t)t);
            pa.push_back(&A.add_point(P));
            Rng Q(seed * 1000 + (uint64_t)created + (uint64_t)t);
            pb.push_back(&B.add_point(Q));
            const int other = (cur + 1 + R.below(nKf - 1)) % nKf;
            k1a.push_back(&A.kfs[(size_t)cur]); k2a.push_back(&A.kfs[(size_t)other]);
            k1b.push_back(&B.kfs[(size_t)cur]); k2b.push_back(&B.kfs[(size_t)other]);
            i1.push_back((size_t)R.below(ROW)); i2.push_back((size_t)R.below(ROW));
            pa.back()->mpRefKF = &A.kfs[(size_t)cur]; pb.back()->mpRefKF = &B.kfs[(size_t)cur];
            pa.back()->mnFirstKFid = pb.back()->mnFirstKFid = (long int)cur;
            for (int k = 0; k < 3; k++) world.push_back(pa.back()->X[k]);
        }
        for (int t = 0; t < nl; t++) {
            la.push_back(&A.add_line()); lb.push_back(&B.add_line());
            const int other = (cur + 1 + R.below(nKf - 1)) % nKf;
            l1a.push_back(&A.kfs[(size_t)cur]); l2a.push_back(&A.kfs[(size_t)other]);
            l1b.push_back(&B.kfs[(size_t)cur]); l2b.push_back(&B.kfs[(size_t)other]);
            j1.push_back((size_t)R.below(LROW)); j2.push_back((size_t)R.below(LROW));
        }
        const std::vector<drfe::MapPointUpkeep> got = single ? T.CreateMapPoints(pa, &A.kfs[(size_t)cur], i1, world.data(), normals)
                                                             : T.CreateMapPoints(pa, k1a, i1, k2a, i2, &A.kfs[(size_t)cur], world.data(), normals);
        if (single) T.CreateMapLines(la, &A.kfs[(size_t)cur], j1);
        else T.CreateMapLines(la, l1a, j1, l2a, j2, &A.kfs[(size_t)cur]);
        /* src/LocalMapping.cc:522-535 and :1019-1031 on the objects alone */
        REQUIRE(got.size() == (size_t)n);
        for (int t = 0; t < n; t++) {
            MapPoint* pMP = pb[(size_t)t];
            pMP->AddObservation(k1b[(size_t)t], i1[(size_t)t]);
            if (!single) pMP->AddObservation(k2b[(size_t)t], i2[(size_t)t]);
            k1b[(size_t)t]->AddMapPoint(pMP, i1[(size_t)t]);
            if (!single) k2b[(size_t)t]->AddMapPoint(pMP, i2[(size_t)t]);
            REQUIRE(got[(size_t)t].status == (normals ? DRFE_UPKEEP_NORMAL : 0));
            if (!normals) continue;
            pMP->UpdateNormalAndDepth();
            REQUIRE(std::memcmp(got[(size_t)t].normal, pMP->normal, sizeof(pMP->normal)) == 0);
            REQUIRE(std::memcmp(&got[(size_t)t].max_distance, &pMP->maxD, sizeof(float)) == 0);
            REQUIRE(std::memcmp(&got[(size_t)t].min_distance, &pMP->minD, sizeof(float)) == 0);
        }
        for (int t = 0; t < nl; t++) {
            MapLine* pML = lb[(size_t)t];
            pML->AddObservation(l1b[(size_t)t], j1[(size_t)t]);
            if (!single) pML->AddObservation(l2b[(size_t)t], j2[(size_t)t]);
            l1b[(size_t)t]->AddMapLine(pML, j1[(size_t)t]);
            if (!single) l2b[(size_t)t]->AddMapLine(pML, j2[(size_t)t]);
        }
        created += n;
        same_worlds(A, B);
        store_holds(T, A);
    }
    int64_t st[8];
    REQUIRE(drfe_lmap_create_stats(T.db(), st) == DRFE_OK);
    REQUIRE(st[0] == 8 && st[2] == (int64_t)created && st[5] == 0 && st[1] == (device ? st[0] : 0));
    return created;
}

}  // namespace create_world

int main(int argc, char** argv)
{
    const bool device = argc > 1 && std::string(argv[1]) == "device";
    int created = 0;
    try {
        for (uint64_t seed = 1; seed <= 5; seed++) created += create_world::run(device, seed, seed % 3 != 0);
    } catch (const std::exception& e) {
        std::printf("create_caller: %s\n", e.what());
        return 1;
    }
    if (created < 100) {
        std::printf("create_caller: only %d points created\n", created);
        return 1;
    }
    std::printf("create_caller %s: ok, %d points created\n", device ? "device" : "host", created);
    return 0;
}
