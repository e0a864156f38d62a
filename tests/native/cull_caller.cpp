/* cull_caller.cpp — Planar_SLAM::LocalMapTracker::SyncCulling / KeyFrameCulling of include/drfe_adaptor.hpp over stand-in classes
 * with the reference's members: a real std::map<KeyFrame*, size_t> of observations and the nObs counter per map point, a real
 * std::map<KeyFrame*, int> of weights, the ordered list, the parent and a std::set<KeyFrame*> of children per key frame, all
 * walked in pointer order.  Their SetBadFlag, EraseConnection, EraseObservation and MapPoint::SetBadFlag restate what the
 * reference's do (src/KeyFrame.cc:574-705, src/MapPoint.cc:145-202).
 *
 *   cull_caller [host | device]
 *
 * The adaptor's KeyFrameCulling lets the store decide and change itself, then calls the objects' own SetBadFlag() on the key
 * frames with a verdict, in order.  After every call every row of the store must equal the objects' accessors: parents, weights,
 * ordered lists, children and flags of every key frame, nObs and the observation indices of every map point, and - through an
 * UpdateLocalMap of all points next to a store synced afresh from the objects - the bad flags, match rows and observations.
 * A key frame the store culls but whose verdict the objects would not reach, or the other way round, shows as a difference. */
#include "drfe_adaptor.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace cull_world {

struct KeyFrame;

struct MapPoint {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    bool mbBad = false;
    int nObs = 0;
    KeyFrame* mpRefKF = nullptr;
    std::map<KeyFrame*, size_t> mObservations;
    bool isBad() const { return mbBad; }
    int Observations() const { return nObs; }
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
    void EraseObservation(KeyFrame* pKF);
    void SetBadFlag();
};

struct MapLine {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    int erased = 0;
    bool isBad() const { return false; }
    void EraseObservation(KeyFrame*) { erased++; }
};

struct Frame {
    long unsigned int mnId = 0;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    void* mpReferenceKF = nullptr;
};

struct KeyPoint {
    int octave = 0;
};

struct KeyFrame {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    bool mbBad = false, mbNotErase = false, mbToBeErased = false, mbNewPlane = false;
    float mThDepth = 40.0f;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvDepth, mvuRight;
    int erasedFromMap = 0;

    bool isBad() const { return mbBad; }
    bool GetNotErase() const { return mbNotErase; }        /* the two getters the integrator adds */
    bool GetToBeErased() const { return mbToBeErased; }
    KeyFrame* GetParent() const { return mpParent; }
    std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
    void AddChild(KeyFrame* pKF) { mspChildrens.insert(pKF); }
    void EraseChild(KeyFrame* pKF) { mspChildrens.erase(pKF); }
    void ChangeParent(KeyFrame* pKF)
    {
        mpParent = pKF;
        pKF->AddChild(this);
    }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) const
    {
        return (int)mvpOrderedConnectedKeyFrames.size() < N
                   ? mvpOrderedConnectedKeyFrames
                   : std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    std::vector<MapLine*> GetMapLineMatches() const { return mvpMapLines; }
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
    void EraseMapPointMatch(size_t idx) { mvpMapPoints[idx] = nullptr; }
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
    void EraseConnection(KeyFrame* pKF)
    {
        if (!mConnectedKeyFrameWeights.erase(pKF)) return;
        UpdateBestCovisibles();
    }
    void SetBadFlag()
    {
        if (mnId == 0) return;
        if (mbNotErase) {
            mbToBeErased = true;
            return;
        }
        for (auto& w : mConnectedKeyFrameWeights) w.first->EraseConnection(this);
        for (MapPoint* p : mvpMapPoints)
            if (p) p->EraseObservation(this);
        for (MapLine* l : mvpMapLines)
            if (l) l->EraseObservation(this);
        mConnectedKeyFrameWeights.clear();
        mvpOrderedConnectedKeyFrames.clear();
        std::set<KeyFrame*> candidates;
        candidates.insert(mpParent);
        while (!mspChildrens.empty()) {
            bool found = false;
            int best = -1;
            KeyFrame *pC = nullptr, *pP = nullptr;
            for (KeyFrame* child : mspChildrens) {
                if (child->isBad()) continue;
                const std::vector<KeyFrame*> connected = child->GetVectorCovisibleKeyFrames();
                for (KeyFrame* c : connected)
                    for (KeyFrame* cand : candidates)
                        if (c->mnId == cand->mnId) {
                            const int w = child->GetWeight(c);
                            if (w > best) {
                                pC = child;
                                pP = c;
                                best = w;
                                found = true;
                            }
                        }
            }
            if (!found) break;
            pC->ChangeParent(pP);
            candidates.insert(pC);
            mspChildrens.erase(pC);
        }
        for (KeyFrame* child : mspChildrens) child->ChangeParent(mpParent);
        mpParent->EraseChild(this);
        mbBad = true;
        erasedFromMap++;                       /* mpMap->EraseKeyFrame(this); mpKeyFrameDB->erase(this); */
    }
};

void MapPoint::EraseObservation(KeyFrame* pKF)
{
    const auto it = mObservations.find(pKF);
    if (it == mObservations.end()) return;
    nObs -= pKF->mvuRight[it->second] >= 0 ? 2 : 1;
    mObservations.erase(it);
    if (mpRefKF == pKF && !mObservations.empty()) mpRefKF = mObservations.begin()->first;   /* the reference reads begin() of an empty map too */
    if (nObs <= 2) SetBadFlag();
}

void MapPoint::SetBadFlag()
{
    mbBad = true;
    const std::map<KeyFrame*, size_t> obs = mObservations;
    mObservations.clear();
    for (const auto& o : obs) o.first->EraseMapPointMatch(o.second);
}

typedef Planar_SLAM::LocalMapTracker<KeyFrame, MapPoint, MapLine, Frame> Tracker;

struct Rng {
    uint64_t s;
    int below(int n)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((s >> 33) % (uint64_t)n);
    }
};

struct World {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
    std::vector<MapLine> mls;

    /* a tree of key frames under key frame 0, points of which most are seen by five to eight key frames at nearby octaves, weights
     * from the points two key frames share */
    World(int nKf, int perKf, uint64_t seed)
    {
        Rng r{seed};
        kfs.resize((size_t)nKf);
        mps.resize((size_t)(nKf * perKf));
        mls.resize(4);
        for (int k = 0; k < nKf; k++) {
            KeyFrame& K = kfs[(size_t)k];
            K.mnId = (long unsigned int)k;
            K.mThDepth = r.below(4) ? 40.0f : 3.0f;
            K.mbNotErase = k > 0 && r.below(12) == 0;
        }
        for (int k = 1; k < nKf; k++) kfs[(size_t)k].ChangeParent(&kfs[(size_t)r.below(k)]);
        for (size_t m = 0; m < mls.size(); m++) mls[m].mnId = (long unsigned int)m;
        kfs[1].mvpMapLines.push_back(&mls[0]);
        kfs[1].mvpMapLines.push_back(nullptr);
        for (size_t p = 0; p < mps.size(); p++) {
            MapPoint& P = mps[p];
            P.mnId = (long unsigned int)(1000 + p);
            const int own = 1 + (int)(p % (size_t)(nKf - 1));
            const bool thin = r.below(100) < (own % 4 == 0 ? 30 : 3);
            const int others = thin ? 1 : 4 + r.below(4);
            std::set<int> seen;
            seen.insert(own);
            while ((int)seen.size() < 1 + others) seen.insert(r.below(nKf));
            const int level = r.below(4);
            for (const int k : seen) {
                KeyFrame& K = kfs[(size_t)k];
                const int jitter = r.below(6);
                KeyPoint kp;
                kp.octave = std::max(0, level + (jitter == 0 ? -1 : jitter == 4 ? 1 : jitter == 5 ? 2 : 0));
                const bool stereo = r.below(10) < 3;
                P.mObservations[&K] = K.mvpMapPoints.size();
                P.nObs += stereo ? 2 : 1;
                K.mvpMapPoints.push_back(&P);
                K.mvKeysUn.push_back(kp);
                K.mvDepth.push_back(r.below(10) == 0 ? 5.0f : 0.25f * (float)r.below(10));
                K.mvuRight.push_back(stereo ? 1.0f : -1.0f);
            }
            P.mpRefKF = &kfs[(size_t)own];
            P.mbBad = r.below(40) == 0;
        }
        for (KeyFrame& K : kfs) {
            if (r.below(3) == 0) {             /* a null entry */
                K.mvpMapPoints.push_back(nullptr);
                K.mvKeysUn.push_back(KeyPoint());
                K.mvDepth.push_back(1.0f);
                K.mvuRight.push_back(-1.0f);
            }
            std::map<KeyFrame*, int> share;
            for (MapPoint* p : K.mvpMapPoints)
                if (p)
                    for (const auto& o : p->mObservations)
                        if (o.first != &K) share[o.first]++;
            K.mConnectedKeyFrameWeights = share;
            K.UpdateBestCovisibles();
        }
    }

    void sync(Tracker& T, bool culling)
    {
        for (KeyFrame& K : kfs) {
            T.Sync(&K);
            T.SyncConnections(&K);
            if (culling) T.SyncCulling(&K);
        }
        for (MapPoint& P : mps) {
            T.Sync(&P);
            if (culling) T.SyncCulling(&P);
        }
        for (MapLine& L : mls) T.Sync(&L);
    }
};

int fails = 0;

void expect(bool ok, const char* what, long a, long b)
{
    if (ok) return;
    if (fails++ < 20) fprintf(stderr, "cull_caller: %s differs (%ld, %ld)\n", what, a, b);
}

/* every row of the store against the objects */
void compare(Tracker& T, World& W, int64_t& frameId)
{
    drfe_lmap* db = T.db();
    const size_t nK = W.kfs.size(), nP = W.mps.size();
    std::vector<int32_t> hs(nK), wOff(nK + 1), oOff(nK + 1), parent(nK), chOff(nK + 1), wKf(nK * nK), wW(nK * nK), oKf(nK * nK), oW(nK * nK),
        ch(nK * nK);
    std::vector<uint8_t> first(nK);
    for (size_t k = 0; k < nK; k++) hs[k] = (int32_t)W.kfs[k].mnId;
    drfe_lmap_conn_rows r = {};
    r.weights_capacity = r.ordered_capacity = (int32_t)(nK * nK);
    r.weight_offsets = wOff.data(); r.weight_kfs = wKf.data(); r.weight_w = wW.data();
    r.ordered_offsets = oOff.data(); r.ordered_kfs = oKf.data(); r.ordered_w = oW.data();
    r.parent = parent.data(); r.first_connection = first.data();
    if (drfe_lmap_get_connections(db, (int32_t)nK, hs.data(), &r, (int32_t)(nK * nK), chOff.data(), ch.data()) != DRFE_OK) {
        fprintf(stderr, "cull_caller: get_connections: %s\n", drfe_lmap_last_error(db));
        exit(2);
    }
    for (size_t k = 0; k < nK; k++) {
        KeyFrame& K = W.kfs[k];
        expect(parent[k] == (K.mpParent ? (int32_t)K.mpParent->mnId : -1), "a parent", (long)k, parent[k]);
        expect((size_t)(wOff[k + 1] - wOff[k]) == K.mConnectedKeyFrameWeights.size(), "a weights row's length", (long)k, wOff[k + 1] - wOff[k]);
        int32_t i = wOff[k];
        if ((size_t)(wOff[k + 1] - wOff[k]) == K.mConnectedKeyFrameWeights.size())
            for (const auto& e : K.mConnectedKeyFrameWeights) {
                expect(wKf[(size_t)i] == (int32_t)e.first->mnId && wW[(size_t)i] == e.second, "a weight", (long)k, wKf[(size_t)i]);
                i++;
            }
        expect((size_t)(oOff[k + 1] - oOff[k]) == K.mvpOrderedConnectedKeyFrames.size(), "an ordered row's length", (long)k, oOff[k + 1] - oOff[k]);
        if ((size_t)(oOff[k + 1] - oOff[k]) == K.mvpOrderedConnectedKeyFrames.size())
            for (size_t j = 0; j < K.mvpOrderedConnectedKeyFrames.size(); j++)
                expect(oKf[(size_t)oOff[k] + j] == (int32_t)K.mvpOrderedConnectedKeyFrames[j]->mnId && oW[(size_t)oOff[k] + j] == K.mvOrderedWeights[j],
                       "an ordered entry", (long)k, (long)j);
        expect((size_t)(chOff[k + 1] - chOff[k]) == K.mspChildrens.size(), "a child set's size", (long)k, chOff[k + 1] - chOff[k]);
        i = chOff[k];
        if ((size_t)(chOff[k + 1] - chOff[k]) == K.mspChildrens.size())
            for (KeyFrame* c : K.mspChildrens) expect(ch[(size_t)i++] == (int32_t)c->mnId, "a child", (long)k, (long)c->mnId);
    }
    /* the attributes: flags per key frame, nObs and indices per point */
    std::vector<int32_t> ps(nP), rowOff(nK + 1), nObs(nP), obsOff(nP + 1), octave, obsIdx;
    std::vector<float> th(nK), depth;
    std::vector<uint8_t> flags(nK), stereo;
    size_t rows = 0, obs = 0;
    for (const KeyFrame& K : W.kfs) rows += K.mvpMapPoints.size();
    for (size_t p = 0; p < nP; p++) {
        ps[p] = (int32_t)W.mps[p].mnId;
        obs += 16;
    }
    octave.resize(rows + 1); depth.resize(rows + 1); stereo.resize(rows + 1); obsIdx.resize(obs + 1);
    drfe_lmap_cull_attributes_out a = {};
    a.n_kfs = (int32_t)nK; a.n_points = (int32_t)nP; a.row_capacity = (int32_t)rows; a.obs_capacity = (int32_t)obs;
    a.kf_handle = hs.data(); a.th_depth = th.data(); a.kf_flags = flags.data(); a.row_offsets = rowOff.data();
    a.octave = octave.data(); a.depth = depth.data(); a.stereo = stereo.data();
    a.point_handle = ps.data(); a.n_obs = nObs.data(); a.obs_offsets = obsOff.data(); a.obs_index = obsIdx.data();
    if (drfe_lmap_get_cull_attributes(db, &a) != DRFE_OK) {
        fprintf(stderr, "cull_caller: get_cull_attributes: %s\n", drfe_lmap_last_error(db));
        exit(2);
    }
    for (size_t k = 0; k < nK; k++) {
        const KeyFrame& K = W.kfs[k];
        expect(flags[k] == ((K.mbNotErase ? 1 : 0) | (K.mnId == 0 ? 2 : 0) | (K.mbToBeErased ? 4 : 0)), "a flags byte", (long)k, flags[k]);
        expect((size_t)(rowOff[k + 1] - rowOff[k]) == K.mvpMapPoints.size(), "an attribute row's length", (long)k, rowOff[k + 1] - rowOff[k]);
    }
    for (size_t p = 0; p < nP; p++) {
        const MapPoint& P = W.mps[p];
        expect(nObs[p] == P.nObs, "nObs", (long)P.mnId, nObs[p]);
        expect((size_t)(obsOff[p + 1] - obsOff[p]) == P.mObservations.size(), "an observation list's length", (long)P.mnId, obsOff[p + 1] - obsOff[p]);
        int32_t i = obsOff[p];
        if ((size_t)(obsOff[p + 1] - obsOff[p]) == P.mObservations.size())
            for (const auto& o : P.mObservations) expect(obsIdx[(size_t)i++] == (int32_t)o.second, "an observation index", (long)P.mnId, (long)o.second);
    }
    /* bad flags, match rows and observations: UpdateLocalMap of a frame with every point, on this store and on one synced afresh */
    Tracker fresh(-1);
    W.sync(fresh, false);
    std::vector<int32_t> pts(ps);
    const int32_t ptOff[2] = {0, (int32_t)nP};
    drfe_lmap* dbs[2] = {db, fresh.db()};
    const int64_t ids[2] = {++frameId, 1};
    std::vector<int32_t> out[2][8];
    std::vector<uint8_t> in[2];
    int32_t size[3] = {0, 0, 0};
    drfe_lmap_size(db, size);
    for (int s = 0; s < 2; s++) {
        drfe_lmap_queries q = {};
        q.n = 1;
        q.frame_id = &ids[s]; q.point_offsets = ptOff; q.points = pts.data();
        drfe_lmap_out o = {};
        o.kf_capacity = size[0]; o.mp_capacity = size[1]; o.ml_capacity = size[2] + 1; o.nulled_capacity = (int32_t)nP;
        const size_t caps[8] = {2, (size_t)size[0] + 1, 1, 2, (size_t)size[1] + 1, 2, (size_t)size[2] + 1, 2};
        for (int f = 0; f < 8; f++) out[s][f].assign(caps[f], 0);
        std::vector<int32_t> nuOff(2, 0), nu(nP + 1, 0), rec(4, 0);
        std::vector<uint8_t> mlIn((size_t)size[2] + 1, 0);
        in[s].assign((size_t)size[1] + 1, 0);
        o.kf_offsets = out[s][0].data(); o.kfs = out[s][1].data(); o.ref_kf = out[s][2].data(); o.mp_offsets = out[s][3].data();
        o.mps = out[s][4].data(); o.mp_in_frame = in[s].data(); o.ml_offsets = out[s][5].data(); o.mls = out[s][6].data();
        o.ml_in_frame = mlIn.data(); o.nulled_offsets = nuOff.data(); o.nulled = nu.data(); o.record = rec.data();
        if (drfe_lmap_update_host(dbs[s], &q, &o) != DRFE_OK) {
            fprintf(stderr, "cull_caller: update: %s\n", drfe_lmap_last_error(dbs[s]));
            exit(2);
        }
        out[s][7] = nu;
        out[s][7].push_back(nuOff[1]);
    }
    for (int f = 0; f < 8; f++) expect(out[0][f] == out[1][f], "UpdateLocalMap after the call", f, (long)out[0][f].size());
    expect(in[0] == in[1], "UpdateLocalMap's in-frame flags after the call", 0, 0);
}

/* the calls of a run; returns culled key frames */
int run(const std::string& mode, int* calls, int* deferred)
{
    const bool device = mode == "device";
    World W(40, 30, 7);
    Tracker T(device ? 0 : -1);
    T.UseDevice(device);
    W.sync(T, true);
    int64_t frameId = 10;
    int culled = 0;
    compare(T, W, frameId);
    const int currents[] = {3, 17, 9, 28, 3, 35, 12};
    for (const int c : currents) {
        KeyFrame& cur = W.kfs[(size_t)c];
        if (cur.isBad()) continue;
        cur.mbNewPlane = c == 9;               /* the early return: nothing may change */
        const std::vector<KeyFrame*> gone = T.KeyFrameCulling(&cur, c == 28);
        for (KeyFrame* k : gone)
            if (!k->isBad() || k->erasedFromMap != 1) expect(false, "a culled key frame's own SetBadFlag", (long)k->mnId, k->erasedFromMap);
        if (cur.mbNewPlane && !gone.empty()) expect(false, "the mbNewPlane return", c, (long)gone.size());
        culled += (int)gone.size();
        (*calls)++;
        compare(T, W, frameId);
    }
    for (const KeyFrame& K : W.kfs) *deferred += K.mbToBeErased ? 1 : 0;
    if (W.mls[0].erased > 1) expect(false, "a map line's EraseObservation", W.mls[0].erased, 1);
    return culled;
}

}  // namespace cull_world

#ifndef CULL_CALLER_NO_MAIN
int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    int calls = 0, deferred = 0;
    const int culled = cull_world::run(mode, &calls, &deferred);
    if (cull_world::fails || culled < 3) {
        fprintf(stderr, "cull_caller: %d differences, %d culled\n", cull_world::fails, culled);
        return 1;
    }
    printf("cull_caller ok (%s, %d calls, %d culled, %d deferred)\n", mode.c_str(), calls, culled, deferred);
    return 0;
}
#endif
