/* gba_propagate_caller.cpp — Planar_SLAM::LocalMapTracker::PropagateGlobalBA of include/drfe_adaptor.hpp next to a restatement of
 * the map update that ends LoopClosing::RunGlobalBundleAdjustment (reference src/LoopClosing.cc:722-783), written here as the
 * reference's pointer walk over stand-in classes with the reference's members: a std::list<KeyFrame*> FIFO, std::set<KeyFrame*>
 * children walked in pointer order, GetPoseInverse() before SetPose, then every map point of the map.
 *
 *   gba_propagate_caller [host | device]
 *
 * Two worlds are built from the same description, so that pointer order is the same in both: the restatement runs on one, the
 * adaptor on the other, and every key frame's pose, mTcwGBA, mTcwBefGBA and stamp and every point's position must come out equal,
 * byte for byte, after three seeded adjustments (a fifth of the key frames and of the points made while each ran) with an edit of
 * poses and positions in between.  The store is synced once and after the edit only: every call reads what the one before
 * committed. */
#include "drfe_adaptor.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace {

typedef drfe_cv::Mat Mat;

Mat matf(int rows, int cols)
{
    Mat m(rows, cols, 4);
    std::memset(m.data, 0, (size_t)rows * cols * 4);
    return m;
}
float& at(Mat& m, int r, int c) { return m.ptr<float>(r)[c]; }
float at(const Mat& m, int r, int c) { return m.ptr<float>(r)[c]; }
Mat clone(const Mat& m)
{
    Mat o = matf(m.rows, m.cols);
    for (int r = 0; r < m.rows; r++)
        for (int c = 0; c < m.cols; c++) at(o, r, c) = at(m, r, c);
    return o;
}

/* cv::Mat C = A * B of two CV_32F matrices, and A * B + C: gemm's small-matrix path, float dots left to right, then
 * (float)(t * 1) or (float)(t * 1 + c * 1) in double */
Mat mul(const Mat& A, const Mat& B, const Mat* C = nullptr)
{
    Mat D = matf(A.rows, B.cols);
    for (int r = 0; r < A.rows; r++)
        for (int c = 0; c < B.cols; c++) {
            float t = at(A, r, 0) * at(B, 0, c);
            for (int k = 1; k < A.cols; k++) t = t + at(A, r, k) * at(B, k, c);
            at(D, r, c) = C ? (float)((double)t * 1.0 + (double)at(*C, r, c) * 1.0) : (float)((double)t * 1.0);
        }
    return D;
}
Mat block(const Mat& T, int r0, int r1, int c0, int c1)
{
    Mat o = matf(r1 - r0, c1 - c0);
    for (int r = r0; r < r1; r++)
        for (int c = c0; c < c1; c++) at(o, r - r0, c - c0) = at(T, r, c);
    return o;
}

struct KeyFrame;
struct MapPoint;

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
    long unsigned int mnBAGlobalForKF = 0;
    bool mbBad = false;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens;
    std::vector<drfe_cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    Mat Tcw, Twc, Ow, mTcwGBA, mTcwBefGBA;

    bool isBad() const { return mbBad; }
    KeyFrame* GetParent() const { return mpParent; }
    std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int&) const { return std::vector<KeyFrame*>(); }
    std::vector<MapPoint*> GetMapPointMatches() const { return std::vector<MapPoint*>(); }
    std::vector<MapLine*> GetMapLineMatches() const { return std::vector<MapLine*>(); }
    Mat GetPose() const { return clone(Tcw); }
    Mat GetPoseInverse() const { return clone(Twc); }
    /* KeyFrame::SetPose (src/KeyFrame.cc:147-167): Rwc = Rcw.t() stored, Ow = -Rwc * tcw through gemm's small-matrix path */
    void SetPose(const Mat& Tcw_)
    {
        Tcw = clone(Tcw_);
        float Rwc[3][3];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Rwc[r][c] = at(Tcw, c, r);
        Ow = matf(3, 1);
        for (int r = 0; r < 3; r++) {
            const float d = Rwc[r][0] * at(Tcw, 0, 3) + Rwc[r][1] * at(Tcw, 1, 3) + Rwc[r][2] * at(Tcw, 2, 3);
            at(Ow, r, 0) = (float)((double)d * -1.0);
        }
        Twc = matf(4, 4);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) at(Twc, r, c) = Rwc[r][c];
            at(Twc, r, 3) = at(Ow, r, 0);
        }
        at(Twc, 3, 3) = 1.0f;
    }
};

struct MapPoint {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0, mnBAGlobalForKF = 0;
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    KeyFrame* mpRefKF = nullptr;
    Mat mWorldPos, mPosGBA;

    bool isBad() const { return mbBad; }
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
    KeyFrame* GetReferenceKeyFrame() const { return mpRefKF; }
    Mat GetWorldPos() const { return clone(mWorldPos); }
    void SetWorldPos(const Mat& P) { mWorldPos = clone(P); }
    void SetNormalAndDepth(const float*, float, float) {}
};

/* src/LoopClosing.cc:722-783 */
void PropagateRestated(unsigned long nLoopKF, const std::vector<KeyFrame*>& mvpKeyFrameOrigins, const std::vector<MapPoint*>& vpMPs)
{
    std::list<KeyFrame*> lpKFtoCheck(mvpKeyFrameOrigins.begin(), mvpKeyFrameOrigins.end());
    while (!lpKFtoCheck.empty()) {
        KeyFrame* pKF = lpKFtoCheck.front();
        const std::set<KeyFrame*> sChilds = pKF->GetChilds();
        Mat Twc = pKF->GetPoseInverse();
        for (std::set<KeyFrame*>::const_iterator sit = sChilds.begin(); sit != sChilds.end(); sit++) {
            KeyFrame* pChild = *sit;
            if (pChild->mnBAGlobalForKF != nLoopKF) {
                Mat Tchildc = mul(pChild->GetPose(), Twc);
                pChild->mTcwGBA = mul(Tchildc, pKF->mTcwGBA);
                pChild->mnBAGlobalForKF = nLoopKF;
            }
            lpKFtoCheck.push_back(pChild);
        }
        pKF->mTcwBefGBA = pKF->GetPose();
        pKF->SetPose(pKF->mTcwGBA);
        lpKFtoCheck.pop_front();
    }
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint* pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        if (pMP->mnBAGlobalForKF == nLoopKF) {
            pMP->SetWorldPos(pMP->mPosGBA);
        } else {
            KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
            if (pRefKF->mnBAGlobalForKF != nLoopKF) continue;
            Mat Rcw = block(pRefKF->mTcwBefGBA, 0, 3, 0, 3);
            Mat tcw = block(pRefKF->mTcwBefGBA, 0, 3, 3, 4);
            Mat Xc = mul(Rcw, pMP->GetWorldPos(), &tcw);
            Mat Twc = pRefKF->GetPoseInverse();
            Mat Rwc = block(Twc, 0, 3, 0, 3);
            Mat twc = block(Twc, 0, 3, 3, 4);
            pMP->SetWorldPos(mul(Rwc, Xc, &twc));
        }
    }
}

typedef Planar_SLAM::LocalMapTracker<KeyFrame, MapPoint, MapLine, Frame> Tracker;

struct Rng {
    uint64_t s;
    int below(int n)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((s >> 33) % (uint64_t)n);
    }
    double unit() { return (double)below(1 << 20) / (double)(1 << 20); }
};

Mat random_pose(Rng& r)
{
    double q[4], nrm = 0;
    for (int k = 0; k < 4; k++) {
        q[k] = r.unit() - 0.5;
        nrm += q[k] * q[k];
    }
    nrm = std::sqrt(nrm) + 1e-9;
    const double x = q[0] / nrm, y = q[1] / nrm, z = q[2] / nrm, w = q[3] / nrm;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    Mat T = matf(4, 4);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) at(T, i, j) = (float)R[i][j];
        at(T, i, 3) = (float)(6.0 * r.unit() - 3.0);
    }
    at(T, 3, 3) = 1.0f;
    return T;
}

Mat random_point(Rng& r)
{
    Mat X = matf(3, 1);
    for (int k = 0; k < 3; k++) at(X, k, 0) = (float)(10.0 * r.unit() - 5.0);
    return X;
}

/* a random spanning tree over nK key frames from two origins, and nP points with a reference key frame each */
struct World {
    std::vector<KeyFrame> kf;
    std::vector<MapPoint> mp;
    World(uint64_t seed, int nK, int nP) : kf((size_t)nK), mp((size_t)nP)
    {
        Rng r{seed};
        for (int i = 0; i < nK; i++) {
            KeyFrame& K = kf[(size_t)i];
            K.mnId = (long unsigned int)(i + 1);
            K.mvScaleFactors = {1.0f};
            K.mnScaleLevels = 1;
            K.mbBad = r.below(20) == 0;
            K.SetPose(random_pose(r));
            if (i >= 2) {
                K.mpParent = &kf[(size_t)r.below(i)];
                K.mpParent->mspChildrens.insert(&K);
            }
        }
        for (int i = 0; i < nP; i++) {
            MapPoint& P = mp[(size_t)i];
            P.mnId = (long unsigned int)(1000 + i);
            P.mbBad = r.below(20) == 0;
            P.mpRefKF = &kf[(size_t)r.below(nK)];
            P.SetWorldPos(random_point(r));
        }
    }
};

int failures = 0;

bool same_mat(const Mat& a, const Mat& b)
{
    if (a.empty() || b.empty()) return a.empty() == b.empty();
    return a.rows == b.rows && a.cols == b.cols && std::memcmp(clone(a).data, clone(b).data, (size_t)a.rows * a.cols * 4) == 0;
}

void same(const char* when, int step, const World& A, const World& B)
{
    for (size_t i = 0; i < A.kf.size(); i++) {
        const KeyFrame &a = A.kf[i], &b = B.kf[i];
        if (!same_mat(a.Tcw, b.Tcw) || !same_mat(a.Twc, b.Twc) || !same_mat(a.mTcwGBA, b.mTcwGBA) ||
            !same_mat(a.mTcwBefGBA, b.mTcwBefGBA) || a.mnBAGlobalForKF != b.mnBAGlobalForKF) {
            failures++;
            fprintf(stderr, "gba_propagate_caller: %s %d: key frame %lu differs\n", when, step, a.mnId);
        }
    }
    for (size_t i = 0; i < A.mp.size(); i++)
        if (!same_mat(A.mp[i].mWorldPos, B.mp[i].mWorldPos)) {
            failures++;
            fprintf(stderr, "gba_propagate_caller: %s %d: map point %lu differs\n", when, step, A.mp[i].mnId);
        }
}

/* what Optimizer::BundleAdjustment's write-back leaves for nLoopKF (src/Optimizer.cc:505-546), the same in both worlds: a fifth of
 * the key frames (never an origin) and of the points count as made while the adjustment ran and are left alone */
void adjust(World& A, World& B, Tracker& tracker, Rng& r, unsigned long nLoopKF)
{
    for (size_t i = 0; i < A.kf.size(); i++) {
        if (i >= 2 && r.below(5) == 0) continue;
        const Mat T = random_pose(r);
        A.kf[i].mTcwGBA = clone(T);
        B.kf[i].mTcwGBA = clone(T);
        A.kf[i].mnBAGlobalForKF = B.kf[i].mnBAGlobalForKF = nLoopKF;
        tracker.SyncGlobalBA(&B.kf[i]);
    }
    for (size_t i = 0; i < A.mp.size(); i++) {
        if (r.below(5) == 0) continue;
        const Mat X = random_point(r);
        A.mp[i].mPosGBA = clone(X);
        B.mp[i].mPosGBA = clone(X);
        A.mp[i].mnBAGlobalForKF = B.mp[i].mnBAGlobalForKF = nLoopKF;
        tracker.SyncGlobalBA(&B.mp[i]);
    }
}

void run(const std::string& mode, int64_t* st)
{
    World A(29, 60, 900), B(29, 60, 900);
    Tracker tracker(mode == "device" ? 0 : -1);
    tracker.UseDevice(mode == "device");
    for (KeyFrame& k : B.kf) {
        tracker.Sync(&k);
        tracker.SyncGeometry(&k);
    }
    for (MapPoint& p : B.mp) {
        tracker.Sync(&p);
        tracker.SyncGeometry(&p);
    }
    Rng r{5};
    std::vector<MapPoint*> allA;
    for (MapPoint& p : A.mp) allA.push_back(&p);
    for (int s = 0; s < 3; s++) {
        const unsigned long nLoopKF = (unsigned long)(40 + s);
        adjust(A, B, tracker, r, nLoopKF);
        PropagateRestated(nLoopKF, {&A.kf[0], &A.kf[1]}, allA);
        const std::vector<KeyFrame*> visited = tracker.PropagateGlobalBA(nLoopKF, {&B.kf[0], &B.kf[1]});
        if (visited.size() != B.kf.size()) failures++;
        same("call", s, A, B);
        if (s == 0)
            for (int e = 0; e < 6; e++) {
                /* an edit in both worlds: new poses and positions, synced */
                const size_t i = (size_t)r.below((int)A.kf.size());
                const Mat T = random_pose(r);
                A.kf[i].SetPose(T);
                B.kf[i].SetPose(T);
                tracker.SyncGeometry(&B.kf[i]);
                const size_t p = (size_t)r.below((int)A.mp.size());
                const Mat X = random_point(r);
                A.mp[p].SetWorldPos(X);
                B.mp[p].SetWorldPos(X);
                tracker.SyncGeometry(&B.mp[p]);
            }
    }
    if (drfe_lmap_gba_stats(tracker.db(), st) != DRFE_OK) throw std::runtime_error("drfe_lmap_gba_stats failed");
    if (st[0] != 3 || st[1] != (mode == "device" ? 3 : 0)) failures++;
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    try {
        int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        run(mode, st);
        if (st[3] < 10 || st[5] < 500 || st[6] < 100) {
            fprintf(stderr, "gba_propagate_caller: the seeded world composed %lld key frames and moved %lld + %lld points\n", (long long)st[3],
                    (long long)st[5], (long long)st[6]);
            return 1;
        }
        if (failures) return 1;
        printf("gba_propagate_caller ok (%s, 3 calls, %lld key frames composed, %lld + %lld points moved, device calls %lld)\n", mode.c_str(),
               (long long)st[3], (long long)st[5], (long long)st[6], (long long)st[1]);
    } catch (const std::exception& e) {
        fprintf(stderr, "gba_propagate_caller: %s\n", e.what());
        return 2;
    }
    return 0;
}
