/* essential_caller.cpp — Planar_SLAM::LocalMapTracker::EssentialEdges and EssentialCommit of include/drfe_adaptor.hpp next to a
 * restatement of what surrounds the solver of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2910-3131), written here
 * as the reference's pointer walk over stand-in classes with the reference's members: std::set<KeyFrame*> and std::map<KeyFrame*,
 * ...> walked in pointer order, std::upper_bound in GetCovisiblesByWeight, a std::set of (min, max) id pairs, Sim3s kept by mnId
 * where a missing entry is default-constructed.
 *
 *   essential_caller [host | device]
 *
 * Two worlds are built from the same description, so that pointer order is the same in both: the restatement runs on one, the
 * adaptor on the other.  The vertices, the edge list in addEdge order with every measurement, vCorrectedSwc, every key frame's
 * pose and centre and every point's position, normal and distances must come out equal, byte for byte, over two loop closures;
 * the second reads what the first committed and the loop edge it added.  The store is synced once. */
#include "drfe_adaptor.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

/* ---- Eigen::Quaterniond and g2o::Sim3, as far as :480-562 use them ---- */
struct Quat {
    double c[4] = {0, 0, 0, 1};
    double& x() { return c[0]; }
    double& y() { return c[1]; }
    double& z() { return c[2]; }
    double& w() { return c[3]; }
    double x() const { return c[0]; }
    double y() const { return c[1]; }
    double z() const { return c[2]; }
    double w() const { return c[3]; }
};

Quat quat_of(const double m[3][3])
{
    Quat q;
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q.w() = 0.5 * t;
        t = 0.5 / t;
        q.x() = (m[2][1] - m[1][2]) * t;
        q.y() = (m[0][2] - m[2][0]) * t;
        q.z() = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q.c[i] = 0.5 * t;
        t = 0.5 / t;
        q.w() = (m[k][j] - m[j][k]) * t;
        q.c[j] = (m[j][i] + m[i][j]) * t;
        q.c[k] = (m[k][i] + m[i][k]) * t;
    }
    return q;
}

void rotation_matrix(const Quat& q, double R[3][3])
{
    const double tx = 2.0 * q.x(), ty = 2.0 * q.y(), tz = 2.0 * q.z();
    const double twx = tx * q.w(), twy = ty * q.w(), twz = tz * q.w();
    const double txx = tx * q.x(), txy = ty * q.x(), txz = tz * q.x();
    const double tyy = ty * q.y(), tyz = tz * q.y(), tzz = tz * q.z();
    R[0][0] = 1.0 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1.0 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1.0 - (txx + tyy);
}

typedef drfe_cv::Vector3d Vec3;

Vec3 cross(const double a[3], const Vec3& b) { return Vec3(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]); }

/* Quaternion::_transformVector */
Vec3 rotate(const Quat& q, const Vec3& v)
{
    Vec3 uv = cross(q.c, v);
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const Vec3 c = cross(q.c, uv);
    return Vec3((v[0] + q.w() * uv[0]) + c[0], (v[1] + q.w() * uv[1]) + c[1], (v[2] + q.w() * uv[2]) + c[2]);
}

struct Sim3 {
    Quat r;
    Vec3 t;
    double s = 1.0;
    Sim3() {}
    Sim3(const Quat& r_, const Vec3& t_, double s_) : r(r_), t(t_), s(s_) {}
    Quat& rotation() { return r; }
    const Quat& rotation() const { return r; }
    Vec3& translation() { return t; }
    const Vec3& translation() const { return t; }
    double& scale() { return s; }
    const double& scale() const { return s; }
    Vec3 map(const Vec3& v) const
    {
        const Vec3 x = rotate(r, v);
        return Vec3(s * x[0] + t[0], s * x[1] + t[1], s * x[2] + t[2]);
    }
    Sim3 inverse() const
    {
        Quat c;
        c.x() = -r.x(); c.y() = -r.y(); c.z() = -r.z(); c.w() = r.w();
        const double m = -1. / s;
        return Sim3(c, rotate(c, Vec3(m * t[0], m * t[1], m * t[2])), 1. / s);
    }
    Sim3 operator*(const Sim3& o) const
    {
        Quat q;
        q.w() = ((r.w() * o.r.w() - r.x() * o.r.x()) - r.y() * o.r.y()) - r.z() * o.r.z();
        q.x() = ((r.w() * o.r.x() + r.x() * o.r.w()) + r.y() * o.r.z()) - r.z() * o.r.y();
        q.y() = ((r.w() * o.r.y() + r.y() * o.r.w()) + r.z() * o.r.x()) - r.x() * o.r.z();
        q.z() = ((r.w() * o.r.z() + r.z() * o.r.w()) + r.x() * o.r.y()) - r.y() * o.r.x();
        return Sim3(q, map(o.t), s * o.s);
    }
};

/* g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of the upper 3x4 of a float pose */
Sim3 sim3_of_pose(const Mat& T)
{
    double m[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[r][c] = (double)at(T, r, c);
    return Sim3(quat_of(m), Vec3((double)at(T, 0, 3), (double)at(T, 1, 3), (double)at(T, 2, 3)), 1.0);
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
    bool mbBad = false;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens, mspLoopEdges;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    std::vector<drfe_cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    Mat Tcw, Twc, Ow;

    bool isBad() const { return mbBad; }
    KeyFrame* GetParent() const { return mpParent; }
    std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
    bool hasChild(KeyFrame* p) const { return mspChildrens.count(p) != 0; }
    std::set<KeyFrame*> GetLoopEdges() const { return mspLoopEdges; }
    std::set<KeyFrame*> GetConnectedKeyFrames() const
    {
        std::set<KeyFrame*> s;
        for (const auto& e : mConnectedKeyFrameWeights) s.insert(e.first);
        return s;
    }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return mvpOrderedConnectedKeyFrames; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int&) const { return std::vector<KeyFrame*>(); }
    static bool weightComp(int a, int b) { return a > b; }
    /* src/KeyFrame.cc:261-276 */
    std::vector<KeyFrame*> GetCovisiblesByWeight(const int& w) const
    {
        if (mvpOrderedConnectedKeyFrames.empty()) return std::vector<KeyFrame*>();
        std::vector<int>::const_iterator it = std::upper_bound(mvOrderedWeights.begin(), mvOrderedWeights.end(), w, KeyFrame::weightComp);
        if (it == mvOrderedWeights.end()) return std::vector<KeyFrame*>();
        const int n = (int)(it - mvOrderedWeights.begin());
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + n);
    }
    int GetWeight(KeyFrame* pKF) const
    {
        const auto it = mConnectedKeyFrameWeights.find(pKF);
        return it == mConnectedKeyFrameWeights.end() ? 0 : it->second;
    }
    std::vector<MapPoint*> GetMapPointMatches() const { return std::vector<MapPoint*>(); }
    std::vector<MapLine*> GetMapLineMatches() const { return std::vector<MapLine*>(); }
    Mat GetPose() const { return Tcw; }
    Mat GetPoseInverse() const { return Twc; }
    Mat GetCameraCenter() const { return Ow; }
    /* KeyFrame::SetPose (src/KeyFrame.cc:147-167): Rwc = Rcw.t() stored, Ow = -Rwc * tcw through gemm's small-matrix path */
    void SetPose(const Mat& Tcw_)
    {
        Tcw = matf(4, 4);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) at(Tcw, r, c) = at(Tcw_, r, c);
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

/* cv::norm of a float 3-vector */
double norm3(const float v[3])
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
    return std::sqrt(s);
}

struct MapPoint {
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    KeyFrame* mpRefKF = nullptr;
    Mat mWorldPos;
    float mNormalVector[3] = {0, 0, 0}, mfMaxDistance = 0, mfMinDistance = 0;

    bool isBad() const { return mbBad; }
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
    KeyFrame* GetReferenceKeyFrame() const { return mpRefKF; }
    Mat GetWorldPos() const { return mWorldPos; }
    void SetWorldPos(const Mat& P)
    {
        mWorldPos = matf(3, 1);
        for (int k = 0; k < 3; k++) at(mWorldPos, k, 0) = at(P, k, 0);
    }
    /* the setter the integrator adds */
    void SetNormalAndDepth(const float n[3], float maxD, float minD)
    {
        for (int k = 0; k < 3; k++) mNormalVector[k] = n[k];
        mfMaxDistance = maxD;
        mfMinDistance = minD;
    }
    /* MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:376-417) */
    void UpdateNormalAndDepth()
    {
        std::map<KeyFrame*, size_t> observations = mObservations;
        if (mbBad || observations.empty()) return;
        float normal[3] = {0, 0, 0};
        int n = 0;
        for (const auto& o : observations) {
            const Mat Owi = o.first->GetCameraCenter();
            float normali[3];
            for (int k = 0; k < 3; k++) normali[k] = at(mWorldPos, k, 0) - at(Owi, k, 0);
            const float a = (float)(1.0 / norm3(normali));
            for (int k = 0; k < 3; k++) normal[k] = normali[k] * a + normal[k];
            n++;
        }
        const Mat Owr = mpRefKF->GetCameraCenter();
        float PC[3];
        for (int k = 0; k < 3; k++) PC[k] = at(mWorldPos, k, 0) - at(Owr, k, 0);
        const float dist = (float)norm3(PC);
        const int level = mpRefKF->mvKeysUn[observations[mpRefKF]].octave;
        mfMaxDistance = dist * mpRefKF->mvScaleFactors[(size_t)level];
        mfMinDistance = mfMaxDistance / mpRefKF->mvScaleFactors[(size_t)mpRefKF->mnScaleLevels - 1];
        const float a = (float)(1.0 / (double)n);
        for (int k = 0; k < 3; k++) mNormalVector[k] = normal[k] * a;
    }
};

typedef std::map<KeyFrame*, Sim3> KeyFrameAndPose;
typedef Planar_SLAM::LocalMapTracker<KeyFrame, MapPoint, MapLine, Frame> Tracker;
typedef Tracker::EssentialGraph<Sim3> Graph;

/* what optimizer.addVertex / addEdge received, in order */
struct Restated {
    struct Vertex { KeyFrame* pKF; Sim3 estimate; bool fixed; };
    struct Edge { KeyFrame *v0, *v1; Sim3 measurement; int kind; };
    std::vector<Vertex> vertices;
    std::vector<Edge> edges;
    std::map<long unsigned int, Sim3> vScw, vCorrectedSwc;   /* a missing entry is the vector's default-constructed one */
};

/* src/Optimizer.cc:2910-3080; vpKFs is Map::GetAllKeyFrames(): set<KeyFrame*> order, the bad ones erased */
void EdgesRestated(const std::vector<KeyFrame*>& vpKFs, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
                   const KeyFrameAndPose& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections, Restated& R)
{
    const int minFeat = 100;
    for (KeyFrame* pKF : vpKFs) {
        if (pKF->isBad()) continue;
        const auto it = CorrectedSim3.find(pKF);
        R.vScw[pKF->mnId] = it != CorrectedSim3.end() ? it->second : sim3_of_pose(pKF->GetPose());
        R.vertices.push_back({pKF, R.vScw[pKF->mnId], pKF == pLoopKF});
    }
    std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
    for (const auto& LoopConnection : LoopConnections) {
        KeyFrame* pKF = LoopConnection.first;
        const long unsigned int nIDi = pKF->mnId;
        const Sim3 Swi = R.vScw[nIDi].inverse();
        for (KeyFrame* spConnection : LoopConnection.second) {
            const long unsigned int nIDj = spConnection->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(spConnection) < minFeat) continue;
            R.edges.push_back({pKF, spConnection, R.vScw[nIDj] * Swi, 0});
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    auto pick = [&](KeyFrame* p) {
        const auto it = NonCorrectedSim3.find(p);
        return it != NonCorrectedSim3.end() ? it->second : R.vScw[p->mnId];
    };
    for (KeyFrame* pKF : vpKFs) {
        if (pKF->isBad()) continue;
        const auto iti = NonCorrectedSim3.find(pKF);
        const Sim3 Swi = iti != NonCorrectedSim3.end() ? iti->second.inverse() : R.vScw[pKF->mnId].inverse();
        KeyFrame* pParentKF = pKF->GetParent();
        if (pParentKF) R.edges.push_back({pKF, pParentKF, pick(pParentKF) * Swi, 1});
        const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();
        for (KeyFrame* pLKF : sLoopEdges)
            if (pLKF->mnId < pKF->mnId) R.edges.push_back({pKF, pLKF, pick(pLKF) * Swi, 2});
        const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (KeyFrame* pKFn : vpConnectedKFs) {
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    R.edges.push_back({pKF, pKFn, pick(pKFn) * Swi, 3});
                }
            }
        }
    }
}

/* src/Optimizer.cc:3088-3131 with `estimates` what the vertices hold after the solver */
void CommitRestated(const std::vector<MapPoint*>& vpMPs, KeyFrame* pCurKF, const std::vector<Sim3>& estimates, Restated& R)
{
    for (size_t v = 0; v < R.vertices.size(); v++) {
        KeyFrame* pKFi = R.vertices[v].pKF;
        const Sim3 CorrectedSiw = estimates[v];
        R.vCorrectedSwc[pKFi->mnId] = CorrectedSiw.inverse();
        double eigR[3][3];
        rotation_matrix(CorrectedSiw.rotation(), eigR);
        Vec3 eigt = CorrectedSiw.translation();
        const double s = CorrectedSiw.scale();
        for (int k = 0; k < 3; k++) eigt[k] = eigt[k] * (1. / s);
        Mat Tiw = matf(4, 4);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) at(Tiw, r, c) = (float)eigR[r][c];
            at(Tiw, r, 3) = (float)eigt[r];
        }
        at(Tiw, 3, 3) = 1.0f;
        pKFi->SetPose(Tiw);
    }
    for (MapPoint* pMP : vpMPs) {
        if (pMP->isBad()) continue;
        const long unsigned int nIDr = pMP->mnCorrectedByKF == pCurKF->mnId ? pMP->mnCorrectedReference : pMP->GetReferenceKeyFrame()->mnId;
        const Sim3 Srw = R.vScw[nIDr], correctedSwr = R.vCorrectedSwc[nIDr];
        const Mat P3Dw = pMP->GetWorldPos();
        const Vec3 X = correctedSwr.map(Srw.map(Vec3((double)at(P3Dw, 0, 0), (double)at(P3Dw, 1, 0), (double)at(P3Dw, 2, 0))));
        Mat P = matf(3, 1);
        for (int k = 0; k < 3; k++) at(P, k, 0) = (float)X[k];
        pMP->SetWorldPos(P);
        pMP->UpdateNormalAndDepth();
    }
}

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

Sim3 random_sim3(Rng& r)
{
    Sim3 S = sim3_of_pose(random_pose(r));
    S.scale() = 0.75 + 0.5 * r.unit();
    return S;
}

/* nK key frames whose mnId runs against their addresses, a spanning tree over the good ones, loop edges between good ones,
 * connection rows with weights on both sides of 100 that also name the bad ones, and nP points */
struct World {
    std::vector<KeyFrame> kf;
    std::vector<MapPoint> mp;
    std::vector<KeyFrame*> good;
    World(uint64_t seed, int nK, int nP) : kf((size_t)nK), mp((size_t)nP)
    {
        Rng r{seed};
        for (int i = 0; i < nK; i++) {
            KeyFrame& K = kf[(size_t)i];
            K.mnId = (long unsigned int)(nK - i);
            K.mvScaleFactors = {1.0f, 1.2f, 1.44f};
            K.mnScaleLevels = 3;
            K.mvKeysUn.resize(4);
            for (int k = 0; k < 4; k++) K.mvKeysUn[(size_t)k].octave = r.below(3);
            K.mbBad = i > 2 && r.below(10) == 0;
            K.SetPose(random_pose(r));
            if (K.mbBad) continue;
            if (!good.empty()) {
                K.mpParent = good[(size_t)r.below((int)good.size())];
                K.mpParent->mspChildrens.insert(&K);
            }
            good.push_back(&K);
        }
        for (int e = 0; e < nK / 3; e++) {
            KeyFrame *a = good[(size_t)r.below((int)good.size())], *b = good[(size_t)r.below((int)good.size())];
            if (a == b) continue;
            a->mspLoopEdges.insert(b);
            b->mspLoopEdges.insert(a);
        }
        for (KeyFrame* K : good) {
            std::vector<std::pair<int, KeyFrame*>> row;
            for (int e = 0; e < 10; e++) {
                KeyFrame* o = &kf[(size_t)r.below(nK)];
                if (o == K || K->mConnectedKeyFrameWeights.count(o)) continue;
                const int w = 60 + r.below(100);
                K->mConnectedKeyFrameWeights[o] = w;
                row.push_back({w, o});
            }
            /* one row in five lies wholly at 100 or above: the end() rule */
            if (r.below(5) == 0)
                for (auto& e : row) K->mConnectedKeyFrameWeights[e.second] = e.first = 100 + e.first % 60;
            std::sort(row.begin(), row.end(), [](const std::pair<int, KeyFrame*>& a, const std::pair<int, KeyFrame*>& b) {
                return a.first != b.first ? a.first > b.first : a.second < b.second;
            });
            for (const auto& e : row) {
                K->mvpOrderedConnectedKeyFrames.push_back(e.second);
                K->mvOrderedWeights.push_back(e.first);
            }
        }
        for (int i = 0; i < nP; i++) {
            MapPoint& P = mp[(size_t)i];
            P.mnId = (long unsigned int)(1000 + i);
            P.mbBad = r.below(20) == 0;
            P.mpRefKF = &kf[(size_t)r.below(nK)];
            const int nObs = r.below(4);
            for (int o = 0; o < nObs; o++) P.mObservations[&kf[(size_t)r.below(nK)]] = (size_t)r.below(4);
            if (r.below(3) == 0) {
                P.mnCorrectedByKF = good.back()->mnId;
                P.mnCorrectedReference = kf[(size_t)r.below(nK)].mnId;
            }
            Mat X = matf(3, 1);
            for (int k = 0; k < 3; k++) at(X, k, 0) = (float)(10.0 * r.unit() - 5.0);
            if (i == 7) at(X, 0, 0) = -0.0f;
            P.SetWorldPos(X);
        }
    }
};

int failures = 0;

void fail(const char* what, long unsigned int id)
{
    failures++;
    fprintf(stderr, "essential_caller: %s %lu differs\n", what, id);
}

bool same_mat(const Mat& a, const Mat& b) { return a.rows == b.rows && a.cols == b.cols && std::memcmp(a.data, b.data, (size_t)a.rows * a.cols * 4) == 0; }
bool same_sim3(const Sim3& a, const Sim3& b)
{
    return std::memcmp(a.r.c, b.r.c, sizeof(a.r.c)) == 0 && a.t[0] == b.t[0] && a.t[1] == b.t[1] && a.t[2] == b.t[2] &&
           std::memcmp(&a.s, &b.s, sizeof(double)) == 0;
}

/* the two worlds hold the same objects at the same indices: a pointer of one names the mnId of the other */
void same_graph(const Restated& R, const Graph& G)
{
    if (R.vertices.size() != G.vertices.size() || R.edges.size() != G.edges.size()) {
        failures++;
        fprintf(stderr, "essential_caller: %zu vertices and %zu edges against %zu and %zu\n", R.vertices.size(), R.edges.size(), G.vertices.size(),
                G.edges.size());
        return;
    }
    for (size_t v = 0; v < R.vertices.size(); v++)
        if (R.vertices[v].pKF->mnId != G.vertices[v].pKF->mnId || R.vertices[v].fixed != G.vertices[v].fixed ||
            !same_sim3(R.vertices[v].estimate, G.vertices[v].Scw))
            fail("vertex", R.vertices[v].pKF->mnId);
    for (size_t e = 0; e < R.edges.size(); e++)
        if (R.edges[e].v0->mnId != G.edges[e].from->mnId || R.edges[e].v1->mnId != G.edges[e].to->mnId || R.edges[e].kind != G.edges[e].kind ||
            !same_sim3(R.edges[e].measurement, G.edges[e].Sji))
            fail("edge", (long unsigned int)e);
}

void same_world(const World& A, const World& B)
{
    for (size_t i = 0; i < A.kf.size(); i++)
        if (!same_mat(A.kf[i].Tcw, B.kf[i].Tcw) || !same_mat(A.kf[i].Twc, B.kf[i].Twc) || !same_mat(A.kf[i].Ow, B.kf[i].Ow)) fail("key frame", A.kf[i].mnId);
    for (size_t i = 0; i < A.mp.size(); i++) {
        const MapPoint &a = A.mp[i], &b = B.mp[i];
        if (!same_mat(a.mWorldPos, b.mWorldPos) || std::memcmp(a.mNormalVector, b.mNormalVector, 12) != 0 ||
            std::memcmp(&a.mfMaxDistance, &b.mfMaxDistance, 4) != 0 || std::memcmp(&a.mfMinDistance, &b.mfMinDistance, 4) != 0)
            fail("map point", a.mnId);
    }
}

/* one loop closure between the oldest and the newest good key frame, in both worlds */
void closure(World& A, World& B, Tracker& tracker, Rng& r, bool tables)
{
    KeyFrameAndPose corA, nonA, corB, nonB;
    std::map<KeyFrame*, std::set<KeyFrame*>> lcA, lcB;
    const size_t nG = A.good.size();
    auto idx = [&](const World& W, KeyFrame* p) { return (size_t)(p - &W.kf[0]); };
    if (tables)
        for (size_t g = nG - 6; g < nG; g++) {
            const Sim3 c = random_sim3(r), n = random_sim3(r);
            const size_t i = idx(A, A.good[g]);
            corA[&A.kf[i]] = c; nonA[&A.kf[i]] = n;
            corB[&B.kf[i]] = c; nonB[&B.kf[i]] = n;
        }
    for (size_t g = nG - 6; g < nG; g++) {
        const size_t i = idx(A, A.good[g]);
        for (int e = 0; e < 4; e++) {
            const size_t j = idx(A, A.good[(size_t)r.below(6)]);
            lcA[&A.kf[i]].insert(&A.kf[j]);
            lcB[&B.kf[i]].insert(&B.kf[j]);
            /* half of them weigh enough, in the key's weights row only */
            if (e % 2 == 0) A.kf[i].mConnectedKeyFrameWeights[&A.kf[j]] = B.kf[i].mConnectedKeyFrameWeights[&B.kf[j]] = 100 + e;
        }
        tracker.SyncConnections(&B.kf[i]);
    }
    KeyFrame *curA = A.good.back(), *loopA = A.good.front(), *curB = B.good.back(), *loopB = B.good.front();
    lcA[curA].insert(loopA);
    lcB[curB].insert(loopB);
    std::vector<KeyFrame*> vpKFs;
    for (KeyFrame& k : A.kf) vpKFs.push_back(&k);
    std::vector<MapPoint*> vpMPs;
    for (MapPoint& p : A.mp) vpMPs.push_back(&p);
    Restated R;
    EdgesRestated(vpKFs, loopA, curA, nonA, corA, lcA, R);
    const Graph G = tracker.EssentialEdges<Sim3>(loopB, curB, nonB, corB, lcB);
    same_graph(R, G);
    if (failures) return;
    /* a stand-in for the solver: every estimate moved by the same small Sim3 */
    Sim3 d;
    d.rotation().x() = 0.01; d.rotation().w() = std::sqrt(1.0 - 0.0001);
    d.translation() = Vec3(0.05, -0.02, 0.01);
    d.scale() = 1.01;
    std::vector<Sim3> estimates;
    for (const auto& v : R.vertices) estimates.push_back(d * v.estimate);
    CommitRestated(vpMPs, curA, estimates, R);
    const std::map<KeyFrame*, Sim3> swc = tracker.EssentialCommit<Sim3>(curB, G, estimates);
    for (const auto& v : G.vertices)
        if (!same_sim3(swc.at(v.pKF), R.vCorrectedSwc[v.pKF->mnId])) fail("vCorrectedSwc of key frame", v.pKF->mnId);
    same_world(A, B);
    /* :618-619 */
    loopA->mspLoopEdges.insert(curA); curA->mspLoopEdges.insert(loopA);
    loopB->mspLoopEdges.insert(curB); curB->mspLoopEdges.insert(loopB);
    tracker.SyncLoopEdges(loopB);
    tracker.SyncLoopEdges(curB);
}

void run(const std::string& mode, int64_t* st)
{
    World A(31, 48, 700), B(31, 48, 700);
    Tracker tracker(mode == "device" ? 0 : -1);
    tracker.UseDevice(mode == "device");
    for (KeyFrame& k : B.kf) {
        tracker.Sync(&k);
        tracker.SyncConnections(&k);
        tracker.SyncLoopEdges(&k);
        tracker.SyncGeometry(&k);
    }
    for (MapPoint& p : B.mp) {
        tracker.Sync(&p);
        tracker.SyncGeometry(&p);
    }
    Rng r{9};
    /* the second closure reads the poses, positions and loop edges the first one left in the store */
    closure(A, B, tracker, r, true);
    if (!failures) closure(A, B, tracker, r, false);
    if (drfe_lmap_essential_stats(tracker.db(), st) != DRFE_OK) throw std::runtime_error("drfe_lmap_essential_stats failed");
    if (!failures && (st[0] != 2 || st[1] != 2 || st[2] != (mode == "device" ? 4 : 0))) failures++;
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    try {
        int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        run(mode, st);
        if (failures) return 1;
        if (st[4] < 60 || st[5] < 1000 || st[6] < 10 || st[7] < 2) {
            fprintf(stderr, "essential_caller: the seeded world gave %lld edges, moved %lld points (%lld through a default entry) and emptied %lld prefixes\n",
                    (long long)st[4], (long long)st[5], (long long)st[6], (long long)st[7]);
            return 1;
        }
        printf("essential_caller ok (%s, 2 closures, %lld vertices, %lld edges, %lld points moved, device calls %lld)\n", mode.c_str(),
               (long long)st[3], (long long)st[4], (long long)st[5], (long long)st[2]);
    } catch (const std::exception& e) {
        fprintf(stderr, "essential_caller: %s\n", e.what());
        return 2;
    }
    return 0;
}
