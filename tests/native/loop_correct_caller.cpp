/* loop_correct_caller.cpp — Planar_SLAM::LocalMapTracker::CorrectLoop of include/drfe_adaptor.hpp next to a restatement of
 * LoopClosing::CorrectLoop's Sim3 propagation (reference src/LoopClosing.cc:480-562), written here as the reference's pointer walk
 * over stand-in classes with the reference's members: a real std::map<KeyFrame*, Sim3> walked in pointer order, SetPose at the
 * end of each key frame's turn, UpdateNormalAndDepth reading whatever centre a key frame has at that moment.
 *
 *   loop_correct_caller [host | device]
 *
 * Two worlds are built from the same description, so that pointer order is the same in both: the restatement runs on one, the
 * adaptor on the other, and every key frame's pose and centre, every point's position, stamps, normal and distances and both
 * returned maps must come out equal, byte for byte, after 8 calls of 1 to 12 key frames, an edit of poses and positions, and one
 * call of 30 key frames.  The store is synced once and after the edit only: every call reads what the one before committed. */
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
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<drfe_cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    Mat Tcw, Twc, Ow;

    bool isBad() const { return mbBad; }
    KeyFrame* GetParent() const { return nullptr; }
    std::set<KeyFrame*> GetChilds() const { return std::set<KeyFrame*>(); }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int&) const { return std::vector<KeyFrame*>(); }
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
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

/* cv::Mat C = A * B of two 4x4 float matrices: gemm's small-matrix path */
Mat mul44(const Mat& A, const Mat& B)
{
    Mat C = matf(4, 4);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const float t = at(A, r, 0) * at(B, 0, c) + at(A, r, 1) * at(B, 1, c) + at(A, r, 2) * at(B, 2, c) + at(A, r, 3) * at(B, 3, c);
            at(C, r, c) = (float)((double)t * 1.0);
        }
    return C;
}

/* src/LoopClosing.cc:480-562 without the UpdateConnections calls */
void CorrectLoopRestated(KeyFrame* mpCurrentKF, const Sim3& mg2oScw, const std::vector<KeyFrame*>& mvpCurrentConnectedKFs,
                         KeyFrameAndPose& CorrectedSim3, KeyFrameAndPose& NonCorrectedSim3)
{
    CorrectedSim3[mpCurrentKF] = mg2oScw;
    const Mat Twc = mpCurrentKF->GetPoseInverse();
    for (KeyFrame* pKFi : mvpCurrentConnectedKFs) {
        const Mat Tiw = pKFi->GetPose();
        if (pKFi != mpCurrentKF) {
            const Mat Tic = mul44(Tiw, Twc);
            CorrectedSim3[pKFi] = sim3_of_pose(Tic) * mg2oScw;
        }
        NonCorrectedSim3[pKFi] = sim3_of_pose(Tiw);
    }
    for (auto mit = CorrectedSim3.begin(); mit != CorrectedSim3.end(); mit++) {
        KeyFrame* pKFi = mit->first;
        const Sim3 g2oCorrectedSiw = mit->second;
        const Sim3 g2oCorrectedSwi = g2oCorrectedSiw.inverse();
        const Sim3 g2oSiw = NonCorrectedSim3[pKFi];
        const std::vector<MapPoint*> vpMPsi = pKFi->GetMapPointMatches();
        for (size_t iMP = 0; iMP < vpMPsi.size(); iMP++) {
            MapPoint* pMPi = vpMPsi[iMP];
            if (!pMPi) continue;
            if (pMPi->isBad()) continue;
            if (pMPi->mnCorrectedByKF == mpCurrentKF->mnId) continue;
            const Mat P3Dw = pMPi->GetWorldPos();
            const Vec3 eigP3Dw((double)at(P3Dw, 0, 0), (double)at(P3Dw, 1, 0), (double)at(P3Dw, 2, 0));
            const Vec3 corrected = g2oCorrectedSwi.map(g2oSiw.map(eigP3Dw));
            Mat cv = matf(3, 1);
            for (int k = 0; k < 3; k++) at(cv, k, 0) = (float)corrected[k];
            pMPi->SetWorldPos(cv);
            pMPi->mnCorrectedByKF = mpCurrentKF->mnId;
            pMPi->mnCorrectedReference = pKFi->mnId;
            pMPi->UpdateNormalAndDepth();
        }
        double eigR[3][3];
        rotation_matrix(g2oCorrectedSiw.rotation(), eigR);
        Vec3 eigt = g2oCorrectedSiw.translation();
        const double s = g2oCorrectedSiw.scale();
        for (int k = 0; k < 3; k++) eigt[k] *= (1. / s);
        Mat correctedTiw = matf(4, 4);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) at(correctedTiw, r, c) = (float)eigR[r][c];
            at(correctedTiw, r, 3) = (float)eigt[r];
        }
        at(correctedTiw, 3, 3) = 1.0f;
        pKFi->SetPose(correctedTiw);
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
    nrm = std::sqrt(nrm);
    Quat u;
    for (int k = 0; k < 4; k++) u.c[k] = q[k] / nrm;
    double R[3][3];
    rotation_matrix(u, R);
    Mat T = matf(4, 4);
    for (int i = 0; i < 3; i++) {
        for (int c = 0; c < 3; c++) at(T, i, c) = (float)R[i][c];
        at(T, i, 3) = (float)(6.0 * r.unit() - 3.0);
    }
    at(T, 3, 3) = 1.0f;
    return T;
}

struct World {
    std::vector<KeyFrame> kf;
    std::vector<MapPoint> mp;
    World(uint64_t seed, int nKf, int nMp, int row) : kf((size_t)nKf), mp((size_t)nMp)
    {
        Rng r{seed};
        std::vector<int> ids((size_t)nKf);
        for (int i = 0; i < nKf; i++) ids[(size_t)i] = i;
        for (int i = nKf - 1; i > 0; i--) std::swap(ids[(size_t)i], ids[(size_t)r.below(i + 1)]);   /* mnId order is not pointer order */
        std::vector<float> sf(8, 1.0f);
        for (size_t l = 1; l < sf.size(); l++) sf[l] = sf[l - 1] * 1.2f;
        for (int i = 0; i < nKf; i++) {
            KeyFrame& k = kf[(size_t)i];
            k.mnId = (long unsigned int)ids[(size_t)i];
            k.mvScaleFactors = sf;
            k.mnScaleLevels = (int)sf.size();
            k.mvKeysUn.resize((size_t)row);
            for (auto& kp : k.mvKeysUn) kp.octave = r.below(8);
            k.SetPose(random_pose(r));
            for (int e = 0; e < row - (i % 5); e++) k.mvpMapPoints.push_back(r.below(8) ? &mp[(size_t)r.below(nMp)] : nullptr);
        }
        for (int p = 0; p < nMp; p++) {
            MapPoint& m = mp[(size_t)p];
            m.mnId = 100 + (long unsigned int)p;
            m.mbBad = r.below(20) == 0;
            for (int o = r.below(6); o > 0; o--) m.mObservations[&kf[(size_t)r.below(nKf)]] = (size_t)r.below(row);
            m.mpRefKF = &kf[(size_t)r.below(nKf)];          /* sometimes an observer, sometimes not */
            Mat X = matf(3, 1);
            for (int k = 0; k < 3; k++) at(X, k, 0) = (float)(10.0 * r.unit() - 5.0);
            m.SetWorldPos(X);
        }
    }
};

int failures = 0;

bool same_mat(const Mat& a, const Mat& b, int rows, int cols)
{
    for (int r = 0; r < rows; r++)
        if (std::memcmp(a.ptr<float>(r), b.ptr<float>(r), (size_t)cols * 4) != 0) return false;
    return true;
}

void same(const char* when, int step, const World& A, const World& B)
{
    bool ok = true;
    for (size_t i = 0; i < A.kf.size(); i++)
        ok = ok && same_mat(A.kf[i].Tcw, B.kf[i].Tcw, 4, 4) && same_mat(A.kf[i].Ow, B.kf[i].Ow, 3, 1) && same_mat(A.kf[i].Twc, B.kf[i].Twc, 4, 4);
    for (size_t i = 0; i < A.mp.size(); i++) {
        const MapPoint &a = A.mp[i], &b = B.mp[i];
        ok = ok && same_mat(a.mWorldPos, b.mWorldPos, 3, 1) && a.mnCorrectedByKF == b.mnCorrectedByKF && a.mnCorrectedReference == b.mnCorrectedReference &&
             std::memcmp(a.mNormalVector, b.mNormalVector, 12) == 0 && std::memcmp(&a.mfMaxDistance, &b.mfMaxDistance, 4) == 0 &&
             std::memcmp(&a.mfMinDistance, &b.mfMinDistance, 4) == 0;
    }
    if (ok) return;
    failures++;
    fprintf(stderr, "loop_correct_caller: %s %d: the two worlds differ\n", when, step);
}

bool same_sims(const KeyFrameAndPose& a, const World& A, const KeyFrameAndPose& b, const World& B)
{
    if (a.size() != b.size()) return false;
    auto ia = a.begin();
    auto ib = b.begin();
    for (; ia != a.end(); ++ia, ++ib) {
        if (ia->first - A.kf.data() != ib->first - B.kf.data()) return false;         /* the same key frame at the same place */
        if (std::memcmp(ia->second.r.c, ib->second.r.c, 32) != 0 || std::memcmp(&ia->second.t, &ib->second.t, 24) != 0 ||
            std::memcmp(&ia->second.s, &ib->second.s, 8) != 0)
            return false;
    }
    return true;
}

void one_call(const char* when, int step, World& A, World& B, Tracker& tracker, Rng& r, int n, double scale)
{
    const int nKf = (int)A.kf.size();
    std::vector<int> order((size_t)nKf);
    for (int i = 0; i < nKf; i++) order[(size_t)i] = i;
    for (int i = nKf - 1; i > 0; i--) std::swap(order[(size_t)i], order[(size_t)r.below(i + 1)]);
    std::vector<KeyFrame*> ca, cb;
    for (int k = 0; k < n; k++) {
        ca.push_back(&A.kf[(size_t)order[(size_t)k]]);
        cb.push_back(&B.kf[(size_t)order[(size_t)k]]);
    }
    const int cur = r.below(n);
    const Sim3 rel = sim3_of_pose(random_pose(r));
    const Sim3 Scw(rel.r, rel.t, scale);
    KeyFrameAndPose corrA, nonA;
    CorrectLoopRestated(ca[(size_t)cur], Scw, ca, corrA, nonA);
    const auto sims = tracker.CorrectLoop(cb[(size_t)cur], Scw, cb);
    same(when, step, A, B);
    if (!same_sims(corrA, A, sims.first, B) || !same_sims(nonA, A, sims.second, B)) {
        failures++;
        fprintf(stderr, "loop_correct_caller: %s %d: the returned Sim3 maps differ\n", when, step);
    }
}

void run(const std::string& mode, int64_t* moved, int64_t* deviceCalls)
{
    World A(91, 48, 600, 40), B(91, 48, 600, 40);
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
    Rng r{17};
    const double scales[4] = {1.0, 2.0, 0.8, 1.37};
    for (int s = 0; s < 8; s++) {
        one_call("call", s, A, B, tracker, r, 1 + r.below(12), scales[s % 4]);
        if (s == 4) {
            /* an edit in both worlds: new poses and positions, synced */
            for (int e = 0; e < 6; e++) {
                const size_t i = (size_t)r.below((int)A.kf.size());
                const Mat T = random_pose(r);
                A.kf[i].SetPose(T);
                B.kf[i].SetPose(T);
                tracker.SyncGeometry(&B.kf[i]);
                const size_t p = (size_t)r.below((int)A.mp.size());
                Mat X = matf(3, 1);
                for (int k = 0; k < 3; k++) at(X, k, 0) = (float)(10.0 * r.unit() - 5.0);
                A.mp[p].SetWorldPos(X);
                B.mp[p].SetWorldPos(X);
                tracker.SyncGeometry(&B.mp[p]);
            }
        }
    }
    one_call("the call of", 30, A, B, tracker, r, 30, 1.1);
    int64_t st[8];
    if (drfe_lmap_correct_stats(tracker.db(), st) != DRFE_OK) throw std::runtime_error("drfe_lmap_correct_stats failed");
    if (st[0] != 9) failures++;
    *moved = st[3];
    *deviceCalls = st[2];
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    try {
        int64_t moved = 0, deviceCalls = 0;
        run(mode, &moved, &deviceCalls);
        if (moved < 500) {
            fprintf(stderr, "loop_correct_caller: the seeded world moved only %lld points\n", (long long)moved);
            return 1;
        }
        if (failures) return 1;
        printf("loop_correct_caller ok (%s, 8 calls, 1 call of 30, %lld points moved, device calls %lld)\n", mode.c_str(), (long long)moved,
               (long long)deviceCalls);
    } catch (const std::exception& e) {
        fprintf(stderr, "loop_correct_caller: %s\n", e.what());
        return 2;
    }
    return 0;
}
