/* plane_cull_caller.cpp — drfe::MapPlaneCulling of include/drfe_adaptor.hpp over stand-in MapPlane / KeyFrame classes, next to the
 * reference's own walk written against the same classes: two equal worlds, one culled by each, then every plane (bad flag,
 * observations, counters, cloud bits), every key frame's match vector and the recent list must be equal.
 *
 * The stand-ins restate what LocalMapping::MapPlaneCulling touches (src/LocalMapping.cc:233-307, src/MapPlane.cc:28-34, 164-296,
 * src/Map.cc:433-448): AddObservation, SetBadFlag, Replace (with its rebuild), ReplaceWithoutRebuild (the member the integration
 * adds), GetFoundRatio, and a point type of 32 bytes (PointXYZRGBA's size) so that the stride is not 12.
 *
 *   plane_cull_caller            the host entry (ctx == nullptr), then the resident map of a context on the device
 *   plane_cull_caller host       the host entry only: no device is opened (plane_cull_asan.mk builds this under the sanitizers) */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <cstdlib>
#include <list>
#include <random>

namespace plane_cull_world {

struct Point { float x, y, z, pad; uint32_t rgba; float more[3]; };
static_assert(sizeof(Point) == 32, "a PointXYZRGBA-sized point");
struct Cloud { std::vector<Point> points; };

struct MapPlane;
struct KeyFrame {
    long unsigned int mnId = 0;
    drfe_cv::Mat Twc;
    std::vector<Cloud> mvPlanePoints;
    std::vector<MapPlane*> mvpMapPlanes;
    drfe_cv::Mat GetPoseInverse() const { return Twc; }
    void ReplaceMapPlaneMatch(size_t idx, MapPlane* p) { mvpMapPlanes[idx] = p; }
    void EraseMapPlaneMatch(size_t idx) { mvpMapPlanes[idx] = nullptr; }
};

struct MapPlane {
    long int mnFirstKFid = 0;
    int nObs = 0, mnVisible = 1, mnFound = 1;
    std::shared_ptr<Cloud> mvPlanePoints = std::make_shared<Cloud>();
    drfe_cv::Mat pos = drfe_cv::Mat(4, 1, 4);
    std::map<KeyFrame*, size_t> mObservations;
    bool mbBad = false;
    MapPlane* mpReplaced = nullptr;

    drfe_cv::Mat GetWorldPos() const { return pos; }
    bool isBad() const { return mbBad; }
    int Observations() const { return nObs; }
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
    bool IsInKeyFrame(KeyFrame* k) const { return mObservations.count(k) != 0; }
    float GetFoundRatio() const { return static_cast<float>(mnFound) / mnVisible; }
    void AddObservation(KeyFrame* k, int idx)
    {
        if (mObservations.count(k)) return;
        mObservations[k] = idx;
        nObs++;
    }
    void SetBadFlag()
    {
        mbBad = true;
        std::map<KeyFrame*, size_t> obs;
        obs.swap(mObservations);
        for (auto& ob : obs) ob.first->EraseMapPlaneMatch(ob.second);
    }
    void ReplaceWithoutRebuild(MapPlane* pMP)
    {
        mbBad = true;
        std::map<KeyFrame*, size_t> obs;
        obs.swap(mObservations);
        const int nvisible = mnVisible, nfound = mnFound;
        mpReplaced = pMP;
        for (auto& ob : obs) {
            if (!pMP->IsInKeyFrame(ob.first)) {
                ob.first->ReplaceMapPlaneMatch(ob.second, pMP);
                pMP->AddObservation(ob.first, (int)ob.second);
            } else
                ob.first->EraseMapPlaneMatch(ob.second);
        }
        pMP->mnFound += nfound;
        pMP->mnVisible += nvisible;
    }
    void Replace(MapPlane* pMP)
    {
        ReplaceWithoutRebuild(pMP);
        drfe::UpdateCoefficientsAndPoints(*pMP);             /* the observation form, on the host */
    }
};

/* Map::PointDistanceFromPlane */
double point_distance(const drfe_cv::Mat& plane, const Cloud& cl)
{
    double res = 100;
    const float a = plane.ptr<float>(0)[0], b = plane.ptr<float>(1)[0], c = plane.ptr<float>(2)[0], d = plane.ptr<float>(3)[0];
    for (const Point& p : cl.points) {
        const double dis = std::abs(a * p.x + b * p.y + c * p.z + d);
        if (dis < res) res = dis;
    }
    return res;
}

/* the reference's walk against the stand-ins */
int reference_culling(const std::vector<MapPlane*>& planes, std::list<MapPlane*>& recent, KeyFrame* cur, double dTh, double aTh)
{
    int merges = 0;
    for (size_t i = 0; i < planes.size(); i++) {
        int best = -1;
        float ldTh = dTh;
        for (size_t j = i + 1; j < planes.size(); j++) {
            MapPlane *p1 = planes[i], *p2 = planes[j];
            if (p1->isBad() || p2->isBad()) continue;
            const drfe_cv::Mat w1 = p1->GetWorldPos(), w2 = p2->GetWorldPos();
            const float angle = w1.ptr<float>(0)[0] * w2.ptr<float>(0)[0] + w1.ptr<float>(1)[0] * w2.ptr<float>(1)[0] +
                                w1.ptr<float>(2)[0] * w2.ptr<float>(2)[0];
            if (angle > aTh || angle < -aTh) {
                const double dis = point_distance(w1, *p2->mvPlanePoints);
                if (dis < ldTh) { ldTh = dis; best = (int)j; }
            }
        }
        if (best < 0) continue;
        merges++;
        if (planes[i]->Observations() > planes[best]->Observations()) planes[best]->Replace(planes[i]);
        else planes[i]->Replace(planes[best]);
    }
    const int id = (int)cur->mnId;
    for (auto lit = recent.begin(); lit != recent.end();) {
        MapPlane* p = *lit;
        if (p->isBad()) lit = recent.erase(lit);
        else if (p->GetFoundRatio() < 0.25f) { p->SetBadFlag(); lit = recent.erase(lit); }
        else if (id - (int)p->mnFirstKFid >= 2 && p->Observations() <= 2) { p->SetBadFlag(); lit = recent.erase(lit); }
        else if (id - (int)p->mnFirstKFid >= 3) lit = recent.erase(lit);
        else ++lit;
    }
    return merges;
}

/* a Manhattan-style world: walls of three axes, several map planes per wall, each seen from a few key frames */
struct World {
    std::vector<KeyFrame> kfs;
    std::vector<MapPlane> store;
    std::vector<MapPlane*> planes;
    std::list<MapPlane*> recent;
    KeyFrame* cur = nullptr;

    static Cloud patch(std::mt19937& g, int axis, float h, int n)
    {
        std::uniform_real_distribution<float> u(-1.f, 1.f), e(-0.004f, 0.004f);
        Cloud c;
        for (int k = 0; k < n; k++) {
            float v[3];
            v[(axis + 1) % 3] = u(g); v[(axis + 2) % 3] = u(g); v[axis] = h + e(g);
            Point p = {};
            p.x = v[0]; p.y = v[1]; p.z = v[2];
            p.pad = std::nanf("");                             /* only x y z may be read */
            c.points.push_back(p);
        }
        return c;
    }

    World(int n_planes, int n_kfs, unsigned seed)
    {
        std::mt19937 g(seed);
        kfs.resize(n_kfs);
        for (int k = 0; k < n_kfs; k++) {
            kfs[k].mnId = 100 + k;
            kfs[k].Twc = drfe_cv::Mat(4, 4, 4);
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) kfs[k].Twc.ptr<float>(r)[c] = r == c ? 1.f : 0.f;
            kfs[k].Twc.ptr<float>(0)[3] = 0.25f * k;
            kfs[k].Twc.ptr<float>(1)[3] = -0.125f * k;
        }
        cur = &kfs[n_kfs - 1];
        store.resize(n_planes);
        for (int p = 0; p < n_planes; p++) {
            MapPlane& m = store[p];
            const int axis = (int)(g() % 3);
            const float h = 1.5f * (float)(g() % 3) + 0.01f * (float)(g() % 5), sign = g() % 4 ? 1.f : -1.f;
            for (int k = 0; k < 4; k++) m.pos.ptr<float>(k)[0] = 0.f;
            m.pos.ptr<float>(axis)[0] = sign;
            m.pos.ptr<float>(3)[0] = -sign * h;
            *m.mvPlanePoints = patch(g, axis, h, 150 + (int)(g() % 300));
            const int nobs = 1 + (int)(g() % 4);
            for (int o = 0; o < nobs; o++) {
                KeyFrame& kf = kfs[g() % n_kfs];
                if (m.IsInKeyFrame(&kf)) continue;
                Cloud c = patch(g, axis, h, 60 + (int)(g() % 60));
                for (Point& q : c.points) { q.x -= kf.Twc.ptr<float>(0)[3]; q.y -= kf.Twc.ptr<float>(1)[3]; }
                kf.mvPlanePoints.push_back(c);
                kf.mvpMapPlanes.push_back(&m);
                m.AddObservation(&kf, (int)kf.mvPlanePoints.size() - 1);
            }
            m.mnFound = 1 + (int)(g() % 8);
            m.mnVisible = 6 + (int)(g() % 6);
            m.mnFirstKFid = (long)cur->mnId - (long)(g() % 5);
            m.mbBad = g() % 11 == 0;
            planes.push_back(&m);
            if (p >= n_planes - 8) recent.push_back(&m);
        }
    }
};

bool equal(const World& a, const World& b)
{
    for (size_t p = 0; p < a.store.size(); p++) {
        const MapPlane &x = a.store[p], &y = b.store[p];
        if (x.mbBad != y.mbBad || x.nObs != y.nObs || x.mnFound != y.mnFound || x.mnVisible != y.mnVisible) return false;
        if ((x.mpReplaced ? x.mpReplaced - &a.store[0] : -1) != (y.mpReplaced ? y.mpReplaced - &b.store[0] : -1)) return false;
        if (x.mObservations.size() != y.mObservations.size()) return false;
        auto i = x.mObservations.begin();
        auto j = y.mObservations.begin();
        for (; i != x.mObservations.end(); ++i, ++j)
            if (i->first - &a.kfs[0] != j->first - &b.kfs[0] || i->second != j->second) return false;
        const auto &cx = x.mvPlanePoints->points, &cy = y.mvPlanePoints->points;
        if (cx.size() != cy.size()) return false;
        for (size_t k = 0; k < cx.size(); k++)
            if (std::memcmp(&cx[k].x, &cy[k].x, 12)) return false;
    }
    for (size_t k = 0; k < a.kfs.size(); k++)
        for (size_t i = 0; i < a.kfs[k].mvpMapPlanes.size(); i++) {
            const MapPlane *x = a.kfs[k].mvpMapPlanes[i], *y = b.kfs[k].mvpMapPlanes[i];
            if ((x ? x - &a.store[0] : -1) != (y ? y - &b.store[0] : -1)) return false;
        }
    if (a.recent.size() != b.recent.size()) return false;
    auto i = a.recent.begin();
    auto j = b.recent.begin();
    for (; i != a.recent.end(); ++i, ++j)
        if (*i - &a.store[0] != *j - &b.store[0]) return false;
    return true;
}

/* the world's planes as drfe_plane_map_upload takes them */
int upload(drfe_ctx* ctx, const World& w)
{
    const int P = (int)w.planes.size();
    std::vector<int32_t> poff = {0, P}, coff(P + 1, 0), qoff = {0, 0};
    std::vector<float> coefs(4 * (size_t)P), xyz;
    std::vector<uint8_t> bad(P);
    for (int p = 0; p < P; p++) {
        for (int k = 0; k < 4; k++) coefs[4 * (size_t)p + k] = w.planes[p]->pos.ptr<float>(k)[0];
        bad[p] = w.planes[p]->mbBad;
        for (const Point& q : w.planes[p]->mvPlanePoints->points) { xyz.push_back(q.x); xyz.push_back(q.y); xyz.push_back(q.z); }
        coff[p + 1] = (int32_t)(xyz.size() / 3);
    }
    static const float none[3] = {0, 0, 0};
    return drfe_plane_map_upload(ctx, 1, poff.data(), coefs.data(), bad.data(), coff.data(), xyz.data(), qoff.data(), none);
}

int run(drfe_ctx* ctx, unsigned seed, int* merges_out)
{
    World ref(24, 10, seed), got(24, 10, seed);
    if (!equal(ref, got)) return 10;
    if (ctx && upload(ctx, got) != DRFE_OK) return 11;
    const int m1 = reference_culling(ref.planes, ref.recent, ref.cur, 0.1, 0.985);
    const int m2 = drfe::MapPlaneCulling(ctx, 0, got.planes, got.recent, got.cur, 0.1, 0.985);
    if (m1 != m2) return 12;
    if (!equal(ref, got)) return 13;
    if (ctx) {                                                 /* the resident clouds are the objects' clouds */
        for (size_t p = 0; p < got.planes.size(); p++) {
            const auto& pts = got.planes[p]->mvPlanePoints->points;
            int n = 0;
            std::vector<float> xyz(3 * pts.size() + 3);
            if (drfe_plane_map_cloud_download(ctx, 0, (int)p, xyz.data(), (int)pts.size(), &n) != DRFE_OK || n != (int)pts.size()) return 14;
            for (int k = 0; k < n; k++)
                if (std::memcmp(&xyz[3 * (size_t)k], &pts[k].x, 12)) return 15;
        }
    }
    *merges_out += m1;
    return 0;
}

}  // namespace plane_cull_world

#ifndef PLANE_CULL_CALLER_NO_MAIN
int main(int argc, char** argv)
{
    using namespace plane_cull_world;
    const bool host_only = argc > 1 && std::string(argv[1]) == "host";
    try {
        int merges = 0;
        for (unsigned seed = 1; seed <= 4; seed++)
            if (int rc = run(nullptr, seed, &merges)) { std::fprintf(stderr, "host seed %u: %d\n", seed, rc); return rc; }
        if (merges < 8) { std::fprintf(stderr, "the worlds merge too little: %d\n", merges); return 20; }
        if (!host_only) {
            drfe_config cfg = {0, 640, 480, 1, 1000, 1.2f, 8, 20, 7};
            drfe_ctx* ctx = nullptr;
            if (drfe_create(&cfg, &ctx) != DRFE_OK) { std::fprintf(stderr, "drfe_create: %s\n", drfe_last_error(nullptr)); return 21; }
            int dm = 0;
            for (unsigned seed = 1; seed <= 4; seed++)
                if (int rc = run(ctx, seed, &dm)) { std::fprintf(stderr, "device seed %u: %d %s\n", seed, rc, drfe_last_error(ctx)); drfe_destroy(ctx); return 30 + rc; }
            drfe_destroy(ctx);
            if (dm != merges) return 22;
        }
        std::printf("plane_cull_caller ok: %d merges%s\n", merges, host_only ? " (host)" : "");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
#endif
