/* plane_cull_asan.cpp — the host entry of LocalMapping::MapPlaneCulling (drfe_plane_map_cull_host, plane_cull.cpp with
 * plane_cull_core.h) as a program of its own, so that the host code can be built with the address and undefined-behaviour
 * sanitizers on its host side only (plane_cull_asan.mk compiles plane_cull.cpp into it; no device is opened).
 *
 * It runs what plane_cull_caller.cpp runs in host mode - two worlds through the adaptor on stand-in objects, every plane, match
 * vector and the recent list compared with the reference's walk - and then the paths that give work back: a rebuilt_capacity one
 * point too small (DRFE_ERR_CAPACITY) and observations out of key-frame order (DRFE_ERR_INVALID). */
#define PLANE_CULL_CALLER_NO_MAIN
#include "plane_cull_caller.cpp"

namespace {

using namespace plane_cull_world;

/* two planes of one wall, one observation each; returns the entry's status with the given capacity and observation order */
int small_call(int capacity, bool ordered, int* rebuilt_points)
{
    const float coefs[8] = {0, 0, 1, 0, 0, 0, 1, -0.03125f};
    const uint8_t bad[2] = {0, 0};
    std::vector<float> cloud;
    for (int k = 0; k < 40; k++) { cloud.push_back(0.1f * (float)(k % 8)); cloud.push_back(0.1f * (float)(k / 8)); cloud.push_back(k < 20 ? 0.f : 0.03125f); }
    const int32_t coff[3] = {0, 20, 40}, found[2] = {5, 5}, visible[2] = {6, 6}, nobs[2] = {2, 2}, first[2] = {9, 9};
    const int32_t ooff[3] = {0, 2, 4}, okf[4] = {0, 1, ordered ? 1 : 2, ordered ? 2 : 1}, oidx[4] = {0, 0, 1, 0};
    const float* oc[4] = {cloud.data(), cloud.data() + 30, cloud.data() + 60, cloud.data() + 90};
    const int32_t on[4] = {10, 10, 10, 10}, recent[3] = {1, 0, -1};
    float Twc[48] = {0};
    for (int k = 0; k < 3; k++) Twc[16 * k] = Twc[16 * k + 5] = Twc[16 * k + 10] = Twc[16 * k + 15] = 1.f;
    drfe_plane_cull_in in = {};
    in.n_planes = 2; in.n_kfs = 3; in.n_recent = 3; in.current_kf_id = 10; in.dTh = 0.1; in.aTh = 0.985;
    in.found = found; in.visible = visible; in.n_obs = nobs; in.first_kf_id = first; in.obs_offsets = ooff; in.obs_kf = okf; in.obs_idx = oidx;
    in.obs_cloud = oc; in.obs_cloud_n = on; in.obs_cloud_stride = 12; in.Twc = Twc; in.recent = recent;
    int32_t events[4], oN[2], oF[2], oV[2], rebuilt[2], rOff[3];
    uint8_t oBad[2], verdicts[3];
    std::vector<float> xyz(3 * (size_t)capacity);            /* exactly as long as the capacity says */
    drfe_plane_cull_out out = {};
    out.events = events; out.bad = oBad; out.n_obs = oN; out.found = oF; out.visible = oV; out.rebuilt = rebuilt; out.rebuilt_offsets = rOff;
    out.rebuilt_xyz = xyz.data(); out.rebuilt_capacity = capacity; out.verdicts = verdicts;
    const int rc = drfe_plane_map_cull_host(&in, coefs, bad, coff, cloud.data(), &out);
    if (rc == DRFE_OK) {
        if (out.n_events != 1 || events[0] != 0 || events[1] != 1 || out.n_rebuilt != 1 || oN[1] != 3 || verdicts[0] != DRFE_PLANE_CULL_KEPT ||
            verdicts[1] != DRFE_PLANE_CULL_ERASED_BAD || verdicts[2] != DRFE_PLANE_CULL_ERASED_BAD)
            return 100;
        *rebuilt_points = rOff[1];
    }
    return rc;
}

}  // namespace

int main()
{
    int merges = 0;
    for (unsigned seed = 1; seed <= 2; seed++)
        if (int rc = run(nullptr, seed, &merges)) { std::fprintf(stderr, "seed %u: %d\n", seed, rc); return rc; }
    int n = 0, m = 0;
    if (int rc = small_call(64, true, &n)) { std::fprintf(stderr, "small call: %d\n", rc); return 40; }
    if (n < 1 || small_call(n, true, &m) != DRFE_OK || m != n) return 41;
    if (small_call(n - 1, true, &m) != DRFE_ERR_CAPACITY) return 42;
    if (small_call(64, false, &m) != DRFE_ERR_INVALID) return 43;
    std::printf("plane_cull_asan ok: %d merges, %d rebuilt points\n", merges, n);
    return 0;
}
