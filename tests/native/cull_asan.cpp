/* cull_asan.cpp — the host entry of LocalMapping::KeyFrameCulling (drfe_lmap_cull_host, lmap_cull.cpp with cull_core.h) as a
 * program of its own, so that the host code can be built with the address and undefined-behaviour sanitizers on its host side
 * only (cull_asan.mk compiles the store's files and lmap_cull.cpp into it; no device is opened: the stores have no context).
 *
 * It runs what cull_caller.cpp runs in host mode - seven calls through the adaptor on stand-in objects, every store row compared
 * with the objects after each - and then the paths that take work back: every output capacity one too small in turn
 * (DRFE_ERR_CAPACITY), and a key frame that the walk culls after others while the store holds no parent for it
 * (DRFE_ERR_STATE).  After each refusal every row of the store must still equal the untouched objects. */
#define CULL_CALLER_NO_MAIN
#include "cull_caller.cpp"

namespace {

using namespace cull_world;

struct Out {
    std::vector<int32_t> rec, culled, touched, parent, wOff, oOff, chOff, nuOff, wKf, wW, oKf, oW, ch, nu, pts, pN, pRef, obOff, ob, obIdx;
    std::vector<float> Tcp;
    std::vector<uint8_t> has, flags, first, pBad;
    int32_t nCulled = 0, nTouched = 0, nPoints = 0;
    /* caps: touched, weights, ordered, children, nulled, points, obs; every array is exactly as long as its capacity says */
    drfe_lmap_cull_out view(size_t n, const int64_t caps[7])
    {
        const size_t t = (size_t)caps[0];
        rec.assign(4 * n, 0); culled.assign(n, 0); Tcp.assign(16 * n, 0.0f); has.assign(n, 0);
        touched.assign(t, 0); flags.assign(t, 0); parent.assign(t, 0); first.assign(t, 0);
        wOff.assign(t + 1, 0); oOff.assign(t + 1, 0); chOff.assign(t + 1, 0); nuOff.assign(t + 1, 0);
        wKf.assign((size_t)caps[1], 0); wW.assign((size_t)caps[1], 0); oKf.assign((size_t)caps[2], 0); oW.assign((size_t)caps[2], 0);
        ch.assign((size_t)caps[3], 0); nu.assign((size_t)caps[4], 0);
        pts.assign((size_t)caps[5], 0); pN.assign((size_t)caps[5], 0); pRef.assign((size_t)caps[5], 0); pBad.assign((size_t)caps[5], 0);
        obOff.assign((size_t)caps[5] + 1, 0); ob.assign((size_t)caps[6], 0); obIdx.assign((size_t)caps[6], 0);
        drfe_lmap_cull_out o = {};
        o.touched_capacity = (int32_t)caps[0]; o.rows.weights_capacity = (int32_t)caps[1]; o.rows.ordered_capacity = (int32_t)caps[2];
        o.children_capacity = (int32_t)caps[3]; o.nulled_capacity = (int32_t)caps[4]; o.points_capacity = (int32_t)caps[5];
        o.obs_capacity = (int32_t)caps[6];
        o.record = rec.data(); o.Tcp = Tcp.data(); o.has_Tcp = has.data(); o.n_culled = &nCulled; o.culled = culled.data();
        o.n_touched = &nTouched; o.touched = touched.data(); o.flags = flags.data();
        o.rows.weight_offsets = wOff.data(); o.rows.weight_kfs = wKf.data(); o.rows.weight_w = wW.data();
        o.rows.ordered_offsets = oOff.data(); o.rows.ordered_kfs = oKf.data(); o.rows.ordered_w = oW.data();
        o.rows.parent = parent.data(); o.rows.first_connection = first.data();
        o.children_offsets = chOff.data(); o.children = ch.data(); o.nulled_offsets = nuOff.data(); o.nulled = nu.data();
        o.n_points = &nPoints; o.points = pts.data(); o.point_n_obs = pN.data(); o.point_ref = pRef.data(); o.point_bad = pBad.data();
        o.obs_offsets = obOff.data(); o.obs = ob.data(); o.obs_index = obIdx.data();
        return o;
    }
};

int refusals()
{
    /* two equal worlds: one call on the second tells what the same call on the first needs */
    World W(40, 30, 7), W2(40, 30, 7);
    Tracker T(-1), T2(-1);
    W.sync(T, true);
    W2.sync(T2, true);
    std::vector<int32_t> handles;
    for (KeyFrame* k : W.kfs[3].GetVectorCovisibleKeyFrames()) handles.push_back((int32_t)k->mnId);
    const int32_t n = (int32_t)handles.size();
    const int64_t big[7] = {64, 1 << 14, 1 << 14, 1 << 12, 1 << 14, 1 << 14, 1 << 17};
    Out probe;
    drfe_lmap_cull_out o = probe.view((size_t)n, big);
    if (drfe_lmap_cull_host(T2.db(), n, handles.data(), 0, &o) != DRFE_OK || probe.nCulled < 2) {
        fprintf(stderr, "cull_asan: the probing call: rc or %d culled: %s\n", probe.nCulled, drfe_lmap_last_error(T2.db()));
        return 1;
    }
    const int64_t need[7] = {probe.nTouched, probe.wOff[(size_t)probe.nTouched], probe.oOff[(size_t)probe.nTouched],
                             probe.chOff[(size_t)probe.nTouched], probe.nuOff[(size_t)probe.nTouched], probe.nPoints,
                             probe.obOff[(size_t)probe.nPoints]};
    int64_t frameId = 10;
    int refused = 0;
    for (int which = 0; which < 7; which++) {
        if (need[which] == 0) continue;
        int64_t caps[7];
        for (int k = 0; k < 7; k++) caps[k] = need[k];
        caps[which]--;
        Out out;
        o = out.view((size_t)n, caps);
        const int rc = drfe_lmap_cull_host(T.db(), n, handles.data(), 0, &o);
        if (rc != DRFE_ERR_CAPACITY) {
            fprintf(stderr, "cull_asan: capacity %d one too small gave %d\n", which, rc);
            return 1;
        }
        refused++;
        compare(T, W, frameId);
    }
    /* a key frame the call culls late loses its parent in the store: everything the earlier ones did is taken back.  Its parent
     * must not be culled before it, or the spanning-tree loop would hand it a new one in time. */
    std::set<int32_t> gone(probe.culled.begin(), probe.culled.begin() + probe.nCulled);
    int pick = 0;
    for (int i = probe.nCulled - 1; i > 0; i--)
        if (!gone.count((int32_t)W.kfs[(size_t)probe.culled[(size_t)i]].mpParent->mnId)) {
            pick = i;
            break;
        }
    KeyFrame& last = W.kfs[(size_t)probe.culled[(size_t)pick]];
    KeyFrame* keep = last.mpParent;
    last.mpParent = nullptr;
    T.Sync(&last);
    last.mpParent = keep;
    Out out;
    o = out.view((size_t)n, big);
    const int rc = drfe_lmap_cull_host(T.db(), n, handles.data(), 0, &o);
    if (rc != DRFE_ERR_STATE || std::string(drfe_lmap_last_error(T.db())).find("no parent") == std::string::npos) {
        fprintf(stderr, "cull_asan: the key frame without a parent gave %d: %s\n", rc, drfe_lmap_last_error(T.db()));
        return 1;
    }
    T.Sync(&last);
    compare(T, W, frameId);
    /* and the exact sizes suffice: the same bytes as the probing call */
    Out exact;
    o = exact.view((size_t)n, need);
    if (drfe_lmap_cull_host(T.db(), n, handles.data(), 0, &o) != DRFE_OK || exact.rec != probe.rec || exact.nu != std::vector<int32_t>(probe.nu.begin(), probe.nu.begin() + need[4]) ||
        exact.ob != std::vector<int32_t>(probe.ob.begin(), probe.ob.begin() + need[6])) {
        fprintf(stderr, "cull_asan: the call with exact capacities: %s\n", drfe_lmap_last_error(T.db()));
        return 1;
    }
    printf("cull_asan: %d capacity refusals and one late refusal undone\n", refused);
    return fails ? 1 : 0;
}

}  // namespace

int main()
{
    int calls = 0, deferred = 0;
    const int culled = cull_world::run("host", &calls, &deferred);
    if (cull_world::fails || culled < 3) {
        fprintf(stderr, "cull_asan: %d differences, %d culled\n", cull_world::fails, culled);
        return 1;
    }
    if (refusals()) return 1;
    printf("cull_asan ok (%d calls, %d culled)\n", calls, culled);
    return 0;
}
