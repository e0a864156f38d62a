/* recent_cull_asan.cpp — the host entry of LocalMapping::MapPointCulling and MapLineCulling (drfe_lmap_recent_cull_host,
 * lmap_recent.cpp with recent_core.h) as a program of its own, so that the host code can be built with the address and
 * undefined-behaviour sanitizers on its host side only (recent_cull_asan.mk compiles the store's files and lmap_recent.cpp into
 * it; no device is opened: the stores have no context).
 *
 * It runs what recent_cull_caller.cpp runs in host mode - eight calls through the adaptor on stand-in objects, the store compared
 * with the objects after each - and then the refusals on a store of its own: an unknown handle, a listed item without
 * attributes, an obs_index outside its observer's row, a line observation that names an unknown key frame, the two undefined line
 * divisions, and each of the two capacities one too small, then exact.  After each refusal the call that follows must answer as
 * on an untouched twin. */
#define RECENT_CULL_CALLER_NO_MAIN
#include "recent_cull_caller.cpp"

#include <climits>

namespace {

using namespace recent_world;

struct Lists {
    std::vector<int32_t> h[2], kept[2], culled[2], off[2], erKf[2], erIdx[2];
    std::vector<uint8_t> action[2];
    int32_t nKept[2] = {0, 0}, nCulled[2] = {0, 0};
    drfe_lmap_recent_list l[2];
    /* every array is exactly as long as its capacity says */
    void view(const std::vector<int32_t>& pts, const std::vector<int32_t>& lns, const int64_t caps[2])
    {
        h[0] = pts;
        h[1] = lns;
        for (int k = 0; k < 2; k++) {
            const size_t n = h[k].size();
            action[k].assign(n, 9); kept[k].assign(n, 0); culled[k].assign(n, 0); off[k].assign(n + 1, 0);
            erKf[k].assign((size_t)caps[k], 0); erIdx[k].assign((size_t)caps[k], 0);
            l[k] = drfe_lmap_recent_list();
            l[k].n = (int32_t)n; l[k].handles = h[k].data(); l[k].erased_capacity = (int32_t)caps[k];
            l[k].action = action[k].data(); l[k].n_kept = &nKept[k]; l[k].kept = kept[k].data(); l[k].n_culled = &nCulled[k];
            l[k].culled = culled[k].data(); l[k].erased_offsets = off[k].data(); l[k].erased_kf = erKf[k].data(); l[k].erased_index = erIdx[k].data();
        }
    }
    bool same(const Lists& o) const
    {
        for (int k = 0; k < 2; k++) {
            if (action[k] != o.action[k] || nKept[k] != o.nKept[k] || nCulled[k] != o.nCulled[k]) return false;
            if (!std::equal(kept[k].begin(), kept[k].begin() + nKept[k], o.kept[k].begin())) return false;
            if (!std::equal(culled[k].begin(), culled[k].begin() + nCulled[k], o.culled[k].begin())) return false;
            if (!std::equal(off[k].begin(), off[k].begin() + nCulled[k] + 1, o.off[k].begin())) return false;
            const int32_t t = off[k][(size_t)nCulled[k]];
            if (!std::equal(erKf[k].begin(), erKf[k].begin() + t, o.erKf[k].begin()) || !std::equal(erIdx[k].begin(), erIdx[k].begin() + t, o.erIdx[k].begin()))
                return false;
        }
        return true;
    }
};

int expect(drfe_lmap* db, int rc, int want, const char* what, const char* names = nullptr)
{
    if (rc != want) return fail(what, rc, want);
    if (names && std::string(drfe_lmap_last_error(db)).find(names) == std::string::npos) {
        std::fprintf(stderr, "recent_cull_asan: %s: \"%s\" does not name \"%s\"\n", what, drfe_lmap_last_error(db), names);
        return 1;
    }
    return 0;
}

int refusals()
{
    World W(20, 200, 80, 9), W2(20, 200, 80, 9);
    Tracker T(-1), T2(-1);
    W.sync(T);
    W2.sync(T2);
    drfe_lmap *db = T.db(), *twin = T2.db();
    std::vector<int32_t> pts, lns;
    for (MapPoint* p : W.recentPoints) pts.push_back((int32_t)p->mnId);
    for (MapLine* l : W.recentLines) lns.push_back((int32_t)l->mnId);
    const int64_t cur = 21, big[2] = {1 << 14, 1 << 14};
    /* what the call needs, from the twin */
    Lists want;
    want.view(pts, lns, big);
    if (drfe_lmap_recent_cull_host(twin, cur, 0, &want.l[0], &want.l[1]) != DRFE_OK) return fail(drfe_lmap_last_error(twin));
    const int64_t need[2] = {want.off[0][(size_t)want.nCulled[0]], want.off[1][(size_t)want.nCulled[1]]};
    if (need[0] < 10 || need[1] < 10) return fail("the call erases too little to test the capacities", (long)need[0], (long)need[1]);
    Lists L;
    /* an unknown handle */
    std::vector<int32_t> bad = pts;
    bad.push_back(77777);
    L.view(bad, lns, big);
    if (expect(db, drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]), DRFE_ERR_INVALID, "an unknown handle")) return 1;
    /* a stored point and line without attributes, listed */
    {
        const int32_t h = 5000, off[2] = {0, 0};
        const uint8_t b = 0;
        drfe_lmap_set_points(db, 1, &h, &b, off, nullptr);
        drfe_lmap_set_lines(db, 1, &h, &b);
        L.view(bad = {5000}, {}, big);
        if (expect(db, drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]), DRFE_ERR_STATE, "a point without attributes", "map point 5000")) return 1;
        L.view({}, {5000}, big);
        if (expect(db, drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]), DRFE_ERR_STATE, "a line without attributes", "map line 5000")) return 1;
        drfe_lmap_remove(db, DRFE_LMAP_POINT, h);
        drfe_lmap_remove(db, DRFE_LMAP_LINE, h);
    }
    /* a line that is kept by the twin's call, with bad attributes in turn */
    const int32_t line = want.kept[1][0];
    int32_t found = 0, visible = 0, nObs = 0, off[2] = {0, 0};
    int64_t first = 0;
    std::vector<int32_t> obs(64), idx(64);
    drfe_lmap_recent_attributes_out g = {};
    g.n_lines = 1; g.line_obs_capacity = 64; g.line_handle = &line; g.line_found = &found; g.line_visible = &visible; g.line_first_kf = &first;
    g.line_n_obs = &nObs; g.line_obs_offsets = off; g.line_obs = obs.data(); g.line_obs_index = idx.data();
    if (drfe_lmap_get_recent_attributes(db, &g) != DRFE_OK) return fail(drfe_lmap_last_error(db));
    auto put = [&](int32_t f, int32_t v, const std::vector<int32_t>& o, const std::vector<int32_t>& i) {
        const int32_t o2[2] = {0, (int32_t)o.size()};
        drfe_lmap_recent_attributes a = {};
        a.n_lines = 1; a.line_handle = &line; a.line_found = &f; a.line_visible = &v; a.line_first_kf = &first; a.line_n_obs = &nObs;
        a.line_obs_offsets = o2; a.line_obs = o.data(); a.line_obs_index = i.data();
        return drfe_lmap_set_recent_attributes(db, &a);
    };
    const std::vector<int32_t> o0(obs.begin(), obs.begin() + off[1]), i0(idx.begin(), idx.begin() + off[1]);
    const std::string name = "map line " + std::to_string(line);
    L.view(pts, lns, big);
    put(found, visible, {1}, {1 << 20});
    if (expect(db, drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]), DRFE_ERR_STATE, "an obs_index outside the row", "obs_index 1048576")) return 1;
    put(found, visible, {4242}, {0});
    if (expect(db, drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]), DRFE_ERR_STATE, "an unknown observer", "unknown handle 4242")) return 1;
    put(5, 0, o0, i0);
    if (expect(db, drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]), DRFE_ERR_STATE, "a division by zero", name.c_str())) return 1;
    put(INT_MIN, -1, o0, i0);
    if (expect(db, drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]), DRFE_ERR_STATE, "INT_MIN / -1", name.c_str())) return 1;
    if (put(found, visible, {3, 3}, {0, 1}) != DRFE_ERR_INVALID) return fail("a key frame twice in a line's observations");
    put(found, visible, o0, i0);
    /* each capacity one too small */
    for (int k = 0; k < 2; k++) {
        int64_t caps[2] = {need[0], need[1]};
        caps[k]--;
        L.view(pts, lns, caps);
        if (expect(db, drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]), DRFE_ERR_CAPACITY, "a capacity one too small", "than erased_capacity")) return 1;
    }
    int64_t st[8];
    drfe_lmap_recent_cull_stats(db, st);
    if (st[0] != 0) return fail("a refused call was counted", (long)st[0]);
    /* the exact sizes: the same answer as the twin's, and the same store afterwards */
    L.view(pts, lns, need);
    if (drfe_lmap_recent_cull_host(db, cur, 0, &L.l[0], &L.l[1]) != DRFE_OK) return fail(drfe_lmap_last_error(db));
    want.erKf[0].resize((size_t)need[0]); want.erIdx[0].resize((size_t)need[0]);
    want.erKf[1].resize((size_t)need[1]); want.erIdx[1].resize((size_t)need[1]);
    if (!L.same(want)) return fail("after the refusals the call answers differently");
    std::vector<int32_t> a, b;
    int64_t f1 = 100, f2 = 100;
    if (local_maps(db, W, &f1, false, a) || local_maps(twin, W2, &f2, false, b)) return 1;
    if (a != b) return fail("after the refusals the stores differ");
    return 0;
}

}  // namespace

int main()
{
    try {
        if (recent_world::run(false)) return 1;
        if (refusals()) return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "recent_cull_asan: %s\n", e.what());
        return 1;
    }
    std::printf("recent_cull_asan ok\n");
    return 0;
}
