/* conn_asan.cpp — a seeded script on the host entries of the local-map store (drfe_lmap_connect_host with conn_core.h,
 * drfe_lmap_get_connections, drfe_lmap_update_host), as a program of its own so that the host code can be built with
 * the address and undefined-behaviour sanitizers on its host side only (conn_asan.mk compiles lmap_store.cpp, lmap.cpp and lmap_conn.cpp into it; no device is
 * opened: the store has no context).
 *
 * 60 calls of 1 .. 12 key frames on a clustered graph of 80 key frames, with bad flags set, rows replaced and a key frame removed
 * (its mentions purged) between them, every call followed by a read-back of all rows and an UpdateLocalMap query, once with
 * every capacity too small.  It checks what can be checked without a second implementation: return codes, that a refused
 * call changed nothing, that an edge's weight is the caller's vote, and that every list is sorted by (weight, rank). */
#include "drfe.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

namespace {

struct Rng {
    uint64_t s;
    int below(int n)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((s >> 33) % (uint64_t)n);
    }
};

void must(int rc, const char* what, drfe_lmap* db)
{
    if (rc == DRFE_OK) return;
    fprintf(stderr, "conn_asan: %s failed (%d): %s\n", what, rc, drfe_lmap_last_error(db));
    exit(2);
}

struct Rows {
    std::vector<int32_t> wOff, wKf, wW, oOff, oKf, oW, parent;
    std::vector<uint8_t> first;
    drfe_lmap_conn_rows view(size_t rows, size_t cap)
    {
        wOff.assign(rows + 1, 0); oOff.assign(rows + 1, 0); parent.assign(rows + 1, 0); first.assign(rows + 1, 0);
        wKf.assign(cap + 1, 0); wW.assign(cap + 1, 0); oKf.assign(cap + 1, 0); oW.assign(cap + 1, 0);
        drfe_lmap_conn_rows r = {};
        r.weights_capacity = r.ordered_capacity = (int32_t)cap;
        r.weight_offsets = wOff.data(); r.weight_kfs = wKf.data(); r.weight_w = wW.data();
        r.ordered_offsets = oOff.data(); r.ordered_kfs = oKf.data(); r.ordered_w = oW.data();
        r.parent = parent.data(); r.first_connection = first.data();
        return r;
    }
};

}  // namespace

int main()
{
    Rng r{99};
    const int nKf = 80, row = 70;
    std::vector<std::vector<int32_t>> kfPoints((size_t)nKf), obs;
    std::vector<uint8_t> mpBad;
    for (int i = 0; i < nKf; i++)
        for (int k = 0; k < row; k++) {
            std::set<int32_t> o;
            o.insert(i);
            for (int j = r.below(5); j > 0; j--) o.insert(std::min(nKf - 1, std::max(0, i - 4 + r.below(9))));
            const int32_t p = (int32_t)obs.size();
            obs.push_back(std::vector<int32_t>(o.begin(), o.end()));
            mpBad.push_back(r.below(20) == 0);
            for (int32_t kf : o)
                if ((int)kfPoints[(size_t)kf].size() < (kf % 7 == 3 ? 12 : row)) kfPoints[(size_t)kf].push_back(r.below(20) ? p : -1);
        }
    drfe_lmap* db = nullptr;
    if (drfe_lmap_create(nullptr, &db) != DRFE_OK) return 2;
    std::vector<uint64_t> rank((size_t)nKf);
    for (int i = 0; i < nKf; i++) rank[(size_t)i] = (uint64_t)((i * 37) % nKf) * 4096 + 8;
    std::set<int32_t> live;
    auto put_kf = [&](int32_t h) {
        const uint8_t bad = 0;
        const int32_t parent = -1, nbr[DRFE_LMAP_NEIGHBOURS] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, zero[2] = {0, 0};
        const int32_t pOff[2] = {0, (int32_t)kfPoints[(size_t)h].size()};
        drfe_lmap_keyframes k = {};
        k.count = 1;
        k.handle = &h; k.rank = &rank[(size_t)h]; k.bad = &bad; k.parent = &parent; k.neighbours = nbr; k.child_offsets = zero;
        k.children = zero; k.point_offsets = pOff; k.points = kfPoints[(size_t)h].data(); k.line_offsets = zero; k.lines = zero;
        must(drfe_lmap_set_keyframes(db, &k), "set_keyframes", db);
    };
    auto put_points = [&]() {
        std::vector<int32_t> h, off(1, 0), flat;
        for (size_t p = 0; p < obs.size(); p++) {
            h.push_back((int32_t)p);
            flat.insert(flat.end(), obs[p].begin(), obs[p].end());
            off.push_back((int32_t)flat.size());
        }
        must(drfe_lmap_set_points(db, (int32_t)h.size(), h.data(), mpBad.data(), off.data(), flat.data()), "set_points", db);
    };
    for (int32_t h = 0; h < nKf; h++) {
        put_kf(h);
        live.insert(h);
        const uint8_t first = h != 0;
        const int32_t zero[2] = {0, 0};
        drfe_lmap_connections c = {};
        c.count = 1;
        c.handle = &h; c.first_connection = &first; c.weight_offsets = zero; c.ordered_offsets = zero;
        must(drfe_lmap_set_connections(db, &c), "set_connections", db);
    }
    put_points();
    int64_t frameId = 1, checkedEdges = 0, checkedLists = 0;
    for (int call = 0; call < 60; call++) {
        std::vector<int32_t> pool(live.begin(), live.end()), hs;
        for (int n = 1 + r.below(12); n > 0 && !pool.empty(); n--) {
            const size_t at = (size_t)r.below((int)pool.size());
            hs.push_back(pool[at]);
            pool.erase(pool.begin() + (std::ptrdiff_t)at);
        }
        const size_t n = hs.size(), nK = live.size(), cap = nK * nK;
        std::vector<int32_t> cOff(n + 1), cKf(n * nK + 1), cV(n * nK + 1), rec(4 * n), np(n), touched(nK + 1);
        std::vector<uint8_t> flags(nK + 1);
        int32_t nTouched = 0;
        Rows R;
        drfe_lmap_connect_out o = {};
        o.counter_capacity = (int32_t)(n * nK); o.touched_capacity = (int32_t)nK;
        o.counter_offsets = cOff.data(); o.counter_kfs = cKf.data(); o.counter_votes = cV.data(); o.record = rec.data();
        o.new_parent = np.data(); o.n_touched = &nTouched; o.touched = touched.data(); o.flags = flags.data();
        o.rows = R.view(nK, cap);
        if (call == 7) {
            /* every array too small: refused, and the same call then gives what it would have given */
            drfe_lmap_connect_out small = o;
            small.counter_capacity = 0; small.touched_capacity = 0; small.rows.weights_capacity = small.rows.ordered_capacity = 0;
            if (drfe_lmap_connect_host(db, (int32_t)n, hs.data(), &small) != DRFE_ERR_CAPACITY) return 3;
        }
        must(drfe_lmap_connect_host(db, (int32_t)n, hs.data(), &o), "connect_host", db);
        /* a listed entry of a called key frame's counter is its edge: the target's final row holds the weight of the last
         * writer, which is the caller when the target is not called after it */
        std::map<int32_t, size_t> posOf, tOf;
        for (size_t p = 0; p < n; p++) posOf[hs[p]] = p;
        for (int32_t t = 0; t < nTouched; t++) tOf[touched[(size_t)t]] = (size_t)t;
        for (size_t p = 0; p < n; p++)
            for (int32_t i = cOff[p]; i < cOff[p + 1]; i++) {
                const int32_t j = cKf[(size_t)i], w = cV[(size_t)i];
                if (w < DRFE_LMAP_CONNECT_TH && !(rec[4 * p + 1] == 1 && rec[4 * p + 3] == j && rec[4 * p + 2] < DRFE_LMAP_CONNECT_TH)) continue;
                if (posOf.count(j) && posOf[j] > p && rec[4 * posOf[j]] > 0) continue;
                const size_t t = tOf.at(j);
                bool found = false;
                for (int32_t e = R.wOff[t]; e < R.wOff[t + 1]; e++) found |= R.wKf[(size_t)e] == hs[p] && R.wW[(size_t)e] == w;
                if (!found) {
                    fprintf(stderr, "conn_asan: call %d: the edge %d -> %d (%d) is not in the target's row\n", call, hs[p], j, w);
                    return 1;
                }
                checkedEdges++;
            }
        for (int32_t t = 0; t < nTouched; t++)
            for (int32_t e = R.oOff[(size_t)t] + 1; e < R.oOff[(size_t)t + 1]; e++) {
                const int32_t a = R.oKf[(size_t)e - 1], b = R.oKf[(size_t)e], wa = R.oW[(size_t)e - 1], wb = R.oW[(size_t)e];
                if (wa < wb || (wa == wb && rank[(size_t)a] < rank[(size_t)b])) {
                    fprintf(stderr, "conn_asan: call %d: the list of %d is out of order\n", call, touched[(size_t)t]);
                    return 1;
                }
                checkedLists++;
            }
        /* read every row back, then UpdateLocalMap on the committed graph */
        std::vector<int32_t> all(live.begin(), live.end()), chOff(all.size() + 1), ch(cap + 1);
        Rows G;
        drfe_lmap_conn_rows g = G.view(all.size(), cap);
        must(drfe_lmap_get_connections(db, (int32_t)all.size(), all.data(), &g, (int32_t)cap, chOff.data(), ch.data()), "get_connections", db);
        {
            int32_t size[3];
            must(drfe_lmap_size(db, size), "size", db);
            const std::vector<int32_t>& pts = kfPoints[(size_t)hs[0]];
            const int32_t pOff[2] = {0, (int32_t)pts.size()};
            std::vector<int32_t> kfOff(2), kfs((size_t)size[0] + 1), ref(1), mpOff(2), mps((size_t)size[1] + 1), mlOff(2), mls(1), nuOff(2), nulled(pts.size() + 1), record(4);
            std::vector<uint8_t> mpIn((size_t)size[1] + 1), mlIn(1);
            drfe_lmap_queries q = {};
            q.n = 1; q.frame_id = &frameId; q.point_offsets = pOff; q.points = pts.data();
            drfe_lmap_out u = {};
            u.kf_capacity = size[0]; u.mp_capacity = size[1]; u.ml_capacity = 0; u.nulled_capacity = (int32_t)pts.size();
            u.kf_offsets = kfOff.data(); u.kfs = kfs.data(); u.ref_kf = ref.data(); u.mp_offsets = mpOff.data(); u.mps = mps.data();
            u.mp_in_frame = mpIn.data(); u.ml_offsets = mlOff.data(); u.mls = mls.data(); u.ml_in_frame = mlIn.data();
            u.nulled_offsets = nuOff.data(); u.nulled = nulled.data(); u.record = record.data();
            must(drfe_lmap_update_host(db, &q, &u), "update_host", db);
            frameId++;
        }
        /* edits */
        const int what = r.below(4);
        if (what == 0) {
            const int32_t h = *std::next(live.begin(), r.below((int)live.size()));
            const uint8_t f = (uint8_t)r.below(2);
            must(drfe_lmap_set_bad(db, DRFE_LMAP_KEYFRAME, 1, &h, &f), "set_bad", db);
            const int32_t p = r.below((int)obs.size());
            mpBad[(size_t)p] = (uint8_t)r.below(2);
            must(drfe_lmap_set_bad(db, DRFE_LMAP_POINT, 1, &p, &mpBad[(size_t)p]), "set_bad", db);
        } else if (what == 1 && call % 9 == 4 && live.size() > 40) {
            /* a key frame leaves: every mention of it goes from the observations, the rows of the others are read back and purged */
            const int32_t gone = *std::next(live.begin(), r.below((int)live.size()));
            for (auto& o2 : obs)
                for (size_t i = 0; i < o2.size(); i++)
                    if (o2[i] == gone) o2.erase(o2.begin() + (std::ptrdiff_t)i--);
            live.erase(gone);
            must(drfe_lmap_remove(db, DRFE_LMAP_KEYFRAME, gone), "remove", db);
            put_points();
            for (size_t k = 0; k < all.size(); k++) {
                if (all[k] == gone) continue;
                std::vector<int32_t> wKf, wW, oKf, oW;
                for (int32_t e = G.wOff[k]; e < G.wOff[k + 1]; e++)
                    if (G.wKf[(size_t)e] != gone) wKf.push_back(G.wKf[(size_t)e]), wW.push_back(G.wW[(size_t)e]);
                for (int32_t e = G.oOff[k]; e < G.oOff[k + 1]; e++)
                    if (G.oKf[(size_t)e] != gone) oKf.push_back(G.oKf[(size_t)e]), oW.push_back(G.oW[(size_t)e]);
                const int32_t wOff[2] = {0, (int32_t)wKf.size()}, oOff[2] = {0, (int32_t)oKf.size()};
                drfe_lmap_connections c = {};
                c.count = 1;
                c.handle = &all[k]; c.first_connection = &G.first[k]; c.weight_offsets = wOff; c.weight_kfs = wKf.data(); c.weight_w = wW.data();
                c.ordered_offsets = oOff; c.ordered_kfs = oKf.data(); c.ordered_w = oW.data();
                must(drfe_lmap_set_connections(db, &c), "set_connections", db);
                put_kf(all[k]);          /* parent, neighbours and children of the rows go back to none */
            }
        } else if (what == 2) {
            const int32_t h = *std::next(live.begin(), r.below((int)live.size()));
            if (kfPoints[(size_t)h].size() > 8) kfPoints[(size_t)h].resize(kfPoints[(size_t)h].size() - 7);
            put_kf(h);
        }
    }
    int64_t st[8];
    must(drfe_lmap_connect_stats(db, st), "connect_stats", db);
    drfe_lmap_destroy(db);
    if (st[0] != 60 || checkedEdges < 100 || checkedLists < 100) return 4;
    printf("conn_asan ok (60 calls, %lld key frames, %lld edges and %lld list steps checked)\n", (long long)st[1], (long long)checkedEdges,
           (long long)checkedLists);
    return 0;
}
