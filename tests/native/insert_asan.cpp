/* insert_asan.cpp — the host entry of the item loops of ProcessNewKeyFrame (drfe_lmap_insert_host, lmap_insert.cpp with
 * insert_core.h) as a program of its own, so that the host code can be built with the address and undefined-behaviour sanitizers
 * on its host side only (insert_asan.mk compiles the store's files and lmap_insert.cpp into it; no device is opened: the stores
 * have no context).
 *
 * It fills seeded stores through the C setters - key frames in a shuffled rank order, points and lines with up to six observers,
 * rows that name items which do not observe the key frame yet, some of them twice, some items bad - and runs rounds of seeded
 * calls with and without normals, with every output array exactly as long as its capacity says.  After each call every action is
 * a defined one and the counts are those of the lists; what the call computes is held by tests/test_insert_cpu.py, this program
 * is about memory.  Then the refusals, each leaving the next call to succeed, and each capacity one too small, then exact. */
#include "drfe.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

namespace {

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::printf("insert_asan: %s failed at line %d\n", #c, __LINE__);   \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

const int N_KF = 12, ROW = 24, LROW = 12, N_PT = 120, N_LN = 30;

struct World {
    drfe_lmap* db = nullptr;
    std::mt19937 rng;
    World(unsigned seed, bool geometry, int pointWithout = -1) : rng(seed)
    {
        REQUIRE(drfe_lmap_create(nullptr, &db) == DRFE_OK);
        std::vector<std::vector<int32_t>> rows(N_KF, std::vector<int32_t>(ROW, -1)), lrows(N_KF, std::vector<int32_t>(LROW, -1));
        std::vector<int32_t> ranks(N_KF);
        for (int k = 0; k < N_KF; k++) ranks[k] = k + 1;
        std::shuffle(ranks.begin(), ranks.end(), rng);
        std::vector<int32_t> ph, poff(1, 0), pobs, pidx, pn, lh, loff(1, 0), lobs, lidx, ln;
        std::vector<uint8_t> pbad, lbad;
        for (int kind = 0; kind < 2; kind++)
            for (int i = 0; i < (kind ? N_LN : N_PT); i++) {
                const int32_t h = (kind ? 5000 : 1000) + i;
                std::vector<int32_t> ks(N_KF);
                for (int k = 0; k < N_KF; k++) ks[k] = k;
                std::shuffle(ks.begin(), ks.end(), rng);
                const int n = (int)(rng() % 7);
                for (int o = 0; o < n; o++) {
                    const int32_t idx = (int32_t)(rng() % (kind ? LROW : ROW));
                    (kind ? lobs : pobs).push_back(10 * (ks[o] + 1));
                    (kind ? lidx : pidx).push_back(idx);
                    (kind ? lrows : rows)[ks[o]][idx] = h;
                }
                (kind ? lh : ph).push_back(h);
                (kind ? loff : poff).push_back((int32_t)(kind ? lobs : pobs).size());
                (kind ? ln : pn).push_back(n + (int)(rng() % 2));
                (kind ? lbad : pbad).push_back(rng() % 12 == 0);
            }
        /* what tracking leaves: entries that name items which do not observe the key frame, now and then one twice */
        for (int k = 0; k < N_KF; k++) {
            for (int i = 0; i < ROW; i++)
                if (rows[k][i] < 0 && rng() % 2) rows[k][i] = 1000 + (int32_t)(rng() % N_PT);
            for (int i = 0; i < LROW; i++)
                if (lrows[k][i] < 0 && rng() % 2) lrows[k][i] = 5000 + (int32_t)(rng() % N_LN);
            rows[k][ROW - 1] = rows[k][0];
        }
        std::vector<int32_t> kh, parent, nbr(N_KF * 10, -1), coff(1, 0), ch, roff(1, 0), rflat, lroff(1, 0), lflat, octave;
        std::vector<uint64_t> rank;
        std::vector<uint8_t> bad, stereo, flags;
        std::vector<float> th, depth, T;
        for (int k = 0; k < N_KF; k++) {
            kh.push_back(10 * (k + 1));
            rank.push_back((uint64_t)ranks[k]);
            bad.push_back(k == 3);
            parent.push_back(-1);
            coff.push_back(0);
            rflat.insert(rflat.end(), rows[k].begin(), rows[k].end());
            roff.push_back((int32_t)rflat.size());
            lflat.insert(lflat.end(), lrows[k].begin(), lrows[k].end());
            lroff.push_back((int32_t)lflat.size());
            th.push_back(40.0f);
            flags.push_back(0);
            for (int i = 0; i < ROW; i++) {
                octave.push_back(0);
                depth.push_back(1.0f);
                stereo.push_back(rng() % 2);
            }
            const float pose[16] = {1, 0, 0, -0.25f * (float)k, 0, 1, 0, 0.5f, 0, 0, 1, 0, 0, 0, 0, 1};
            T.insert(T.end(), pose, pose + 16);
        }
        drfe_lmap_keyframes K = {};
        K.count = N_KF; K.handle = kh.data(); K.rank = rank.data(); K.bad = bad.data(); K.parent = parent.data(); K.neighbours = nbr.data();
        K.child_offsets = coff.data(); K.children = ch.data(); K.point_offsets = roff.data(); K.points = rflat.data();
        K.line_offsets = lroff.data(); K.lines = lflat.data();
        REQUIRE(drfe_lmap_set_keyframes(db, &K) == DRFE_OK);
        REQUIRE(drfe_lmap_set_points(db, N_PT, ph.data(), pbad.data(), poff.data(), pobs.data()) == DRFE_OK);
        REQUIRE(drfe_lmap_set_lines(db, N_LN, lh.data(), lbad.data()) == DRFE_OK);
        drfe_lmap_cull_attributes A = {};
        A.n_kfs = N_KF; A.n_points = N_PT; A.kf_handle = kh.data(); A.th_depth = th.data(); A.kf_flags = flags.data(); A.row_offsets = roff.data();
        A.octave = octave.data(); A.depth = depth.data(); A.stereo = stereo.data(); A.point_handle = ph.data(); A.n_obs = pn.data();
        A.obs_offsets = poff.data(); A.obs_index = pidx.data();
        REQUIRE(drfe_lmap_set_cull_attributes(db, &A) == DRFE_OK);
        std::vector<int32_t> one(N_PT, 3), lone(N_LN, 3);
        std::vector<int64_t> first(N_PT, 0), lfirst(N_LN, 0);
        drfe_lmap_recent_attributes R = {};
        R.n_points = N_PT; R.n_lines = N_LN; R.point_handle = ph.data(); R.point_found = one.data(); R.point_visible = one.data();
        R.point_first_kf = first.data(); R.line_handle = lh.data(); R.line_found = lone.data(); R.line_visible = lone.data();
        R.line_first_kf = lfirst.data(); R.line_n_obs = ln.data(); R.line_obs_offsets = loff.data(); R.line_obs = lobs.data();
        R.line_obs_index = lidx.data();
        REQUIRE(drfe_lmap_set_recent_attributes(db, &R) == DRFE_OK);
        if (!geometry) return;
        const float scales[3] = {1.0f, 1.2f, 1.44f};
        REQUIRE(drfe_lmap_set_scales(db, 3, scales) == DRFE_OK);
        REQUIRE(drfe_lmap_set_poses(db, N_KF, kh.data(), T.data()) == DRFE_OK);
        std::vector<int32_t> gh, ref, level;
        std::vector<float> world;
        for (int i = 0; i < N_PT; i++) {
            if (i == pointWithout) continue;
            gh.push_back(1000 + i);
            ref.push_back(10 * (1 + i % N_KF));
            level.push_back(i % 3);
            for (int k = 0; k < 3; k++) world.push_back(0.5f * (float)((i + k) % 9) + 0.125f);
        }
        drfe_lmap_point_geometry G = {};
        G.count = (int32_t)gh.size(); G.handle = gh.data(); G.world = world.data(); G.ref_kf = ref.data(); G.ref_level = level.data();
        REQUIRE(drfe_lmap_set_point_geometry(db, &G) == DRFE_OK);
    }
    ~World() { drfe_lmap_destroy(db); }
};

/* a call with arrays exactly as long as the capacities say */
struct Call {
    std::vector<int32_t> handles, poff, loff, ap, apk, api, al, alk, ali, rp, rl;
    std::vector<uint8_t> pact, lact, status;
    std::vector<float> nrm, maxD, minD;
    int32_t nAdded[2] = {0, 0}, nRecent[2] = {0, 0};
    drfe_lmap_insert_call c = {};
    drfe_lmap_insert_call* view(const std::vector<int32_t>& hs, bool normals, int32_t capAction, int32_t capAdded, int32_t capRecent)
    {
        handles = hs;
        const size_t n = hs.size(), a = (size_t)capAction, d = (size_t)capAdded, r = (size_t)capRecent;
        poff.assign(n + 1, -1); loff.assign(n + 1, -1);
        pact.assign(a, 99); lact.assign(a, 99);
        ap.assign(d, -1); apk.assign(d, -1); api.assign(d, -1); al.assign(d, -1); alk.assign(d, -1); ali.assign(d, -1);
        nrm.assign(3 * d, 0.0f); maxD.assign(d, 0.0f); minD.assign(d, 0.0f); status.assign(d, 99);
        rp.assign(r, -1); rl.assign(r, -1);
        c = drfe_lmap_insert_call{};
        c.n = (int32_t)n; c.handles = handles.data();
        for (int k = 0; k < 2; k++) {
            c.action_capacity[k] = capAction;
            c.added_capacity[k] = capAdded;
            c.recent_capacity[k] = capRecent;
        }
        c.point_offsets = poff.data(); c.point_action = pact.data(); c.line_offsets = loff.data(); c.line_action = lact.data();
        c.n_added = nAdded; c.added_points = ap.data(); c.added_point_kf = apk.data(); c.added_point_index = api.data();
        c.normal = normals ? nrm.data() : nullptr; c.max_distance = maxD.data(); c.min_distance = minD.data(); c.status = status.data();
        c.added_lines = al.data(); c.added_line_kf = alk.data(); c.added_line_index = ali.data();
        c.n_recent = nRecent; c.recent_points = rp.data(); c.recent_lines = rl.data();
        return &c;
    }
    void check() const
    {
        int32_t added[2] = {0, 0}, recent[2] = {0, 0};
        for (int k = 0; k < 2; k++) {
            const std::vector<int32_t>& off = k ? loff : poff;
            const std::vector<uint8_t>& act = k ? lact : pact;
            REQUIRE(off[0] == 0);
            for (int32_t e = 0; e < off.back(); e++) {
                REQUIRE(act[(size_t)e] <= DRFE_LMAP_INSERT_ADDED);
                added[k] += act[(size_t)e] == DRFE_LMAP_INSERT_ADDED;
                recent[k] += act[(size_t)e] == DRFE_LMAP_INSERT_RECENT;
            }
            REQUIRE(added[k] == nAdded[k] && recent[k] == nRecent[k]);
        }
        if (c.normal)
            for (int32_t t = 0; t < nAdded[0]; t++) REQUIRE(status[(size_t)t] == DRFE_UPKEEP_NORMAL);
    }
};

std::vector<int32_t> some_keyframes(std::mt19937& rng, int n)
{
    std::vector<int32_t> ks(N_KF);
    for (int k = 0; k < N_KF; k++) ks[k] = 10 * (k + 1);
    std::shuffle(ks.begin(), ks.end(), rng);
    ks.resize((size_t)n);
    return ks;
}

}  // namespace

int main()
{
    int64_t calls = 0;
    for (unsigned seed = 1; seed <= 6; seed++) {
        World w(seed, true);
        for (int round = 0; round < 4; round++) {
            const std::vector<int32_t> hs = some_keyframes(w.rng, round == 3 ? 0 : 1 + (int)(w.rng() % 5));
            const int32_t cap = (int32_t)hs.size() * ROW;
            Call c;
            REQUIRE(drfe_lmap_insert_host(w.db, c.view(hs, round % 2 == 0, cap, cap, cap)) == DRFE_OK);
            c.check();
            /* the same key frames again: nothing is left to add, and the lists fit exactly */
            Call again;
            const int32_t seenP = c.nAdded[0] + c.nRecent[0], seenL = c.nAdded[1] + c.nRecent[1];
            REQUIRE(drfe_lmap_insert_host(w.db, again.view(hs, round % 2 == 1, cap, 0, std::max(seenP, seenL))) == DRFE_OK);
            again.check();
            REQUIRE(again.nAdded[0] == 0 && again.nAdded[1] == 0 && again.nRecent[0] == seenP && again.nRecent[1] == seenL);
            calls += 2;
        }
    }
    {
        /* the refusals: nothing changes, so the call that follows finds what an untouched twin finds */
        World w(77, true), twin(77, true);
        Call c, t;
        const std::vector<int32_t> hs = {10, 20, 30};
        const int32_t cap = 3 * ROW;
        REQUIRE(drfe_lmap_insert_host(w.db, c.view({10, 999}, true, cap, cap, cap)) == DRFE_ERR_INVALID);
        REQUIRE(drfe_lmap_insert_host(w.db, c.view({10, 20, 10}, true, cap, cap, cap)) == DRFE_ERR_INVALID);
        REQUIRE(drfe_lmap_insert_host(w.db, c.view(hs, true, cap - 1, cap, cap)) == DRFE_ERR_CAPACITY);
        REQUIRE(drfe_lmap_insert_host(twin.db, t.view(hs, true, cap, cap, cap)) == DRFE_OK);
        REQUIRE(t.nAdded[0] > 1 && t.nRecent[0] > 0 && t.nAdded[1] > 0);
        REQUIRE(drfe_lmap_insert_host(w.db, c.view(hs, true, cap, t.nAdded[0] - 1, cap)) == DRFE_ERR_CAPACITY);
        REQUIRE(drfe_lmap_insert_host(w.db, c.view(hs, true, cap, cap, std::max(t.nRecent[0], t.nRecent[1]) - 1)) == DRFE_ERR_CAPACITY);
        const int32_t exact = std::max(t.nAdded[0], t.nAdded[1]), exactRecent = std::max(t.nRecent[0], t.nRecent[1]);
        REQUIRE(drfe_lmap_insert_host(w.db, c.view(hs, true, cap, exact, exactRecent)) == DRFE_OK);
        c.check();
        REQUIRE(c.pact == t.pact && c.lact == t.lact && c.nAdded[0] == t.nAdded[0] && c.nRecent[1] == t.nRecent[1]);
        for (int32_t i = 0; i < c.nAdded[0]; i++) REQUIRE(c.ap[(size_t)i] == t.ap[(size_t)i] && c.maxD[(size_t)i] == t.maxD[(size_t)i]);
        /* a store without geometry: refused with normals, served without; one point without a position: refused when it is added */
        World bare(78, false);
        REQUIRE(drfe_lmap_insert_host(bare.db, c.view(hs, true, cap, cap, cap)) == DRFE_ERR_STATE);
        REQUIRE(drfe_lmap_insert_host(bare.db, c.view(hs, false, cap, cap, cap)) == DRFE_OK);
        c.check();
        World hole(77, true, t.ap[0] - 1000);
        REQUIRE(drfe_lmap_insert_host(hole.db, c.view(hs, true, cap, cap, cap)) == DRFE_ERR_STATE);
        REQUIRE(std::string(drfe_lmap_last_error(hole.db)).find(std::to_string(t.ap[0])) != std::string::npos);
        REQUIRE(drfe_lmap_insert_host(hole.db, c.view(hs, false, cap, cap, cap)) == DRFE_OK);
        calls += 4;
    }
    std::printf("insert_asan: %lld calls, clean\n", (long long)calls);
    return 0;
}
