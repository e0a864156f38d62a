/* fuse_asan.cpp — the host entry of the fuse commit (drfe_lmap_fuse_host, lmap_fuse.cpp with fuse_core.h) as a program of its
 * own, so that the host code can be built with the address and undefined-behaviour sanitizers on its host side only
 * (fuse_asan.mk compiles the store's files and lmap_fuse.cpp into it; no device is opened: the stores have no context).
 *
 * It fills seeded stores through the C setters - key frames in a shuffled rank order, points and lines with up to six observers,
 * stale entries where two items were given one row entry, some items bad - and runs rounds of seeded calls of every form, with
 * every output array exactly as long as its capacity says.  After each call every action is a defined one, every loser is bad
 * in the store and has a `replaced` entry, and the counts are those of a twin store given ample room; what the call computes is
 * held by tests/test_fuse_cpu.py, this program is about memory.  Then the refusals on a store of its own, each
 * followed by the call an untouched twin answers the same way, and each capacity one too small, then exact. */
#include "drfe.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

namespace {

#define REQUIRE(c)                                                            \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("fuse_asan: %s failed at line %d\n", #c, __LINE__);   \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

const int N_KF = 12, ROW = 24, LROW = 12, N_PT = 120, N_LN = 30;

struct World {
    drfe_lmap* db = nullptr;
    std::mt19937 rng;
    explicit World(unsigned seed) : rng(seed)
    {
        REQUIRE(drfe_lmap_create(nullptr, &db) == DRFE_OK);
        std::vector<std::vector<int32_t>> rows(N_KF, std::vector<int32_t>(ROW, -1)), lrows(N_KF, std::vector<int32_t>(LROW, -1));
        std::vector<int32_t> ranks(N_KF);
        for (int k = 0; k < N_KF; k++) ranks[k] = k + 1;
        std::shuffle(ranks.begin(), ranks.end(), rng);
        /* the items first: their observations write the rows */
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
        std::vector<int32_t> kh, parent, nbr(N_KF * 10, -1), coff(1, 0), ch, roff(1, 0), rflat, lroff(1, 0), lflat, octave;
        std::vector<uint64_t> rank;
        std::vector<uint8_t> bad, stereo, flags;
        std::vector<float> th, depth;
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
    }
    ~World() { drfe_lmap_destroy(db); }
};

/* a call with arrays exactly as long as the capacities say */
struct Call {
    std::vector<drfe_lmap_fuse_step> steps;
    std::vector<std::vector<int32_t>> cand, best, rep;
    std::vector<std::vector<uint8_t>> action;
    std::vector<int32_t> fused, rkind, loser, winner, off, rkf, ridx, tp, tl;
    std::vector<uint8_t> moved;
    int32_t nRep = 0, nTouched[2] = {0, 0};
    drfe_lmap_fuse_call c = {};
    void add(int32_t kf, int kind, int form, const std::vector<int32_t>& cs, const std::vector<int32_t>& bs)
    {
        cand.push_back(cs);
        best.push_back(bs);
        rep.emplace_back(cs.size(), -7);
        action.emplace_back(cs.size(), 99);
        drfe_lmap_fuse_step s = {};
        s.keyframe = kf; s.kind = kind; s.form = form; s.n = (int32_t)cs.size();
        steps.push_back(s);
    }
    drfe_lmap_fuse_call* view(int32_t capRep, int32_t capRec, int32_t capTouched)
    {
        fused.assign(steps.size(), -1);
        for (size_t i = 0; i < steps.size(); i++) {
            steps[i].candidates = cand[i].data(); steps[i].best_idx = best[i].data(); steps[i].action = action[i].data();
            steps[i].n_fused = &fused[i]; steps[i].replace = rep[i].data();
        }
        rkind.assign((size_t)capRep, 0); loser.assign((size_t)capRep, 0); winner.assign((size_t)capRep, 0); off.assign((size_t)capRep + 1, 0);
        rkf.assign((size_t)capRec, 0); ridx.assign((size_t)capRec, 0); moved.assign((size_t)capRec, 0);
        tp.assign((size_t)capTouched, 0); tl.assign((size_t)capTouched, 0);
        c = drfe_lmap_fuse_call();
        c.n_steps = (int32_t)steps.size(); c.steps = steps.data(); c.replaced_capacity = capRep; c.record_capacity = capRec; c.touched_capacity = capTouched;
        c.n_replaced = &nRep; c.replaced_kind = rkind.data(); c.loser = loser.data(); c.winner = winner.data(); c.record_offsets = off.data();
        c.record_kf = rkf.data(); c.record_index = ridx.data(); c.record_moved = moved.data(); c.n_touched = nTouched;
        c.touched_points = tp.data(); c.touched_lines = tl.data();
        return &c;
    }
};

void seeded_steps(World& w, Call& call)
{
    for (int s = 0; s < 5; s++) {
        const int32_t kf = 10 * (1 + (int32_t)(w.rng() % N_KF));
        const unsigned u = w.rng() % 100;
        const int kind = u < 25 ? DRFE_LMAP_LINE : DRFE_LMAP_POINT;
        const int form = u < 55 ? DRFE_LMAP_FUSE_NEIGHBOURS : u < 80 ? DRFE_LMAP_FUSE_LOOP : DRFE_LMAP_FUSE_MATCHED;
        const int width = kind == DRFE_LMAP_LINE ? LROW : ROW, pool = kind == DRFE_LMAP_LINE ? N_LN : N_PT, base = kind == DRFE_LMAP_LINE ? 5000 : 1000;
        std::vector<int32_t> cs, bs;
        const int n = form == DRFE_LMAP_FUSE_MATCHED ? width : 40;
        for (int i = 0; i < n; i++) {
            const bool null = form == DRFE_LMAP_FUSE_MATCHED ? w.rng() % 10 < 7 : form == DRFE_LMAP_FUSE_NEIGHBOURS && w.rng() % 10 == 0;
            cs.push_back(null ? -1 : base + (int32_t)(w.rng() % pool));
            bs.push_back(w.rng() % 2 ? (int32_t)(w.rng() % width) : -1);
        }
        call.add(kf, kind, form, cs, bs);
    }
}

/* the exact sizes of a call: a run with ample room on a twin store */
void sizes_of(unsigned seed, int rounds, int32_t out[3])
{
    World w(seed);
    for (int r = 0; r <= rounds; r++) {
        Call call;
        seeded_steps(w, call);
        REQUIRE(drfe_lmap_fuse_host(w.db, call.view(4096, 65536, 4096)) == DRFE_OK);
        out[0] = call.nRep;
        out[1] = call.off[(size_t)call.nRep];
        out[2] = std::max(call.nTouched[0], call.nTouched[1]);
    }
}

void hold_to_the_store(World& w, const Call& call)
{
    for (size_t s = 0; s < call.steps.size(); s++)
        for (size_t i = 0; i < call.cand[s].size(); i++) REQUIRE(call.action[s][i] <= DRFE_LMAP_FUSE_RECORDED);
    for (int r = 0; r < call.nRep; r++) {
        uint8_t bad = 0;
        int32_t n = -1, rep = -2, none[1];
        /* its observers are not looked at: a loser may win again later in the call, as a bad candidate of MATCHED or of a pass 2 */
        const int rc = drfe_lmap_get_observers(w.db, call.rkind[(size_t)r], call.loser[(size_t)r], 0, &bad, &n, none);
        REQUIRE((rc == DRFE_OK || rc == DRFE_ERR_CAPACITY) && bad == 1);
        REQUIRE(drfe_lmap_get_replaced(w.db, call.rkind[(size_t)r], 1, &call.loser[(size_t)r], &rep) == DRFE_OK && rep >= 0);
    }
}

void refusals()
{
    World w(7), twin(7);
    auto refused = [&](int kf, int kind, int form, std::vector<int32_t> cs, std::vector<int32_t> bs, int rc) {
        Call bad;
        bad.add(kf, kind, form, cs, bs);
        REQUIRE(drfe_lmap_fuse_host(w.db, bad.view(64, 1024, 64)) == rc);
        REQUIRE(std::string(drfe_lmap_last_error(w.db)).find("lmap_fuse") != std::string::npos);
    };
    refused(999, DRFE_LMAP_POINT, DRFE_LMAP_FUSE_NEIGHBOURS, {1000}, {1}, DRFE_ERR_INVALID);
    refused(10, DRFE_LMAP_POINT, DRFE_LMAP_FUSE_NEIGHBOURS, {4242}, {1}, DRFE_ERR_INVALID);
    refused(10, DRFE_LMAP_POINT, 9, {1000}, {1}, DRFE_ERR_INVALID);
    refused(10, 0, DRFE_LMAP_FUSE_NEIGHBOURS, {1000}, {1}, DRFE_ERR_INVALID);
    refused(10, DRFE_LMAP_LINE, DRFE_LMAP_FUSE_LOOP, {5000}, {1}, DRFE_ERR_STATE);
    refused(10, DRFE_LMAP_POINT, DRFE_LMAP_FUSE_LOOP, {1000, -1}, {1, 2}, DRFE_ERR_STATE);
    refused(10, DRFE_LMAP_POINT, DRFE_LMAP_FUSE_MATCHED, {1000, 1001}, {0, 0}, DRFE_ERR_STATE);
    refused(10, DRFE_LMAP_POINT, DRFE_LMAP_FUSE_NEIGHBOURS, {1000}, {ROW}, DRFE_ERR_STATE);
    refused(10, DRFE_LMAP_LINE, DRFE_LMAP_FUSE_NEIGHBOURS, {5000}, {LROW}, DRFE_ERR_STATE);
    /* each capacity one too small, then exact, against the twin */
    int32_t need[3];
    sizes_of(7, 0, need);
    REQUIRE(need[0] > 0 && need[1] > 0 && need[2] > 0);
    for (int which = 0; which < 3; which++) {
        Call small;
        World probe(7);
        seeded_steps(probe, small);
        int32_t caps[3] = {need[0], need[1], need[2]};
        caps[which]--;
        REQUIRE(drfe_lmap_fuse_host(w.db, small.view(caps[0], caps[1], caps[2])) == DRFE_ERR_CAPACITY);
    }
    Call a, b;
    seeded_steps(w, a);
    seeded_steps(twin, b);
    REQUIRE(drfe_lmap_fuse_host(w.db, a.view(need[0], need[1], need[2])) == DRFE_OK);
    REQUIRE(drfe_lmap_fuse_host(twin.db, b.view(need[0], need[1], need[2])) == DRFE_OK);
    REQUIRE(a.nRep == b.nRep && a.loser == b.loser && a.winner == b.winner && a.rkf == b.rkf && a.ridx == b.ridx && a.moved == b.moved);
    REQUIRE(a.action == b.action && a.fused == b.fused && a.rep == b.rep && a.tp == b.tp && a.tl == b.tl);
    int64_t st[8];
    REQUIRE(drfe_lmap_fuse_stats(w.db, st) == DRFE_OK && st[0] == 1 && st[2] == 0 && st[7] == 0);
}

}  // namespace

int main()
{
    int calls = 0, replaced = 0, records = 0;
    for (unsigned seed = 1; seed <= 6; seed++) {
        World w(seed);
        for (int round = 0; round < 4; round++) {
            int32_t need[3];
            sizes_of(seed, round, need);
            Call call;
            seeded_steps(w, call);
            REQUIRE(drfe_lmap_fuse_host(w.db, call.view(need[0], need[1], need[2])) == DRFE_OK);
            REQUIRE(call.nRep == need[0] && call.off[(size_t)call.nRep] == need[1]);
            hold_to_the_store(w, call);
            calls++;
            replaced += call.nRep;
            records += need[1];
        }
    }
    refusals();
    std::printf("fuse_asan ok (host, %d calls, %d replaced, %d records, refusals)\n", calls, replaced, records);
    return 0;
}
