/* lmap_fuse.cpp — the fuse commit on the local-map store, behind the C-ABI of include/drfe.h: ORBmatcher::Fuse and LSDmatcher::Fuse
 * (reference src/ORBmatcher.cc:845-976, src/LSDmatcher.cpp:897-1012), the Sim3 form with SearchAndFuse's loop (:1001-1101,
 * src/LoopClosing.cc:650-657), the matched-point loop of CorrectLoop (src/LoopClosing.cc:566-581), with MapPoint::Replace /
 * MapLine::Replace and AddObservation.  The checks, the host walk, the device entry (fuse_kernels.hip), the replay that commits
 * either walk's decisions to the rows by handle and to the image, and the counters.  Both sides evaluate fuse_core.h.  The host
 * walk runs on the image under a journal and is undone; one replay then applies what either walk decided - marking for upload what
 * the host entry changed, and only the spliced observation arrays after the device entry, which stored the rest in the resident
 * blocks itself.  DESIGN.md section 32.  Parity with a build of the reference's ORBmatcher.cc, LSDmatcher.cpp, MapPoint.cc,
 * MapLine.cpp and LoopClosing.cc is not pinned: they cannot be built here. */
#include "lmap_call.h"

#include <algorithm>
#include <cstring>
#include <unordered_set>

using namespace lmap_store;

namespace {

/* the arrays of one kind by slot */
struct KindView {
    std::vector<uint8_t>* bad;
    std::vector<int32_t>*nObs, *found, *visible, *row, *obsOff, *obs, *obsIdx;
    const std::vector<int32_t>*rowOff, *handle;
    const std::vector<uint8_t>* has;
    const char* name;
};

KindView kind_view(drfe_lmap* db, int kind)
{
    Image& G = db->img;
    RecentAttr& Q = db->rec;
    if (kind == FUSE_POINT)
        return KindView{&G.mpBad, &db->cull.nObs, &Q.mpFound, &Q.mpVisible, &G.kfMp, &G.obsOff, &G.obs, &db->cull.obsIdx, &G.kfMpOff, &G.mpHandle, &Q.mpHas, "map point"};
    return KindView{&G.mlBad, &Q.mlNObs, &Q.mlFound, &Q.mlVisible, &G.kfMl, &Q.mlObsOff, &Q.mlObs, &Q.mlObsIdx, &G.kfMlOff, &G.mlHandle, &Q.mlHas, "map line"};
}

/* a place in the walk: step, pass, flat candidate */
struct Cursor {
    int32_t step, pass, cand;
    bool operator<(const Cursor& o) const { return step != o.step ? step < o.step : pass != o.pass ? pass < o.pass : cand < o.cand; }
};

/* a checked call, in slots */
struct FusePlan {
    std::vector<FuseStep> step;
    std::vector<int32_t> tileStep, cand, best;
    int32_t live = 0, liveKind[2] = {0, 0};
    bool is_live(const FuseStep& S, int32_t c) const { return fuse_live(S.form, cand[(size_t)c], best[(size_t)c]); }
    int32_t index(const FuseStep& S, int32_t c) const { return S.form == FUSE_MATCHED ? c - S.candOff : best[(size_t)c]; }
    Cursor end() const { return Cursor{(int32_t)step.size(), 0, 0}; }
};

/* what a walk decided */
struct FuseWork {
    std::vector<uint8_t> action, recMoved;
    std::vector<int32_t> rep, nFused, rKind, rLoser, rWinner, rOff, recKf, recIdx;     /* slots */
    size_t replayed = 0;                       /* Replace calls the replay has applied */
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

bool call_ok(const drfe_lmap_fuse_call* c)
{
    if (!c || c->n_steps < 0 || (c->n_steps > 0 && !c->steps) || c->replaced_capacity < 0 || c->record_capacity < 0 || c->touched_capacity < 0 ||
        !c->n_replaced || !c->record_offsets || !c->n_touched)
        return false;
    if (c->replaced_capacity > 0 && (!c->replaced_kind || !c->loser || !c->winner)) return false;
    if (c->record_capacity > 0 && (!c->record_kf || !c->record_index || !c->record_moved)) return false;
    if (c->touched_capacity > 0 && (!c->touched_points || !c->touched_lines)) return false;
    for (int s = 0; s < c->n_steps; s++) {
        const drfe_lmap_fuse_step& S = c->steps[s];
        if (S.n < 0 || !S.n_fused) return false;
        if (S.n > 0 && (!S.candidates || !S.action || (S.form != DRFE_LMAP_FUSE_MATCHED && !S.best_idx) || (S.form == DRFE_LMAP_FUSE_LOOP && !S.replace)))
            return false;
    }
    return true;
}

int fuse_plan(drfe_lmap* db, const drfe_lmap_fuse_call* c, FusePlan& P)
{
    int64_t total = 0;
    for (int s = 0; s < c->n_steps; s++) total += c->steps[s].n;
    if (total > DRFE_LMAP_FUSE_MAX_CANDIDATES) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_fuse: more than DRFE_LMAP_FUSE_MAX_CANDIDATES candidates in a call");
    const int rc = lmap_build_recent(db);
    if (rc) return rc;
    const Image& G = db->img;
    P.cand.reserve((size_t)total);
    P.best.reserve((size_t)total);
    /* every item the call could touch, with the forms it takes part in */
    std::vector<uint8_t> part[2];
    part[0].assign(G.mpHandle.size(), 0);
    part[1].assign(G.mlHandle.size(), 0);
    for (int s = 0; s < c->n_steps; s++) {
        const drfe_lmap_fuse_step& S = c->steps[s];
        const std::string who = "lmap_fuse: step " + std::to_string(s);
        if (S.kind != DRFE_LMAP_POINT && S.kind != DRFE_LMAP_LINE) return lmap_fail(db, DRFE_ERR_INVALID, who + ": unknown kind");
        if (S.form != DRFE_LMAP_FUSE_NEIGHBOURS && S.form != DRFE_LMAP_FUSE_LOOP && S.form != DRFE_LMAP_FUSE_MATCHED)
            return lmap_fail(db, DRFE_ERR_INVALID, who + ": unknown form");
        const auto kf = G.kfSlot.find(S.keyframe);
        if (kf == G.kfSlot.end()) return lmap_fail(db, DRFE_ERR_INVALID, who + " names unknown key frame " + std::to_string(S.keyframe));
        const int kind = S.kind == DRFE_LMAP_POINT ? FUSE_POINT : FUSE_LINE;
        if (kind == FUSE_LINE && S.form != DRFE_LMAP_FUSE_NEIGHBOURS) return lmap_fail(db, DRFE_ERR_STATE, who + ": the form is for map points, the step names map lines");
        const KindView V = kind_view(db, kind);
        const std::unordered_map<int32_t, int32_t>& slot = kind == FUSE_POINT ? G.mpSlot : G.mlSlot;
        const size_t k = (size_t)kf->second;
        const int32_t rowBase = (*V.rowOff)[k], rowLen = (*V.rowOff)[k + 1] - rowBase;
        if (S.form == DRFE_LMAP_FUSE_MATCHED && S.n != rowLen)
            return lmap_fail(db, DRFE_ERR_STATE, who + ": a MATCHED list of " + std::to_string(S.n) + " candidates on key frame " + std::to_string(S.keyframe) + " whose row has " + std::to_string(rowLen));
        if (kind == FUSE_POINT && db->cull.kfHas[k] != 2)
            return lmap_fail(db, DRFE_ERR_STATE, who + ": key frame " + std::to_string(S.keyframe) + " has no culling attributes that fit its row");
        FuseStep F{};
        F.kf = kf->second;
        F.kind = kind;
        F.form = S.form;
        F.n = S.n;
        F.candOff = (int32_t)P.cand.size();
        F.tile0 = (int32_t)P.tileStep.size();
        F.tile1 = F.tile0 + (S.n + FUSE_TILE - 1) / FUSE_TILE;
        P.tileStep.insert(P.tileStep.end(), (size_t)(F.tile1 - F.tile0), s);
        for (int i = 0; i < S.n; i++) {
            int32_t item = -1;
            const int32_t b = S.form == DRFE_LMAP_FUSE_MATCHED ? i : (S.best_idx[i] < 0 ? -1 : S.best_idx[i]);
            if (S.candidates[i] >= 0) {
                const auto it = slot.find(S.candidates[i]);
                if (it == slot.end()) return lmap_fail(db, DRFE_ERR_INVALID, who + " names unknown " + V.name + " " + std::to_string(S.candidates[i]));
                item = it->second;
            } else if (S.form == DRFE_LMAP_FUSE_LOOP) {
                return lmap_fail(db, DRFE_ERR_STATE, who + ": a null candidate at " + std::to_string(i) + " in the LOOP form");
            }
            if (b >= rowLen)
                return lmap_fail(db, DRFE_ERR_STATE, who + ": best_idx " + std::to_string(b) + " of candidate " + std::to_string(i) + " lies outside the row of key frame " + std::to_string(S.keyframe));
            P.cand.push_back(item);
            P.best.push_back(b);
            if (!fuse_live(S.form, item, b)) continue;
            P.live++;
            P.liveKind[kind]++;
            const uint8_t bit = S.form == DRFE_LMAP_FUSE_MATCHED ? 2 : 1;
            part[kind][(size_t)item] |= bit;
            const int32_t occ = (*V.row)[(size_t)(rowBase + b)];
            if (occ >= 0) part[kind][(size_t)occ] |= bit;
        }
        P.step.push_back(F);
    }
    if (db->rec.complete) return DRFE_OK;
    for (int kind = 0; kind < 2; kind++) {
        const KindView V = kind_view(db, kind);
        for (size_t s = 0; s < part[kind].size(); s++) {
            /* NEIGHBOURS and LOOP never touch an item that is bad when the call begins */
            if (!part[kind][s] || (part[kind][s] == 1 && (*V.bad)[s])) continue;
            const std::string who = std::string("lmap_fuse: ") + V.name + " " + std::to_string((*V.handle)[s]);
            if (!(*V.has)[s])
                return lmap_fail(db, DRFE_ERR_STATE, who + (kind == FUSE_POINT ? " has no recent-list counters, or no culling attributes that fit its observations"
                                                                              : " has no recent-list state"));
            for (int32_t o = (*V.obsOff)[s]; o < (*V.obsOff)[s + 1]; o++) {
                const size_t k = (size_t)(*V.obs)[(size_t)o];
                const int32_t idx = (*V.obsIdx)[(size_t)o];
                if (idx < 0 || idx >= (*V.rowOff)[k + 1] - (*V.rowOff)[k])
                    return lmap_fail(db, DRFE_ERR_STATE, who + ": obs_index " + std::to_string(idx) + " lies outside the row of key frame " + std::to_string(G.kfHandle[k]));
            }
        }
    }
    return DRFE_OK;
}

/* the place of a new observer in a stored list: in front of the first stored observer of greater rank (slot) */
template <class List, class SlotOf>
size_t rank_place(const List& l, int32_t kf, SlotOf slot_of)
{
    size_t at = 0;
    while (at < l.size() && slot_of(l[at]) <= kf) at++;
    return at;
}

/* The reference's loops on the image, candidate after candidate, every Replace to its end before the next one.  The arrays of
 * the image are written in place under a journal, the observation lists of the items it touches are copies. */
struct HostWalk {
    drfe_lmap* db;
    const FusePlan& P;
    FuseWork& W;
    KindView V[2];
    const std::vector<uint8_t>& stereo;
    std::unordered_map<int32_t, std::vector<std::pair<int32_t, int32_t>>> lists[2];
    std::vector<std::pair<int32_t*, int32_t>> j32;
    std::vector<std::pair<uint8_t*, uint8_t>> j8;
    std::vector<int32_t> snap;

    HostWalk(drfe_lmap* d, const FusePlan& p, FuseWork& w) : db(d), P(p), W(w), V{kind_view(d, 0), kind_view(d, 1)}, stereo(d->cull.stereo)
    {
        snap.assign(d->img.mpHandle.size(), 0);
    }
    void set(int32_t& x, int32_t v)
    {
        j32.emplace_back(&x, x);
        x = v;
    }
    void undo()
    {
        for (size_t i = j32.size(); i-- > 0;) *j32[i].first = j32[i].second;
        for (size_t i = j8.size(); i-- > 0;) *j8[i].first = j8[i].second;
        j32.clear();
        j8.clear();
    }
    std::vector<std::pair<int32_t, int32_t>>& list(int kind, int32_t item)
    {
        const auto it = lists[kind].find(item);
        if (it != lists[kind].end()) return it->second;
        std::vector<std::pair<int32_t, int32_t>>& l = lists[kind][item];
        for (int32_t o = (*V[kind].obsOff)[(size_t)item]; o < (*V[kind].obsOff)[(size_t)item + 1]; o++)
            l.emplace_back((*V[kind].obs)[(size_t)o], (*V[kind].obsIdx)[(size_t)o]);
        return l;
    }
    bool member(int kind, int32_t item, int32_t kf)
    {
        for (const auto& e : list(kind, item))
            if (e.first == kf) return true;
        return false;
    }
    void gain(int kind, int32_t item, int32_t kf, int32_t idx)
    {
        auto& l = list(kind, item);
        l.insert(l.begin() + (ptrdiff_t)rank_place(l, kf, [](const std::pair<int32_t, int32_t>& e) { return e.first; }), std::make_pair(kf, idx));
        const size_t at = (size_t)(*V[kind].rowOff)[(size_t)kf] + (size_t)idx;
        int32_t& n = (*V[kind].nObs)[(size_t)item];
        set(n, n + fuse_obs_weight(kind, kind == FUSE_POINT ? stereo[at] : 0));
    }
    void add(int kind, int32_t item, int32_t kf, int32_t idx, bool gains)
    {
        set((*V[kind].row)[(size_t)(*V[kind].rowOff)[(size_t)kf] + (size_t)idx], item);
        if (gains) gain(kind, item, kf, idx);
    }
    void replace(int kind, int32_t loser, int32_t winner)
    {
        const KindView& K = V[kind];
        uint8_t& bad = (*K.bad)[(size_t)loser];
        j8.emplace_back(&bad, bad);
        bad = 1;
        std::vector<std::pair<int32_t, int32_t>> obs;
        obs.swap(list(kind, loser));
        W.rKind.push_back(kind);
        W.rLoser.push_back(loser);
        W.rWinner.push_back(winner);
        for (const auto& e : obs) {
            const bool moved = !member(kind, winner, e.first);
            set((*K.row)[(size_t)(*K.rowOff)[(size_t)e.first] + (size_t)e.second], moved ? winner : -1);
            if (moved) gain(kind, winner, e.first, e.second);
            W.recKf.push_back(e.first);
            W.recIdx.push_back(e.second);
            W.recMoved.push_back(moved ? 1 : 0);
        }
        W.rOff.push_back((int32_t)W.recKf.size());
        set((*K.found)[(size_t)winner], fuse_wrap_add((*K.found)[(size_t)winner], (*K.found)[(size_t)loser]));
        set((*K.visible)[(size_t)winner], fuse_wrap_add((*K.visible)[(size_t)winner], (*K.visible)[(size_t)loser]));
    }
    /* from `from` to the end of the call; resumed: the step at `from` has begun (its snapshot is in the actions, `fused` counted) */
    void run(Cursor from, bool resumed, int32_t fused0)
    {
        for (int32_t s = from.step; s < (int32_t)P.step.size(); s++) {
            const FuseStep& S = P.step[(size_t)s];
            const KindView& K = V[S.kind];
            const bool mid = resumed && s == from.step;
            const size_t rowBase = (size_t)(*K.rowOff)[(size_t)S.kf];
            int32_t fused = mid ? fused0 : 0;
            if (!mid)
                for (int32_t c = S.candOff; c < S.candOff + S.n; c++) {
                    W.rep[(size_t)c] = -1;
                    if (!P.is_live(S, c)) W.action[(size_t)c] = FUSE_NONE;
                }
            if (S.form == FUSE_LOOP && !mid) {
                for (int32_t e = (*K.rowOff)[(size_t)S.kf]; e < (*K.rowOff)[(size_t)S.kf + 1]; e++)
                    if ((*K.row)[(size_t)e] >= 0) snap[(size_t)(*K.row)[(size_t)e]] = s + 1;
                for (int32_t c = S.candOff; c < S.candOff + S.n; c++) {
                    const int32_t item = P.cand[(size_t)c];
                    if (P.is_live(S, c)) W.action[(size_t)c] = (*K.bad)[(size_t)item] || snap[(size_t)item] == s + 1 ? FUSE_SKIPPED : FUSE_PENDING;
                }
            }
            for (int pass = mid ? from.pass : 0; pass < (S.form == FUSE_LOOP ? 2 : 1); pass++)
                for (int32_t c = S.candOff; c < S.candOff + S.n; c++) {
                    if (mid && pass == from.pass && c < from.cand) continue;
                    if (!P.is_live(S, c)) continue;
                    const int32_t item = P.cand[(size_t)c], bi = P.index(S, c);
                    uint8_t& act = W.action[(size_t)c];
                    if (pass == 1) {
                        if (act == FUSE_RECORDED && W.rep[(size_t)c] != item) replace(S.kind, W.rep[(size_t)c], item);
                        continue;
                    }
                    if (S.form == FUSE_NEIGHBOURS) {
                        if ((*K.bad)[(size_t)item] || (fuse_asks_in_keyframe(S.kind) && member(S.kind, item, S.kf))) {
                            act = FUSE_SKIPPED;
                            continue;
                        }
                        const int32_t occ = (*K.row)[rowBase + (size_t)bi];
                        if (occ < 0) {
                            const bool gains = fuse_asks_in_keyframe(S.kind) || !member(S.kind, item, S.kf);
                            add(S.kind, item, S.kf, bi, gains);
                            act = gains ? FUSE_ADDED : FUSE_ROW_ONLY;
                        } else if ((*K.bad)[(size_t)occ]) {
                            act = FUSE_OCC_BAD;
                        } else if (occ == item) {
                            act = FUSE_SELF;
                        } else if (fuse_candidate_loses((*K.nObs)[(size_t)occ], (*K.nObs)[(size_t)item])) {
                            replace(S.kind, item, occ);
                            act = FUSE_CAND_REPLACED;
                        } else {
                            replace(S.kind, occ, item);
                            act = FUSE_OCC_REPLACED;
                        }
                    } else if (S.form == FUSE_LOOP) {
                        if (act != FUSE_PENDING) continue;
                        const int32_t occ = (*K.row)[rowBase + (size_t)bi];
                        if (occ >= 0) {
                            act = (*K.bad)[(size_t)occ] ? FUSE_OCC_BAD : FUSE_RECORDED;
                            if (act == FUSE_RECORDED) W.rep[(size_t)c] = occ;
                        } else {
                            const bool gains = !member(S.kind, item, S.kf);
                            add(S.kind, item, S.kf, bi, gains);
                            act = gains ? FUSE_ADDED : FUSE_ROW_ONLY;
                        }
                    } else {
                        const int32_t occ = (*K.row)[rowBase + (size_t)bi];
                        if (occ < 0) {
                            const bool gains = !member(S.kind, item, S.kf);
                            add(S.kind, item, S.kf, bi, gains);
                            act = gains ? FUSE_ADDED : FUSE_ROW_ONLY;
                        } else if (occ == item) {
                            act = FUSE_SELF;
                        } else {
                            replace(S.kind, occ, item);
                            act = FUSE_OCC_REPLACED;
                        }
                    }
                    fused += fuse_counts(act);
                }
            W.nFused[(size_t)s] = fused;
        }
    }
};

void work_begin(const FusePlan& P, FuseWork& W)
{
    W.action.assign(P.cand.size(), 0);
    W.rep.assign(P.cand.size(), -1);
    W.nFused.assign(P.step.size(), 0);
    W.rOff.assign(1, 0);
}

/* the events of the call in execution order, from what a walk left: f(step, candidate, replacement or -1 for an add) */
template <class F>
void for_events(const FusePlan& P, const FuseWork& W, Cursor from, Cursor to, size_t r, F&& f)
{
    for (int32_t s = from.step; s < (int32_t)P.step.size() && s <= to.step; s++) {
        const FuseStep& S = P.step[(size_t)s];
        for (int pass = 0; pass < (S.form == FUSE_LOOP ? 2 : 1); pass++)
            for (int32_t c = S.candOff; c < S.candOff + S.n; c++) {
                const Cursor at{s, pass, c};
                if (at < from) continue;
                if (!(at < to)) return;
                const int a = W.action[(size_t)c];
                if (pass == 0 && (a == FUSE_ADDED || a == FUSE_ROW_ONLY)) f(S, c, (size_t)-1);
                else if (pass == 0 ? (a == FUSE_CAND_REPLACED || a == FUSE_OCC_REPLACED) : (a == FUSE_RECORDED && W.rep[(size_t)c] != P.cand[(size_t)c])) f(S, c, r++);
            }
    }
}

/* every winner and every item that gained an observation, once each, in the order first met */
void touched_of(const FusePlan& P, const FuseWork& W, std::vector<int32_t> out[2])
{
    std::unordered_set<int32_t> seen[2];
    for_events(P, W, Cursor{0, 0, 0}, P.end(), 0, [&](const FuseStep& S, int32_t c, size_t r) {
        int32_t item;
        if (r == (size_t)-1) {
            if (W.action[(size_t)c] != FUSE_ADDED) return;
            item = P.cand[(size_t)c];
        } else {
            item = W.rWinner[r];
        }
        if (seen[S.kind].insert(item).second) out[S.kind].push_back(item);
    });
}

/* more changed entries than this go up as the whole section rather than one by one */
const size_t kEntriesOneByOne = 1024;

/* Applies the events of [from, to) to the rows by handle and to the image.  deviceOrder: the records of a Replace lie as the walk
 * of the device leaves them - the loser's stored list, then what the call had added to it - and are put into stored order here,
 * against the list by handle; the device already holds the rows, flags and counters, so only the spliced observations travel. */
int replay(drfe_lmap* db, const FusePlan& P, FuseWork& W, Cursor from, Cursor to, bool onDevice)
{
    Image& G = db->img;
    CullAttr& A = db->cull;
    KindView V[2] = {kind_view(db, 0), kind_view(db, 1)};
    ResidentBlock &rows = db->blk[drfe_lmap::ROWS], &attr = db->blk[drfe_lmap::ATTR], &recent = db->blk[drfe_lmap::RECENT];
    std::unordered_set<int32_t> changed[2];
    std::vector<size_t> entries[2];
    bool flags = false, counters = false, nobs[2] = {false, false};
    struct ByHandle {
        std::vector<int32_t>*obs, *idx;
        int32_t* nObs;
    };
    auto by_handle = [&](int kind, int32_t h) {
        if (kind == FUSE_POINT) {
            MpCull& C = db->mpCull.at(h);
            return ByHandle{&db->mp.at(h).obs, &C.obsIdx, &C.nObs};
        }
        MlObs& O = db->mlObs.at(h);
        return ByHandle{&O.obs, &O.obsIdx, &O.nObs};
    };
    auto slot_of = [&](int32_t kfHandle) { return G.kfSlot.at(kfHandle); };
    auto store = [&](int kind, int32_t kf, int32_t idx, int32_t item) {
        const size_t at = (size_t)(*V[kind].rowOff)[(size_t)kf] + (size_t)idx;
        (*V[kind].row)[at] = item;
        KfRow& K = db->kf.at(G.kfHandle[(size_t)kf]);
        (kind == FUSE_POINT ? K.mps : K.mls)[(size_t)idx] = item < 0 ? -1 : (*V[kind].handle)[(size_t)item];
        entries[kind].push_back(at);
    };
    auto gain = [&](int kind, int32_t item, int32_t kf, int32_t idx) {
        const ByHandle B = by_handle(kind, (*V[kind].handle)[(size_t)item]);
        const size_t at = rank_place(*B.obs, kf, slot_of);
        B.obs->insert(B.obs->begin() + (ptrdiff_t)at, G.kfHandle[(size_t)kf]);
        B.idx->insert(B.idx->begin() + (ptrdiff_t)at, idx);
        const int32_t w = fuse_obs_weight(kind, kind == FUSE_POINT ? A.stereo[(size_t)G.kfMpOff[(size_t)kf] + (size_t)idx] : 0);
        *B.nObs += w;
        (*V[kind].nObs)[(size_t)item] = *B.nObs;
        nobs[kind] = true;
        changed[kind].insert(item);
    };
    int bad = DRFE_OK;
    for_events(P, W, from, to, W.replayed, [&](const FuseStep& S, int32_t c, size_t r) {
        const int kind = S.kind;
        if (r == (size_t)-1) {
            store(kind, S.kf, P.index(S, c), P.cand[(size_t)c]);
            if (W.action[(size_t)c] == FUSE_ADDED) {
                gain(kind, P.cand[(size_t)c], S.kf, P.index(S, c));
                W.st[3]++;
            }
            return;
        }
        if (bad || r + 1 >= W.rOff.size()) {
            bad = DRFE_ERR_STATE;
            return;
        }
        const int32_t loser = W.rLoser[r], winner = W.rWinner[r];
        const int32_t lh = (*V[kind].handle)[(size_t)loser], wh = (*V[kind].handle)[(size_t)winner];
        const ByHandle Lo = by_handle(kind, lh);
        const size_t r0 = (size_t)W.rOff[r], n = (size_t)W.rOff[r + 1] - r0;
        if (n != Lo.obs->size()) {
            bad = DRFE_ERR_STATE;
            return;
        }
        if (onDevice) {
            /* into stored order: a loser's key frames are distinct */
            std::unordered_map<int32_t, std::pair<int32_t, uint8_t>> by;
            for (size_t t = r0; t < r0 + n; t++) by[W.recKf[t]] = std::make_pair(W.recIdx[t], W.recMoved[t]);
            for (size_t i = 0; i < n; i++) {
                const auto it = by.find(slot_of((*Lo.obs)[i]));
                if (it == by.end() || it->second.first != (*Lo.idx)[i]) {
                    bad = DRFE_ERR_STATE;
                    return;
                }
                W.recKf[r0 + i] = it->first;
                W.recIdx[r0 + i] = it->second.first;
                W.recMoved[r0 + i] = it->second.second;
            }
        }
        Lo.obs->clear();
        Lo.idx->clear();
        changed[kind].insert(loser);
        changed[kind].insert(winner);
        (*V[kind].bad)[(size_t)loser] = 1;
        flags = true;
        if (kind == FUSE_POINT) {
            db->mp.at(lh).bad = 1;
            db->mpReplaced[lh] = wh;
        } else {
            db->ml.at(lh) = 1;
            db->mlReplaced[lh] = wh;
        }
        for (size_t t = r0; t < r0 + n; t++) {
            store(kind, W.recKf[t], W.recIdx[t], W.recMoved[t] ? winner : -1);
            if (W.recMoved[t]) gain(kind, winner, W.recKf[t], W.recIdx[t]);
            W.st[W.recMoved[t] ? 5 : 6]++;
        }
        ItemRecent &Rl = (kind == FUSE_POINT ? db->mpRec : db->mlRec).at(lh), &Rw = (kind == FUSE_POINT ? db->mpRec : db->mlRec).at(wh);
        Rw.found = fuse_wrap_add(Rw.found, Rl.found);
        Rw.visible = fuse_wrap_add(Rw.visible, Rl.visible);
        (*V[kind].found)[(size_t)winner] = Rw.found;
        (*V[kind].visible)[(size_t)winner] = Rw.visible;
        counters = true;
        W.st[4]++;
        W.replayed = r + 1;
    });
    if (bad) return lmap_fail(db, bad, "lmap_fuse: the records of the walk do not fit the stored observations");
    /* the observation arrays of the image with the changed rows spliced in, from the lists by handle */
    for (int kind = 0; kind < 2; kind++) {
        if (changed[kind].empty()) continue;
        std::vector<int32_t> nOff(1, 0), nObsA, nIdx;
        const std::vector<int32_t>&off = *V[kind].obsOff, &a = *V[kind].obs, &b = *V[kind].obsIdx;
        nObsA.reserve(a.size() + changed[kind].size());
        nIdx.reserve(a.size() + changed[kind].size());
        for (size_t s = 0; s + 1 < off.size(); s++) {
            if (changed[kind].count((int32_t)s)) {
                const ByHandle B = by_handle(kind, (*V[kind].handle)[s]);
                for (size_t i = 0; i < B.obs->size(); i++) {
                    nObsA.push_back(slot_of((*B.obs)[i]));
                    nIdx.push_back((*B.idx)[i]);
                }
            } else {
                nObsA.insert(nObsA.end(), a.begin() + off[s], a.begin() + off[s + 1]);
                nIdx.insert(nIdx.end(), b.begin() + off[s], b.begin() + off[s + 1]);
            }
            nOff.push_back((int32_t)nObsA.size());
        }
        V[kind].obsOff->swap(nOff);
        V[kind].obs->swap(nObsA);
        V[kind].obsIdx->swap(nIdx);
        if (kind == FUSE_POINT) {
            A.live.assign(G.obs.size(), 1);
            rows.stale(db->secObsOff);
            attr.stale(db->secObsIdx);
        } else {
            recent.stale(db->secRecObsOff);
        }
    }
    if (onDevice) return DRFE_OK;
    /* what the device copy lacks after a walk of the host */
    if (flags) rows.stale(0, db->secMlBad);
    for (int kind = 0; kind < 2; kind++) {
        const int sec = kind == FUSE_POINT ? db->secKfMp : db->secKfMl;
        if (entries[kind].size() > kEntriesOneByOne) rows.stale(sec, sec);
        else
            for (const size_t at : entries[kind]) rows.stale_at(sec, at);
    }
    if (nobs[FUSE_POINT]) attr.stale(db->secNObs, db->secNObs);
    if (nobs[FUSE_LINE]) recent.stale(db->secRecObsOff - 1, db->secRecObsOff - 1);   /* the lines' nObs: bound right before the offsets */
    if (counters) recent.stale(0, db->secRecCounters);
    return DRFE_OK;
}

/* what a device call takes of the scratch */
struct FuseFit {
    int64_t fixed = 0, whole = 0;
};

FuseFit fuse_fit(const drfe_lmap* db, int64_t tiles)
{
    FuseFit F;
    F.fixed = FUSE_FIXED_BYTES;
    F.whole = F.fixed + 4 * (2 * (int64_t)db->img.mpHandle.size() + (int64_t)db->img.mlHandle.size()) + 48 + FUSE_TILE_BYTES * tiles;
    return F;
}

/* The two launches, everything but the records back in one copy, the records at the count the walk reports.  *stop is where the
 * walk handed the rest of the call back, or the end of the call; *fused what the step at *stop had counted. */
int fuse_device(drfe_lmap* db, const FusePlan& P, FuseWork& W, Cursor* stop, int32_t* fused, void* stream)
{
    LmapCall call{db, "lmap fuse"};
    if (const int rc = call.begin(LMAP_NEED_RECENT, stream)) return rc;
    const Image& G = db->img;
    const size_t n = P.cand.size(), nS = P.step.size(), nT = P.tileStep.size(), nP = G.mpHandle.size(), nL = G.mlHandle.size(), live = (size_t)P.live;
    StageLayout<16> in, out, scr;
    const auto sStep = in.add<FuseStep>(nS);
    const auto sTile = in.add<int32_t>(nT);
    const auto sCand = in.add<int32_t>(n);
    const auto sBest = in.add<int32_t>(n);
    const auto oHead = out.add<int32_t>(FUSE_HEAD_WORDS);
    const auto oAction = out.add<uint8_t>(n);
    const auto oRep = out.add<int32_t>(n);
    const auto oFused = out.add<int32_t>(nS);
    const auto oKind = out.add<int32_t>(live);
    const auto oLoser = out.add<int32_t>(live);
    const auto oWinner = out.add<int32_t>(live);
    const auto oOff = out.add<int32_t>(live + 1);
    const auto xSnap = scr.add<int32_t>(nP);
    const auto xClearP = scr.add<int32_t>(nP);
    const auto xClearL = scr.add<int32_t>(nL);
    const auto xPacked = scr.add<int32_t>(nT * FUSE_TILE);
    const auto xCnt = scr.add<int32_t>(nT);
    const auto xLog = scr.add<int32_t>(3 * (size_t)FUSE_LOG_ENTRIES);
    const auto xRecKf = scr.add<int32_t>(FUSE_REC_ENTRIES);
    const auto xRecIdx = scr.add<int32_t>(FUSE_REC_ENTRIES);
    const auto xRecMoved = scr.add<uint8_t>(FUSE_REC_ENTRIES);
    if (const int rc = call.stage(in.bytes(), out.bytes(), scr.bytes())) return rc;
    const auto [h, d, dO, dS, r] = call.at;
    sStep.put(h, P.step.data());
    sTile.put(h, P.tileStep.data());
    sCand.put(h, P.cand.data());
    sBest.put(h, P.best.data());
    FuseLaunch L{};
    L.I = db->dView;
    L.A = db->dCull;
    L.R = db->dRec;
    L.nSteps = (int32_t)nS;
    L.nTiles = (int32_t)nT;
    L.logCap = FUSE_LOG_ENTRIES;
    L.recCap = FUSE_REC_ENTRIES;
    L.step = sStep.at(d);
    L.tileStep = sTile.at(d);
    L.cand = sCand.at(d);
    L.best = sBest.at(d);
    L.packed = xPacked.at(dS);
    L.tileCnt = xCnt.at(dS);
    L.snap = xSnap.at(dS);
    L.clearedAt[0] = xClearP.at(dS);
    L.clearedAt[1] = xClearL.at(dS);
    L.log = xLog.at(dS);
    L.recKf = xRecKf.at(dS);
    L.recIdx = xRecIdx.at(dS);
    L.recMoved = xRecMoved.at(dS);
    L.head = oHead.at(dO);
    L.action = oAction.at(dO);
    L.rep = oRep.at(dO);
    L.nFused = oFused.at(dO);
    L.rKind = oKind.at(dO);
    L.rLoser = oLoser.at(dO);
    L.rWinner = oWinner.at(dO);
    L.rOff = oOff.at(dO);
    if (const int rc = call.send()) return rc;
    hipError_t e = 2 * nP + nL ? hipMemsetAsync(xSnap.at(dS), 0, xClearL.off + xClearL.bytes() - xSnap.off, call.st) : hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync(dO, 0, out.bytes(), call.st);
    /* the walk stores into the rows, the attribute and the recent-list block */
    LmapWrites writes(db->blk[drfe_lmap::ROWS], &db->blk[drfe_lmap::ATTR]);
    LmapWrites writesRecent(db->blk[drfe_lmap::RECENT]);
    if (e == hipSuccess) e = drfe_launch_fuse(L, call.st);
    if (const int rc = call.back(e)) return rc;
    const int32_t* head = oHead.at(r);
    const int32_t nRepl = head[FUSE_HEAD_REPL], nRec = head[FUSE_HEAD_REC];
    const bool stopped = head[FUSE_HEAD_STOPPED] != 0;
    if (nRepl < 0 || (size_t)nRepl > live || nRec < 0 || nRec > FUSE_REC_ENTRIES || oOff.at(r)[nRepl] != nRec ||
        (stopped && (head[FUSE_HEAD_STEP] < 0 || (size_t)head[FUSE_HEAD_STEP] >= nS || head[FUSE_HEAD_CAND] < 0 || (size_t)head[FUSE_HEAD_CAND] >= n)))
        return lmap_fail(db, DRFE_ERR_STATE, "lmap fuse device call: the device's totals do not fit the call");
    LmapFetch F;
    const auto fKf = F.add(L.recKf, (size_t)nRec);
    const auto fIdx = F.add(L.recIdx, (size_t)nRec);
    const auto fMoved = F.add(L.recMoved, (size_t)nRec);
    if (const int rc = call.fetch(F)) return rc;
    writes.done();
    writesRecent.done();
    W.action.assign(oAction.at(r), oAction.at(r) + n);
    W.rep.assign(oRep.at(r), oRep.at(r) + n);
    W.nFused.assign(oFused.at(r), oFused.at(r) + nS);
    W.rKind.assign(oKind.at(r), oKind.at(r) + nRepl);
    W.rLoser.assign(oLoser.at(r), oLoser.at(r) + nRepl);
    W.rWinner.assign(oWinner.at(r), oWinner.at(r) + nRepl);
    W.rOff.assign(oOff.at(r), oOff.at(r) + nRepl + 1);
    W.recKf.assign(F.at(fKf), F.at(fKf) + nRec);
    W.recIdx.assign(F.at(fIdx), F.at(fIdx) + nRec);
    W.recMoved.assign(F.at(fMoved), F.at(fMoved) + nRec);
    *stop = stopped ? Cursor{head[FUSE_HEAD_STEP], head[FUSE_HEAD_PASS], head[FUSE_HEAD_CAND]} : P.end();
    *fused = head[FUSE_HEAD_FUSED];
    return DRFE_OK;
}

/* the counts of a finished walk against the caller's capacities, or the name of the one that is too small */
const char* fuse_capacity(const FusePlan& P, const FuseWork& W, const drfe_lmap_fuse_call* c, std::vector<int32_t> touched[2])
{
    touched[0].clear();
    touched[1].clear();
    touched_of(P, W, touched);
    if ((int64_t)W.rKind.size() > c->replaced_capacity) return "replaced_capacity";
    if ((int64_t)W.recKf.size() > c->record_capacity) return "record_capacity";
    if ((int64_t)touched[0].size() > c->touched_capacity || (int64_t)touched[1].size() > c->touched_capacity) return "touched_capacity";
    return nullptr;
}

void fuse_fill(drfe_lmap* db, const FusePlan& P, const FuseWork& W, drfe_lmap_fuse_call* c, const std::vector<int32_t> touched[2])
{
    const Image& G = db->img;
    for (size_t s = 0; s < P.step.size(); s++) {
        const FuseStep& S = P.step[s];
        drfe_lmap_fuse_step& O = c->steps[s];
        const std::vector<int32_t>& handle = S.kind == FUSE_POINT ? G.mpHandle : G.mlHandle;
        if (S.n) std::memcpy(O.action, W.action.data() + S.candOff, (size_t)S.n);
        *O.n_fused = W.nFused[s];
        if (O.replace)
            for (int i = 0; i < S.n; i++) {
                const int32_t v = W.rep[(size_t)(S.candOff + i)];
                O.replace[i] = v < 0 ? -1 : handle[(size_t)v];
            }
    }
    const size_t nR = W.rKind.size();
    *c->n_replaced = (int32_t)nR;
    for (size_t r = 0; r < nR; r++) {
        const std::vector<int32_t>& handle = W.rKind[r] == FUSE_POINT ? G.mpHandle : G.mlHandle;
        c->replaced_kind[r] = W.rKind[r] == FUSE_POINT ? DRFE_LMAP_POINT : DRFE_LMAP_LINE;
        c->loser[r] = handle[(size_t)W.rLoser[r]];
        c->winner[r] = handle[(size_t)W.rWinner[r]];
        c->record_offsets[r] = W.rOff[r];
    }
    c->record_offsets[nR] = W.rOff[nR];
    for (size_t t = 0; t < W.recKf.size(); t++) {
        c->record_kf[t] = G.kfHandle[(size_t)W.recKf[t]];
        c->record_index[t] = W.recIdx[t];
        c->record_moved[t] = W.recMoved[t];
    }
    for (int k = 0; k < 2; k++) {
        c->n_touched[k] = (int32_t)touched[k].size();
        int32_t* o = k ? c->touched_lines : c->touched_points;
        const std::vector<int32_t>& handle = k ? G.mlHandle : G.mpHandle;
        for (size_t i = 0; i < touched[k].size(); i++) o[i] = handle[(size_t)touched[k][i]];
    }
}

/* a walk of the host from `from`, undone: what it decided is in W */
void host_dry(drfe_lmap* db, const FusePlan& P, FuseWork& W, Cursor from, bool resumed, int32_t fused)
{
    HostWalk H(db, P, W);
    H.run(from, resumed, fused);
    H.undo();
}

/* mode: 0 host, 1 device, 2 by the crossover */
int fuse_entry_point(drfe_lmap* db, drfe_lmap_fuse_call* c, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (mode == 1 && !db->ctx) return lmap_fail(db, DRFE_ERR_STATE, "lmap_fuse: a device call on a store without a context");
    if (!call_ok(c)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_fuse: invalid call or output arrays");
    FusePlan P;
    int rc = fuse_plan(db, c, P);
    if (rc) return rc;
    const int64_t total = (int64_t)P.cand.size();
    bool dev = total > 0 && (mode == 1 || (mode == 2 && db->ctx && total >= DRFE_LMAP_FUSE_DEVICE_FROM));
    if (dev) {
        const bool fits = fuse_fit(db, (int64_t)P.tileStep.size()).whole <= db->scratchBytes && db->img.kfHandle.size() <= FUSE_MAX_KFS;
        if (!fits && mode == 1)
            return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_fuse: the call does not fit the configured device scratch, or the store has more key frames than the walk's observer bitmap");
        dev = fits;
    }
    FuseWork W;
    std::vector<int32_t> touched[2];
    const char* small = nullptr;
    work_begin(P, W);
    if (dev) {
        /* the device commits as it goes, so the capacities are settled first: by the bounds, or by a walk of the host */
        const int64_t nK = (int64_t)db->img.kfHandle.size();
        if (P.live > c->replaced_capacity || (int64_t)P.live * nK > c->record_capacity || std::max(P.liveKind[0], P.liveKind[1]) > c->touched_capacity) {
            FuseWork H;
            work_begin(P, H);
            host_dry(db, P, H, Cursor{0, 0, 0}, false, 0);
            small = fuse_capacity(P, H, c, touched);
        }
        if (!small) {
            Cursor stop{0, 0, 0};
            int32_t fused = 0;
            rc = fuse_device(db, P, W, &stop, &fused, stream);
            if (rc) return rc;
            rc = replay(db, P, W, Cursor{0, 0, 0}, stop, true);
            if (rc) {
                /* cannot be with a correct walk; the host's arrays are what the next device call gets */
                for (const int b : {drfe_lmap::ROWS, drfe_lmap::ATTR, drfe_lmap::RECENT}) db->blk[b].stale_all();
                return rc;
            }
            W.st[2] = 1;
            if (stop < P.end()) {
                /* the walk's log or record room was full: the host finishes the call from the state the device left */
                W.st[7] = 1;
                host_dry(db, P, W, stop, true, fused);
                rc = replay(db, P, W, stop, P.end(), false);
                if (rc) return rc;
            }
            small = fuse_capacity(P, W, c, touched);   /* cannot be: the same decisions */
        }
    } else {
        host_dry(db, P, W, Cursor{0, 0, 0}, false, 0);
        small = fuse_capacity(P, W, c, touched);
        if (!small) {
            rc = replay(db, P, W, Cursor{0, 0, 0}, P.end(), false);
            if (rc) return rc;
        }
    }
    if (small) return lmap_fail(db, DRFE_ERR_CAPACITY, std::string("lmap_fuse: the call returns more than ") + small);
    fuse_fill(db, P, W, c, touched);
    W.st[0] = 1;
    W.st[1] = total;
    for (int i = 0; i < 8; i++) db->fuseStats[i] += W.st[i];
    return DRFE_OK;
}

}  // namespace

extern "C" {

int drfe_lmap_fuse_host(drfe_lmap* db, drfe_lmap_fuse_call* call) { return fuse_entry_point(db, call, 0, nullptr); }
int drfe_lmap_fuse_device(drfe_lmap* db, drfe_lmap_fuse_call* call, void* stream) { return fuse_entry_point(db, call, 1, stream); }
int drfe_lmap_fuse_batch(drfe_lmap* db, drfe_lmap_fuse_call* call, void* stream) { return fuse_entry_point(db, call, 2, stream); }

int drfe_lmap_fuse_limits(int32_t* out8)
{
    if (!out8) return DRFE_ERR_INVALID;
    out8[0] = FUSE_TILE;
    out8[1] = 64;
    out8[2] = FUSE_LOG_ENTRIES;
    out8[3] = FUSE_REC_ENTRIES;
    out8[4] = FUSE_MAX_KFS;
    out8[5] = FUSE_TILE_BYTES;
    out8[6] = DRFE_LMAP_FUSE_MAX_CANDIDATES;
    out8[7] = DRFE_LMAP_FUSE_DEVICE_FROM;
    return DRFE_OK;
}

int drfe_lmap_fuse_scratch(drfe_lmap* db, int64_t n_candidates, int64_t n_steps, int64_t* out3)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!out3 || n_candidates < 0 || n_steps < 0) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_fuse_scratch: invalid argument");
    const int rc = lmap_build_image(db);
    if (rc) return rc;
    const FuseFit F = fuse_fit(db, n_candidates / FUSE_TILE + n_steps);
    out3[0] = F.whole;
    out3[1] = F.whole;
    out3[2] = F.fixed;
    return DRFE_OK;
}

int drfe_lmap_fuse_stats(drfe_lmap* db, int64_t* stats) { return lmap_stats(db, &drfe_lmap::fuseStats, stats); }

int drfe_lmap_get_replaced(drfe_lmap* db, int kind, int32_t count, const int32_t* handles, int32_t* out)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !out))) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_replaced: invalid argument");
    if (kind != DRFE_LMAP_POINT && kind != DRFE_LMAP_LINE) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_replaced: unknown kind");
    const std::unordered_map<int32_t, int32_t>& rep = kind == DRFE_LMAP_POINT ? db->mpReplaced : db->mlReplaced;
    for (int i = 0; i < count; i++)
        if (kind == DRFE_LMAP_POINT ? db->mp.find(handles[i]) == db->mp.end() : db->ml.find(handles[i]) == db->ml.end())
            return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_replaced: unknown handle");
    for (int i = 0; i < count; i++) {
        const auto it = rep.find(handles[i]);
        out[i] = it == rep.end() ? -1 : it->second;
    }
    return DRFE_OK;
}

int drfe_lmap_get_match_row(drfe_lmap* db, int kind, int32_t keyframe, int32_t capacity, int32_t* n, int32_t* out)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!n || capacity < 0 || (capacity > 0 && !out)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_match_row: invalid argument");
    if (kind != DRFE_LMAP_POINT && kind != DRFE_LMAP_LINE) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_match_row: unknown kind");
    const auto it = db->kf.find(keyframe);
    if (it == db->kf.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_match_row: unknown handle");
    const std::vector<int32_t>& row = kind == DRFE_LMAP_POINT ? it->second.mps : it->second.mls;
    *n = (int32_t)row.size();
    if ((int64_t)row.size() > capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_get_match_row: the output array is too small");
    if (!row.empty()) std::memcpy(out, row.data(), sizeof(int32_t) * row.size());
    return DRFE_OK;
}

int drfe_lmap_get_observers(drfe_lmap* db, int kind, int32_t handle, int32_t capacity, uint8_t* bad, int32_t* n, int32_t* out)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!n || !bad || capacity < 0 || (capacity > 0 && !out)) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_observers: invalid argument");
    const std::vector<int32_t>* obs = nullptr;
    static const std::vector<int32_t> none;
    if (kind == DRFE_LMAP_POINT) {
        const auto it = db->mp.find(handle);
        if (it == db->mp.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_observers: unknown handle");
        *bad = it->second.bad;
        obs = &it->second.obs;
    } else if (kind == DRFE_LMAP_LINE) {
        const auto it = db->ml.find(handle);
        if (it == db->ml.end()) return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_observers: unknown handle");
        *bad = it->second;
        const auto ob = db->mlObs.find(handle);
        obs = ob == db->mlObs.end() ? &none : &ob->second.obs;
    } else {
        return lmap_fail(db, DRFE_ERR_INVALID, "lmap_get_observers: unknown kind");
    }
    *n = (int32_t)obs->size();
    if ((int64_t)obs->size() > capacity) return lmap_fail(db, DRFE_ERR_CAPACITY, "lmap_get_observers: the output array is too small");
    if (!obs->empty()) std::memcpy(out, obs->data(), sizeof(int32_t) * obs->size());
    return DRFE_OK;
}

}  // extern "C"
