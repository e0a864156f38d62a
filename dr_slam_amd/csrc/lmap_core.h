/* lmap_core.h — the rules of Tracking::UpdateLocalKeyFrames / UpdateLocalPoints / UpdateLocalLines (reference
 * src/Tracking.cc:3396-3541), once, for lmap.cpp and lmap_kernels.hip.  DESIGN.md section 25.  Integer-only.
 *
 * Both sides read the same image of the graph: key frames are slots 0 .. nK in rank order (ascending slot is the reference's walk
 * over map<KeyFrame*, int> and set<KeyFrame*>), map points and map lines are slots of their own, every reference is a slot or -1. */
#ifndef DRFE_LMAP_CORE_H
#define DRFE_LMAP_CORE_H

#include "../../include/drfe_math.h"
#include <stdint.h>

#define LMAP_NEIGHBOURS 10
/* mvpLocalKeyFrames.size() > 80 ends the expansion */
#define LMAP_MAX_LOCAL 80
/* a claim no entry has made */
#define LMAP_NO_CLAIM 0x7f7f7f7f

struct LmapImage {
    int32_t nK, nP, nL;
    const uint8_t* kfBad;          /* nK */
    const int32_t* kfParent;       /* nK */
    const int32_t* kfNbr;          /* nK x 10 */
    const int32_t* childOff;       /* nK + 1 */
    const int32_t* child;          /* ascending slot = rank order */
    const int32_t* kfMpOff;        /* nK + 1 */
    const int32_t* kfMp;           /* mvpMapPoints of the key frames */
    const int32_t* kfMlOff;        /* nK + 1 */
    const int32_t* kfMl;
    const uint8_t* mpBad;          /* nP */
    const int32_t* obsOff;         /* nP + 1 */
    const int32_t* obs;            /* key-frame slots */
    const uint8_t* mlBad;          /* nL */
};

/* mnTrackReferenceForFrame == mCurrentFrame.mnId of a key frame: a bit per slot, clear at the start of a query */
DRFE_HD bool lmap_marked(const uint32_t* mark, int32_t s) { return (mark[s >> 5] >> (s & 31)) & 1u; }
DRFE_HD void lmap_mark(uint32_t* mark, int32_t s) { mark[s >> 5] |= 1u << (s & 31); }

/* what a frame point does (:3451-3460): 0 nothing (null), 1 votes, 2 is set to NULL */
DRFE_HD int lmap_frame_point(int32_t p, const uint8_t* mpBad) { return p < 0 ? 0 : (mpBad[p] ? 2 : 1); }

/* the vote loop's test of one counter entry (:3478): listed when it has a vote and is not bad */
DRFE_HD bool lmap_listed(int32_t votes, uint8_t bad) { return votes > 0 && !bad; }

/* `if (it->second > max)` over listed key frames in slot order, as an order-free comparison: more votes, then the lower slot.
 * Votes of a listed key frame are >= 1, so max = 0 never holds against one. */
DRFE_HD bool lmap_better(int32_t votes, int32_t slot, int32_t bestVotes, int32_t bestSlot)
{
    return votes > bestVotes || (votes == bestVotes && slot < bestSlot);
}

/* The expansion loop (:3492-3535) over list[0 .. nListed), which the vote loop left and marked.  Pushes behind nListed; returns
 * the number pushed.  Sequential by definition. */
DRFE_HD int32_t lmap_expand(const LmapImage& I, int32_t* list, int32_t nListed, uint32_t* mark)
{
    int32_t n = nListed;
    for (int32_t it = 0; it < nListed; it++) {
        if (n > LMAP_MAX_LOCAL) break;
        const int32_t kf = list[it];
        for (int k = 0; k < LMAP_NEIGHBOURS; k++) {
            const int32_t nb = I.kfNbr[(size_t)kf * LMAP_NEIGHBOURS + k];
            if (nb < 0) continue;
            if (!I.kfBad[nb] && !lmap_marked(mark, nb)) {
                list[n++] = nb;
                lmap_mark(mark, nb);
                break;
            }
        }
        for (int32_t c = I.childOff[kf]; c < I.childOff[kf + 1]; c++) {
            const int32_t ch = I.child[c];
            if (!I.kfBad[ch] && !lmap_marked(mark, ch)) {
                list[n++] = ch;
                lmap_mark(mark, ch);
                break;
            }
        }
        const int32_t pa = I.kfParent[kf];
        if (pa >= 0 && !lmap_marked(mark, pa)) {
            list[n++] = pa;
            lmap_mark(mark, pa);
            break;
        }
    }
    return n - nListed;
}

/* UpdateLocalPoints / UpdateLocalLines as a closed form.  The entry (position j in the local list, index i in that key frame's
 * match row) has the walk rank j * rowStride + i, rowStride above every row length.  An item is listed by the entry of the lowest
 * rank that names it (the later ones meet the stamp), and only when it is not bad (a bad item is never stamped, and never listed). */
DRFE_HD int32_t lmap_walk_rank(int32_t j, int32_t i, int32_t rowStride) { return j * rowStride + i; }
DRFE_HD bool lmap_entry_kept(int32_t item, int32_t rank, const int32_t* claim, const uint8_t* bad)
{
    return item >= 0 && claim[item] == rank && !bad[item];
}

#endif
