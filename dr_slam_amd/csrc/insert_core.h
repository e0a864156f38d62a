/* insert_core.h — the rules of the item loops of LocalMapping::ProcessNewKeyFrame (reference src/LocalMapping.cc:113-173) with
 * MapPoint::AddObservation and UpdateNormalAndDepth (src/MapPoint.cc:124-138, :370-417) and MapLine::AddObservation
 * (src/MapLine.cpp:91-100), once, for lmap_insert.cpp and insert_kernels.hip.  DESIGN.md section 33.
 *
 * The loops set nothing bad and move no pose, and IsInKeyFrame(k) of an item changes only through the additions of k's own row.
 * So the verdict of an entry (called key frame j, index i) is a closed form over the stored state and the row: RECENT when k is a
 * stored observer or the item stands at a lower index of the same row, else ADDED.  The observer list an ADDED point's
 * UpdateNormalAndDepth walks is a closed form too.  The insertion rule puts a new observer x in front of the first listed observer
 * of greater slot.  Applied one addition after another to a stored list s_0 .. s_{m-1} (in any order), every added x lands in
 * front of the first stored s_t > x, and the added ones that land in front of the same s_t stand in ascending slot: a later x'
 * below an earlier x meets x first, a later x' above x passes it.  Walking the stored list and emitting, in front of s_t, every
 * added observer below s_t that is not yet out, in ascending slot, and the rest at the end, gives that list. */
#ifndef DRFE_INSERT_CORE_H
#define DRFE_INSERT_CORE_H

#include "correct_core.h"
#include "fuse_core.h"

/* drfe_lmap_insert_call's action bytes */
enum { INS_NULL = 0, INS_BAD = 1, INS_RECENT = 2, INS_ADDED = 3 };
/* no further adder */
#define INS_NO_ADDER 0x7fffffff

/* The rows of a call as one flat entry space: segment q < n is the point row of called key frame q, segment n + q its line row;
 * segOff has 2n + 1 offsets from 0.  The segment of entry e: the last one that starts at or before e and is not empty there. */
DRFE_HD int32_t ins_segment(const int32_t* segOff, int32_t nSeg, int32_t e)
{
    int32_t lo = 0, hi = nSeg;         /* segOff[lo] <= e < segOff[hi] */
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (segOff[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* whether key frame kf is among the stored observers [o0, o1) */
DRFE_HD bool ins_observes(const int32_t* obs, int32_t o0, int32_t o1, int32_t kf)
{
    for (int32_t o = o0; o < o1; o++)
        if (obs[o] == kf) return true;
    return false;
}

/* the verdict of an entry: `observes` of the stored list, `first` = no lower index of the row names the item */
DRFE_HD int ins_verdict(int32_t item, uint8_t bad, bool observes, bool first)
{
    if (item < 0) return INS_NULL;
    if (bad) return INS_BAD;
    return observes || !first ? INS_RECENT : INS_ADDED;
}

/* The called key frames that add one point, as a bit per called key frame in ascending slot: bit r stands for position byRank[r]
 * of the call, whose slot is called[byRank[r]].  upTo: the positions after it have not run yet. */
struct InsAdders {
    const uint32_t* bits;
    int32_t words;
    const int32_t* byRank;
    const int32_t* called;
    int32_t upTo;
};

/* the slot of the next adder at or after bit *r, in ascending slot, or INS_NO_ADDER; *r moves behind it */
DRFE_HD int32_t ins_next_adder(const InsAdders& A, int32_t* r)
{
    while (*r < 32 * A.words) {
        const uint32_t w = A.bits[*r >> 5] >> (*r & 31);
        if (!w) {
            *r = ((*r >> 5) + 1) << 5;
            continue;
        }
        *r += __builtin_ctz(w);
        const int32_t j = A.byRank[*r];
        (*r)++;
        if (j <= A.upTo) return A.called[j];
    }
    return INS_NO_ADDER;
}

/* UpdateNormalAndDepth of point p right after an addition: the stored observers [obsOff[p], obsOff[p + 1]) merged with the adders
 * as above, every sum in that order inside the caller.  At least one observer: the adder at hand. */
DRFE_HD uint8_t ins_point_normal(const CorrImage& G, const int32_t* obsOff, const int32_t* obs, const InsAdders& A, int32_t p,
                                 float nrm[3], float* maxD, float* minD)
{
    const float* X = G.mpWorld + 3 * (size_t)p;
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    int32_t r = 0, n = 0;
    int32_t next = ins_next_adder(A, &r);
    for (int32_t o = obsOff[p]; o < obsOff[p + 1]; o++) {
        const int32_t s = obs[o];
        while (next < s) {
            mu_point_obs(nrm, X, G.kfOw + 3 * (size_t)next);
            n++;
            next = ins_next_adder(A, &r);
        }
        mu_point_obs(nrm, X, G.kfOw + 3 * (size_t)s);
        n++;
    }
    while (next != INS_NO_ADDER) {
        mu_point_obs(nrm, X, G.kfOw + 3 * (size_t)next);
        n++;
        next = ins_next_adder(A, &r);
    }
    mu_point_finish(nrm, n, X, G.kfOw + 3 * (size_t)G.mpRef[p], G.scale[G.mpLevel[p]], G.scale[G.nLevels - 1], maxD, minD);
    return DRFE_UPKEEP_NORMAL;
}

#endif
