/* cull_core.h — the rules of LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:1226-1285) and of what
 * KeyFrame::SetBadFlag does to map points (MapPoint::EraseObservation, MapPoint::SetBadFlag; src/KeyFrame.cc:574-683,
 * src/MapPoint.cc:145-202), once, for lmap_cull.cpp's host walk and cull_kernels.hip.  DESIGN.md section 28.  Integer-only but for
 * the depth test and the verdict's one double product.  Parity with a build of the reference's LocalMapping.cc and KeyFrame.cc is
 * not pinned: neither can be built without OpenCV, Eigen and PCL.
 *
 * Both sides read the image of lmap_core.h (key frames are slots in rank order) and a working state of four arrays that a call
 * changes as it goes: the match rows (an entry becomes -1 when MapPoint::SetBadFlag nulls it), the points' bad flags, the nObs
 * counters and one live flag per stored observation (an erased observation stays in place with its flag cleared until the commit
 * compacts the row).  The attributes are read-only: mThDepth and the flags per key frame, octave, depth and stereo parallel to
 * the match row, the index mit->second parallel to the observations.
 *
 * The host walks the called key frames one after another with cull_entry.  The kernels evaluate the closed form, which rests on
 * three facts:
 *   - only a called key frame can be culled by the call, and a culled key frame erases only its own observation, so an observer
 *     that is not called stays in the list of a point for as long as the point is not bad; a point that loses every observer at
 *     once (MapPoint::SetBadFlag) is bad from then on and its entries are skipped before the list is looked at;
 *   - so the observers of an entry that are not called count once (cull_record) and only the called observers are looked at
 *     again (cull_replay); and the counts of a whole key frame, taken side by side with all the others before the walk, stand
 *     when the walk reaches it unless an entry of its row was nulled or a point of its row lost an observation in between
 *     (cull_entry_changed): a call that culls nothing never looks at a row twice;
 *   - the erasures of one culled key frame touch disjoint state per point: EraseObservation(k) changes the point's own counter,
 *     list and flag, and the rows of other key frames than k at indices that only this point's list names or to the one value -1;
 *     a point that stands in k's row twice is erased by the first entry and not found by the second.  The points of one row are
 *     therefore erased side by side (cull_erase), and the key frames one after another. */
#ifndef DRFE_CULL_CORE_H
#define DRFE_CULL_CORE_H

#include "../../include/drfe_math.h"
#include <stdint.h>

/* `int nObs = 3; const int thObs = nObs;` */
#define CULL_TH_OBS 3
/* `if (nObs <= 2) bBad = true;` of EraseObservation */
#define CULL_POINT_MIN_OBS 2

/* flags byte of a key frame */
enum { CULL_KF_NOT_ERASE = 1, CULL_KF_ORIGIN = 2, CULL_KF_TO_BE_ERASED = 4 };
/* what a call did with a called key frame */
enum { CULL_KEPT = 0, CULL_CULLED = 1, CULL_DEFERRED = 2, CULL_ORIGIN = 3 };

struct CullState {
    /* the image */
    const int32_t* kfMpOff;        /* nK + 1 */
    const int32_t* obsOff;         /* nP + 1 */
    const int32_t* obs;            /* key-frame slots */
    /* working */
    int32_t* row;                  /* the match rows: point slot or -1 */
    uint8_t* mpBad;                /* nP */
    int32_t* nObs;                 /* nP */
    uint8_t* live;                 /* per stored observation */
    /* attributes */
    const float* thDepth;          /* nK */
    const uint8_t* kfFlags;        /* nK */
    const int32_t* octave;         /* parallel to the match rows */
    const float* depth;
    const uint8_t* stereo;
    const int32_t* obsIdx;         /* parallel to obs */
};

/* `if (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0) continue;` as written: a NaN depth fails both and counts */
DRFE_HD bool cull_depth_skips(float depth, float thDepth) { return depth > thDepth || depth < 0; }

/* `if (scaleLeveli <= scaleLevel + 1)` */
DRFE_HD bool cull_observer_counts(int32_t levelObserver, int32_t level) { return levelObserver <= level + 1; }

/* `if (nRedundantObservations > 0.9 * nMPs)`: the product in double */
DRFE_HD bool cull_verdict(int32_t nRedundant, int32_t nMPs) { return (double)nRedundant > 0.9 * (double)nMPs; }

DRFE_HD int cull_action(bool verdict, uint8_t flags)
{
    if (flags & CULL_KF_ORIGIN) return CULL_ORIGIN;
    if (!verdict) return CULL_KEPT;
    return (flags & CULL_KF_NOT_ERASE) ? CULL_DEFERRED : CULL_CULLED;
}

DRFE_HD int32_t cull_observer_level(const CullState& S, int32_t o) { return S.octave[S.kfMpOff[S.obs[o]] + S.obsIdx[o]]; }

/* Entry i of key frame k as the walk meets it: 0 skipped, 1 counted in nMPs, 2 counted and redundant.  *walked gains the
 * observers of the list the reference copies (GetObservations()) when it looks at one.  The reference leaves its loop at the
 * third counting observer; the count is the same when it does not. */
DRFE_HD int cull_entry(const CullState& S, int32_t k, int32_t i, int monocular, int32_t* walked)
{
    const int32_t e = S.kfMpOff[k] + i, p = S.row[e];
    if (p < 0 || S.mpBad[p]) return 0;
    if (!monocular && cull_depth_skips(S.depth[e], S.thDepth[k])) return 0;
    if (S.nObs[p] <= CULL_TH_OBS) return 1;
    const int32_t level = S.octave[e];
    int32_t n = 0;
    for (int32_t o = S.obsOff[p]; o < S.obsOff[p + 1]; o++) {
        if (!S.live[o]) continue;
        (*walked)++;
        if (S.obs[o] == k) continue;
        if (cull_observer_counts(cull_observer_level(S, o), level)) n++;
    }
    return n >= CULL_TH_OBS ? 2 : 1;
}

/* What of an entry the rest of the call cannot change, taken from the working state at some moment of the call (pos[slot] =
 * position in the call or -1): the point, or -1 when the entry is null by then or fails the depth test, and of the point's
 * observers that are not called how many there are and how many count, the latter saturated at CULL_TH_OBS. */
struct CullRecord {
    int32_t point;
    int32_t others;                /* (observers that are not called << 2) | counting ones, at most 3 */
};

DRFE_HD CullRecord cull_record(const CullState& S, const int32_t* pos, int32_t k, int32_t i, int monocular)
{
    CullRecord R;
    R.point = -1;
    R.others = 0;
    const int32_t e = S.kfMpOff[k] + i, p = S.row[e];
    if (p < 0) return R;
    if (!monocular && cull_depth_skips(S.depth[e], S.thDepth[k])) return R;
    R.point = p;
    const int32_t level = S.octave[e];
    int32_t n = 0, all = 0;
    for (int32_t o = S.obsOff[p]; o < S.obsOff[p + 1]; o++) {
        if (pos[S.obs[o]] >= 0) continue;
        all++;
        if (n < CULL_TH_OBS && cull_observer_counts(cull_observer_level(S, o), level)) n++;
    }
    R.others = (all << 2) | n;
    return R;
}

/* cull_entry from the record: the working state says whether the entry still stands, the called observers are looked at */
DRFE_HD int cull_replay(const CullState& S, const int32_t* pos, const CullRecord& R, int32_t k, int32_t i, int32_t* walked)
{
    const int32_t e = S.kfMpOff[k] + i, p = R.point;
    if (p < 0 || S.row[e] < 0 || S.mpBad[p]) return 0;
    if (S.nObs[p] <= CULL_TH_OBS) return 1;
    const int32_t level = S.octave[e];
    int32_t n = R.others & 3;
    *walked += R.others >> 2;
    for (int32_t o = S.obsOff[p]; o < S.obsOff[p + 1]; o++) {
        if (pos[S.obs[o]] < 0 || !S.live[o]) continue;
        (*walked)++;
        if (S.obs[o] == k) continue;
        if (cull_observer_counts(cull_observer_level(S, o), level)) n++;
    }
    return n >= CULL_TH_OBS ? 2 : 1;
}

/* Whether the entry may count otherwise than cull_replay said when its record was taken: its row entry was nulled since, or its
 * point lost an observation since (touched[point], which the caller of cull_erase sets) - nothing else moves a counter, a bad
 * flag or a live flag. */
DRFE_HD bool cull_entry_changed(const CullState& S, const uint8_t* touched, const CullRecord& R, int32_t k, int32_t i)
{
    return R.point >= 0 && (S.row[S.kfMpOff[k] + i] < 0 || touched[R.point]);
}

/* MapPoint::EraseObservation(k) of point q, and MapPoint::SetBadFlag when the counter says so.  Returns 0 when the observations
 * do not hold k, else 1, or 3 when the point went bad.  *front is the lowest remaining observer right after the erasure, or -1:
 * what `mObservations.begin()->first` names (slots are in rank order).  The caller sees to it that nothing else touches q. */
DRFE_HD int cull_erase(const CullState& S, int32_t k, int32_t q, int32_t* front)
{
    int32_t at = -1;
    for (int32_t o = S.obsOff[q]; o < S.obsOff[q + 1]; o++)
        if (S.obs[o] == k && S.live[o]) {
            at = o;
            break;
        }
    *front = -1;
    if (at < 0) return 0;
    S.nObs[q] -= S.stereo[S.kfMpOff[k] + S.obsIdx[at]] ? 2 : 1;
    S.live[at] = 0;
    int32_t lowest = -1;
    for (int32_t o = S.obsOff[q]; o < S.obsOff[q + 1]; o++)
        if (S.live[o] && (lowest < 0 || S.obs[o] < lowest)) lowest = S.obs[o];
    *front = lowest;
    if (S.nObs[q] > CULL_POINT_MIN_OBS) return 1;
    S.mpBad[q] = 1;
    for (int32_t o = S.obsOff[q]; o < S.obsOff[q + 1]; o++) {
        if (!S.live[o]) continue;
        S.live[o] = 0;
        S.row[S.kfMpOff[S.obs[o]] + S.obsIdx[o]] = -1;     /* EraseMapPointMatch(mit->second): whatever stands there */
    }
    return 3;
}

#endif
