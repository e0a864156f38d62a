/* fuse_core.h — the rules of the fuse commit (ORBmatcher::Fuse, LSDmatcher::Fuse, the matched-point loop of CorrectLoop and
 * MapPoint::Replace / MapLine::Replace; reference src/ORBmatcher.cc:845-976 and :1001-1101, src/LSDmatcher.cpp:897-1012,
 * src/LoopClosing.cc:566-581 and :650-657, src/MapPoint.cc:223-261, src/MapLine.cpp:178-214), once, for lmap_fuse.cpp and
 * fuse_kernels.hip.  DESIGN.md section 32.  Integer-only. */
#ifndef DRFE_FUSE_CORE_H
#define DRFE_FUSE_CORE_H

#include "../../include/drfe_math.h"
#include <stdint.h>

enum { FUSE_POINT = 0, FUSE_LINE = 1 };
enum { FUSE_NEIGHBOURS = 0, FUSE_LOOP = 1, FUSE_MATCHED = 2 };
/* drfe_lmap_fuse_step.action; FUSE_PENDING stands in a LOOP step between its snapshot and its turn and is never returned */
enum { FUSE_NONE = 0, FUSE_SKIPPED = 1, FUSE_ADDED = 2, FUSE_ROW_ONLY = 3, FUSE_OCC_BAD = 4, FUSE_CAND_REPLACED = 5,
       FUSE_OCC_REPLACED = 6, FUSE_SELF = 7, FUSE_RECORDED = 8, FUSE_PENDING = 255 };

/* what no state can revive: a null candidate, no answer where the form reads one */
DRFE_HD bool fuse_live(int form, int32_t cand, int32_t best) { return cand >= 0 && (form == FUSE_MATCHED || best >= 0); }

/* ORBmatcher::Fuse skips a candidate that IsInKeyFrame(pKF); LSDmatcher::Fuse does not ask (its test is commented out at
 * src/LSDmatcher.cpp:1043): a line that already observes the key frame goes on, and on an empty entry its AddObservation is a no-op */
DRFE_HD bool fuse_asks_in_keyframe(int kind) { return kind == FUSE_POINT; }

/* AddObservation's step of nObs: a point counts a stereo observation twice, a line counts one */
DRFE_HD int32_t fuse_obs_weight(int kind, uint8_t stereo) { return kind == FUSE_POINT && stereo ? 2 : 1; }

/* `pMPinKF->Observations() > pMP->Observations()` on the stored counters: the candidate loses; on a tie the occupant does */
DRFE_HD bool fuse_candidate_loses(int32_t nObsOccupant, int32_t nObsCandidate) { return nObsOccupant > nObsCandidate; }

/* what a candidate's action adds to nFused */
DRFE_HD int fuse_counts(int action) { return action >= FUSE_ADDED && action != FUSE_PENDING; }

/* mnFound += found of the loser, with wrap-around */
DRFE_HD int32_t fuse_wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }

#endif
