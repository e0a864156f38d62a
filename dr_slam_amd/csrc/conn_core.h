/* conn_core.h — the rules of KeyFrame::UpdateConnections, AddConnection and UpdateBestCovisibles (reference src/KeyFrame.cc:200-234,
 * 366-500), once, for lmap_conn.cpp's host walk and conn_kernels.hip.  DESIGN.md section 26.  Integer-only.
 *
 * Both sides read the image of lmap_core.h (key frames are slots in rank order) and two rows per key frame: the weights
 * (mConnectedKeyFrameWeights) as (slot, weight) pairs in ascending slot, and the ordered list (mvpOrderedConnectedKeyFrames with
 * mvOrderedWeights) as (slot, weight) pairs in the reference's order.
 *
 * A call names key frames s_0 .. s_{n-1}, each once, and gives what the reference's calls made one after another in that order
 * give.  The host walk makes them one after another.  The kernels evaluate the closed form, which rests on three facts:
 *   - the counter C_k, the listed set L_k, pKFmax and the new parent of k read only match rows and observations, which the call
 *     does not change: they are independent per k;
 *   - entry k of j's weights is written by at most one AddConnection of the call (k is called once), and j's own call replaces
 *     j's weights by C_j: conn_prior_in_counter says where the value just before that AddConnection stands;
 *   - the ordered list of j follows the last changing event on j: conn_edge_applies says which edges land after j's own call,
 *     conn_list_mode which of the three lists j ends with. */
#ifndef DRFE_CONN_CORE_H
#define DRFE_CONN_CORE_H

#include "../../include/drfe_math.h"
#include <stdint.h>

/* `int th = 15` of UpdateConnections */
#define CONN_TH 15

/* a match-row entry votes when it is neither null nor bad */
DRFE_HD bool conn_point_votes(int32_t p, const uint8_t* mpBad) { return p >= 0 && !mpBad[p]; }

/* `if (mit->first->mnId == mnId) continue;`: the store's handle is mnId and slots are one per handle */
DRFE_HD bool conn_obs_votes(int32_t obsSlot, int32_t self) { return obsSlot != self; }

DRFE_HD bool conn_listed(int32_t votes) { return votes >= CONN_TH; }

/* `if (mit->second > nmax)` over the counter in slot order from nmax = 0, as an order-free comparison: more votes, then the
 * lower slot.  A counter entry has at least one vote. */
DRFE_HD bool conn_better(int32_t votes, int32_t slot, int32_t bestVotes, int32_t bestSlot)
{
    return votes > bestVotes || (votes == bestVotes && slot < bestSlot);
}

/* pair<int, KeyFrame*> sorted ascending and reversed: descending weight, then descending slot.  One key per pair, distinct
 * within a row; a list is its keys in descending order. */
DRFE_HD uint64_t conn_key(int32_t weight, int32_t slot) { return ((uint64_t)(uint32_t)weight << 32) | (uint32_t)slot; }
DRFE_HD int32_t conn_key_weight(uint64_t key) { return (int32_t)(key >> 32); }
DRFE_HD int32_t conn_key_slot(uint64_t key) { return (int32_t)(key & 0xffffffffu); }

/* index of `slot` in a row sorted by ascending slot, or -1 */
DRFE_HD int32_t conn_find(const int32_t* rowSlot, int32_t n, int32_t slot)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (rowSlot[mid] < slot)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && rowSlot[lo] == slot ? lo : -1;
}

/* AddConnection: `if (!count(pKF)) ... else if (mConnectedKeyFrameWeights[pKF] != weight) ... else return;` */
DRFE_HD bool conn_changes(bool present, int32_t prior, int32_t weight) { return !present || prior != weight; }

/* The value of j's entry for k just before k's AddConnection at call position p: in C_j when j was called earlier with a counter
 * that was not empty (posJ: j's position or -1, nCj: its counter's size), else in the stored row. */
DRFE_HD bool conn_prior_in_counter(int32_t posJ, int32_t nCj, int32_t p) { return posJ >= 0 && posJ < p && nCj > 0; }

/* j's own call with a counter that is not empty replaces its weights: an edge made at position p is in the final row unless it
 * was made before that call */
DRFE_HD bool conn_edge_applies(int32_t posJ, int32_t nCj, int32_t p) { return !(posJ >= 0 && nCj > 0 && p < posJ); }

/* which list a touched key frame ends with: CONN_LIST_FULL after a changing edge that applies (UpdateBestCovisibles: every entry
 * of the weights), else CONN_LIST_OWN after its own call (the listed pairs), else the stored one */
enum { CONN_LIST_STORED = 0, CONN_LIST_OWN = 1, CONN_LIST_FULL = 2 };
DRFE_HD int conn_list_mode(bool ownCall, bool changingEdgeApplied) { return changingEdgeApplied ? CONN_LIST_FULL : (ownCall ? CONN_LIST_OWN : CONN_LIST_STORED); }

#endif
