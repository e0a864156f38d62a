/* fuse_kernels.hip — the fuse commit on the device: ORBmatcher::Fuse, LSDmatcher::Fuse, the Sim3 form with
 * SearchAndFuse's loop, the matched-point loop of CorrectLoop, with MapPoint::Replace / MapLine::Replace and AddObservation, on
 * the resident blocks of the local-map store.
 *
 *   k_fuse_live   a lane per candidate of every step, a step starting a tile of its own: what no state can revive (a null
 *                 candidate, no answer) gets action 0, the rest is packed per tile in list order (rank by ballot).
 *   k_fuse_walk   one workgroup walks the live candidates of step after step in order, on the match rows, bad flags, nObs and
 *                 counters of the resident blocks.  A LOOP step begins with its snapshot: the lanes stamp the points its row
 *                 names, then give every live candidate "skipped" or "pending" - so the snapshot is taken after the walk of the
 *                 steps before it, by the walker itself.  Per candidate the decision is uniform (every lane reads the same
 *                 words); a Replace spreads the loser's observations over the lanes.
 *
 * What an item observes is its stored list, unless a Replace cleared it (clearedAt), plus the entries the call appended to the
 * log for it since.  Membership in a winner is a bitmap over the key-frame slots in LDS, filled from both by the workgroup before
 * the lanes test their observations against it; the gained observations are appended in order (ballot rank), nObs grows by an
 * LDS sum.  A loser's key frames are distinct (the store refuses a key frame twice in a list and the call keeps that), so no two
 * lanes of a Replace name one row entry.  Barriers separate the candidates.  When the log or the record room cannot take what the
 * candidate at hand may append, the walk stops in front of it and says where: the host finishes the call. */
#include "lmap_device.h"

namespace {

struct Kind {
    uint8_t* bad;
    int32_t *nObs, *found, *visible, *row;
    const int32_t *obsOff, *obs, *obsIdx, *rowOff;
};

__device__ inline Kind kind_of(const FuseLaunch& L, int kind)
{
    Kind V;
    if (kind == FUSE_POINT) {
        V.bad = const_cast<uint8_t*>(L.I.mpBad);
        V.nObs = const_cast<int32_t*>(L.A.nObs);
        V.row = const_cast<int32_t*>(L.I.kfMp);
        V.obsOff = L.I.obsOff;
        V.obs = L.I.obs;
        V.obsIdx = L.A.obsIdx;
        V.rowOff = L.I.kfMpOff;
    } else {
        V.bad = const_cast<uint8_t*>(L.I.mlBad);
        V.nObs = const_cast<int32_t*>(L.R.mlNObs);
        V.row = const_cast<int32_t*>(L.I.kfMl);
        V.obsOff = L.R.mlObsOff;
        V.obs = L.R.mlObs;
        V.obsIdx = L.R.mlObsIdx;
        V.rowOff = L.I.kfMlOff;
    }
    V.found = const_cast<int32_t*>(L.R.found[kind]);
    V.visible = const_cast<int32_t*>(L.R.visible[kind]);
    return V;
}

__global__ __launch_bounds__(FUSE_TILE) void k_fuse_live(FuseLaunch L)
{
    __shared__ int32_t shWave[FUSE_TILE / 64];
    const int t = blockIdx.x;
    const FuseStep S = L.step[L.tileStep[t]];
    const int c = S.candOff + (t - S.tile0) * FUSE_TILE + (int)threadIdx.x;
    const bool valid = c < S.candOff + S.n;
    const bool live = valid && fuse_live(S.form, L.cand[c], S.form == FUSE_MATCHED ? 0 : L.best[c]);
    if (valid) {
        L.rep[c] = -1;
        if (!live) L.action[c] = FUSE_NONE;
    }
    int total;
    unsigned long long ballot;
    const int r = block_rank(live, shWave, &total, &ballot);
    if (live) L.packed[(size_t)t * FUSE_TILE + r] = c;
    if (threadIdx.x == 0) L.tileCnt[t] = total;
}

struct Walk {
    const FuseLaunch& L;
    int32_t* shWave;
    int32_t* sFlag;
    uint32_t* sBits;
    int32_t logLen, nRepl, nRec;

    /* whether key frame kf is among the observers of the item now */
    __device__ bool member(const Kind& V, int kind, int32_t item, int32_t kf)
    {
        const int tid = threadIdx.x;
        __syncthreads();
        if (tid == 0) *sFlag = 0;
        __syncthreads();
        const int32_t ca = L.clearedAt[kind][item], key = item * 2 + kind;
        if (ca == 0)
            for (int32_t o = V.obsOff[item] + tid; o < V.obsOff[item + 1]; o += FUSE_TILE)
                if (V.obs[o] == kf) *sFlag = 1;
        for (int32_t j = (ca ? ca - 1 : 0) + tid; j < logLen; j += FUSE_TILE)
            if (L.log[3 * j] == key && L.log[3 * j + 1] == kf) *sFlag = 1;
        __syncthreads();
        return *sFlag != 0;
    }

    /* AddObservation when the key frame is no observer yet, and the row entry; the caller has made room in the log */
    __device__ void add(const Kind& V, int kind, int32_t item, int32_t kf, int32_t idx, bool gains)
    {
        if (threadIdx.x == 0) {
            const int32_t at = V.rowOff[kf] + idx;
            V.row[at] = item;
            if (gains) {
                L.log[3 * logLen] = item * 2 + kind;
                L.log[3 * logLen + 1] = kf;
                L.log[3 * logLen + 2] = idx;
                V.nObs[item] += fuse_obs_weight(kind, kind == FUSE_POINT ? L.A.stereo[at] : 0);
            }
        }
        if (gains) logLen++;
        __syncthreads();
    }

    /* the former observations of the loser the call has to have room for */
    __device__ int32_t held(const Kind& V, int kind, int32_t item)
    {
        const int32_t ca = L.clearedAt[kind][item], key = item * 2 + kind;
        int32_t n = ca == 0 ? V.obsOff[item + 1] - V.obsOff[item] : 0;
        for (int32_t j0 = ca ? ca - 1 : 0; j0 < logLen; j0 += FUSE_TILE) {
            const int32_t j = j0 + (int)threadIdx.x;
            n += __syncthreads_count(j < logLen && L.log[3 * j] == key);
        }
        return n;
    }

    /* one former observation of the loser, a lane each: the row entry, the record, and whether the winner gains it */
    __device__ bool settle(const Kind& V, int kind, int32_t winner, int32_t kf, int32_t idx, int32_t recAt, int32_t* weight)
    {
        const bool moved = !((sBits[kf >> 5] >> (kf & 31)) & 1u);
        const int32_t at = V.rowOff[kf] + idx;
        V.row[at] = moved ? winner : -1;
        L.recKf[recAt] = kf;
        L.recIdx[recAt] = idx;
        L.recMoved[recAt] = moved ? 1 : 0;
        if (moved) *weight = fuse_obs_weight(kind, kind == FUSE_POINT ? L.A.stereo[at] : 0);
        return moved;
    }

    /* MapPoint::Replace / MapLine::Replace; the caller has made room for the loser's observations in the log and the records */
    __device__ void replace(const Kind& V, int kind, int32_t loser, int32_t winner)
    {
        const int tid = threadIdx.x;
        const int32_t caL = L.clearedAt[kind][loser], caW = L.clearedAt[kind][winner];
        const int32_t keyL = loser * 2 + kind, keyW = winner * 2 + kind;
        const int32_t logEnd = logLen, rec0 = nRec;
        __syncthreads();
        for (int w = tid; w < (L.I.nK + 31) / 32; w += FUSE_TILE) sBits[w] = 0;
        if (tid == 0) *sFlag = 0;
        __syncthreads();
        if (caW == 0)
            for (int32_t o = V.obsOff[winner] + tid; o < V.obsOff[winner + 1]; o += FUSE_TILE) atomicOr(&sBits[V.obs[o] >> 5], 1u << (V.obs[o] & 31));
        for (int32_t j = (caW ? caW - 1 : 0) + tid; j < logEnd; j += FUSE_TILE)
            if (L.log[3 * j] == keyW) atomicOr(&sBits[L.log[3 * j + 1] >> 5], 1u << (L.log[3 * j + 1] & 31));
        __syncthreads();
        int32_t sum = 0;
        int total;
        unsigned long long ballot;
        /* the stored list, in stored order */
        if (caL == 0) {
            const int32_t o0 = V.obsOff[loser], n1 = V.obsOff[loser + 1] - o0;
            for (int32_t b = 0; b < n1; b += FUSE_TILE) {
                const int32_t o = b + tid;
                int32_t w = 0, kf = 0, idx = 0;
                bool moved = false;
                if (o < n1) {
                    kf = V.obs[o0 + o];
                    idx = V.obsIdx[o0 + o];
                    moved = settle(V, kind, winner, kf, idx, nRec + o, &w);
                }
                const int r = block_rank(moved, shWave, &total, &ballot);
                if (moved) {
                    L.log[3 * (logLen + r)] = keyW;
                    L.log[3 * (logLen + r) + 1] = kf;
                    L.log[3 * (logLen + r) + 2] = idx;
                    sum += w;
                }
                logLen += total;
            }
            nRec += n1;
        }
        /* what the call added to the loser since, in the order it was added */
        for (int32_t j0 = caL ? caL - 1 : 0; j0 < logEnd; j0 += FUSE_TILE) {
            const int32_t j = j0 + tid;
            const bool is = j < logEnd && L.log[3 * j] == keyL;
            const int r = block_rank(is, shWave, &total, &ballot);
            const int32_t found = total;
            int32_t w = 0, kf = 0, idx = 0;
            bool moved = false;
            if (is) {
                kf = L.log[3 * j + 1];
                idx = L.log[3 * j + 2];
                moved = settle(V, kind, winner, kf, idx, nRec + r, &w);
            }
            const int r2 = block_rank(moved, shWave, &total, &ballot);
            if (moved) {
                L.log[3 * (logLen + r2)] = keyW;
                L.log[3 * (logLen + r2) + 1] = kf;
                L.log[3 * (logLen + r2) + 2] = idx;
                sum += w;
            }
            logLen += total;
            nRec += found;
        }
        if (sum) atomicAdd(sFlag, sum);
        __syncthreads();
        if (tid == 0) {
            V.bad[loser] = 1;
            L.clearedAt[kind][loser] = logLen + 1;
            V.nObs[winner] += *sFlag;
            V.found[winner] = fuse_wrap_add(V.found[winner], V.found[loser]);
            V.visible[winner] = fuse_wrap_add(V.visible[winner], V.visible[loser]);
            L.rKind[nRepl] = kind;
            L.rLoser[nRepl] = loser;
            L.rWinner[nRepl] = winner;
            L.rOff[nRepl] = rec0;
            L.rOff[nRepl + 1] = nRec;
        }
        nRepl++;
        __syncthreads();
    }

    __device__ bool room(int32_t appends) const { return logLen + appends <= L.logCap && nRec + appends <= L.recCap; }
};

__global__ __launch_bounds__(FUSE_TILE) void k_fuse_walk(FuseLaunch L)
{
    __shared__ int32_t shWave[FUSE_TILE / 64];
    __shared__ int32_t sFlag;
    __shared__ uint32_t sBits[FUSE_MAX_KFS / 32];
    const int tid = threadIdx.x;
    Walk W{L, shWave, &sFlag, sBits, 0, 0, 0};
    if (tid == 0) L.rOff[0] = 0;
    int stopped = 0, stopStep = 0, stopPass = 0, stopCand = 0, stopFused = 0;
    for (int s = 0; s < L.nSteps && !stopped; s++) {
        const FuseStep S = L.step[s];
        const Kind V = kind_of(L, S.kind);
        const int32_t rowBase = V.rowOff[S.kf], rowLen = V.rowOff[S.kf + 1] - rowBase;
        int32_t fused = 0;
        if (S.form == FUSE_LOOP) {
            /* spAlreadyFound and the bad flags as the step finds them */
            for (int32_t e = tid; e < rowLen; e += FUSE_TILE) {
                const int32_t it = V.row[rowBase + e];
                if (it >= 0) L.snap[it] = s + 1;
            }
            __syncthreads();
            for (int t = S.tile0; t < S.tile1; t++)
                for (int j = tid; j < L.tileCnt[t]; j += FUSE_TILE) {
                    const int c = L.packed[(size_t)t * FUSE_TILE + j];
                    const int32_t item = L.cand[c];
                    L.action[c] = V.bad[item] || L.snap[item] == s + 1 ? FUSE_SKIPPED : FUSE_PENDING;
                }
            __syncthreads();
        }
        const int passes = S.form == FUSE_LOOP ? 2 : 1;
        for (int pass = 0; pass < passes && !stopped; pass++)
            for (int t = S.tile0; t < S.tile1 && !stopped; t++) {
                const int cnt = L.tileCnt[t];
                for (int j = 0; j < cnt && !stopped; j++) {
                    const int c = L.packed[(size_t)t * FUSE_TILE + j];
                    const int32_t item = L.cand[c];
                    const int32_t bi = S.form == FUSE_MATCHED ? c - S.candOff : L.best[c];
                    int action = -1;
                    if (pass == 1) {
                        /* replace[i]->Replace(candidate[i]) of the Sim3 form */
                        if (L.action[c] != FUSE_RECORDED) continue;
                        const int32_t loser = L.rep[c];
                        if (loser == item) continue;
                        if (!W.room(W.held(V, S.kind, loser))) stopped = 1;
                        else W.replace(V, S.kind, loser, item);
                    } else if (S.form == FUSE_NEIGHBOURS) {
                        if (V.bad[item] || (fuse_asks_in_keyframe(S.kind) && W.member(V, S.kind, item, S.kf))) {
                            action = FUSE_SKIPPED;
                        } else {
                            const int32_t occ = V.row[rowBase + bi];
                            if (occ < 0) {
                                if (!W.room(1)) stopped = 1;
                                else {
                                    const bool gains = fuse_asks_in_keyframe(S.kind) || !W.member(V, S.kind, item, S.kf);
                                    W.add(V, S.kind, item, S.kf, bi, gains);
                                    action = gains ? FUSE_ADDED : FUSE_ROW_ONLY;
                                }
                            } else if (V.bad[occ]) {
                                action = FUSE_OCC_BAD;
                            } else if (occ == item) {
                                action = FUSE_SELF;
                            } else {
                                const bool candLoses = fuse_candidate_loses(V.nObs[occ], V.nObs[item]);
                                const int32_t loser = candLoses ? item : occ, winner = candLoses ? occ : item;
                                if (!W.room(W.held(V, S.kind, loser))) stopped = 1;
                                else {
                                    W.replace(V, S.kind, loser, winner);
                                    action = candLoses ? FUSE_CAND_REPLACED : FUSE_OCC_REPLACED;
                                }
                            }
                        }
                    } else if (S.form == FUSE_LOOP) {
                        if (L.action[c] != FUSE_PENDING) continue;
                        const int32_t occ = V.row[rowBase + bi];
                        if (occ >= 0) {
                            action = V.bad[occ] ? FUSE_OCC_BAD : FUSE_RECORDED;
                            if (action == FUSE_RECORDED && tid == 0) L.rep[c] = occ;
                        } else if (!W.room(1)) {
                            stopped = 1;
                        } else {
                            const bool gains = !W.member(V, S.kind, item, S.kf);
                            W.add(V, S.kind, item, S.kf, bi, gains);
                            action = gains ? FUSE_ADDED : FUSE_ROW_ONLY;
                        }
                    } else {
                        const int32_t occ = V.row[rowBase + bi];
                        if (occ < 0) {
                            if (!W.room(1)) stopped = 1;
                            else {
                                const bool gains = !W.member(V, S.kind, item, S.kf);
                                W.add(V, S.kind, item, S.kf, bi, gains);
                                action = gains ? FUSE_ADDED : FUSE_ROW_ONLY;
                            }
                        } else if (occ == item) {
                            action = FUSE_SELF;
                        } else if (!W.room(W.held(V, S.kind, occ))) {
                            stopped = 1;
                        } else {
                            W.replace(V, S.kind, occ, item);
                            action = FUSE_OCC_REPLACED;
                        }
                    }
                    if (stopped) {
                        stopStep = s;
                        stopPass = pass;
                        stopCand = c;
                        stopFused = fused;
                    } else if (action >= 0) {
                        fused += fuse_counts(action);
                        if (tid == 0) L.action[c] = (uint8_t)action;
                        __syncthreads();
                    }
                }
            }
        if (tid == 0 && !stopped) L.nFused[s] = fused;
    }
    if (tid == 0) {
        L.head[FUSE_HEAD_STOPPED] = stopped;
        L.head[FUSE_HEAD_STEP] = stopStep;
        L.head[FUSE_HEAD_PASS] = stopPass;
        L.head[FUSE_HEAD_CAND] = stopCand;
        L.head[FUSE_HEAD_FUSED] = stopFused;
        L.head[FUSE_HEAD_REPL] = W.nRepl;
        L.head[FUSE_HEAD_REC] = W.nRec;
        L.head[FUSE_HEAD_LOG] = W.logLen;
    }
}

}  // namespace

hipError_t drfe_launch_fuse(const FuseLaunch& L, hipStream_t s)
{
    if (L.nTiles > 0) hipLaunchKernelGGL(k_fuse_live, dim3((unsigned)L.nTiles), dim3(FUSE_TILE), 0, s, L);
    hipLaunchKernelGGL(k_fuse_walk, dim3(1), dim3(FUSE_TILE), 0, s, L);
    return hipGetLastError();
}
