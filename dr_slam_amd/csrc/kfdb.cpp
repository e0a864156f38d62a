/* kfdb.cpp — KeyFrameDatabase (reference src/KeyFrameDatabase.cc:40-309) behind the C-ABI of include/drfe.h: the key-frame table,
 * the argument checks, the host entries, the device entries (kfdb_kernels.hip) and the counters.  Both sides evaluate
 * kfdb_core.h.  A call is checked as a whole, run on a copy of what it may change, and committed only when its results fit the
 * caller's arrays.  DESIGN.md section 23. */
#include "kfdb_internal.h"
#include "stage_layout.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace {

struct KfdbKf {
    int32_t handle = -1;               /* -1: a free slot */
    int64_t seq = -1;                  /* sequence number of the latest add; -1: not in the inverted file */
    std::vector<int32_t> ids;          /* mBowVec */
    std::vector<double> vals;
    int32_t nbr[KFDB_NEIGHBOURS];      /* GetBestCovisibilityKeyFrames(10) as handles, -1 = none */
    float relocScore = 0.0f;           /* mRelocScore */
    uint8_t relocWritten = 0;
    KfdbKf() { for (int k = 0; k < KFDB_NEIGHBOURS; k++) nbr[k] = -1; }
};

/* a checked call: both kinds of query in the form the host loop and the kernels read */
struct Call {
    bool reloc = false;
    int n = 0;
    std::vector<int32_t> qOff, qIds;
    std::vector<double> qVals;
    std::vector<int32_t> connOff, conn, covOff, cov;   /* slots */
    std::vector<float> minScoreIn;
    std::vector<uint8_t> useCov;
    std::vector<int64_t> seq;          /* per slot during this call, add_after included */
    std::vector<int32_t> from;         /* per slot: first query of the call that sees it */
    int64_t nextSeq = 0, lastId = 0;
};

struct Result {
    std::vector<KfdbQueryRec> rec;
    std::vector<int32_t> candOff, cand;   /* slots */
    std::vector<float> relocScore;
    std::vector<uint8_t> relocWritten;
};

}  // namespace

struct drfe_kfdb {
    drfe_ctx* ctx = nullptr;
    int device = 0;                    /* the context's, kept for the buffers' release */
    std::mutex mu;
    std::string err;
    std::vector<KfdbKf> kf;            /* slots; std::vector grows by doubling */
    std::unordered_map<int32_t, int32_t> slotOf;
    std::vector<int32_t> freeSlots;
    int32_t nVisible = 0;
    int64_t nextSeq = 0, lastLoopId = 0, lastRelocId = 0;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    /* what the device copy lacks */
    bool wordsDirty = true, nbrDirty = true, relocDirty = true;
    DevBuf<int32_t> dWordOff, dWordIds, dNbr;
    DevBuf<double> dWordVals;
    DevBuf<float> dReloc;
    DevBuf<uint8_t> dWritten;
    StagePair io;
    DevBuf<char> scratch;
    PinnedBuf<char> hup;               /* staging of an upload of the tables */
};

namespace {

/* pairs (query, slot) above which a device call is refused: its scratch is 37 bytes a pair */
const int64_t KFDB_DEVICE_MAX_PAIRS = (int64_t)1 << 26;

int fail(drfe_kfdb* db, int rc, const char* why)
{
    db->err = why;
    return rc;
}

int slot_of(const drfe_kfdb* db, int32_t handle)
{
    const auto it = db->slotOf.find(handle);
    return it == db->slotOf.end() ? -1 : it->second;
}

bool ascending(const int32_t* ids, int n)
{
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || (i > 0 && ids[i] <= ids[i - 1])) return false;
    return true;
}

bool offsets_ok(const int32_t* off, int n)
{
    if (!off || off[0] != 0) return false;
    for (int k = 0; k < n; k++)
        if (off[k + 1] < off[k]) return false;
    return true;
}

int check_out(drfe_kfdb* db, int n, const drfe_kfdb_out* o)
{
    if (!o || o->cand_capacity < 0 || !o->cand_offsets || !o->record || (o->cand_capacity > 0 && !o->candidates))
        return fail(db, DRFE_ERR_INVALID, "kfdb: invalid output arrays");
    (void)n;
    return DRFE_OK;
}

int check_ids(drfe_kfdb* db, int n, const int64_t* id, int64_t last)
{
    if (!id) return fail(db, DRFE_ERR_INVALID, "kfdb: invalid argument");
    for (int k = 0; k < n; k++) {
        if (id[k] == 0 || id[k] <= last) return fail(db, DRFE_ERR_INVALID, "kfdb: a query id is 0 or does not exceed the last id used on this database");
        last = id[k];
    }
    return DRFE_OK;
}

void call_visibility(const drfe_kfdb* db, Call& C)
{
    const size_t nS = db->kf.size();
    C.seq.resize(nS);
    C.from.assign(nS, 0);
    for (size_t s = 0; s < nS; s++) C.seq[s] = db->kf[s].seq;
    C.nextSeq = db->nextSeq;
}

int plan_loop(drfe_kfdb* db, const drfe_kfdb_loop_queries* q, const drfe_kfdb_out* o, Call& C)
{
    if (!q || q->n < 0) return fail(db, DRFE_ERR_INVALID, "kfdb: invalid argument");
    if (q->n > DRFE_KFDB_MAX_QUERIES) return fail(db, DRFE_ERR_INVALID, "kfdb: more than DRFE_KFDB_MAX_QUERIES queries in a call");
    int rc = check_out(db, q->n, o);
    if (rc) return rc;
    const int n = q->n;
    C.reloc = false;
    C.n = n;
    if (n == 0) return DRFE_OK;
    if (!q->handle) return fail(db, DRFE_ERR_INVALID, "kfdb: invalid argument");
    rc = check_ids(db, n, q->id, db->lastLoopId);
    if (rc) return rc;
    if (!offsets_ok(q->connected_offsets, n) || (q->connected_offsets[n] > 0 && !q->connected))
        return fail(db, DRFE_ERR_INVALID, "kfdb: connected_offsets do not start at 0 or decrease");
    if (!q->min_score && (!offsets_ok(q->covisible_offsets, n) || (q->covisible_offsets[n] > 0 && !q->covisible)))
        return fail(db, DRFE_ERR_INVALID, "kfdb: neither min_score nor a valid covisible list");
    call_visibility(db, C);
    C.qOff.assign(1, 0);
    C.connOff.assign(1, 0);
    C.covOff.assign(1, 0);
    C.minScoreIn.assign((size_t)n, 0.0f);
    C.useCov.assign((size_t)n, q->min_score ? 0 : 1);
    for (int k = 0; k < n; k++) {
        const int s = slot_of(db, q->handle[k]);
        if (s < 0) return fail(db, DRFE_ERR_INVALID, "kfdb: unknown query handle");
        const KfdbKf& K = db->kf[(size_t)s];
        C.qIds.insert(C.qIds.end(), K.ids.begin(), K.ids.end());
        C.qVals.insert(C.qVals.end(), K.vals.begin(), K.vals.end());
        C.qOff.push_back((int32_t)C.qIds.size());
        for (int i = q->connected_offsets[k]; i < q->connected_offsets[k + 1]; i++) {
            const int t = slot_of(db, q->connected[i]);
            if (t < 0) return fail(db, DRFE_ERR_INVALID, "kfdb: unknown connected handle");
            C.conn.push_back(t);
        }
        C.connOff.push_back((int32_t)C.conn.size());
        if (q->min_score) {
            C.minScoreIn[(size_t)k] = q->min_score[k];
        } else {
            for (int i = q->covisible_offsets[k]; i < q->covisible_offsets[k + 1]; i++) {
                const int t = slot_of(db, q->covisible[i]);
                if (t < 0) return fail(db, DRFE_ERR_INVALID, "kfdb: unknown covisible handle");
                C.cov.push_back(t);
            }
        }
        C.covOff.push_back((int32_t)C.cov.size());
        if (q->add_after && q->add_after[k]) {
            if (C.seq[(size_t)s] >= 0) return fail(db, DRFE_ERR_INVALID, "kfdb: add_after of a key frame that is in the inverted file");
            C.seq[(size_t)s] = C.nextSeq++;
            C.from[(size_t)s] = k + 1;
        }
    }
    C.lastId = q->id[n - 1];
    return DRFE_OK;
}

int plan_reloc(drfe_kfdb* db, const drfe_kfdb_reloc_queries* q, const drfe_kfdb_out* o, Call& C)
{
    if (!q || q->n < 0) return fail(db, DRFE_ERR_INVALID, "kfdb: invalid argument");
    if (q->n > DRFE_KFDB_MAX_QUERIES) return fail(db, DRFE_ERR_INVALID, "kfdb: more than DRFE_KFDB_MAX_QUERIES queries in a call");
    int rc = check_out(db, q->n, o);
    if (rc) return rc;
    const int n = q->n;
    C.reloc = true;
    C.n = n;
    if (n == 0) return DRFE_OK;
    rc = check_ids(db, n, q->id, db->lastRelocId);
    if (rc) return rc;
    if (!offsets_ok(q->word_offsets, n) || (q->word_offsets[n] > 0 && (!q->word_ids || !q->values)))
        return fail(db, DRFE_ERR_INVALID, "kfdb: word_offsets do not start at 0 or decrease");
    for (int k = 0; k < n; k++)
        if (!ascending(q->word_ids + q->word_offsets[k], q->word_offsets[k + 1] - q->word_offsets[k]))
            return fail(db, DRFE_ERR_INVALID, "kfdb: word ids of a query are not ascending");
    call_visibility(db, C);
    const int nW = q->word_offsets[n];
    C.qOff.assign(q->word_offsets, q->word_offsets + n + 1);
    C.qIds.assign(q->word_ids, q->word_ids + nW);
    C.qVals.assign(q->values, q->values + nW);
    C.lastId = q->id[n - 1];
    return DRFE_OK;
}

/* the neighbour test and score of the host loop (KfdbLook of kfdb_kernels.hip reads the same from the marks of all queries) */
struct HostLook {
    bool reloc;
    const uint8_t* flag;
    const float* score;
    const float* relocScore;
    const uint8_t* relocWritten;
    int32_t uninit;
    bool operator()(int32_t nb, float* s)
    {
        if (!reloc) {
            if (!(flag[nb] & KFDB_F_SCORED)) return false;
            *s = score[nb];
            return true;
        }
        if (!(flag[nb] & KFDB_F_LISTED)) return false;
        /* scored by this query: already written; else what an earlier query left */
        if (relocWritten[nb]) {
            *s = relocScore[nb];
        } else {
            *s = 0.0f;
            uninit++;
        }
        return true;
    }
};

/* neighbour handles as slots, -1 where the key frame is gone */
void neighbour_slots(const drfe_kfdb* db, std::vector<int32_t>& nbr)
{
    const size_t nS = db->kf.size();
    nbr.assign(nS * KFDB_NEIGHBOURS, -1);
    for (size_t s = 0; s < nS; s++)
        if (db->kf[s].handle >= 0)
            for (int k = 0; k < KFDB_NEIGHBOURS; k++)
                if (db->kf[s].nbr[k] >= 0) nbr[s * KFDB_NEIGHBOURS + k] = slot_of(db, db->kf[s].nbr[k]);
}

void run_host(const drfe_kfdb* db, const Call& C, Result& R)
{
    const size_t nS = db->kf.size();
    const int n = C.n;
    R.rec.assign((size_t)n, KfdbQueryRec{});
    R.candOff.assign(1, 0);
    R.relocScore.resize(nS);
    R.relocWritten.resize(nS);
    for (size_t s = 0; s < nS; s++) {
        R.relocScore[s] = db->kf[s].relocScore;
        R.relocWritten[s] = db->kf[s].relocWritten;
    }
    std::vector<int32_t> nbr;
    neighbour_slots(db, nbr);
    std::vector<int32_t> cnt(nS), first(nS), kept, best, minEntry(nS);
    std::vector<float> score(nS), acc;
    std::vector<uint8_t> flag(nS);
    for (int k = 0; k < n; k++) {
        KfdbQueryRec& Q = R.rec[(size_t)k];
        const int32_t* qi = C.qIds.data() + C.qOff[(size_t)k];
        const double* qv = C.qVals.data() + C.qOff[(size_t)k];
        const int nQw = C.qOff[(size_t)k + 1] - C.qOff[(size_t)k];
        std::fill(flag.begin(), flag.end(), 0);
        float minScore = 0.0f;
        if (!C.reloc) {
            for (int i = C.connOff[(size_t)k]; i < C.connOff[(size_t)k + 1]; i++) flag[(size_t)C.conn[(size_t)i]] = KFDB_F_CONNECTED;
            if (C.useCov[(size_t)k]) {
                minScore = 1.0f;
                for (int i = C.covOff[(size_t)k]; i < C.covOff[(size_t)k + 1]; i++) {
                    const KfdbKf& K = db->kf[(size_t)C.cov[(size_t)i]];
                    int32_t c, f;
                    double sum;
                    kfdb_walk(qi, qv, nQw, K.ids.data(), K.vals.data(), (int)K.ids.size(), &c, &f, &sum);
                    const float sc = kfdb_score(sum);
                    if (sc < minScore) minScore = sc;
                }
            } else {
                minScore = C.minScoreIn[(size_t)k];
            }
        }
        Q.minScore = minScore;
        for (size_t s = 0; s < nS; s++) {
            if (!(C.seq[s] >= 0 && C.from[s] <= k)) continue;
            const KfdbKf& K = db->kf[s];
            double sum;
            kfdb_walk(qi, qv, nQw, K.ids.data(), K.vals.data(), (int)K.ids.size(), &cnt[s], &first[s], &sum);
            score[s] = kfdb_score(sum);
            if (cnt[s] > 0 && !(flag[s] & KFDB_F_CONNECTED)) {
                flag[s] |= KFDB_F_LISTED;
                Q.listed++;
                if (cnt[s] > Q.maxCommon) Q.maxCommon = cnt[s];
            }
        }
        Q.minCommon = kfdb_min_common(Q.maxCommon);
        kept.clear();
        for (size_t s = 0; s < nS; s++) {
            if (!(flag[s] & KFDB_F_LISTED) || cnt[s] <= Q.minCommon) continue;
            flag[s] |= KFDB_F_SCORED;
            Q.scored++;
            if (C.reloc) {
                R.relocScore[s] = score[s];
                R.relocWritten[s] = 1;
            }
            if (C.reloc || score[s] >= minScore) kept.push_back((int32_t)s);
        }
        Q.kept = (int32_t)kept.size();
        std::sort(kept.begin(), kept.end(), [&](int32_t a, int32_t b) {
            return kfdb_before(first[(size_t)a], C.seq[(size_t)a], first[(size_t)b], C.seq[(size_t)b]) != 0;
        });
        acc.resize(kept.size());
        best.resize(kept.size());
        float bestAcc = C.reloc ? 0.0f : minScore;
        HostLook look{C.reloc, flag.data(), score.data(), R.relocScore.data(), R.relocWritten.data(), 0};
        for (size_t e = 0; e < kept.size(); e++) {
            const int32_t s = kept[e];
            kfdb_accumulate(score[(size_t)s], s, nbr.data() + (size_t)KFDB_NEIGHBOURS * (size_t)s, look, &acc[e], &best[e]);
            if (acc[e] > bestAcc) bestAcc = acc[e];
        }
        Q.uninit = look.uninit;
        const float retain = kfdb_retain(bestAcc);
        for (size_t e = 0; e < kept.size(); e++)
            if (acc[e] > retain) minEntry[(size_t)best[e]] = -1;
        for (size_t e = 0; e < kept.size(); e++)
            if (acc[e] > retain && minEntry[(size_t)best[e]] == -1) {
                minEntry[(size_t)best[e]] = 0;
                R.cand.push_back(best[e]);
                Q.nCand++;
            }
        R.candOff.push_back((int32_t)R.cand.size());
    }
}

/* the tables the kernels read, brought up to date; then one call */
int run_device(drfe_kfdb* db, const Call& C, Result& R, int32_t capacity, void* stream)
{
    drfe_ctx* c = db->ctx;
    const size_t nS = db->kf.size();
    const int n = C.n;
    R.rec.assign((size_t)n, KfdbQueryRec{});
    R.candOff.assign((size_t)n + 1, 0);
    if (n == 0 || nS == 0) return DRFE_OK;
    if ((int64_t)n * (int64_t)nS > KFDB_DEVICE_MAX_PAIRS) return fail(db, DRFE_ERR_CAPACITY, "kfdb: queries x key frames exceed the device scratch bound");
    HIPCHK_TO(db->err, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (db->wordsDirty || db->nbrDirty || db->relocDirty) {
        std::vector<int32_t> off(nS + 1, 0), nbr;
        for (size_t s = 0; s < nS; s++) off[s + 1] = off[s] + (int32_t)db->kf[s].ids.size();
        const size_t nW = (size_t)off[nS];
        neighbour_slots(db, nbr);
        StageLayout<16> up;
        const auto uOff = up.add<int32_t>(nS + 1);
        const auto uIds = up.add<int32_t>(nW);
        const auto uVals = up.add<double>(nW);
        const auto uNbr = up.add<int32_t>(nS * KFDB_NEIGHBOURS);
        const auto uSc = up.add<float>(nS);
        const auto uWr = up.add<uint8_t>(nS);
        /* a table that no longer fits is allocated at twice the size */
        HIPCHK_TO(db->err, db->hup.grow(db->hup.capacity() >= up.bytes() ? up.bytes() : 2 * up.bytes()));
        char* h = db->hup;
        uOff.put(h, off.data());
        uNbr.put(h, nbr.data());
        for (size_t s = 0; s < nS; s++) {
            const KfdbKf& K = db->kf[s];
            if (!K.ids.empty()) {
                std::memcpy(uIds.at(h) + off[s], K.ids.data(), K.ids.size() * sizeof(int32_t));
                std::memcpy(uVals.at(h) + off[s], K.vals.data(), K.vals.size() * sizeof(double));
            }
            uSc.at(h)[s] = K.relocScore;
            uWr.at(h)[s] = K.relocWritten;
        }
        if (db->wordsDirty) {
            HIPCHK_TO(db->err, db->dWordOff.grow(db->dWordOff.capacity() >= nS + 1 ? nS + 1 : 2 * (nS + 1)));
            HIPCHK_TO(db->err, db->dWordIds.grow(db->dWordIds.capacity() >= nW ? nW : 2 * nW));
            HIPCHK_TO(db->err, db->dWordVals.grow(db->dWordVals.capacity() >= nW ? nW : 2 * nW));
            HIPCHK_TO(db->err, hipMemcpyAsync(db->dWordOff, uOff.at(h), uOff.bytes(), hipMemcpyHostToDevice, st));
            if (nW) {
                HIPCHK_TO(db->err, hipMemcpyAsync(db->dWordIds, uIds.at(h), uIds.bytes(), hipMemcpyHostToDevice, st));
                HIPCHK_TO(db->err, hipMemcpyAsync(db->dWordVals, uVals.at(h), uVals.bytes(), hipMemcpyHostToDevice, st));
            }
            db->stats[5]++;
        }
        if (db->nbrDirty) {
            HIPCHK_TO(db->err, db->dNbr.grow(db->dNbr.capacity() >= uNbr.n ? uNbr.n : 2 * uNbr.n));
            HIPCHK_TO(db->err, hipMemcpyAsync(db->dNbr, uNbr.at(h), uNbr.bytes(), hipMemcpyHostToDevice, st));
        }
        if (db->relocDirty) {
            HIPCHK_TO(db->err, db->dReloc.grow(db->dReloc.capacity() >= nS ? nS : 2 * nS));
            HIPCHK_TO(db->err, db->dWritten.grow(db->dWritten.capacity() >= nS ? nS : 2 * nS));
            HIPCHK_TO(db->err, hipMemcpyAsync(db->dReloc, uSc.at(h), uSc.bytes(), hipMemcpyHostToDevice, st));
            HIPCHK_TO(db->err, hipMemcpyAsync(db->dWritten, uWr.at(h), uWr.bytes(), hipMemcpyHostToDevice, st));
        }
        /* the staging block is written again by the next upload */
        HIPCHK_TO(db->err, hipStreamSynchronize(st));
        db->wordsDirty = db->nbrDirty = db->relocDirty = false;
    }
    const size_t nP = (size_t)n * nS;
    StageLayout<16> in, out, scr;
    const auto sSeq = in.add<int64_t>(nS);
    const auto sFrom = in.add<int32_t>(nS);
    const auto sQOff = in.add<int32_t>((size_t)n + 1);
    const auto sQIds = in.add<int32_t>(C.qIds.size());
    const auto sQVals = in.add<double>(C.qVals.size());
    const auto sConnOff = in.add<int32_t>(C.connOff.size());
    const auto sConn = in.add<int32_t>(C.conn.size());
    const auto sCovOff = in.add<int32_t>(C.covOff.size());
    const auto sCov = in.add<int32_t>(C.cov.size());
    const auto sMin = in.add<float>(C.minScoreIn.size());
    const auto sUse = in.add<uint8_t>(C.useCov.size());
    const auto oRec = out.add<KfdbQueryRec>((size_t)n);
    const auto oOff = out.add<int32_t>((size_t)n + 1);
    const auto oSc = out.add<float>(nS);
    const auto oWr = out.add<uint8_t>(nS);
    const size_t headBytes = out.bytes();
    const auto oCand = out.add<int32_t>(std::min(nP, (size_t)capacity));
    const auto xFlag = scr.add<uint8_t>(nP);
    const auto xMinEntry = scr.add<int32_t>(nP);
    const auto xCnt = scr.add<int32_t>(nP);
    const auto xFirst = scr.add<int32_t>(nP);
    const auto xScore = scr.add<float>(nP);
    const auto xKeptTmp = scr.add<int32_t>(nP);
    const auto xKeptOrd = scr.add<int32_t>(nP);
    const auto xAcc = scr.add<float>(nP);
    const auto xBest = scr.add<int32_t>(nP);
    const auto xCand = scr.add<int32_t>(nP);
    const auto xPacked = scr.add<int32_t>(nP);
    HIPCHK_TO(db->err, db->io.grow(in.bytes(), out.bytes()));
    HIPCHK_TO(db->err, db->scratch.grow(scr.bytes()));
    char* h = db->io.hin;
    sSeq.put(h, C.seq.data());
    sFrom.put(h, C.from.data());
    sQOff.put(h, C.qOff.data());
    sQIds.put(h, C.qIds.data());
    sQVals.put(h, C.qVals.data());
    sConnOff.put(h, C.connOff.data());
    sConn.put(h, C.conn.data());
    sCovOff.put(h, C.covOff.data());
    sCov.put(h, C.cov.data());
    sMin.put(h, C.minScoreIn.data());
    sUse.put(h, C.useCov.data());
    const char* d = db->io.din;
    char* dO = db->io.dout;
    char* dS = db->scratch;
    HIPCHK_TO(db->err, hipMemcpyAsync(db->io.din, h, in.bytes(), hipMemcpyHostToDevice, st));
    HIPCHK_TO(db->err, hipMemsetAsync(xFlag.at(dS), 0, xFlag.bytes(), st));
    HIPCHK_TO(db->err, hipMemsetAsync(xMinEntry.at(dS), 0x7f, xMinEntry.bytes(), st));
    KfdbLaunch L{};
    L.nQueries = n;
    L.nSlots = (int)nS;
    L.reloc = C.reloc ? 1 : 0;
    L.wordOff = db->dWordOff;
    L.wordIds = db->dWordIds;
    L.wordVals = db->dWordVals;
    L.nbr = db->dNbr;
    L.relocScore = db->dReloc;
    L.relocWritten = db->dWritten;
    L.seq = sSeq.at(d);
    L.from = sFrom.at(d);
    L.qOff = sQOff.at(d);
    L.qIds = sQIds.at(d);
    L.qVals = sQVals.at(d);
    L.connOff = sConnOff.at(d);
    L.conn = sConn.at(d);
    L.covOff = sCovOff.at(d);
    L.cov = sCov.at(d);
    L.minScoreIn = sMin.at(d);
    L.useCov = sUse.at(d);
    L.flag = xFlag.at(dS);
    L.minEntry = xMinEntry.at(dS);
    L.cnt = xCnt.at(dS);
    L.first = xFirst.at(dS);
    L.score = xScore.at(dS);
    L.keptTmp = xKeptTmp.at(dS);
    L.keptOrd = xKeptOrd.at(dS);
    L.acc = xAcc.at(dS);
    L.best = xBest.at(dS);
    L.cand = xCand.at(dS);
    L.rec = oRec.at(dO);
    L.candOff = oOff.at(dO);
    L.candPacked = xPacked.at(dS);
    /* from here on the resident mRelocScore may differ from the host's until the call is committed */
    if (C.reloc) db->relocDirty = true;
    hipError_t e = drfe_launch_kfdb(L, st);
    if (e == hipSuccess && C.reloc) {
        e = hipMemcpyAsync(oSc.at(dO), db->dReloc, oSc.bytes(), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(oWr.at(dO), db->dWritten, oWr.bytes(), hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(db->io.hout, dO, headBytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { db->err = std::string("kfdb device call: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
    const char* ho = db->io.hout;
    std::memcpy(R.rec.data(), oRec.at(ho), oRec.bytes());
    std::memcpy(R.candOff.data(), oOff.at(ho), oOff.bytes());
    if (C.reloc) {
        R.relocScore.assign(oSc.at(ho), oSc.at(ho) + nS);
        R.relocWritten.assign(oWr.at(ho), oWr.at(ho) + nS);
    }
    const int32_t total = R.candOff[(size_t)n];
    if (total > capacity) return DRFE_OK;       /* the caller refuses it; the second copy would not fit */
    if (total > 0) {
        HIPCHK_TO(db->err, hipMemcpyAsync(oCand.at(db->io.hout.get()), xPacked.at(dS), (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK_TO(db->err, hipStreamSynchronize(st));
        R.cand.assign(oCand.at(ho), oCand.at(ho) + total);
    }
    return DRFE_OK;
}

/* results into the caller's arrays and the call's changes into the database, or neither */
int finish(drfe_kfdb* db, const Call& C, const Result& R, drfe_kfdb_out* o, bool onDevice)
{
    const int n = C.n;
    const int32_t total = n ? R.candOff[(size_t)n] : 0;
    if (total > o->cand_capacity) return fail(db, DRFE_ERR_CAPACITY, "kfdb: more candidates than cand_capacity");
    o->cand_offsets[0] = 0;
    int64_t uninit = 0;
    for (int k = 0; k < n; k++) {
        const KfdbQueryRec& Q = R.rec[(size_t)k];
        o->cand_offsets[k + 1] = R.candOff[(size_t)k + 1];
        o->record[4 * k + 0] = Q.listed;
        o->record[4 * k + 1] = Q.scored;
        o->record[4 * k + 2] = Q.kept;
        o->record[4 * k + 3] = Q.maxCommon;
        if (o->min_score) o->min_score[k] = Q.minScore;
        if (o->uninit_reads) o->uninit_reads[k] = Q.uninit;
        uninit += Q.uninit;
    }
    for (int32_t i = 0; i < total; i++) o->candidates[i] = db->kf[(size_t)R.cand[(size_t)i]].handle;
    if (n == 0) return DRFE_OK;
    if (C.reloc) {
        db->lastRelocId = C.lastId;
        for (size_t s = 0; s < db->kf.size() && s < R.relocScore.size(); s++) {
            db->kf[s].relocScore = R.relocScore[s];
            db->kf[s].relocWritten = R.relocWritten[s];
        }
        /* the device copy holds exactly this after a device call; a host call leaves it behind */
        db->relocDirty = !onDevice;
    } else {
        db->lastLoopId = C.lastId;
        for (size_t s = 0; s < db->kf.size(); s++)
            if (db->kf[s].seq < 0 && C.seq[s] >= 0) {
                db->kf[s].seq = C.seq[s];
                db->nVisible++;
            }
        db->nextSeq = C.nextSeq;
    }
    db->stats[C.reloc ? 2 : 0]++;
    db->stats[C.reloc ? 3 : 1] += n;
    if (onDevice) db->stats[4]++;
    db->stats[6] += total;
    db->stats[7] += uninit;
    return DRFE_OK;
}

/* mode: 0 host, 1 device, 2 by the crossover */
int run(drfe_kfdb* db, Call& C, drfe_kfdb_out* o, int mode, void* stream)
{
    bool dev = mode == 1;
    if (mode == 1 && !db->ctx) return fail(db, DRFE_ERR_STATE, "kfdb: a device call on a database without a context");
    if (mode == 2)
        dev = db->ctx && C.n >= DRFE_KFDB_DEVICE_FROM && (int64_t)C.n * (int64_t)db->kf.size() <= KFDB_DEVICE_MAX_PAIRS;
    Result R;
    if (dev && C.n > 0 && !db->kf.empty()) {
        const int rc = run_device(db, C, R, o->cand_capacity, stream);
        if (rc) return rc;
    } else {
        dev = false;
        run_host(db, C, R);
    }
    return finish(db, C, R, o, dev);
}

}  // namespace

extern "C" {

int drfe_kfdb_create(drfe_ctx* ctx, int scoring, drfe_kfdb** out)
{
    if (!out) return DRFE_ERR_INVALID;
    *out = nullptr;
    if (scoring != DRFE_KFDB_L1_NORM) return DRFE_ERR_INVALID;   /* only the ORB vocabulary's L1 is built */
    drfe_kfdb* db = new drfe_kfdb();
    db->ctx = ctx;
    if (ctx) db->device = ctx->device;
    *out = db;
    return DRFE_OK;
}

void drfe_kfdb_destroy(drfe_kfdb* db)
{
    if (!db) return;
    if (db->ctx) (void)hipSetDevice(db->device);
    delete db;
}

const char* drfe_kfdb_last_error(const drfe_kfdb* db) { return db ? db->err.c_str() : "kfdb: no database"; }

int drfe_kfdb_put(drfe_kfdb* db, int32_t handle, int32_t n, const int32_t* word_ids, const double* values)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (handle < 0 || n < 0 || (n > 0 && (!word_ids || !values))) return fail(db, DRFE_ERR_INVALID, "kfdb_put: invalid argument");
    if (!ascending(word_ids, n)) return fail(db, DRFE_ERR_INVALID, "kfdb_put: word ids are not ascending");
    if (slot_of(db, handle) >= 0) return fail(db, DRFE_ERR_INVALID, "kfdb_put: the handle is stored already");
    int32_t s;
    if (!db->freeSlots.empty()) {
        s = db->freeSlots.back();
        db->freeSlots.pop_back();
    } else {
        s = (int32_t)db->kf.size();
        db->kf.emplace_back();
    }
    KfdbKf& K = db->kf[(size_t)s];
    K = KfdbKf();
    K.handle = handle;
    K.ids.assign(word_ids, word_ids + n);
    K.vals.assign(values, values + n);
    db->slotOf[handle] = s;
    db->wordsDirty = db->nbrDirty = db->relocDirty = true;
    return DRFE_OK;
}

int drfe_kfdb_add(drfe_kfdb* db, int32_t handle)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    const int s = slot_of(db, handle);
    if (s < 0) return fail(db, DRFE_ERR_INVALID, "kfdb_add: unknown handle");
    if (db->kf[(size_t)s].seq >= 0) return fail(db, DRFE_ERR_INVALID, "kfdb_add: the key frame is in the inverted file already");
    db->kf[(size_t)s].seq = db->nextSeq++;
    db->nVisible++;
    return DRFE_OK;
}

int drfe_kfdb_erase(drfe_kfdb* db, int32_t handle)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    const int s = slot_of(db, handle);
    if (s < 0) return fail(db, DRFE_ERR_INVALID, "kfdb_erase: unknown handle");
    if (db->kf[(size_t)s].seq < 0) return fail(db, DRFE_ERR_INVALID, "kfdb_erase: the key frame is not in the inverted file");
    db->kf[(size_t)s].seq = -1;
    db->nVisible--;
    return DRFE_OK;
}

int drfe_kfdb_clear(drfe_kfdb* db)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    for (KfdbKf& K : db->kf) K.seq = -1;
    db->nVisible = 0;
    return DRFE_OK;
}

int drfe_kfdb_remove(drfe_kfdb* db, int32_t handle)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    const int s = slot_of(db, handle);
    if (s < 0) return fail(db, DRFE_ERR_INVALID, "kfdb_remove: unknown handle");
    if (db->kf[(size_t)s].seq >= 0) db->nVisible--;
    db->kf[(size_t)s] = KfdbKf();
    db->slotOf.erase(handle);
    db->freeSlots.push_back(s);
    db->wordsDirty = db->nbrDirty = db->relocDirty = true;
    return DRFE_OK;
}

int drfe_kfdb_set_neighbours(drfe_kfdb* db, int32_t count, const int32_t* handles, const int32_t* nbr)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    if (count < 0 || (count > 0 && (!handles || !nbr))) return fail(db, DRFE_ERR_INVALID, "kfdb_set_neighbours: invalid argument");
    for (int i = 0; i < count; i++) {
        if (slot_of(db, handles[i]) < 0) return fail(db, DRFE_ERR_INVALID, "kfdb_set_neighbours: unknown handle");
        for (int k = 0; k < KFDB_NEIGHBOURS; k++) {
            const int32_t h = nbr[(size_t)i * KFDB_NEIGHBOURS + k];
            if (h < -1 || (h >= 0 && slot_of(db, h) < 0)) return fail(db, DRFE_ERR_INVALID, "kfdb_set_neighbours: unknown neighbour handle");
        }
    }
    for (int i = 0; i < count; i++)
        std::memcpy(db->kf[(size_t)slot_of(db, handles[i])].nbr, nbr + (size_t)i * KFDB_NEIGHBOURS, sizeof(int32_t) * KFDB_NEIGHBOURS);
    if (count) db->nbrDirty = true;
    return DRFE_OK;
}

int drfe_kfdb_size(drfe_kfdb* db, int32_t* out2)
{
    if (!db || !out2) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    out2[0] = (int32_t)db->slotOf.size();
    out2[1] = db->nVisible;
    return DRFE_OK;
}

static int loop_entry(drfe_kfdb* db, const drfe_kfdb_loop_queries* q, drfe_kfdb_out* o, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    Call C;
    const int rc = plan_loop(db, q, o, C);
    return rc ? rc : run(db, C, o, mode, stream);
}

static int reloc_entry(drfe_kfdb* db, const drfe_kfdb_reloc_queries* q, drfe_kfdb_out* o, int mode, void* stream)
{
    if (!db) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    Call C;
    const int rc = plan_reloc(db, q, o, C);
    return rc ? rc : run(db, C, o, mode, stream);
}

int drfe_kfdb_loop_queries_host(drfe_kfdb* db, const drfe_kfdb_loop_queries* q, drfe_kfdb_out* o) { return loop_entry(db, q, o, 0, nullptr); }
int drfe_kfdb_loop_queries_device(drfe_kfdb* db, const drfe_kfdb_loop_queries* q, drfe_kfdb_out* o, void* stream) { return loop_entry(db, q, o, 1, stream); }
int drfe_kfdb_loop_queries_batch(drfe_kfdb* db, const drfe_kfdb_loop_queries* q, drfe_kfdb_out* o, void* stream) { return loop_entry(db, q, o, 2, stream); }
int drfe_kfdb_reloc_queries_host(drfe_kfdb* db, const drfe_kfdb_reloc_queries* q, drfe_kfdb_out* o) { return reloc_entry(db, q, o, 0, nullptr); }
int drfe_kfdb_reloc_queries_device(drfe_kfdb* db, const drfe_kfdb_reloc_queries* q, drfe_kfdb_out* o, void* stream) { return reloc_entry(db, q, o, 1, stream); }
int drfe_kfdb_reloc_queries_batch(drfe_kfdb* db, const drfe_kfdb_reloc_queries* q, drfe_kfdb_out* o, void* stream) { return reloc_entry(db, q, o, 2, stream); }

int drfe_kfdb_score(int32_t na, const int32_t* ia, const double* va, int32_t nb, const int32_t* ib, const double* vb, float* score)
{
    if (na < 0 || nb < 0 || !score || (na > 0 && (!ia || !va)) || (nb > 0 && (!ib || !vb))) return DRFE_ERR_INVALID;
    if (!ascending(ia, na) || !ascending(ib, nb)) return DRFE_ERR_INVALID;
    int32_t c, f;
    double sum;
    kfdb_walk(ia, va, na, ib, vb, nb, &c, &f, &sum);
    *score = kfdb_score(sum);
    return DRFE_OK;
}

int drfe_kfdb_stats(drfe_kfdb* db, int64_t* stats)
{
    if (!db || !stats) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    std::memcpy(stats, db->stats, sizeof(db->stats));
    return DRFE_OK;
}

}  // extern "C"
