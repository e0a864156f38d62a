"""KeyFrameDatabase restated on its own (reference src/KeyFrameDatabase.cc:40-309, DBoW2 ScoringObject.cpp:23-68, the minScore loop
of src/LoopClosing.cc:137-151): one Python list of key frames per word, walked as the reference walks its std::lists, mutable
mnLoopQuery / mnLoopWords / mLoopScore / mnReloc* fields per key frame, np.float32 / np.float64 where the reference has float /
double, queries strictly one by one.  It shares nothing with dr_slam_amd/csrc/kfdb_core.h: in particular the order of the listed
key frames comes from the walk, not from the (smallest shared word, sequence number) pair the library sorts by."""
import numpy as np

COUNTERS = ("connected_met", "below_min_score", "neighbour_added", "best_replaced", "duplicate_dropped", "stale_read",
            "uninit_read", "empty_loop_no_shared", "empty_loop_none_kept", "empty_reloc_no_shared")

F32 = np.float32
F64 = np.float64


def l1_score(v1, v2):
    """L1Scoring::score over two BowVectors (dicts word -> float64 walked in ascending word id), then TemplatedVocabulary::score's
    return narrowed to the float the callers store it in"""
    k1, k2 = sorted(v1), sorted(v2)
    i = j = 0
    score = F64(0.0)
    while i < len(k1) and j < len(k2):
        if k1[i] == k2[j]:
            vi, wi = F64(v1[k1[i]]), F64(v2[k2[j]])
            score = score + (np.abs(vi - wi) - np.abs(vi) - np.abs(wi))
            i += 1
            j += 1
        elif k1[i] < k2[j]:
            while i < len(k1) and k1[i] < k2[j]:       # lower_bound
                i += 1
        else:
            while j < len(k2) and k2[j] < k1[i]:
                j += 1
    score = -score / F64(2.0)
    return F32(score)


class KF:
    def __init__(self, handle, bow):
        self.handle = handle
        self.bow = dict(bow)
        self.neighbours = []                 # GetBestCovisibilityKeyFrames(10), key frames
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = F32(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = None              # never initialised by the reference's constructors


class Database:
    def __init__(self):
        self.inverted = {}                   # word -> list of KF, mvInvertedFile
        self.kfs = {}
        self.counters = dict.fromkeys(COUNTERS, 0)

    def put(self, handle, ids, vals):
        self.kfs[handle] = KF(handle, zip([int(i) for i in ids], [F64(v) for v in vals]))

    def add(self, handle):
        kf = self.kfs[handle]
        for w in sorted(kf.bow):
            self.inverted.setdefault(w, []).append(kf)

    def erase(self, handle):
        kf = self.kfs[handle]
        for w in sorted(kf.bow):
            lst = self.inverted.get(w, [])
            for i, k in enumerate(lst):
                if k is kf:
                    del lst[i]
                    break

    def clear(self):
        self.inverted = {}

    def remove(self, handle):
        self.erase(handle)
        del self.kfs[handle]

    def set_neighbours(self, handles, nbr):
        for h, row in zip(handles, nbr):
            self.kfs[h].neighbours = [int(x) for x in row if int(x) >= 0][:10]

    def _neighbours(self, kf):
        return [self.kfs[h] for h in kf.neighbours if h in self.kfs]

    def min_score(self, handle, covisible):
        cur = self.kfs[handle].bow
        m = F32(1)
        for h in covisible:
            s = l1_score(cur, self.kfs[h].bow)
            if s < m:
                m = s
        return m

    def detect_loop(self, handle, qid, connected, min_score):
        """-> (candidate handles, (listed, scored, kept, maxCommonWords))"""
        c = self.counters
        pKF = self.kfs[handle]
        connected = set(connected)
        min_score = F32(min_score)
        sharing = []
        for w in sorted(pKF.bow):
            for kfi in self.inverted.get(w, []):
                if kfi.mnLoopQuery != qid:
                    kfi.mnLoopWords = 0
                    if kfi.handle not in connected:
                        kfi.mnLoopQuery = qid
                        sharing.append(kfi)
                    else:
                        c["connected_met"] += 1
                kfi.mnLoopWords += 1
        if not sharing:
            c["empty_loop_no_shared"] += 1
            return [], (0, 0, 0, 0)
        max_common = 0
        for kfi in sharing:
            if kfi.mnLoopWords > max_common:
                max_common = kfi.mnLoopWords
        min_common = int(F32(max_common) * F32(0.8))
        score_and_match = []
        nscores = 0
        for kfi in sharing:
            if kfi.mnLoopWords > min_common:
                nscores += 1
                si = l1_score(pKF.bow, kfi.bow)
                kfi.mLoopScore = si
                if si >= min_score:
                    score_and_match.append((si, kfi))
                else:
                    c["below_min_score"] += 1
        rec = (len(sharing), nscores, len(score_and_match), max_common)
        if not score_and_match:
            c["empty_loop_none_kept"] += 1
            return [], rec
        acc_and_match = []
        best_acc = min_score
        for si, kfi in score_and_match:
            best_score = si
            acc = si
            best = kfi
            for kf2 in self._neighbours(kfi):
                if kf2.mnLoopQuery == qid and kf2.mnLoopWords > min_common:
                    acc = F32(acc + kf2.mLoopScore)
                    c["neighbour_added"] += 1
                    if kf2.mLoopScore > best_score:
                        best = kf2
                        best_score = kf2.mLoopScore
                        c["best_replaced"] += 1
            acc_and_match.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc), rec

    def _retain(self, acc_and_match, best_acc):
        retain = F32(F32(0.75) * best_acc)
        out, seen = [], set()
        for acc, kf in acc_and_match:
            if acc > retain:
                if kf.handle not in seen:
                    out.append(kf.handle)
                    seen.add(kf.handle)
                else:
                    self.counters["duplicate_dropped"] += 1
        return out

    def detect_reloc(self, qid, ids, vals):
        """-> (candidate handles, record, reads of a never-written mRelocScore)"""
        c = self.counters
        bow = dict(zip([int(i) for i in ids], [F64(v) for v in vals]))
        sharing = []
        for w in sorted(bow):
            for kfi in self.inverted.get(w, []):
                if kfi.mnRelocQuery != qid:
                    kfi.mnRelocWords = 0
                    kfi.mnRelocQuery = qid
                    sharing.append(kfi)
                kfi.mnRelocWords += 1
        if not sharing:
            c["empty_reloc_no_shared"] += 1
            return [], (0, 0, 0, 0), 0
        max_common = 0
        for kfi in sharing:
            if kfi.mnRelocWords > max_common:
                max_common = kfi.mnRelocWords
        min_common = int(F32(max_common) * F32(0.8))
        score_and_match = []
        for kfi in sharing:
            if kfi.mnRelocWords > min_common:
                si = l1_score(bow, kfi.bow)
                kfi.mRelocScore = si
                score_and_match.append((si, kfi))
        rec = (len(sharing), len(score_and_match), len(score_and_match), max_common)
        acc_and_match = []
        best_acc = F32(0)
        uninit = 0
        for si, kfi in score_and_match:
            best_score = si
            acc = si
            best = kfi
            for kf2 in self._neighbours(kfi):
                if kf2.mnRelocQuery != qid:
                    continue
                if kf2.mnRelocWords <= min_common:
                    c["stale_read"] += 1
                s2 = kf2.mRelocScore
                if s2 is None:                       # the reference reads an uninitialised float here: 0.0f, counted
                    s2 = F32(0)
                    uninit += 1
                    c["uninit_read"] += 1
                acc = F32(acc + s2)
                c["neighbour_added"] += 1
                if s2 > best_score:
                    best = kf2
                    best_score = s2
                    c["best_replaced"] += 1
            acc_and_match.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc), rec, uninit

    # the batch forms of the library, one query after another
    def loop_queries(self, queries):
        cands, recs, mins = [], [], []
        for q in queries:
            ms = F32(q["min_score"]) if "min_score" in q else self.min_score(q["handle"], q.get("covisible", ()))
            cd, rec = self.detect_loop(q["handle"], q["id"], q.get("connected", ()), ms)
            cands.append(cd)
            recs.append(rec)
            mins.append(ms)
            if q.get("add_after"):
                self.add(q["handle"])
        return {"candidates": cands, "record": np.array(recs, np.int32).reshape(-1, 4), "min_score": np.array(mins, np.float32)}

    def reloc_queries(self, queries):
        cands, recs, un = [], [], []
        for qid, ids, vals in queries:
            cd, rec, u = self.detect_reloc(qid, ids, vals)
            cands.append(cd)
            recs.append(rec)
            un.append(u)
        return {"candidates": cands, "record": np.array(recs, np.int32).reshape(-1, 4), "uninit_reads": np.array(un, np.int32)}


def same(lib_result, np_result):
    """the library's result of a call against the restatement's: candidates in order, records, and minScore / uninit_reads by bytes"""
    assert [list(map(int, c)) for c in lib_result["candidates"]] == [list(c) for c in np_result["candidates"]]
    assert np.array_equal(lib_result["record"], np_result["record"])
    if "min_score" in np_result:
        assert lib_result["min_score"].tobytes() == np_result["min_score"].tobytes()
    if "uninit_reads" in np_result:
        assert np.array_equal(lib_result["uninit_reads"], np_result["uninit_reads"])
