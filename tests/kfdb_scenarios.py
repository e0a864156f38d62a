"""Scripts for the KeyFrameDatabase tests: a script is a list of operations that tests/kfdb_numpy.py's Database and
dr_slam_amd.lib.KeyFrameDatabase both understand; play() runs one and returns the results of its query operations.

Hand-built scripts carry the candidate lists worked out by hand (the arithmetic is in each builder's docstring: all values are
powers of two, and for positive values a common word adds min(vi, wi) to the score)."""
import numpy as np

Q4 = ([1, 2, 3, 4], [0.25] * 4)


def play(ops, db, **kw):
    out = []
    for op in ops:
        name = op[0]
        if name == "put":
            db.put(op[1], op[2], op[3])
        elif name in ("add", "erase", "remove"):
            getattr(db, name)(op[1])
        elif name == "clear":
            db.clear()
        elif name == "nbr":
            db.set_neighbours(op[1], op[2])
        elif name == "loop":
            out.append(db.loop_queries(op[1], **kw))
        elif name == "reloc":
            out.append(db.reloc_queries(op[1], **kw))
        else:
            raise ValueError(name)
    return out


def _kf(h, vals, ids=(1, 2, 3, 4)):
    return ("put", h, list(ids), list(vals))


def same_first_word():
    """10 and 11 are equal to the query (score 1): both kept, in the order of their latest add"""
    ops = [_kf(10, Q4[1]), _kf(11, Q4[1]), _kf(1, Q4[1]), ("add", 10), ("add", 11),
           ("loop", [dict(handle=1, id=1, min_score=0.0)]),
           ("erase", 10), ("add", 10),
           ("loop", [dict(handle=1, id=2, min_score=0.0)])]
    return ops, [[[10, 11]], [[11, 10]]]


def truncation(M):
    """the query has M words of 0.125; key frame 100 + c shares c of them (score 0.125 c).  (int)(M * 0.8f) is 4, 4 and 8 for
    M = 5, 6, 10: key frames with c > that are scored.  M = 5: only c = 5 (c = 4 has 0.5 > 0.75 * 0.625 and would be returned if
    scored).  M = 6: c = 5, 6 (0.625 > 0.75 * 0.75).  M = 10: c = 9, 10 (c = 8 has 1.0 > 0.75 * 1.25 and would be returned)."""
    words = list(range(1, M + 1))
    ops = [("put", 1, words, [0.125] * M)]
    for c in range(M, max(M - 4, 0), -1):
        ops += [("put", 100 + c, words[:c], [0.125] * c), ("add", 100 + c)]
    ops.append(("loop", [dict(handle=1, id=7, min_score=0.0)]))
    expect = {5: [105], 6: [106, 105], 10: [110, 109]}[M]
    scored = {5: 1, 6: 2, 10: 2}[M]
    return ops, [[expect]], scored


def score_equals_min_score(min_score):
    """key frame 10 scores exactly 1.0f; 11 shares one word of two (1 > (int)1.6 fails: not scored)"""
    ops = [("put", 1, [1, 2], [0.5, 0.5]), ("put", 10, [1, 2], [0.5, 0.5]), ("put", 11, [1, 3], [0.5, 0.5]), ("add", 10), ("add", 11),
           ("loop", [dict(handle=1, id=3, min_score=min_score)])]
    return ops


def acc_equals_retain():
    """scores: 10 -> 1.0, 11 -> 0.75 (= 0.75f * 1.0: strict >, dropped), 12 -> 0.875"""
    ops = [_kf(1, Q4[1]), _kf(10, Q4[1]), _kf(11, [0.25, 0.25, 0.125, 0.125]), _kf(12, [0.25, 0.25, 0.25, 0.125]),
           ("add", 10), ("add", 11), ("add", 12), ("loop", [dict(handle=1, id=5, min_score=0.0)])]
    return ops, [[[10, 12]]]


def same_best_neighbour():
    """10 and 11 score 0.5, their neighbour 12 scores 1.0: both reach 1.5 and elect 12; 12 itself stays at 1.0 < 0.75 * 1.5"""
    ops = [_kf(1, Q4[1]), _kf(10, [0.125] * 4), _kf(11, [0.125] * 4), _kf(12, Q4[1]), ("add", 10), ("add", 11), ("add", 12),
           ("nbr", [10, 11], [[12], [12]]), ("loop", [dict(handle=1, id=5, min_score=0.0)])]
    return ops, [[[12]]]


def connected_best(connected):
    """12 scores 1.0 and is 10's neighbour (10 scores 0.5).  Connected to the query it is neither listed nor a neighbour: [10].
    Not connected: 10 reaches 1.5 and elects 12, 12 stays at 1.0 < 1.125: [12]."""
    ops = [_kf(1, Q4[1]), _kf(10, [0.125] * 4), _kf(12, Q4[1]), ("add", 10), ("add", 12), ("nbr", [10], [[12]]),
           ("loop", [dict(handle=1, id=5, min_score=0.0, connected=[12] if connected else [])])]
    return ops, [[[10] if connected else [12]]]


RELOC_S = (90, [4, 50, 51, 52], [0.25] * 4)            # scores S (key frame 20) with 1.0, shares one word with key frame 10
RELOC_A = (91, [1, 2, 3, 4], [0.125] * 4)              # scores key frame 10 with 0.5, shares one word with S


def reloc_stale(how):
    """key frame 10 = {1,2,3,4}, its neighbour 20 = {4,50,51,52}.  Query A scores 10 with 0.5; 20 shares word 4 only (not scored) and
    adds whatever mRelocScore holds: nothing yet (0.0f, one uninitialised read, [10]), or the 1.0 query S left (10 reaches 1.5 and
    elects 20: [20]) in the same call or in an earlier one."""
    ops = [_kf(10, Q4[1]), ("put", 20, RELOC_S[1], RELOC_S[2]), ("add", 10), ("add", 20), ("nbr", [10], [[20]])]
    if how == "none":
        ops.append(("reloc", [RELOC_A]))
        return ops, [[[10]]], [[1]]
    if how == "same_call":
        ops.append(("reloc", [RELOC_S, RELOC_A]))
        return ops, [[[20], [20]]], [[0, 0]]
    ops += [("reloc", [RELOC_S]), ("reloc", [RELOC_A])]
    return ops, [[[20]], [[20]]], [[0], [0]]


def no_shared_word():
    ops = [_kf(1, Q4[1], ids=(70, 71, 72, 73)), _kf(10, Q4[1]), ("add", 10), ("loop", [dict(handle=1, id=5, min_score=0.0)]),
           ("reloc", [(5, [70, 71], [0.5, 0.5])])]
    return ops, [[[]], [[]]]


def below_min_score():
    ops = [_kf(1, Q4[1]), _kf(10, Q4[1]), ("add", 10), ("loop", [dict(handle=1, id=5, min_score=2.0)])]
    return ops, [[[]]]


def add_after_queue():
    """9 (score 0.5) is in the database; 1, 2, 3 equal each other and go through one call with add_after: the first sees 9, the second
    9 and 1 (1.0; 9 falls below 0.75), the third 9, 1 and 2"""
    ops = [_kf(9, [0.125] * 4), ("add", 9), _kf(1, Q4[1]), _kf(2, Q4[1]), _kf(3, Q4[1]),
           ("loop", [dict(handle=h, id=h, min_score=0.0, add_after=True) for h in (1, 2, 3)])]
    return ops, [[[9], [1], [1, 2]]]


def covisible_min_score():
    """covisible 30 (in the database, 0.75) and 31 (put only, 0.5): minScore 0.5.  10 scores 0.5 (kept at equality), 11 scores 0.375;
    30 is connected.  Without 31 minScore would be 0.75 and nothing would be kept."""
    ops = [_kf(1, Q4[1]), _kf(30, [0.25, 0.25, 0.125, 0.125]), _kf(31, [0.125] * 4), _kf(10, [0.125] * 4),
           _kf(11, [0.125, 0.125, 0.0625, 0.0625]), ("add", 30), ("add", 10), ("add", 11),
           ("loop", [dict(handle=1, id=5, connected=[30], covisible=[30, 31])])]
    return ops, [[[10]]], np.float32(0.5)


def random_script(seed, n_kf=300, n_words=1000):
    """A walk over 24 places that keeps coming back: a place is a fixed vector of 5 to 57 words in an 80-word window that overlaps
    the next place's; a key frame (or a lost frame) seen there keeps about nine words in ten, adds up to three and jitters the
    weights, L1-normalised, so key frames of one place overlap heavily and score alike.  Each key frame is put, queried as
    DetectLoop does (covisible = connected = the last few key frames, some still waiting for their add), added a little later,
    sometimes erased, re-added or removed; relocalisation calls of 1 to 6 frames come in between.  Most key frames have no
    covisibility neighbours (those that have any dominate the accumulated score, and a query would return one candidate)."""
    rng = np.random.RandomState(seed)
    ops, stored, visible, waiting = [], [], [], []
    next_reloc = [1]

    n_places = 24
    places = []
    for p in range(n_places):
        lo = p * 38
        ids = np.sort(rng.choice(np.arange(lo, lo + 80), size=rng.randint(5, 58), replace=False))
        places.append((lo, ids, rng.rand(len(ids)) + 0.2))

    def vector(p):
        lo, ids, w = places[p]
        keep = rng.rand(len(ids)) < 0.9
        keep[rng.randint(len(ids))] = True
        extra = rng.choice(np.arange(lo, lo + 80), size=rng.randint(0, 4), replace=False)
        extra = np.array([e for e in extra if e not in ids], np.int64)
        allw = np.concatenate([w[keep] * (1.0 + 0.2 * rng.rand(int(keep.sum()))), 0.2 + rng.rand(len(extra))])
        alli = np.concatenate([ids[keep], extra])
        order = np.argsort(alli)
        allw = allw[order] / allw.sum()
        return [int(i) for i in alli[order]], [float(x) for x in allw]

    def centre(i):
        return int(round((n_places - 1) * (0.5 + 0.5 * np.sin(i * 0.045)) + rng.randint(-1, 2))) % n_places

    def reloc_call():
        qs = []
        for _ in range(rng.randint(1, 7)):
            c = n_words - 10 if rng.rand() < 0.04 else centre(rng.randint(0, max(1, len(stored))) if stored else 0)
            ids, vals = ([n_words - 5, n_words - 3], [0.5, 0.5]) if c == n_words - 10 else vector(c)
            qs.append((next_reloc[0], ids, vals))
            next_reloc[0] += rng.randint(1, 4)
        ops.append(("reloc", qs))

    for i in range(n_kf):
        h = i + 1
        ids, vals = vector(centre(i))
        ops.append(("put", h, ids, vals))
        recent = [x for x in stored[-rng.randint(1, 6):]]
        stored.append(h)
        pool = stored[:-1]
        if pool:
            cand = [pool[j] for j in rng.choice(len(pool), size=min(len(pool), rng.randint(1, 11) if rng.rand() < 0.15 else 0), replace=False)]
            near = sorted(cand, key=lambda x: abs(x - h))
            ops.append(("nbr", [h], [near]))
            if rng.rand() < 0.05:
                o = pool[rng.randint(len(pool))]
                ops.append(("nbr", [o], [[pool[j] for j in rng.choice(len(pool), size=min(len(pool), 10), replace=False)]]))
        q = dict(handle=h, id=h, connected=recent)
        if rng.rand() < 0.7:
            q["covisible"] = recent
        else:
            q["min_score"] = float(np.float32(rng.rand() * 0.2))
        q["add_after"] = bool(rng.rand() < 0.5)
        ops.append(("loop", [q]))
        if q["add_after"]:
            visible.append(h)
        else:
            waiting.append(h)
        if waiting and rng.rand() < 0.6:
            w = waiting.pop(0)
            ops.append(("add", w))
            visible.append(w)
        r = rng.rand()
        if r < 0.08 and len(visible) > 5:
            v = visible.pop(rng.randint(len(visible) - 3))
            ops.append(("erase", v))
            if rng.rand() < 0.5:
                ops.append(("add", v))
                visible.append(v)
            elif rng.rand() < 0.5 and v not in recent:
                ops.append(("remove", v))
                stored.remove(v)
        if rng.rand() < 0.35:
            reloc_call()
    return ops


def sized_script(n_visible, n_queries, seed, long_vectors=False):
    """n_visible key frames in the inverted file (plus three that are only stored), then a loop call and two relocalisation calls of
    n_queries queries each.  Eight places, so that every query meets many key frames; every fourth key frame has neighbours; key
    frame 2 has a single word; with long_vectors one stored vector and one query vector have 3000 words."""
    rng = np.random.RandomState(seed)
    base = [np.sort(rng.choice(np.arange(p * 30, p * 30 + 60), size=rng.randint(8, 40), replace=False)) for p in range(8)]

    def vector(p):
        ids = base[p][rng.rand(len(base[p])) < 0.9]
        if len(ids) == 0:
            ids = base[p][:1]
        w = rng.rand(len(ids)) + 0.5
        return [int(i) for i in ids], [float(x) for x in w / w.sum()]

    ops, handles = [], []
    for i in range(n_visible + 3):
        h = 1000 + i
        ids, vals = vector(i % 8)
        if i == 2:
            ids, vals = [int(base[2][0])], [1.0]
        if long_vectors and i == 1:
            ids = list(range(5, 3005))
            vals = [1.0 / 3000] * 3000
        ops.append(("put", h, ids, vals))
        handles.append(h)
    rows = [[handles[j] for j in rng.choice(len(handles), size=min(len(handles), rng.randint(1, 11)), replace=False)]
            for _ in handles[::4]]
    ops.append(("nbr", handles[::4], rows))
    ops += [("add", h) for h in handles[:n_visible]]
    queue = []
    for k in range(n_queries):
        h = 5000 + k
        ids, vals = vector(k % 8)
        if long_vectors and k == 0:
            ids = list(range(0, 6000, 2))
            vals = [1.0 / 3000] * 3000
        ops.append(("put", h, ids, vals))
        conn = [handles[j] for j in rng.choice(len(handles), size=min(len(handles), 3), replace=False)]
        queue.append(dict(handle=h, id=h, connected=conn, covisible=conn + queue_handles(queue)[-2:], add_after=bool(k % 3 != 1)))
    ops.append(("loop", queue))
    for call in range(2):
        qs = []
        for k in range(n_queries):
            ids, vals = vector((k + call) % 8)
            if long_vectors and k == 0 and call == 0:
                ids = list(range(1, 6001, 2))
                vals = [1.0 / 3000] * 3000
            qs.append((1 + call * n_queries + k, ids, vals))
        ops.append(("reloc", qs))
    return ops


def queue_handles(queue):
    return [q["handle"] for q in queue]
