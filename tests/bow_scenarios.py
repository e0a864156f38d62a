"""Hand-built vocabularies and frames that put the bag-of-words path on its decision points: the vocabulary descent
(TemplatedVocabulary::transform), ORBmatcher::SearchByBoW in both overloads and SearchForTriangulation.

Every scenario states its outcome by hand, with the reference line it exercises.  tests/test_bow_edges_cpu.py holds the
oracle and the numpy restatement (tests/bow_numpy.py) to these outcomes; tests/test_gpu_bow_edges.py holds the device to
all three.

Descriptor layout.  Bits 0..255 of a descriptor (np.packbits order).  Level l of a vocabulary owns a region of bits; a node
at level l is its parent's descriptor plus one bit in that region: the bit of its position among its siblings, or of an
explicit `code` (two siblings with one code are identical).  A feature sets bits per level.  At level l the distance from a
feature to a child is then a constant shared by all siblings plus |F_l xor {code}|: the nearest children are the ones whose
code the feature sets (distance ties: several set codes, or two siblings with one code), and with no matching code all
siblings tie.  Bits past the last region ("noise") add the same amount to every distance.  Vocabularies are written with
Vocabulary.to_text and read back, in DBoW2's creation order (HKmeansStep, TemplatedVocabulary.h:643-815: the children of a
node get consecutive ids, then each child's subtree is numbered before the next child's).
"""
from dataclasses import dataclass, field

import numpy as np

from dr_slam_amd import vocabulary as V

F32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
W, H, FX, FY, CX, CY = 640, 480, 256.0, 256.0, 320.0, 240.0
REF_DESCENT = "Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1216-1259"


# ----------------------------------------------------------------------------------------------------------------------
# vocabularies

class T:
    """Tree spec: T(child, child, ...) is an inner node, T(w=...) a leaf; `code` overrides the node's bit."""

    def __init__(self, *children, w=1.0, code=None):
        self.children, self.w, self.code = list(children), w, code


def leaves(n, w=1.0):
    return [T(w=w) for _ in range(n)]


@dataclass
class Tree:
    voc: V.Vocabulary
    text: str
    offsets: list          # bit offset of level l's region at index l - 1
    noise_at: int          # first bit past the regions
    path_id: dict          # path of sibling positions -> node id
    depth: np.ndarray      # per node


def build_tree(root, k, L, scoring=V.L1_NORM, weighting=V.TF_IDF):
    # widths of the level regions
    widths = [0] * L

    def scan(t, lvl):
        if t.children:
            widths[lvl] = max(widths[lvl], len(t.children), *[(c.code or 0) + 1 for c in t.children])
            for c in t.children:
                scan(c, lvl + 1)
    scan(root, 0)
    offsets = list(np.cumsum([0] + widths[:-1]))
    assert sum(widths) <= 256
    parent, leaf, weight, bits, depth = [0], [0], [0.0], [frozenset()], [0]
    path_id = {(): 0}

    def step(t, nid, path, lvl):             # HKmeansStep: create the children, then descend into each in turn
        ids = []
        for pos, c in enumerate(t.children):
            cid = len(parent)
            parent.append(nid)
            leaf.append(0 if c.children else 1)
            weight.append(0.0 if c.children else float(c.w))
            bits.append(bits[nid] | {offsets[lvl] + (pos if c.code is None else c.code)})
            depth.append(lvl + 1)
            path_id[path + (pos,)] = cid
            ids.append(cid)
        for pos, (c, cid) in enumerate(zip(t.children, ids)):
            if c.children:
                step(c, cid, path + (pos,), lvl + 1)
    step(root, 0, (), 0)
    n = len(parent)
    desc = np.zeros((n, 32), np.uint8)
    for i, b in enumerate(bits):
        desc[i] = _pack(b)
    voc = V.Vocabulary(k, L, scoring, weighting, np.array(parent, np.int32), np.array(leaf, np.uint8), desc,
                       np.array(weight, np.float64))
    text = voc.to_text()
    back = V.Vocabulary.from_text(text)
    assert np.array_equal(back.parent, voc.parent) and np.array_equal(back.desc, voc.desc)
    return Tree(back, text, offsets, int(sum(widths)), path_id, np.array(depth, np.int32))


def _pack(bitset):
    v = np.zeros(256, np.uint8)
    v[list(bitset)] = 1
    return np.packbits(v)


def feature(tree, levels, noise=0):
    """levels: {level: [codes set at that level]}; noise: bits past the regions."""
    b = set()
    for lvl, codes in levels.items():
        b |= {tree.offsets[lvl - 1] + c for c in codes}
    b |= set(range(tree.noise_at, tree.noise_at + noise))
    assert max(b, default=0) < 256
    return _pack(b)


@dataclass
class DescentScenario:
    name: str
    ref: str
    tree: Tree
    levelsups: list
    desc: np.ndarray       # [n, 32]
    paths: list            # expected leaf per feature, as sibling positions from the root (stated by hand)
    why: list

    def expected(self, levelsup):
        """(word, weight, nid) per feature; nid None where the reference leaves it unset (a leaf above m_L - levelsup:
        `NodeId nid;` is never written) - the product's stated choice there is 0."""
        voc, t = self.tree.voc, self.tree
        word_of = np.full(voc.n_nodes, -1, np.int32)
        word_of[np.flatnonzero(voc.is_leaf)] = np.arange(int(voc.is_leaf.sum()))
        nid_level = voc.L - levelsup
        word, weight, nid = [], [], []
        for p in self.paths:
            leaf = t.path_id[tuple(p)]
            word.append(word_of[leaf])
            weight.append(voc.weight[leaf])
            if nid_level <= 0:
                nid.append(0)                                  # :1233 `if(nid_level <= 0 && nid != NULL) *nid = 0;`
            elif len(p) >= nid_level:
                nid.append(t.path_id[tuple(p[:nid_level])])    # :1252
            else:
                nid.append(None)
        return np.array(word, np.int32), np.array(weight, np.float64), nid


def unbalanced_tree():
    """k = 10, L = 6; 1, 2, 3, 10 and 20 children per node, leaves at depths 1..6, stopped leaves, and under the last root
    child two identical leaves (positions 3 and 9, the last) for a tie at distance 0."""
    c = T(*leaves(1), T(*leaves(2, 0.75), T(w=0.0)), T(*leaves(1)))          # depth 4: three children, leaves at 5 and 6
    b = T(*[T(w=0.5 + 0.1 * i) for i in range(9)], c)                        # depth 3: 10 children, the last internal
    a = T(b, T(w=2.5))                                                       # depth 2: 2 children (subtree, leaf at depth 3)
    root = T(T(w=1.5),                                                       # 0: leaf at depth 1
             T(T(w=1.25)),                                                   # 1: a single child
             T(*[T(w=0.0 if i == 5 else 1.0 + 0.05 * i) for i in range(20)]),   # 2: 20 children, position 5 stopped
             T(a),                                                           # 3: single child down to depth 6
             T(T(w=3.0), T(w=0.0)),                                          # 4: a live and a stopped leaf
             T(w=4.0), T(w=4.5), T(w=5.0), T(w=5.5),                         # 5..8: leaves at depth 1
             T(*[T(w=6.0 + 0.1 * i, code=3 if i == 9 else None) for i in range(10)]))   # 9: leaf 9 coded like leaf 3
    return build_tree(root, 10, 6)


def descent_scenarios():
    out = []
    t = unbalanced_tree()
    rows = [  # (levels, noise, expected path, why)
        ({1: [0]}, 0, (0,), "leaf at depth 1"),
        ({1: [2], 2: [19]}, 0, (2, 19), "the 20th child"),
        ({1: [2], 2: [7, 13]}, 0, (2, 7), "tie at distance 1 between non-adjacent children 7 and 13: the first"),
        ({1: [3], 2: [0], 3: [0], 4: [9], 5: [1], 6: [1]}, 0, (3, 0, 0, 9, 1, 1), "leaf at depth 6"),
        ({1: [3, 9]}, 0, (3, 0, 0, 0), "tie with the last root child; then all siblings tie at every level: first each time"),
        ({}, 9, (0,), "every distance equal (9 + 1): the first child"),
        ({1: [2], 2: [5]}, 0, (2, 5), "stopped leaf (weight 0)"),
        ({1: [3], 2: [0], 3: [1]}, 0, (3, 0, 1), "leaf at depth 3"),
        ({1: [9], 2: [9]}, 20, (9, 0), "code 9 is nobody's under node 9 (leaf 9 carries code 3): all tie, the first"),
        ({1: [3], 3: [0], 4: [9], 5: [0]}, 0, (3, 0, 0, 9, 0), "leaf at depth 5 (no level-2 bit: a single child)"),
        ({1: [3], 3: [0], 4: [9], 5: [2]}, 0, (3, 0, 0, 9, 2, 0), "a single child at depth 6"),
        ({1: [4], 2: [1]}, 0, (4, 1), "stopped leaf beside a live one"),
        ({1: [3], 3: [0], 4: [0, 9]}, 0, (3, 0, 0, 0), "tie between a leaf (position 0) and the last, inner child"),
        ({1: [9], 2: [3]}, 0, (9, 3), "tie at distance 0 between leaf 3 and the last leaf (same code): the first"),
        ({1: [9], 2: [3]}, 17, (9, 3), "the same tie at distance 17"),
        ({1: [1], 2: [0]}, 5, (1, 0), "a chain link"),
    ]
    out.append(DescentScenario("unbalanced", REF_DESCENT + ", :643-815, :1365-1424", t, [0, 4, 6, 7],
                               np.stack([feature(t, lv, nz) for lv, nz, _, _ in rows]), [p for _, _, p, _ in rows],
                               [w for *_, w in rows]))
    t = build_tree(T(*[T(w=1.0 + i) for i in range(32)]), 20, 1)
    rows = [({1: [31]}, 0, (31,), "lane 31 is the nearest"), ({1: [30, 31]}, 3, (30,), "tie 30 / 31"),
            ({1: [5, 31]}, 0, (5,), "tie 5 / 31: the first"), ({}, 0, (0,), "all tie"), ({1: [16]}, 0, (16,), "lane 16")]
    out.append(DescentScenario("wide32", REF_DESCENT, t, [0, 1], np.stack([feature(t, lv, nz) for lv, nz, _, _ in rows]),
                               [p for _, _, p, _ in rows], [w for *_, w in rows]))
    chain = T(w=7.0)
    for _ in range(9):
        chain = T(chain)
    t = build_tree(T(chain, T(w=0.25)), 10, 10)
    rows = [({1: [0]}, 0, (0,) * 10, "down the chain to depth 10"), ({1: [1]}, 4, (1,), "the leaf at depth 1"),
            ({}, 0, (0,) * 10, "tie at the root: the chain")]
    out.append(DescentScenario("chain10", REF_DESCENT, t, [0, 4, 9, 10, 11],
                               np.stack([feature(t, lv, nz) for lv, nz, _, _ in rows]), [p for _, _, p, _ in rows],
                               [w for *_, w in rows]))
    return out


def wide33_tree():
    """33 children under the root: DBoW2 loads it, the device rejects it at upload (32 lanes per descent step)."""
    return build_tree(T(*[T(w=1.0) for _ in range(33)]), 20, 1)


def leaf_flag_mismatch():
    """(parent, is_leaf) pairs a DBoW2 file never holds: an internal flag without children (the reference would give it
    word_id 0 from Node()'s initialiser), and a leaf flag on a node with children."""
    t = build_tree(T(T(w=1.0), T(T(w=1.0), T(w=2.0))), 10, 2)
    v = t.voc
    inner_childless = V.Vocabulary(v.k, v.L, v.scoring, v.weighting, v.parent, v.is_leaf.copy(), v.desc, v.weight)
    inner_childless.is_leaf[1] = 0
    leaf_with_children = V.Vocabulary(v.k, v.L, v.scoring, v.weighting, v.parent, v.is_leaf.copy(), v.desc, v.weight)
    leaf_with_children.is_leaf[2] = 1
    return v, inner_childless, leaf_with_children


# ----------------------------------------------------------------------------------------------------------------------
# matchers: a flat vocabulary of 20 groups, each with a live and a stopped leaf; levelsup 1 puts the FeatureVector at the
# groups.  Features carry their group and leaf bits plus a 192-bit payload (bits 64..255) that no node has: the distance
# between two features of one leaf is the Hamming distance of their payloads.

GROUPS = 20
PAYLOAD_AT = 64
MATCH_LEVELSUP = 1


def matcher_tree():
    return build_tree(T(*[T(T(w=1.0 + 0.5 * g), T(w=0.0)) for g in range(GROUPS)]), 20, 2)


class Payloads:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def base(self):
        return self.rng.integers(0, 2, 192, dtype=np.uint8)

    @staticmethod
    def flip(p, n, at=0):
        assert at + n <= 192
        q = p.copy()
        q[at:at + n] ^= 1
        return q


def fdesc(tree, group, payload, stopped=False):
    b = {tree.offsets[0] + group, tree.offsets[1] + (1 if stopped else 0)}
    b |= {PAYLOAD_AT + i for i in np.flatnonzero(payload)}
    return _pack(b)


@dataclass
class Side:
    desc: list = field(default_factory=list)
    angle: list = field(default_factory=list)
    mp: list = field(default_factory=list)
    x: list = field(default_factory=list)
    y: list = field(default_factory=list)
    octave: list = field(default_factory=list)
    u_right: list = field(default_factory=list)
    default_mp: int = 1    # SearchByBoW wants map points (>= 0) on the keyframe side, SearchForTriangulation none (-1)

    def add(self, tree, group, payload, angle=10.0, mp=None, stopped=False, x=None, y=None, octave=0, u_right=-1.0):
        i = len(self.desc)
        mp = self.default_mp if mp is None else mp
        self.desc.append(fdesc(tree, group, payload, stopped))
        self.angle.append(angle)
        self.mp.append(mp)
        self.x.append(20.0 + 10 * (i % 60) if x is None else x)
        self.y.append(20.0 + 10 * (i // 60) if y is None else y)
        self.octave.append(octave)
        self.u_right.append(u_right)
        return i

    def arrays(self):
        n = len(self.desc)
        k = np.zeros(n, KP_DTYPE)
        k["x"], k["y"], k["angle"], k["octave"] = self.x, self.y, self.angle, self.octave
        k["size"], k["response"], k["class_id"] = 31.0, 1.0, -1
        return (k, np.stack(self.desc).astype(np.uint8), np.array(self.mp, np.int32), np.array(self.u_right, np.float32))


@dataclass
class MatchScenario:
    """expected[overload][check_ori] = {F (KF2) keypoint: KF (KF1) keypoint}; overload 'frame' = SearchByBoW(pKF, F),
    'kf' = SearchByBoW(pKF1, pKF2) (both sides need a map point, `< TH_LOW`, vbMatched2)."""
    name: str
    ref: str
    kf: Side
    f: Side
    nnratio: float
    expected: dict

    def expected_array(self, overload, check_ori):
        m = np.full(len(self.f.desc), -1, np.int32)
        for i_f, i_kf in self.expected[overload][check_ori].items():
            m[i_f] = i_kf
        return len(self.expected[overload][check_ori]), m


REF_BOW = "src/ORBmatcher.cc:190-262 (frame), :556-628 (keyframes)"


def _same(d):
    return {False: d, True: d}


def match_scenarios():
    tree = matcher_tree()
    P = Payloads(7)
    out = []

    def scen(name, ref, kf, f, nnratio, frame, kfo=None):
        out.append(MatchScenario(name, ref, kf, f, nnratio, {"frame": frame, "kf": frame if kfo is None else kfo}))

    # best in the third chunk, second best in the first: 20 < 0.9 * 25
    kf, f, B = Side(), Side(), P.base()
    kf.add(tree, 0, B)
    for i in range(200):
        f.add(tree, 0, P.flip(B, 90) if i not in (10, 130) else P.flip(B, 25 if i == 10 else 20, 100))
    scen("chunks200_best_late", REF_BOW + ": best and second best across 64-lane chunks", kf, f, 0.9, _same({130: 0}))

    # second best in the last chunk fails the ratio: 20 < 0.75 * 25 is false
    kf, f, B = Side(), Side(), P.base()
    kf.add(tree, 1, B)
    for i in range(200):
        f.add(tree, 1, P.flip(B, 90) if i not in (10, 199) else P.flip(B, 20 if i == 10 else 25, 100))
    scen("chunks200_second_late", REF_BOW + ": bestDist2 from a later chunk", kf, f, 0.75, _same({}))

    # groups of 1, 63, 64, 65 on the F side: best (20) at the last position, second (30) at position 0; the lone candidate
    # at distance 50 passes `<= TH_LOW` (frame) but not `< TH_LOW` (keyframes)
    kf, f = Side(), Side()
    want, want_kf = {}, {}
    for g, n in ((2, 63), (3, 64), (4, 65)):
        B = P.base()
        q = kf.add(tree, g, B)
        for i in range(n):
            j = f.add(tree, g, P.flip(B, 20 if i == n - 1 else (30 if i == 0 else 80), 50))
            if i == n - 1:
                want[j] = want_kf[j] = q
    B = P.base()
    q = kf.add(tree, 5, B)
    want[f.add(tree, 5, P.flip(B, 50))] = q
    scen("groups_1_63_64_65", REF_BOW + ": wavefront chunk edges, bestDist2 = 256", kf, f, 0.75, _same(want), _same(want_kf))

    # 200 keyframe features in one node, the first 130 without a map point: #130 claims the best, #131 the lone rest
    kf, f, B = Side(), Side(), P.base()
    for i in range(200):
        kf.add(tree, 6, B, mp=1 if i >= 130 else -1)
    f.add(tree, 6, P.flip(B, 10))
    f.add(tree, 6, P.flip(B, 40, 20))
    scen("kf_group200_claims", REF_BOW + ": `if(!pMP) continue;`, claims", kf, f, 0.75, _same({0: 130, 1: 131}))

    # equal distances across chunks (nnratio 1.5 lets a tie through): the first position wins, the second query takes the other
    kf, f, B = Side(), Side(), P.base()
    kf.add(tree, 7, B)
    kf.add(tree, 7, B)
    for i in range(100):
        f.add(tree, 7, P.flip(B, 20, 30 if i == 5 else 60) if i in (5, 70) else P.flip(B, 90))
    scen("equal_across_chunks", REF_BOW + ": strict `dist < bestDist1` keeps the first", kf, f, 1.5, _same({5: 0, 70: 1}))

    # TH_LOW: lone candidates at 49, 50, 51
    kf, f = Side(), Side()
    frame, kfo = {}, {}
    for g, d in ((8, 49), (9, 50), (10, 51)):
        B = P.base()
        q = kf.add(tree, g, B)
        j = f.add(tree, g, P.flip(B, d))
        if d <= 50:
            frame[j] = q
        if d < 50:
            kfo[j] = q
    scen("th_low_49_50_51", "src/ORBmatcher.cc:230 `bestDist1<=TH_LOW`, :606 `bestDist1<TH_LOW`", kf, f, 0.75, _same(frame),
         _same(kfo))

    # the ratio test at equality: 30 < 0.75f * 40 = 30 is false; 29 / 40 and 30 / 41 pass
    kf, f = Side(), Side()
    want = {}
    for g, (d1, d2) in ((11, (30, 40)), (12, (29, 40)), (13, (30, 41))):
        B = P.base()
        q = kf.add(tree, g, B)
        j = f.add(tree, g, P.flip(B, d1))
        f.add(tree, g, P.flip(B, d2, 60))
        if d1 < 0.75 * d2:
            want[j] = q
    scen("ratio_equality", "src/ORBmatcher.cc:232 `static_cast<float>(bestDist1)<mfNNratio*static_cast<float>(bestDist2)`",
         kf, f, 0.75, _same(want))

    # a claim chain inside one node, with a keyframe keypoint without a map point in the middle
    kf, f, B = Side(), Side(), P.base()
    for mp in (1, -1, 1, 1, 1):
        kf.add(tree, 14, B, mp=mp)
    for d, at in ((10, 0), (20, 30), (26, 60), (40, 100)):
        f.add(tree, 14, P.flip(B, d, at))
    scen("claim_chain", REF_BOW + ": `if(vpMapPointMatches[realIdxF]) continue;` / vbMatched2", kf, f, 0.8,
         _same({0: 0, 1: 2, 2: 3, 3: 4}))

    # keyframe overload: a KF2 keypoint without a map point at distance 0 is skipped there, not in the frame overload
    kf, f, B = Side(), Side(), P.base()
    kf.add(tree, 15, B)
    f.add(tree, 15, B.copy(), mp=-1)
    f.add(tree, 15, P.flip(B, 10))
    scen("kf2_map_points", "src/ORBmatcher.cc:576-582 `if(vbMatched2[idx2] || !pMP2)`", kf, f, 0.75, _same({0: 0}),
         _same({1: 0}))

    # stopped features (weight 0) never enter the FeatureVector: the stopped query does not claim, the stopped candidate
    # (distance 2) does not beat the live one (10)
    kf, f, B = Side(), Side(), P.base()
    kf.add(tree, 16, B, stopped=True)
    kf.add(tree, 16, B)
    f.add(tree, 16, B.copy(), stopped=True)
    f.add(tree, 16, P.flip(B, 10))
    scen("stopped_words", "Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1156-1160 `if(w > 0)`", kf, f, 0.75, _same({1: 1}))

    # nodes on one side only: groups 17 (KF) and 19 (F) hold identical payloads, only group 18 is common
    kf, f, B, C = Side(), Side(), P.base(), P.base()
    kf.add(tree, 17, B)
    kf.add(tree, 18, C)
    f.add(tree, 18, P.flip(C, 5))
    f.add(tree, 19, B.copy())
    scen("one_sided_nodes", "src/ORBmatcher.cc:264-275 (the merge walk over two FeatureVectors)", kf, f, 0.75, _same({0: 1}))

    # rotation histograms: independent pairs (distance 3, ~96 from every other pair), split over groups 0 and 1
    def rot_pairs(name, bins, ref, keep):
        kf, f = Side(), Side()
        want = {}
        for i, (b, (a_kf, a_f)) in enumerate(bins):
            B = P.base()
            q = kf.add(tree, i % 2, B, angle=a_kf)
            j = f.add(tree, i % 2, P.flip(B, 3, 7 * (i % 20)), angle=a_f)
            want[j] = (q, b)
        scen(name, ref, kf, f, 0.75, {False: {j: q for j, (q, b) in want.items()},
                                       True: {j: q for j, (q, b) in want.items() if b in keep}})
        for i in range(len(kf.desc)):
            for j in range(len(f.desc)):
                d = int(np.unpackbits(kf.desc[i] ^ f.desc[j]).sum())
                assert d == 3 if i == j else d >= 60

    bin0, bin3, bin12, wrap12 = (0, (10.0, 10.0)), (3, (100.0, 10.0)), (12, (355.0, 5.0)), (12, (5.0, 15.0))
    rot_pairs("rot_bin12_kept_at_tenth", [bin0] * 10 + [bin12],
              "src/ORBmatcher.cc:241-247 (factor 1/30: rot in [345, 360) is bin 12), :1698 `max2<0.1f*(float)max1` "
              "(1 < 0.1f * 10 = 1 is false: kept)", {0, 12})
    rot_pairs("rot_below_tenth", [bin0] * 11 + [bin3], "src/ORBmatcher.cc:1698 (1 < 0.1f * 11: bin 3 dropped)", {0})
    rot_pairs("rot_three_maxima_ties", [(2, (70.0, 10.0))] * 3 + [(4, (130.0, 10.0))] * 3 + [(6, (190.0, 10.0))] * 3
              + [(8, (250.0, 10.0))] * 3 + [wrap12],
              "src/ORBmatcher.cc:1666-1697 (equal counts: the lower bins 2, 4, 6 win over 8; the wrap -10 + 360 is bin 12)",
              {2, 4, 6})
    return tree, out


# ----------------------------------------------------------------------------------------------------------------------
# SearchForTriangulation.  F12 makes the epipolar line of (x1, y1) the row y = y1 (a = 0, b = 1, c = -y1) so the gate is
# (y2 - y1)^2 < 3.84 * sigma2; the epipole sits at (fx * Cw1.x / Cw1.z + cx, fy * Cw1.y / Cw1.z + cy) with T2w = I.

F_ROW = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
F_DEN0 = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], np.float32)
C_FAR = np.array([2.0, 0.0, 1.0], np.float32)       # epipole (832, 240): outside the image
C_MID = np.array([0.0, 0.0, 1.0], np.float32)       # epipole (320, 240)
REF_TRI = "src/ORBmatcher.cc:695-760"


def gate_edge(y1=100.0, sigma2=1.0):
    """The largest float y2 > y1 with (y2 - y1)^2 < 3.84 * sigma2 in CheckDistEpipolarLine's arithmetic (:147-157)."""
    y = F32(y1 + np.sqrt(3.84 * sigma2))
    ok = lambda v: float(F32(F32(v - F32(y1)) * F32(v - F32(y1)))) < 3.84 * sigma2
    while not ok(y):
        y = np.nextafter(y, F32(-np.inf))
    while ok(np.nextafter(y, F32(np.inf))):
        y = np.nextafter(y, F32(np.inf))
    return float(y)


@dataclass
class TriScenario:
    name: str
    ref: str
    k1: Side
    k2: Side
    F12: np.ndarray
    Cw1: np.ndarray
    expected: dict         # (only_stereo, check_ori) -> {i1: i2}

    def expected_array(self, only_stereo, check_ori):
        m = np.full(len(self.k1.desc), -1, np.int32)
        e = self.expected[(only_stereo, check_ori)]
        for i1, i2 in e.items():
            m[i1] = i2
        return len(e), m


def _all4(d):
    return {(s, o): d for s in (False, True) for o in (False, True)}


def tri_scenarios():
    tree = matcher_tree()
    P = Payloads(11)
    out = []

    def mono(e):
        return {(False, False): e, (False, True): e, (True, False): {}, (True, True): {}}

    # the LAST of equal minima: positions 3, 10 (chunk 0) and 90 (chunk 1) at 20; then 5 and 6 in one chunk
    k1, k2 = Side(default_mp=-1), Side(default_mp=-1)
    B = P.base()
    k1.add(tree, 0, B, x=100.0, y=100.0)
    for i in range(100):
        k2.add(tree, 0, P.flip(B, 20, 3 * (i % 30)) if i in (3, 10, 90) else P.flip(B, 70), y=100.0)
    C = P.base()
    k1.add(tree, 1, C, x=100.0, y=100.0)
    for i in range(8):
        k2.add(tree, 1, P.flip(C, 20, 40 + i) if i in (5, 6) else P.flip(C, 45), y=100.0)
    out.append(TriScenario("last_of_equal_minima", REF_TRI + ": `if(dist>TH_LOW || dist>bestDist) continue;`", k1, k2, F_ROW,
                           C_FAR, mono({0: 90, 1: 100 + 6})))

    # dist = 50 passes, 51 does not
    k1, k2 = Side(default_mp=-1), Side(default_mp=-1)
    for g, d in ((2, 50), (3, 51)):
        B = P.base()
        k1.add(tree, g, B, y=120.0)
        k2.add(tree, g, P.flip(B, d), y=120.0)
    out.append(TriScenario("th_low_50", REF_TRI + ": TH_LOW is inclusive here", k1, k2, F_ROW, C_FAR, mono({0: 0})))

    # the epipole radius (mono-mono): sqrt(100) px at octave 0, +-1 ulp on either side; stereo on one side skips it
    k1, k2 = Side(default_mp=-1), Side(default_mp=-1)
    e = {}
    for g, (x2, ur1, ur2, ok) in enumerate(((np.nextafter(F32(330), F32(0)), -1, -1, False), (330.0, -1, -1, True),
                                            (np.nextafter(F32(310), F32(1000)), -1, -1, False), (310.0, -1, -1, True),
                                            (320.0, -1, 5.0, True), (320.0, 5.0, -1, True)), start=4):
        B = P.base()
        i1 = k1.add(tree, g, B, x=100.0, y=240.0, u_right=ur1)
        i2 = k2.add(tree, g, P.flip(B, 4), x=float(x2), y=240.0, u_right=ur2)
        if ok:
            e[i1] = i2
    out.append(TriScenario("epipole_radius", "src/ORBmatcher.cc:741-747 `distex*distex+distey*distey<100*...`", k1, k2, F_ROW,
                           C_MID, {(False, False): e, (False, True): e,
                                   (True, False): {}, (True, True): {}}))     # only-stereo: no pair has stereo on both sides

    # bOnlyStereo: a stereo KF1 keypoint sees a mono candidate at 5 and a stereo one at 10; a mono KF1 keypoint is skipped
    k1, k2 = Side(default_mp=-1), Side(default_mp=-1)
    B = P.base()
    k1.add(tree, 10, B, y=50.0, u_right=80.0)
    k2.add(tree, 10, P.flip(B, 5), y=50.0)
    k2.add(tree, 10, P.flip(B, 10, 20), y=50.0, u_right=40.0)
    C = P.base()
    k1.add(tree, 11, C, y=60.0)
    k2.add(tree, 11, P.flip(C, 5), y=60.0)
    both = {0: 0, 1: 2}
    out.append(TriScenario("only_stereo", REF_TRI + ": `if(bOnlyStereo) if(!bStereo1)` / `if(!bStereo2)`", k1, k2, F_ROW, C_FAR,
                           {(False, False): both, (False, True): both, (True, False): {0: 1}, (True, True): {0: 1}}))

    # the 3.84 * sigma2 gate, +-1 ulp above and below the row, at octave 0
    y_up = gate_edge(100.0)
    y_dn = 200.0 - y_up                                  # exact: 100 - (y_up - 100)
    k1, k2 = Side(default_mp=-1), Side(default_mp=-1)
    e = {}
    for g, (y2, ok) in enumerate(((y_up, True), (float(np.nextafter(F32(y_up), F32(1e9))), False), (y_dn, True),
                                  (float(np.nextafter(F32(y_dn), F32(0))), False)), start=12):
        B = P.base()
        i1 = k1.add(tree, g, B, y=100.0)
        i2 = k2.add(tree, g, P.flip(B, 8), y=y2)
        if ok:
            e[i1] = i2
    out.append(TriScenario("epipolar_gate", "src/ORBmatcher.cc:141-158 `dsqr<3.84*pKF2->mvLevelSigma2[kp2.octave]`", k1, k2,
                           F_ROW, C_FAR, mono(e)))

    # den == 0: no pair passes, even at distance 0
    k1, k2 = Side(default_mp=-1), Side(default_mp=-1)
    B = P.base()
    k1.add(tree, 16, B, y=100.0)
    k2.add(tree, 16, B.copy(), y=100.0)
    out.append(TriScenario("den_zero", "src/ORBmatcher.cc:153 `if(den==0) return false;`", k1, k2, F_DEN0, C_FAR, _all4({})))

    # map points on either side skip; vbMatched2 is never set, so two KF1 keypoints share one KF2 keypoint
    k1, k2 = Side(default_mp=-1), Side(default_mp=-1)
    B = P.base()
    k1.add(tree, 17, B, y=100.0, mp=5)
    k1.add(tree, 17, B, y=100.0, mp=-1)
    k1.add(tree, 17, P.flip(B, 2, 100), y=100.0, mp=-1)
    k2.add(tree, 17, B.copy(), y=100.0, mp=3)
    k2.add(tree, 17, P.flip(B, 6), y=100.0, mp=-1)
    out.append(TriScenario("map_points_and_sharing", REF_TRI + ": `if(pMP1) continue;`, `if(vbMatched2[idx2] || pMP2)`", k1, k2,
                           F_ROW, C_FAR, mono({1: 1, 2: 1})))

    # rotation: 11 pairs in bin 0, one in bin 3 (1 < 0.1f * 11: dropped)
    k1, k2 = Side(default_mp=-1), Side(default_mp=-1)
    e, e_ori = {}, {}
    for i in range(12):
        B = P.base()
        a1 = 100.0 if i == 11 else 10.0
        i1 = k1.add(tree, 18 + i % 2, B, angle=a1, y=30.0 + i)
        i2 = k2.add(tree, 18 + i % 2, P.flip(B, 3, 5 * i), angle=10.0, y=30.0 + i)
        e[i1] = i2
        if i != 11:
            e_ori[i1] = i2
    out.append(TriScenario("rotation_tenth", "src/ORBmatcher.cc:776-815, :1698", k1, k2, F_ROW, C_FAR,
                           {(False, False): e, (False, True): e_ori, (True, False): {}, (True, True): {}}))
    return tree, out


def scale_tables(nlevels=8, scale=1.2):
    s = np.ones(nlevels, np.float32)
    for k in range(1, nlevels):
        s[k] = F32(s[k - 1] * F32(scale))
    return s, (s * s).astype(np.float32)
