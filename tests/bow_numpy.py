"""Plain numpy/Python restatement of the bag-of-words path, written from the reference (not from oracle/bow_oracle.cpp):

  TemplatedVocabulary::loadFromTextFile          Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424
  TemplatedVocabulary::transform (one feature)   :1216-1259 (do-while descent, strict `d < best_d`, nid at m_L - levelsup)
  TemplatedVocabulary::transform (FeatureVector) :1127-1190 (features with w > 0 only, in feature order)
  ORBmatcher::SearchByBoW(pKF, F)                src/ORBmatcher.cc:160-292
  ORBmatcher::SearchByBoW(pKF1, pKF2)            :526-660
  ORBmatcher::SearchForTriangulation             :661-827 with CheckDistEpipolarLine :141-158
  ORBmatcher::ComputeThreeMaxima                 :1666-1707

float32 steps are numpy float32 scalars (each operation rounds like the reference's float); comparisons the reference makes
in double (`rot < 0.0`, `dsqr < 3.84 * sigma2`) are made in Python floats.
"""
import numpy as np

F32 = np.float32
TH_LOW, HISTO_LENGTH = 50, 30


class Node:
    __slots__ = ("id", "parent", "children", "desc", "weight", "word_id")

    def __init__(self, nid):
        self.id, self.parent, self.children = nid, 0, []
        self.desc, self.weight = np.zeros(32, np.uint8), 0.0
        self.word_id = 0            # DBoW2's Node() initialises word_id to 0


class TextVocabulary:
    """loadFromTextFile: node id = line number (root 0), children in file order, word ids in file order of the leaf flags."""

    def __init__(self, text):
        rows = text.split("\n")
        head = rows[0].split()
        self.k, self.L, n1, n2 = (int(v) for v in head[:4])
        if self.k < 0 or self.k > 20 or self.L < 1 or self.L > 10 or n1 < 0 or n1 > 5 or n2 < 0 or n2 > 3:
            raise ValueError("Vocabulary loading failure: This is not a correct text file!")
        self.scoring, self.weighting = n1, n2
        self.nodes = [Node(0)]
        self.words = []
        for r in rows[1:]:
            t = r.split()
            if not t:
                continue
            nd = Node(len(self.nodes))
            nd.parent = int(t[0])
            self.nodes.append(nd)
            self.nodes[nd.parent].children.append(nd.id)
            nd.desc = np.array([int(v) for v in t[2:34]], np.uint8)
            nd.weight = float(t[34])
            if int(t[1]) > 0:
                nd.word_id = len(self.words)
                self.words.append(nd.id)

    def is_leaf(self, nid):
        return not self.nodes[nid].children

    def transform_one(self, feature, levelsup):
        """-> (word_id, weight, nid); nid is None where the reference leaves it unset (a leaf above m_L - levelsup)."""
        nid_level = self.L - levelsup
        nid = 0 if nid_level <= 0 else None
        final_id, level = 0, 0
        while True:
            level += 1
            nodes = self.nodes[final_id].children
            final_id = nodes[0]
            best_d = hamming(feature, self.nodes[final_id].desc)
            for cid in nodes[1:]:
                d = hamming(feature, self.nodes[cid].desc)
                if d < best_d:
                    best_d, final_id = d, cid
            if level == nid_level:
                nid = final_id
            if self.is_leaf(final_id):
                break
        return self.nodes[final_id].word_id, self.nodes[final_id].weight, nid

    def transform_each(self, desc, levelsup):
        out = [self.transform_one(d, levelsup) for d in desc]
        return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.float64), [o[2] for o in out])


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def feature_vector(nid, weight):
    """FeatureVector::addFeature for every feature with w > 0: {node: [feature index, ...]} in key order."""
    fv = {}
    for i, (n, w) in enumerate(zip(nid, weight)):
        if w > 0:
            fv.setdefault(int(n), []).append(i)
    return dict(sorted(fv.items()))


def rotation_bin(angle1, angle2):
    rot = F32(F32(angle1) - F32(angle2))
    if float(rot) < 0.0:
        rot = F32(rot + F32(360.0))
    v = float(F32(rot * F32(F32(1.0) / F32(HISTO_LENGTH))))           # factor = 1.0f / HISTO_LENGTH: bins 0..12 only
    b = int(np.floor(v + 0.5))                                          # round(): halves away from zero (v >= 0 here)
    return 0 if b == HISTO_LENGTH else b


def three_maxima(counts):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if float(max2) < float(F32(F32(0.1) * F32(max1))):
        ind2 = ind3 = -1
    elif float(max3) < float(F32(F32(0.1) * F32(max1))):
        ind3 = -1
    return ind1, ind2, ind3


def _filter_rotation(hist, out, nmatches, clear):
    keep = three_maxima([len(h) for h in hist])
    for i in range(HISTO_LENGTH):
        if i in keep:
            continue
        for idx in hist[i]:
            clear(out, idx)
            nmatches -= 1
    return nmatches


def _common_nodes(fv1, fv2):
    return [n for n in fv1 if n in fv2]            # the merge walk over two sorted maps visits exactly the common keys


def search_by_bow(fv_kf, fv_f, desc_kf, angle_kf, kf_mp, desc_f, angle_f, n_f, nnratio, check_ori):
    """SearchByBoW(pKF, F): out[F keypoint] = KF keypoint or -1; `<= TH_LOW`; claims through vpMapPointMatches."""
    out = np.full(n_f, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    n = 0
    ratio = F32(nnratio)
    for node in _common_nodes(fv_kf, fv_f):
        for ikf in fv_kf[node]:
            if kf_mp[ikf] < 0:
                continue
            best1, best_idx, best2 = 256, -1, 256
            for i_f in fv_f[node]:
                if out[i_f] >= 0:
                    continue
                d = hamming(desc_kf[ikf], desc_f[i_f])
                if d < best1:
                    best2, best1, best_idx = best1, d, i_f
                elif d < best2:
                    best2 = d
            if best1 <= TH_LOW and float(F32(best1)) < float(F32(ratio * F32(best2))):
                out[best_idx] = ikf
                if check_ori:
                    hist[rotation_bin(angle_kf[ikf], angle_f[best_idx])].append(best_idx)
                n += 1
    if check_ori:
        n = _filter_rotation(hist, out, n, lambda o, i: o.__setitem__(i, -1))
    return n, out


def search_by_bow_kf(fv1, fv2, desc1, angle1, mp1, desc2, angle2, mp2, nnratio, check_ori):
    """SearchByBoW(pKF1, pKF2): vpMatches12[idx1] = map point of idx2, returned as out2[idx2] = idx1; `< TH_LOW`; both
    sides need a map point; vbMatched2 claims."""
    m12 = np.full(len(mp1), -1, np.int32)
    matched2 = np.zeros(len(mp2), bool)
    hist = [[] for _ in range(HISTO_LENGTH)]
    n = 0
    ratio = F32(nnratio)
    for node in _common_nodes(fv1, fv2):
        for i1 in fv1[node]:
            if mp1[i1] < 0:
                continue
            best1, best_idx, best2 = 256, -1, 256
            for i2 in fv2[node]:
                if matched2[i2] or mp2[i2] < 0:
                    continue
                d = hamming(desc1[i1], desc2[i2])
                if d < best1:
                    best2, best1, best_idx = best1, d, i2
                elif d < best2:
                    best2 = d
            if best1 < TH_LOW and float(F32(best1)) < float(F32(ratio * F32(best2))):
                m12[i1] = best_idx
                matched2[best_idx] = True
                if check_ori:
                    hist[rotation_bin(angle1[i1], angle2[best_idx])].append(i1)
                n += 1
    if check_ori:
        n = _filter_rotation(hist, m12, n, lambda o, i: o.__setitem__(i, -1))
    out2 = np.full(len(mp2), -1, np.int32)
    for i1, i2 in enumerate(m12):
        if i2 >= 0:
            out2[i2] = i1
    return n, out2


def epipolar_ok(x1, y1, x2, y2, F, sigma2):
    """CheckDistEpipolarLine: F is F12 row-major (F12.at<float>(r, c) = F[3 r + c])."""
    F = [F32(v) for v in np.asarray(F, np.float32).reshape(9)]
    x1, y1, x2, y2 = F32(x1), F32(y1), F32(x2), F32(y2)
    a = F32(F32(F32(x1 * F[0]) + F32(y1 * F[3])) + F[6])
    b = F32(F32(F32(x1 * F[1]) + F32(y1 * F[4])) + F[7])
    c = F32(F32(F32(x1 * F[2]) + F32(y1 * F[5])) + F[8])
    num = F32(F32(F32(a * x2) + F32(b * y2)) + c)
    den = F32(F32(a * a) + F32(b * b))
    if float(den) == 0.0:
        return False
    dsqr = F32(F32(num * num) / den)
    return float(dsqr) < 3.84 * float(F32(sigma2))


def epipole(T2w, Cw1, fx, fy, cx, cy):
    """C2 = R2w * Cw + t2w (float), ex = fx * C2.x * invz + cx (src/ORBmatcher.cc:667-674)."""
    T = np.asarray(T2w, np.float32).reshape(4, 4)
    C = np.asarray(Cw1, np.float32).reshape(3)
    C2 = []
    for r in range(3):
        d = F32(F32(F32(T[r, 0] * C[0]) + F32(T[r, 1] * C[1])) + F32(T[r, 2] * C[2]))
        C2.append(F32(d + T[r, 3]))
    invz = F32(F32(1.0) / C2[2])
    return F32(F32(F32(F32(fx) * C2[0]) * invz) + F32(cx)), F32(F32(F32(F32(fy) * C2[1]) * invz) + F32(cy))


def search_for_triangulation(kf1, kf2, F12, ex, ey, scale_factors, level_sigma2, only_stereo, check_ori):
    """kf = dict(x, y, angle, u_right, octave, mp, fv, desc).  vbMatched2 is never set in this reference, so a KF2
    keypoint can serve several KF1 keypoints; among the candidates that pass, the LAST with the smallest distance wins
    (`dist > bestDist` -> continue lets equal distances replace)."""
    out = np.full(len(kf1["mp"]), -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    n = 0
    ex, ey = F32(ex), F32(ey)
    for node in _common_nodes(kf1["fv"], kf2["fv"]):
        for i1 in kf1["fv"][node]:
            if kf1["mp"][i1] >= 0:
                continue
            stereo1 = float(kf1["u_right"][i1]) >= 0
            if only_stereo and not stereo1:
                continue
            best_d, best_idx = TH_LOW, -1
            for i2 in kf2["fv"][node]:
                if kf2["mp"][i2] >= 0:
                    continue
                stereo2 = float(kf2["u_right"][i2]) >= 0
                if only_stereo and not stereo2:
                    continue
                d = hamming(kf1["desc"][i1], kf2["desc"][i2])
                if d > TH_LOW or d > best_d:
                    continue
                o2 = int(kf2["octave"][i2])
                if not stereo1 and not stereo2:
                    dx, dy = F32(ex - F32(kf2["x"][i2])), F32(ey - F32(kf2["y"][i2]))
                    if float(F32(F32(dx * dx) + F32(dy * dy))) < float(F32(F32(100) * F32(scale_factors[o2]))):
                        continue
                if epipolar_ok(kf1["x"][i1], kf1["y"][i1], kf2["x"][i2], kf2["y"][i2], F12, level_sigma2[o2]):
                    best_idx, best_d = i2, d
            if best_idx >= 0:
                out[i1] = best_idx
                n += 1
                if check_ori:
                    hist[rotation_bin(kf1["angle"][i1], kf2["angle"][best_idx])].append(i1)
    if check_ori:
        n = _filter_rotation(hist, out, n, lambda o, i: o.__setitem__(i, -1))
    return n, out
