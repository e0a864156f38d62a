"""The CPU oracle of the bag-of-words path and the numpy restatement of the reference (tests/bow_numpy.py) against the
outcomes stated by hand for the vocabularies and frames of tests/bow_scenarios.py: the vocabulary descent at its ties, chunk
and level edges, both SearchByBoW overloads at their thresholds, claims and rotation histograms, and SearchForTriangulation
at its gates.  tests/test_gpu_bow_edges.py holds the device to the same outcomes."""
import numpy as np
import pytest

import bow_numpy as bn
import bow_scenarios as bs

DESCENT = {s.name: s for s in bs.descent_scenarios()}
MTREE, MATCH_LIST = bs.match_scenarios()
MATCH = {s.name: s for s in MATCH_LIST}
TTREE, TRI_LIST = bs.tri_scenarios()
TRI = {s.name: s for s in TRI_LIST}
DESCENT_CASES = [(n, lu) for n, s in sorted(DESCENT.items()) for lu in s.levelsups]


def test_scenarios_cite_the_reference():
    for s in list(DESCENT.values()) + MATCH_LIST + TRI_LIST:
        assert "TemplatedVocabulary.h" in s.ref or "src/ORBmatcher.cc" in s.ref, s.name


def test_text_loader_ids_and_words(oracle_mod):
    """Node ids are line numbers, children keep file order, word ids follow the leaf flags in file order (:1365-1424)."""
    for s in DESCENT.values():
        tv = bn.TextVocabulary(s.tree.text)
        v = s.tree.voc
        parent, word, desc, weight = oracle_mod.VocabularyOracle(s.tree.text).nodes()
        assert len(tv.nodes) == v.n_nodes == len(parent)
        assert np.array_equal(parent[1:], [nd.parent for nd in tv.nodes[1:]]) and np.array_equal(parent, v.parent)
        assert np.array_equal(desc, np.stack([nd.desc for nd in tv.nodes])) and np.array_equal(desc, v.desc)
        assert np.array_equal(weight.view(np.uint64), np.array([nd.weight for nd in tv.nodes]).view(np.uint64))
        leaf = v.is_leaf > 0
        assert np.array_equal(word[leaf], [tv.nodes[i].word_id for i in np.flatnonzero(leaf)])
        assert np.array_equal(word[leaf], np.arange(leaf.sum())) and (word[~leaf] == -1).all()
        for nd in tv.nodes:                                   # children in id order, ids of a node's children consecutive
            assert nd.children == sorted(nd.children)
            assert nd.children == list(range(nd.children[0], nd.children[0] + len(nd.children))) if nd.children else True
    t = DESCENT["unbalanced"].tree                           # depth-first creation: a grandchild precedes a later child's kids
    assert t.path_id[(3, 0)] < t.path_id[(4, 0)] and t.path_id[(3, 0, 0, 9, 0)] < t.path_id[(4, 0)]
    assert sorted(set(t.depth[np.flatnonzero(t.voc.is_leaf)])) == [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("name,levelsup", DESCENT_CASES)
def test_descent(oracle_mod, name, levelsup):
    s = DESCENT[name]
    ew, ewt, enid = s.expected(levelsup)
    w, wt, nid = bn.TextVocabulary(s.tree.text).transform_each(s.desc, levelsup)
    assert np.array_equal(w, ew), [s.why[i] for i in np.flatnonzero(w != ew)]
    assert np.array_equal(wt, ewt)
    assert nid == enid
    ow, owt, onid = oracle_mod.VocabularyOracle(s.tree.text).transform_each(s.desc, levelsup)
    assert np.array_equal(ow, ew) and np.array_equal(owt.view(np.uint64), ewt.view(np.uint64))
    # where the reference leaves nid unset (a leaf above m_L - levelsup) the oracle and the product give 0
    assert np.array_equal(onid, [0 if e is None else e for e in enid])


def test_descent_covers_the_edges():
    s = DESCENT["unbalanced"]
    _, wt, _ = s.expected(4)
    assert (wt == 0).sum() == 2                                           # two stopped leaves reached
    assert any(e is None for e in s.expected(4)[2]) and any(e is None for e in s.expected(0)[2])
    assert DESCENT["wide32"].paths[0] == (31,) and len(DESCENT["chain10"].paths[0]) == 10


def test_wide33_loads_in_the_reference(oracle_mod):
    """DBoW2 itself has no child limit; the device's 32-lane descent does (tests/test_gpu_bow_edges.py: rejected)."""
    t = bs.wide33_tree()
    f = bs.feature(t, {1: [32]})[None]
    w, _, _ = bn.TextVocabulary(t.text).transform_each(f, 0)
    ow, _, _ = oracle_mod.VocabularyOracle(t.text).transform_each(f, 0)
    assert w[0] == ow[0] == 32


def test_leaf_flag_mismatch_is_what_the_device_rejects(oracle_mod):
    """A node flagged internal without children: the reference stops there (isLeaf() is children.empty()) and returns
    Node()'s word_id 0, the oracle -1.  DBoW2 never writes such a file; the device rejects it at upload."""
    good, inner_childless, _ = bs.leaf_flag_mismatch()
    text = inner_childless.to_text()
    f = good.desc[1][None]                                   # nearest to node 1
    w, wt, _ = bn.TextVocabulary(text).transform_each(f, 0)
    ow, _, _ = oracle_mod.VocabularyOracle(text).transform_each(f, 0)
    assert (w[0], ow[0]) == (0, -1)


def _side(s, tree_text, levelsup, orc=None):
    kps, desc, mp, ur = s.arrays()
    if orc is None:
        w, wt, nid = bn.TextVocabulary(tree_text).transform_each(desc, levelsup)
        return kps, desc, mp, ur, bn.feature_vector(nid, wt)
    _, wt, nid = orc.VocabularyOracle(tree_text).transform_each(desc, levelsup)
    return kps, desc, mp, ur, np.where(wt > 0, nid, -1)


@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("overload", ["frame", "kf"])
@pytest.mark.parametrize("name", sorted(MATCH))
def test_search_by_bow(oracle_mod, name, overload, check_ori):
    s = MATCH[name]
    n_e, m_e = s.expected_array(overload, check_ori)
    kk, dk, mpk, _, fvk = _side(s.kf, MTREE.text, bs.MATCH_LEVELSUP)
    kf, df, mpf, _, fvf = _side(s.f, MTREE.text, bs.MATCH_LEVELSUP)
    _, _, _, _, nk = _side(s.kf, MTREE.text, bs.MATCH_LEVELSUP, oracle_mod)
    _, _, _, _, nf = _side(s.f, MTREE.text, bs.MATCH_LEVELSUP, oracle_mod)
    if overload == "frame":
        n, m = bn.search_by_bow(fvk, fvf, dk, kk["angle"], mpk, df, kf["angle"], len(df), s.nnratio, check_ori)
        n_o, m_o = oracle_mod.search_by_bow(nk, nf, dk, kk["angle"], mpk, df, kf["angle"], s.nnratio, check_ori)
    else:
        n, m = bn.search_by_bow_kf(fvk, fvf, dk, kk["angle"], mpk, df, kf["angle"], mpf, s.nnratio, check_ori)
        n_o, m_o = oracle_mod.search_by_bow_kf(nk, nf, dk, kk["angle"], mpk, df, kf["angle"], mpf, s.nnratio, check_ori)
    assert (n, n_o) == (n_e, n_e) and np.array_equal(m, m_e) and np.array_equal(m_o, m_e), \
        (n, n_o, n_e, np.flatnonzero(m != m_e)[:8], np.flatnonzero(m_o != m_e)[:8])


def tri_inputs(s, tree_text, orc=None):
    out = []
    for side in (s.k1, s.k2):
        kps, desc, mp, ur, g = _side(side, tree_text, bs.MATCH_LEVELSUP, orc)
        d = dict(x=kps["x"], y=kps["y"], angle=kps["angle"], u_right=ur, octave=kps["octave"], mp=mp, desc=desc)
        d["nid" if orc is not None else "fv"] = g
        out.append(d)
    return out


@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("only_stereo", [False, True])
@pytest.mark.parametrize("name", sorted(TRI))
def test_search_for_triangulation(oracle_mod, name, only_stereo, check_ori):
    s = TRI[name]
    n_e, m_e = s.expected_array(only_stereo, check_ori)
    scale, sigma2 = bs.scale_tables()
    ex, ey = bn.epipole(np.eye(4, dtype=np.float32), s.Cw1, bs.FX, bs.FY, bs.CX, bs.CY)
    k1, k2 = tri_inputs(s, TTREE.text)
    n, m = bn.search_for_triangulation(k1, k2, s.F12, ex, ey, scale, sigma2, only_stereo, check_ori)
    o1, o2 = tri_inputs(s, TTREE.text, oracle_mod)
    n_o, m_o = oracle_mod.search_for_triangulation(o1, o2, s.F12, ex, ey, scale, sigma2, only_stereo, check_ori)
    assert (n, n_o) == (n_e, n_e) and np.array_equal(m, m_e) and np.array_equal(m_o, m_e), (n, n_o, n_e, m, m_o)


def test_float_edges_are_where_they_are_claimed():
    f32 = np.float32
    y = bs.gate_edge(100.0)
    assert bn.epipolar_ok(0, 100, 0, y, bs.F_ROW, 1.0) and not bn.epipolar_ok(0, 100, 0, np.nextafter(f32(y), f32(1e9)), bs.F_ROW, 1.0)
    assert not bn.epipolar_ok(0, 100, 0, 100, bs.F_DEN0, 1.0)                       # den == 0
    assert bn.epipole(np.eye(4), bs.C_MID, bs.FX, bs.FY, bs.CX, bs.CY) == (320.0, 240.0)
    assert f32(f32(0.75) * f32(40)) == 30.0 and f32(f32(0.1) * f32(10)) == 1.0 and f32(f32(0.1) * f32(11)) > 1.0
    assert [bn.rotation_bin(a, b) for a, b in ((355, 5), (5, 15), (10, 10), (100, 10), (359.9, 0))] == [12, 12, 0, 3, 12]
    assert bn.three_maxima([0, 0, 3, 0, 3, 0, 3, 0, 3, 0, 0, 0, 1] + [0] * 17) == (2, 4, 6)
    assert bn.three_maxima([10] + [0] * 11 + [1] + [0] * 17) == (0, 12, -1)
    assert bn.three_maxima([11, 0, 0, 1] + [0] * 26) == (0, -1, -1)
