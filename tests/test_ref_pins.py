"""Pins against the REFERENCE ITSELF, for the slice of it that compiles without OpenCV / Eigen / PCL: oracle/_ref/libdrslam_ref.so
is built by `make -C oracle ref` from the reference's own Thirdparty/DBoW2/DBoW2/{BowVector,FeatureVector}.cpp and
include/peac/{AHCParamSet,DisjointSet}.hpp where a reference checkout exists (oracle/ref_shim.cpp is the C entry layer;
nothing of the reference is copied).  The oracle's restatements - and the product's host-side container code - must agree
with it bit for bit.  Everything else on the hot path needs OpenCV 3.4 / Eigen / PCL: still unpinned.

The library's outputs on these inputs are recorded in tests/golden/ref_pins.npz (tests/golden/make_ref_pins.py), so the pins
hold on every checkout; where oracle/_ref has been built, the live library is checked against that record as well."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libdrslam_ref.so")
GOLD = os.path.join(HERE, "golden", "ref_pins.npz")

DS_CASES = ((3072, 4000), (3072, 200), (16, 64), (2, 5), (1, 0))
BOW_CASES = [(0, 0), (0, 1), (1, 5), (2, 0), (3, 1), (1, 2), (3, 5)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the reference's entry points (oracle/ref_shim.cpp): used by the tests where the library exists, and by make_ref_pins.py

def ref_thresholds(lib, zs):
    """ahc::ParamSet::T_mse / T_ang / T_dz for every phase and depth: (3, len(zs), 3) float64"""
    lib.ref_ahc_thresholds.argtypes = [C.c_int, C.c_double, C.c_void_p]
    lib.ref_ahc_thresholds.restype = None
    out = np.zeros((3, len(zs), 3))
    a = np.zeros(3)
    for phase in (0, 1, 2):
        for i, z in enumerate(zs):
            lib.ref_ahc_thresholds(phase, float(z), _p(a))
            out[phase, i] = a
    return out


def ref_disjoint_set(lib, n, pairs, m):
    """DisjointSet::Union return values, then Find / getSetSize of every element"""
    lib.ref_ahc_disjoint_set.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ref_ahc_disjoint_set.restype = None
    u, f, s = np.zeros(max(m, 1), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.ref_ahc_disjoint_set(n, _p(pairs), m, _p(u), _p(f), _p(s))
    return u[:m].copy(), f, s


def ref_bow_containers(lib, word, weight, nid, weighting, scoring):
    """BowVector (ids, values) and FeatureVector (nodes, counts, features back to back) in map order"""
    n = len(word)
    lib.ref_bow_containers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    ids, vals = np.zeros(n, np.int32), np.zeros(n)
    fvn, fvc, fvf = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    nw, nn = C.c_int(0), C.c_int(0)
    lib.ref_bow_containers(_p(word), _p(weight), _p(nid), n, weighting, scoring, _p(ids), _p(vals), C.byref(nw), _p(fvn), _p(fvc),
                           _p(fvf), C.byref(nn))
    return ids[:nw.value], vals[:nw.value], fvn[:nn.value], fvc[:nn.value], fvf[:int(fvc[:nn.value].sum())]


def bow_inputs(orc, weighting, scoring):
    """The synthetic vocabulary, the descriptors and the per-feature (word, weight, node) triples of the oracle's tree descent"""
    from dr_slam_amd import vocabulary as V
    voc = V.make_synthetic(6, 3, seed=3 + weighting, scoring=scoring, weighting=weighting, stop_fraction=0.05)
    ov = orc.VocabularyOracle(voc.to_text())
    rng = np.random.default_rng(10 * weighting + scoring)
    n = 900
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    desc[100:400] = desc[:300]                                   # repeated words: addWeight accumulates, addIfNotExist does not
    word, weight, nid = ov.transform_each(desc, levelsup=2)
    return voc, ov, desc, word, weight, nid


# ---- the tests

@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def live():
    """the reference library itself where oracle/_ref has been built, else None"""
    return C.CDLL(REF) if os.path.exists(REF) else None


def test_ahc_thresholds_equal_the_reference_paramset(gold, live, oracle_mod):
    """ahc::ParamSet::T_mse / T_ang / T_dz (include/peac/AHCParamSet.hpp:95-153) in all three phases, over depths inside and
    outside [z_near, z_far] (mm), negative and zero included."""
    L = oracle_mod.lib()
    L.orc_ahc_thresholds.argtypes = [C.c_int, C.c_double, C.c_void_p]
    L.orc_ahc_thresholds.restype = None
    zs, want = gold["thr_z"], gold["thr"]
    if live is not None:
        assert np.array_equal(ref_thresholds(live, zs).view(np.uint64), want.view(np.uint64))
    b = np.zeros(3)
    for phase in (0, 1, 2):
        for i, z in enumerate(zs):
            L.orc_ahc_thresholds(phase, float(z), _p(b))
            assert np.array_equal(want[phase, i].view(np.uint64), b.view(np.uint64)), (phase, z, want[phase, i], b)


def test_disjoint_set_equals_the_reference(gold, live, oracle_mod):
    """DisjointSet::Union / Find / getSetSize (include/peac/DisjointSet.hpp): same roots (union by size, ties to x), same
    return values, on the 64 x 48 block grid's size and on small sets with many repeated unions."""
    L = oracle_mod.lib()
    L.orc_ahc_disjoint_set.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.orc_ahc_disjoint_set.restype = None
    for n, m in DS_CASES:
        key = "ds_%d_%d_" % (n, m)
        pairs = gold[key + "pairs"]
        want = (gold[key + "union"], gold[key + "find"], gold[key + "size"])
        if live is not None:
            for x, y in zip(ref_disjoint_set(live, n, pairs, m), want):
                assert np.array_equal(x, y), (n, m)
        u, f, s = np.zeros(max(m, 1), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        L.orc_ahc_disjoint_set(n, _p(pairs), m, _p(u), _p(f), _p(s))
        for x, y in zip((u[:m], f, s), want):
            assert np.array_equal(x, y), (n, m)
        if m >= 64:
            assert len(np.unique(want[1])) < n


@pytest.mark.parametrize("weighting,scoring", BOW_CASES)
def test_bow_containers_equal_the_reference(gold, live, oracle_mod, weighting, scoring):
    """BowVector::addWeight / addIfNotExist / normalize and FeatureVector::addFeature of the reference, fed with the
    per-feature (word, weight, node) triples of the oracle's tree descent in feature order as TemplatedVocabulary::transform
    does: the oracle's BowVector (ids and float64 values) and the product's host-side containers
    (dr_slam_amd.vocabulary.bow_and_feature_vectors, what Frame::ComputeBoW's adaptor builds from the device's per-feature
    results) are identical, values bit for bit."""
    from dr_slam_amd import vocabulary as V
    voc, ov, desc, word, weight, nid = bow_inputs(oracle_mod, weighting, scoring)
    assert (weight == 0).any() and (weight > 0).sum() > 500      # stopped words are skipped by both containers
    key = "bow_%d_%d_" % (weighting, scoring)
    # the recorded outputs belong to exactly these inputs
    assert np.array_equal(word, gold[key + "word"]) and np.array_equal(nid, gold[key + "nid"])
    assert np.array_equal(weight.view(np.uint64), gold[key + "weight"].view(np.uint64))
    ids, vals, fvn, fvc, fvf = (gold[key + k] for k in ("ids", "vals", "fv_nodes", "fv_counts", "fv_features"))
    if live is not None:
        for x, y in zip(ref_bow_containers(live, word, weight, nid, weighting, scoring), (ids, vals, fvn, fvc, fvf)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # the oracle's transform()
    o_ids, o_vals = ov.bow_vector(desc, levelsup=2)
    assert np.array_equal(ids, o_ids)
    assert np.array_equal(vals.view(np.uint64), o_vals.view(np.uint64))
    # the product's host-side containers
    p_ids, p_vals, p_fv = V.bow_and_feature_vectors(voc, word, weight, nid)
    assert np.array_equal(ids, p_ids) and np.array_equal(vals.view(np.uint64), p_vals.view(np.uint64))
    off = np.concatenate([[0], np.cumsum(fvc)])
    r_fv = {int(fvn[i]): fvf[off[i]:off[i + 1]].tolist() for i in range(len(fvn))}
    assert list(r_fv) == list(p_fv) and r_fv == p_fv
    if scoring in (0, 2):
        assert abs(np.abs(vals).sum() - 1) < 1e-12
