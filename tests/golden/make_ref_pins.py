#!/usr/bin/env python3
"""Regenerate tests/golden/ref_pins.npz: the outputs of the reference's own DBoW2 containers and PEAC ParamSet / DisjointSet
(oracle/_ref/libdrslam_ref.so, `make -C oracle ref` where a reference checkout exists) on the inputs of tests/test_ref_pins.py,
together with those inputs.  Unlike the other fixtures this one records the REFERENCE, not the oracle: the pins then hold on
every checkout, whether or not the reference can be built there."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as orc       # noqa: E402

spec = importlib.util.spec_from_file_location("test_ref_pins", os.path.join(ROOT, "tests", "test_ref_pins.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)

OUT = os.path.dirname(os.path.abspath(__file__))
if not os.path.exists(T.REF):
    sys.exit("%s not built: make -C oracle ref (needs the reference checkout)" % T.REF)
lib = C.CDLL(T.REF)
orc.lib()
g = {}

rng = np.random.default_rng(0)
zs = np.concatenate([[0.0, -1.0, 499.999, 500.0, 4000.0, 4000.001, 1e6], rng.uniform(-100, 9000, 500), rng.uniform(0, 5, 200)])
g["thr_z"], g["thr"] = zs, T.ref_thresholds(lib, zs)

rng = np.random.default_rng(1)
for n, m in T.DS_CASES:
    key = "ds_%d_%d_" % (n, m)
    pairs = rng.integers(0, n, (max(m, 1), 2)).astype(np.int32)
    g[key + "pairs"] = pairs
    g[key + "union"], g[key + "find"], g[key + "size"] = T.ref_disjoint_set(lib, n, pairs, m)

for weighting, scoring in T.BOW_CASES:
    key = "bow_%d_%d_" % (weighting, scoring)
    _, _, _, word, weight, nid = T.bow_inputs(orc, weighting, scoring)
    g[key + "word"], g[key + "weight"], g[key + "nid"] = word, weight, nid
    out = T.ref_bow_containers(lib, word, weight, nid, weighting, scoring)
    for k, v in zip(("ids", "vals", "fv_nodes", "fv_counts", "fv_features"), out):
        g[key + k] = v

path = os.path.join(OUT, "ref_pins.npz")
np.savez_compressed(path, **g)
print("ref_pins.npz", os.path.getsize(path), "bytes,", len(g), "arrays")
