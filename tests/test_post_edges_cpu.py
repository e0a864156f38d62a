"""CPU tests of the plane post-processing on hand-built clouds and planes (tests/post_scenarios.py): the product's host entry
points (drfe_plane_voxel_grid, the host loop behind drfe_debug_plane_refit) against the oracle (oracle/post_oracle.cpp: std::sort
itself, a hand-written twister) bit for bit, the scenarios' own premises (the centroid bits do depend on std::sort's order; the
float64 definition holds), and the host predicate that says which inputs the device sorts may hand back.
tests/test_gpu_post_edges.py holds k_voxel_grid and k_plane_refit to the same scenarios."""
import numpy as np
import pytest

import post_scenarios as S


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _all_voxel_cases():
    return S.pattern_clouds() + S.geometric_cases() + S.job_list()[0]


def test_voxel_scenarios_equal_the_oracle_bit_for_bit(oracle_mod):
    """Every voxel scenario (8 key patterns x 20 sizes, the geometric edges, the 256-cloud job list) through
    drfe_plane_voxel_grid (the restated introsort) against the oracle, which calls std::sort: same number of leaves, same centroid
    bits.  Where the grid exceeds int32 both return the input cloud, and the scenarios state where that is."""
    from dr_slam_amd import lib
    kept = 0
    for c in _all_voxel_cases():
        a, b = lib.plane_voxel_grid(c.pts), oracle_mod.post_voxel_grid(c.pts)
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), c.name
        keeps = len(c.pts) > 0 and S.leaf_keys(c.pts) is None
        assert keeps == c.keeps_input, c.name
        if keeps:
            assert np.array_equal(_bits(b), _bits(c.pts)), c.name
            kept += 1
        elif len(c.pts):
            # the oracle's centroids are the sums in std::sort's order of the records the scenarios state
            import ctypes as C
            r = S.records_of(c.pts)
            assert lib.load().drfe_debug_order_sort(r.ctypes.data_as(C.c_void_p), len(r), 1, 0, -1, 0) == 0
            assert np.array_equal(_bits(S.centroids_in_order(c.pts, r)), _bits(b)), c.name
    assert kept == 2                                     # the geometric case and its copy in the job list


def test_voxel_scenarios_meet_the_float64_definition(oracle_mod):
    """The same scenarios against the float64 definition of tests/test_post_cpu.py (means of the leaves in ascending index
    order), with that test's bound of 2e-6, for the oracle and for the host entry point."""
    from dr_slam_amd import lib
    worst = 0.0
    for c in _all_voxel_cases():
        if c.keeps_input or not len(c.pts):
            continue
        ref = S.float64_definition(c.pts)
        for vg in (oracle_mod.post_voxel_grid, lib.plane_voxel_grid):
            vox = vg(c.pts)
            assert len(vox) == len(ref), c.name
            err = float(np.abs(vox - ref).max())
            worst = max(worst, err)
            assert err < 2e-6, (c.name, err)
    print(f"largest distance from the float64 definition: {worst:.3g}")


def test_centroid_bits_depend_on_the_sort_order(oracle_mod):
    """The premise of the bit-for-bit comparisons, proven on the reference alone: for every key pattern, adding a leaf's points
    in point-index order (what a stable sort would leave) gives other bits than the oracle's std::sort order in at least one
    leaf - so a wrong permutation of equal keys is visible in the centroids.  A scenario that fails this is vacuous and has to
    be changed."""
    per_pattern = {p: 0 for p in S.PATTERNS}
    clouds = {p: 0 for p in S.PATTERNS}
    for c in S.pattern_clouds():
        if len(c.pts) < 2:
            continue
        k = S.order_sensitive_leaves(c.pts, oracle_mod.post_voxel_grid(c.pts))
        per_pattern[c.pattern] += k
        clouds[c.pattern] += k > 0
        if len(c.pts) == 20000:
            assert k > 0, c.name                         # the one size above every threshold shows it in every pattern
    print("order-sensitive leaves per pattern:", per_pattern, "clouds:", clouds)
    for p in S.PATTERNS:
        assert per_pattern[p] > 0 and clouds[p] >= 2, (p, per_pattern[p], clouds[p])
    # the geometric edges with populated leaves show it too
    for c in S.geometric_cases():
        if c.name in ("negative coordinates", "straddling zero", "flat in z"):
            assert S.order_sensitive_leaves(c.pts, oracle_mod.post_voxel_grid(c.pts)) > 0, c.name


def test_refit_scenarios_equal_the_oracle_and_the_gates(oracle_mod):
    """Every refit scenario through the host loop (drfe_debug_plane_refit, on_device = 0: drfe_ahc_post_from_coarse) against the
    three gates written out in numpy followed by the oracle's MaxPointDistanceFromPlane: accepted flags, voxel counts and
    coefficient bits, and the outcomes the scenarios state by hand."""
    from dr_slam_amd import lib
    cases = S.refit_cases()
    assert {c.edge for c in cases} >= set(S.REFIT_EDGES)
    seen = {1: 0, 2: 0, 3: 0, None: 0}
    flips = 0
    for (maxd, th), idx in S.refit_groups(cases).items():
        post, status = lib.debug_plane_refit(None, False, np.array([cases[i].plane() for i in idx]), [cases[i].cloud for i in idx], maxd, th)
        assert (status[:-1] == 0).all() and status[-1] == -1
        for rec, i in zip(post, idx):
            c = cases[i]
            g = S.gates(c)
            seen[g] += 1
            coef, ok = c.coef(), False
            if g is None or g == 3:
                ok, fitted = oracle_mod.post_refit(coef, c.cloud, th)
                assert not (g == 3 and ok), c.name               # the oracle's own gate agrees with the numpy one
                if ok:
                    flips += int(np.sign(fitted[3]) == np.sign(coef[3]) and c.edge == "flip")
                    coef = fitted
            assert bool(rec["accepted"]) == ok and rec["n_voxels"] == len(c.cloud), c.name
            assert np.array_equal(_bits(rec["coef"]), _bits(coef)), c.name
            if c.accepted is not None:
                assert ok == c.accepted, c.name
    assert seen[1] == 1 and seen[2] == 1 and seen[3] == 1 and seen[None] > 30
    assert flips == 2                                    # both signs of the extractor's d keep their side


def test_refit_hook_counts_and_marks(oracle_mod):
    """vcounts_override: a count >= 0 replaces the cloud's on the host side too (99 of 150 voxels: gate 2), a negative one is the
    device's mark and leaves the host loop alone."""
    from dr_slam_amd import lib
    c = [k for k in S.refit_cases() if k.name == "n % 64 = 0 (128)"][0]
    planes, clouds = np.array([c.plane()] * 3), [c.cloud] * 3
    post, status = lib.debug_plane_refit(None, False, planes, clouds, 9.0, 0.05, vcounts_override=[99, -1, 100])
    assert list(status) == [0, 0, 0, -1]
    assert list(post["n_voxels"]) == [99, 128, 100] and list(post["accepted"]) == [0, 1, 1]
    ok, want = oracle_mod.post_refit(c.coef(), c.cloud[:100], 0.05)
    assert ok and np.array_equal(_bits(post[2]["coef"]), _bits(want))


def test_order_sort_heap_max_is_the_plain_transcription():
    """drfe_debug_order_sort_heap_max: the same permutation as drfe_debug_order_sort's mode 3 at every depth limit, for both record
    kinds; no range reaches the heap sort under a depth limit far above 2 lg n; at depth 0 the whole array does."""
    import ctypes as C
    from dr_slam_amd import lib
    L = lib.load()
    rng = np.random.default_rng(5)
    for kind, dt in ((0, np.uint32), (1, np.uint64)):
        for n in (0, 1, 16, 17, 100, 1024, 1025, 5000):
            bins = rng.integers(0, 40, n)
            idx = np.arange(n)
            recs = ((bins << 22) | idx).astype(dt) if kind == 0 else ((bins.astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)).astype(dt)
            lg = int(np.log2(max(1, n)))
            for depth in (-1, 0, 1, 3, 64, 2 * lg + 40):
                want = recs.copy()
                assert L.drfe_debug_order_sort(want.ctypes.data_as(C.c_void_p), n, kind, 3, depth, 0) == 0 or n == 0
                got, longest = lib.debug_order_sort_heap_max(recs, kind, depth)
                assert np.array_equal(got, want), (kind, n, depth)
                if depth >= 64:
                    assert longest == 0, (kind, n, depth)
                if depth == 0:
                    assert longest == (n if n > 16 else 0), (kind, n)
                assert longest <= n


def test_hand_back_share_of_the_voxel_scenarios():
    """From the host predicate alone (the longest range libstdc++'s introsort hands to std::__partial_sort; the device hands a
    cloud back if and only if it exceeds 1024 records): at most one natural-depth scenario in ten is a hand-back, and the
    forced-depth grid of tests/test_gpu_post_edges.py compares permutations in more than 200 cases - counting only clouds of more
    than 16 points, and separately those in which a range did reach the heap sort."""
    from dr_slam_amd import lib
    clouds = S.pattern_clouds()
    natural = [lib.debug_order_sort_heap_max(S.records_of(c.pts), 1)[1] for c in clouds]
    handed = [c.name for c, l in zip(clouds, natural) if l > S.ORD_HEAP_MAX]
    print("natural depth: handed back", handed, "; a range reached the heap sort in", sum(0 < l <= S.ORD_HEAP_MAX for l in natural))
    assert 1 <= len(handed) <= len(clouds) // 10
    assert sum(0 < l <= S.ORD_HEAP_MAX for l in natural) >= 5
    compared = heap = back = 0
    for c in clouds:
        n = len(c.pts)
        if n <= 16:
            continue
        for depth in S.forced_depths(n):
            l = lib.debug_order_sort_heap_max(S.records_of(c.pts), 1, depth)[1]
            back += l > S.ORD_HEAP_MAX
            compared += l <= S.ORD_HEAP_MAX
            heap += 0 < l <= S.ORD_HEAP_MAX
    print(f"forced depth: {compared} compare permutations ({heap} through the heap sort), {back} handed back")
    assert compared > 200 and heap > 200 and back > 50
    # the job list's marked clouds are what they are meant to be
    jobs, wide, pipe = S.job_list()
    assert S.leaf_keys(jobs[wide].pts) is None
    assert lib.debug_order_sort_heap_max(S.records_of(jobs[pipe].pts), 1)[1] > S.ORD_HEAP_MAX
    others = [lib.debug_order_sort_heap_max(S.records_of(c.pts), 1)[1] for k, c in enumerate(jobs) if k not in (wide, pipe) and len(c.pts)]
    assert max(others) <= S.ORD_HEAP_MAX
