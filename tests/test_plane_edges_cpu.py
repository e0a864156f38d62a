"""CPU tests of the hand-built plane-extractor scenarios (tests/plane_edge_scenarios.py): every scenario's precondition - the
property its docstring claims, proven from the oracle's outputs alone -, the host half of the product's AHC extractor
(drfe_planes_ahc_from_blocks: graph, clustering, membership, flood fill, re-merge, labels) against the oracle bit for bit on
every AHC scenario, and the oracle itself against the closed form where the scene has one.  tests/test_gpu_plane_edges.py holds
k_ahc_cluster / k_ahc_refine / k_ahc_labels_* and k_cape_frame to the same scenarios."""
import numpy as np
import pytest

import plane_edge_scenarios as S
from plane_scenarios import check_planes
from test_planes_analytic import AHC_TOL


def _ahc_frames():
    seen, out = set(), []
    for c in S.ahc_calls():
        for f in c.frames:
            if id(f) not in seen:
                seen.add(id(f))
                out.append((c, f))
    return out


def test_ahc_preconditions(oracle_mod):
    """Every AHC scenario has the property it claims (printed: the measured values the summary quotes)."""
    for c, f in _ahc_frames():
        print(f"{c.name} / {f.name}: {f.pre(f, S.ahc_oracle(oracle_mod, f))}")
    f = S.refused_frame()
    print(f"{f.name}: {f.pre(f, S.ahc_oracle(oracle_mod, f))}")
    # the union's list length follows from the short comb's layout: 3 columns x 47 rows of teeth beside flat blocks
    short = S.ahc_call("tum3_640x480").frames[0]
    assert short.info["teeth"] == 3 * 47 == 141 and 64 < 141 <= 376 and not short.to_host


def test_a_noisy_frame_fails_the_tie_precondition(oracle_mod):
    """The preconditions are what notices a scenario that lost its property: the tie wall with +-2 counts of plain noise instead
    of mirrored noise has no block MSEs equal as doubles."""
    noisy = S.tie_wall()
    noisy.depth = (noisy.depth.astype(np.int64) + np.random.default_rng(0).integers(-2, 3, noisy.depth.shape)).astype(np.uint16)
    with pytest.raises(AssertionError):
        S.tie_precondition(noisy, oracle_mod.ahc_planes(noisy.depth, noisy.K4, S.INV))


def test_cape_preconditions(oracle_mod):
    for c in S.cape_calls():
        for f in c.frames:
            print(f"{c.name} / {f.name}: {f.pre(f, S.cape_oracle(oracle_mod, f))}, expected hand-backs {S.cape_expected_to_host(oracle_mod, f)}")
    hb = {f.name for c in S.cape_calls() for f in c.frames if S.cape_expected_to_host(oracle_mod, f)}
    assert hb == {"cape_capacity", "cape_axis_wall_0"}


def _same(g, o):
    assert len(g["planes"]) == len(o["planes"])
    assert np.array_equal(g["planes"]["normal"].view(np.uint64), o["planes"][:, 0:3].view(np.uint64))
    assert np.array_equal(g["planes"]["center"].view(np.uint64), o["planes"][:, 3:6].view(np.uint64))
    assert np.array_equal(g["planes"]["mse"].view(np.uint64), o["planes"][:, 6].view(np.uint64))
    assert np.array_equal(g["planes"]["curvature"].view(np.uint64), o["planes"][:, 7].view(np.uint64))
    assert np.array_equal(g["planes"]["n_points"], o["N"]) and np.array_equal(g["planes"]["rid"], o["rid"])
    assert np.array_equal(g["seg"], o["seg"])
    assert len(g["members"]) == len(o["members"])
    for a, b in zip(g["members"], o["members"]):
        assert np.array_equal(a, b)


def test_ahc_host_stages_equal_the_oracle(oracle_mod):
    """drfe_planes_ahc_from_blocks on the oracle's block fits: plane records (uint64 views), n_points, rid, label image and member
    lists equal the oracle's on every AHC scenario.  At the cap the host does not truncate: planes_ahc_core returns
    DRFE_ERR_CAPACITY ("plane buffer too small") when the final plane count exceeds `cap`, and the same error above 254 planes
    whatever the cap (a CV_8U label image holds no more) - so a frame with 84 or 165 planes is compared with a cap that holds
    them and must be refused with cap = 64, and the 336-facet frame is refused with any cap."""
    from dr_slam_amd import lib
    for c, f in _ahc_frames():
        o = S.ahc_oracle(oracle_mod, f)
        n = len(o["planes"])
        g = lib.planes_ahc_from_blocks(o["blocks"], o["block_valid"], o["block_N"], f.depth, f.K4, S.INV, cap=max(64, n))
        _same(g, o)
        if n > 64:
            with pytest.raises(lib.DrfeError):
                lib.planes_ahc_from_blocks(o["blocks"], o["block_valid"], o["block_N"], f.depth, f.K4, S.INV, cap=64)
    f = S.refused_frame()
    o = S.ahc_oracle(oracle_mod, f)
    assert len(o["planes"]) > 254
    with pytest.raises(lib.DrfeError):
        lib.planes_ahc_from_blocks(o["blocks"], o["block_valid"], o["block_N"], f.depth, f.K4, S.INV, cap=512)


def test_oracle_finds_the_closed_form_planes(oracle_mod):
    """The grid-edge, switch and crease scenes have closed-form planes: the oracle must find them where they were put, with the
    bounds of tests/test_planes_analytic.py (0.5 degrees, 1.5 cm, labels exact beyond 1 px of a true boundary), unwidened.  The
    labels are compared inside the block grid: PEAC labels a pixel through a block or through the flood fill, which starts at
    borders between blocks of the grid, so the spare pixels right of / below the grid of a one-plane frame (19 x 400: nine
    columns) keep no label - in the reference as in the oracle."""
    checked = 0
    for c, f in _ahc_frames():
        if f.truth is None:
            continue
        o = S.ahc_oracle(oracle_mod, f)
        normals, centers = o["planes"][:, :3], o["planes"][:, 3:6]
        gh, gw = f.size[1] // S.WIN * S.WIN, f.size[0] // S.WIN * S.WIN
        check_planes(normals, np.einsum("ij,ij->i", normals, centers), o["seg"][:gh, :gw], f.truth[0], f.truth[1][:gh, :gw], **AHC_TOL)
        checked += 1
    assert checked >= 2 * len(S.GRID_EDGE_SIZES) + 2 * len(S.SWITCH_SIZES) + 2
