"""GPU tests of the three Levenberg kernels (k_pose_opt, k_trans_opt, k_sim3_opt) on the hand-built degenerate systems of
tests/lm_edge_scenarios.py: the same bytes as the host entry and as the restatement on every scene alone;
the scenes of an optimiser in one call between plain ones, in three orders and as a 65-problem call; the hand-back counter rises
by exactly the scenes whose arguments the device cannot certify; a small call after one a chunk and an edge long on the same
buffers."""
import pytest

import lm_edge_scenarios as L
from dr_slam_amd import lib

pytestmark = pytest.mark.gpu
HOST = {"pose_opt": lib.pose_opt_host, "trans_opt": lib.trans_opt_host, "sim3_opt": lib.sim3_opt_host}
MAX_PER_CALL = 70


def _device(ctx, optimiser, P):
    return getattr(ctx, optimiser + "_batch")(P)


def _handed_back(ctx, optimiser):
    return getattr(ctx, optimiser + "_stats")()["handed_back"]


@pytest.mark.parametrize("optimiser", L.OPTIMISERS)
def test_every_scene_alone_and_its_hand_back(optimiser):
    """a fresh context: scene after scene, device == host == restatement, and the counter moves by one exactly at the scenes
    paths() says hold an argument outside the certificates' ranges"""
    m = L.MODULE[optimiser]
    c = lib.Context()
    try:
        differs, miscounted = [], []
        assert _handed_back(c, optimiser) == 0
        for name, sc in L.scenes(optimiser).items():
            P = m.pack([sc["scene"]])
            before = _handed_back(c, optimiser)
            d = _device(c, optimiser, P)
            want = L.expected_table(optimiser, [name])
            if m.tables_equal(d, HOST[optimiser](P)) or m.tables_equal(d, want):
                differs.append((name, m.tables_equal(d, want)))
            if _handed_back(c, optimiser) - before != L.hand_backs(optimiser, [name]):
                miscounted.append((name, _handed_back(c, optimiser) - before))
        assert differs == [] and miscounted == []
        assert _handed_back(c, optimiser) == L.hand_backs(optimiser, L.scenes(optimiser)) > 0
    finally:
        c.close()


@pytest.mark.parametrize("order", ("listed", "reversed", "by_trials", "listed_65"))
@pytest.mark.parametrize("optimiser", L.OPTIMISERS)
def test_scenes_between_plain_ones_in_one_call(optimiser, order):
    """workgroups that leave their loops after 2 to 132 trials side by side: every problem keeps the rows it has alone, the plain
    ones beside a handed-back one too, and the call hands back the scenes it must and nothing else"""
    m = L.MODULE[optimiser]
    names = list(L.scenes(optimiser))
    items = L.interleaved(optimiser, names, order.split("_65")[0])
    if order == "listed_65":                        # a second wavefront's worth of workgroups
        items += [(None, L.plain(optimiser, 600 + k)) for k in range(65 - len(items))]
        assert len(items) == 65
    assert len(items) <= MAX_PER_CALL
    P = m.pack([s for _, s in items])
    c = lib.Context()
    try:
        d = _device(c, optimiser, P)
        assert _handed_back(c, optimiser) == L.hand_backs(optimiser, names)
    finally:
        c.close()
    assert m.tables_equal(d, L.expected_table_of(optimiser, items)) == []
    assert m.tables_equal(d, HOST[optimiser](P)) == []


@pytest.mark.parametrize("big", ("negative", "seam"))
@pytest.mark.parametrize("optimiser", L.OPTIMISERS)
def test_a_small_call_after_a_257_edge_one(optimiser, big):
    """one edge more than a chunk (257 points, for Sim3 129 matches) of negative information, all of them or the last one alone;
    then twelve plain edges in the same slot; then the first again: neither the err scratch nor the flags of the larger call leak"""
    m = L.MODULE[optimiser]
    sim3 = optimiser == "sim3_opt"
    big = {"negative": "negative_129" if sim3 else "negative_257", "seam": "seam_match_128" if sim3 else "seam_point_256"}[big]
    small = L.plain(optimiser, 700, n=6 if sim3 else 12)
    A, B = m.pack([L.scenes(optimiser)[big]["scene"]]), m.pack([small])
    c = lib.Context()
    try:
        a1, b1, a2 = _device(c, optimiser, A), _device(c, optimiser, B), _device(c, optimiser, A)
        handed = _handed_back(c, optimiser)
    finally:
        c.close()
    want = L.expected_table(optimiser, [big])
    assert m.tables_equal(a1, want) == [] and m.tables_equal(a2, want) == []
    assert m.tables_equal(b1, L.expected_table_of(optimiser, [(None, small)])) == [] and m.tables_equal(b1, HOST[optimiser](B)) == []
    assert handed == 2 * L.hand_backs(optimiser, [big])
