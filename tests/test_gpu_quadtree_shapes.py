"""GPU tests of every k_quadtree instantiation (DRFE_QT_INSTANCES) and of the plan that picks them, bit for bit against the CPU
oracle with the comparison of tests/test_gpu_orb_edges.py (pyramid, blur, candidates, keypoint bit patterns, descriptors and their
order); drfe_batch_check(ctx) == 0 after every case.  DRFE_QT_FORCE=<threads>,<kpt> forces one instantiation on every level it is
legal for; lib.quadtree_plan tells, without a device, which one a level really runs, and each case asserts it.

  scenarios: response ties, lattice ties at eleven quotas, sort ties, three roots, midpoints (orb_edge_scenarios.quadtree_scenarios)
      through <512,16,*>, <256,12,256> and, where the quota leaves kpCap <= 128, the wavefront <64,20,128>
  wave boundary: nfeatures 124 (kpCap 128) runs <64,20,128>, 125 (kpCap 129) does not
  register / global seam of the wavefront instance: 1280 = 64 x 20 and 1281 candidates (dot lattice), and a noise frame far above
  empty (flat frame) and single (one dot) levels through every instantiation
  mixed batch: 8 frames x 8 levels at 640x480 as the library plans them (one launch) and with the plan of a 512-frame batch forced
      level by level (every instantiation of that plan in one batch)"""
import numpy as np
import pytest

import orb_edge_scenarios as S
import test_gpu_orb_edges as E

pytestmark = pytest.mark.gpu

FORCES = [(512, 16), (256, 12), (64, 20)]
WAVE = (64, 20)


def _runs(params, nframes, force):
    from dr_slam_amd import lib
    return [(r["threads"], r["kpt"]) for r in lib.quadtree_plan(params[3], params[4], params[0], params[1], params[2], nframes, force)]


def _lattice(w, h, n, step=6):
    """The first n dots (row-major) of a lattice with `step` pixels between dots, well inside the evaluated area."""
    pts = [(x, y, S.BG + 100) for y in range(S.EDGE + 6, h - S.EDGE - 6, step) for x in range(S.EDGE + 6, w - S.EDGE - 6, step)]
    assert len(pts) >= n
    return pts[:n]


@pytest.mark.parametrize("threads,kpt", FORCES)
def test_scenarios_through_every_instantiation(oracle_mod, monkeypatch, threads, kpt):
    force = f"{threads},{kpt}"
    monkeypatch.setenv("DRFE_QT_FORCE", force)
    made, ran = {}, 0
    try:
        for s in S.quadtree_scenarios():
            if _runs(s.params, 1, force) != [(threads, kpt)]:
                assert (threads, kpt) == WAVE and s.params[0] > 124, s.name      # the only pair a one-level scenario can refuse
                continue
            if s.params not in made:
                made[s.params] = E._ctx(s.params)
            E._single(made[s.params], oracle_mod, s)
            ran += 1
    finally:
        for c in made.values():
            c.close()
    assert ran >= 26


@pytest.mark.parametrize("nfeatures,wave", [(124, True), (125, False)])
def test_wave_boundary(oracle_mod, monkeypatch, nfeatures, wave):
    from dr_slam_amd import synth
    monkeypatch.setenv("DRFE_QT_FORCE", "64,20")
    params = (nfeatures, 1.2, 1, 160, 120)
    g = synth.noise_frame(7, 160, 120)
    r = E._ref(oracle_mod, (125, 1.2, 1, 160, 120), g)
    assert len(r["kps"]) >= 125
    assert (_runs(params, 1, "64,20") == [WAVE]) == wave
    ctx = E._ctx(params)
    try:
        kps, desc = ctx.orb_extract(g)
        E._check_slot(ctx, 0, kps, desc, E._ref(oracle_mod, params, g), ("wave boundary", nfeatures))
        assert ctx.L.drfe_batch_check(ctx.h) == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("what", ["exact", "plus_one", "noise"])
def test_wave_register_global_seam(oracle_mod, monkeypatch, what):
    from dr_slam_amd import synth
    monkeypatch.setenv("DRFE_QT_FORCE", "64,20")
    w, h = 333, 250
    params = (100, 1.2, 1, w, h)
    assert _runs(params, 1, "64,20") == [WAVE]
    cap = WAVE[0] * WAVE[1]
    if what == "noise":
        g = synth.noise_frame(7, w, h)
        assert len(E._ref(oracle_mod, params, g)["cand"][0]) > 2 * cap
    else:
        n = cap + (what == "plus_one")
        dots = _lattice(w, h, n)
        assert S.dots_are_independent(dots)
        g = S.dot_image(w, h, dots)
        assert len(E._ref(oracle_mod, params, g)["cand"][0]) == n
    ctx = E._ctx(params)
    try:
        kps, desc = ctx.orb_extract(g)
        E._check_slot(ctx, 0, kps, desc, E._ref(oracle_mod, params, g), ("wave seam", what))
        assert ctx.L.drfe_batch_check(ctx.h) == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("threads,kpt", FORCES)
def test_empty_and_single(oracle_mod, monkeypatch, threads, kpt):
    force = f"{threads},{kpt}"
    monkeypatch.setenv("DRFE_QT_FORCE", force)
    params = (100, 1.2, 1, 160, 120)
    assert _runs(params, 1, force) == [(threads, kpt)]
    ctx = E._ctx(params)
    try:
        for name, dots, n in (("flat", [], 0), ("single", [(80, 60, S.BG + 100)], 1)):
            g = S.dot_image(160, 120, dots)
            r = E._ref(oracle_mod, params, g)
            assert len(r["cand"][0]) == n and len(r["kps"]) == n
            kps, desc = ctx.orb_extract(g)
            E._check_slot(ctx, 0, kps, desc, r, (name, force))
            assert ctx.L.drfe_batch_check(ctx.h) == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("plan", ["own", "of_512_frames"])
def test_mixed_batch(oracle_mod, monkeypatch, plan):
    """Stage frames, a flat frame and the noise frame in one launch: every slot equals the oracle and its single-frame result."""
    from dr_slam_amd import synth
    params = (1000, 1.2, 8, 640, 480)
    if plan == "of_512_frames":
        big = _runs(params, 512, None)
        force = ";".join(f"{t},{k}" for t, k in big)
        monkeypatch.setenv("DRFE_QT_FORCE", force)
        assert _runs(params, 8, force) == big and len(set(big)) >= 2
    else:
        assert set(_runs(params, 8, None)) == {(512, 16)}
    frames = [s.images[0] for s in S.stage_scenarios(640, 480)][:6] + [np.full((480, 640), 77, np.uint8), synth.noise_frame(7, 640, 480)]
    assert len(frames) == 8
    ctx = E._ctx(params, max_batch=8)
    try:
        alone = [ctx.orb_extract(f) for f in frames]
        got = E._batch(ctx, oracle_mod, params, frames, ("mixed batch", plan), stages=False)
        for (k0, d0), (k1, d1) in zip(alone, got):
            assert k0.tobytes() == k1.tobytes() and d0.tobytes() == d1.tobytes()
    finally:
        ctx.close()
