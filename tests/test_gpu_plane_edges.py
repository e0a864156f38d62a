"""GPU tests of the device plane extractors on the hand-built depth images of tests/plane_edge_scenarios.py: k_ahc_cluster /
k_ahc_refine (small and big forms) with the three k_ahc_labels_* kernels, and k_cape_frame, at their capacities, ties, grid
edges and hand-backs.  Every result is compared bit for bit with the CPU oracle and with the host-extractor path of the same
call, and the counters of the device path must show exactly the hand-backs each scenario was designed for: a frame built to
overflow a capacity that stays on the device misses its branch, a frame built to stay that is handed back is a finding.
tests/test_plane_edges_cpu.py proves the scenarios' preconditions without a device.  No comparison here has a tolerance.

Scenario: branch aimed at | precondition proven with the oracle | frames expected back from the device, of frames sent
  grid_edge 19x400 .. 70x70 (8 sizes): initGraph at j == Nw - 1 / i == Nh - 1 | all 40 .. 3072 blocks valid, one plane | 0 of 2 each
  switch 800x400 / 810x400 / 1000x600: NB <= 3200 | 3200 / 3240 / 6000 blocks, three planes | 0 of 2 each
  comb, 141 teeth: Lp + Lc > 64 | one plane, list 141 | 0;  comb, 1504 teeth: Lp > 376 | one plane, list 1504 | 1
  comb 1280x960, 6080 teeth: Lp > 1024 | one plane, list 6080 | 2 of 2
  tie_wall / tie_raised_pixel / tie_mirrored_noise 400x300: heap ties | 2502 / 1815 / 855 float-only ties, 92 / 0 / 1 double | 0
  tie_mirrored_noise 640x480: heap ties | 2195 float-only ties, 1 double | 1 (observed, cause inferred: see the builder)
  support_threshold: N >= 3000, dsSize * 100 >= 3000 | six planes with N == 3000, two 29-block facets without | 0
  crease vertical / diagonal: same-pixel chains | 48 of 48 crease blocks carry both labels | 0
  many_planes 640x480 / 1000x600: nFinal > 64 / nEx >= 128 | 84 / 165 planes | 1 / 2 of 2;  1280x960: 336 planes | refused alike
  mixed batch (ordered, reversed, one thread): hand-backs in mid-launch | each frame's own precondition | 3 of 8, three times
  cape_bin_tie | two bins of 384 | 0;  cape_seed_slip | literal seed 482, arg-min 481 | 0;  cape_four_cells | 4 candidates | 0
  cape_axis_wall 0 / 1 degree: Xq == 0 | 768 cells in bin 0; quotient exactly 0 / 0.106 | 1 (uncertified, as stated) / 0
  cape_capacity: S.np >= 63 | 80 planes | both of the two sent;  cape_cells 640 / 650 / 645 | 3072 / 3120 cells / w % patch | device / pool / refused"""
import numpy as np
import pytest

import plane_edge_scenarios as S

pytestmark = pytest.mark.gpu

MAXD, TH, THREADS = 9.0, 0.10, 4


@pytest.fixture(scope="module")
def ctx_of():
    """One context per image size, made when the size is first asked for."""
    from dr_slam_amd import lib
    made = {}

    def get(size):
        if size not in made:
            made[size] = lib.Context(max_batch=1)
        return made[size]
    yield get
    for c in made.values():
        c.close()


def _on_device(ctx, on):
    ctx.planes_configure_extractor(on_device=on)
    ctx.planes_configure(device_voxel_grid=1 if on else 0)


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _equals_oracle(rec, seg, o, members=None):
    assert len(rec) == len(o["planes"])
    for name, cols in (("normal", slice(0, 3)), ("center", slice(3, 6)), ("mse", 6), ("curvature", 7)):
        assert np.ascontiguousarray(rec[name]).tobytes() == np.ascontiguousarray(o["planes"][:, cols]).tobytes(), name
    assert np.array_equal(rec["n_points"], o["N"]) and np.array_equal(rec["rid"], o["rid"])
    assert seg.tobytes() == o["seg"].tobytes()
    if members is not None:
        assert len(members) == len(o["members"])
        for a, b in zip(members, o["members"]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _run_ahc(ctx, orc, frames, cap, n_threads=THREADS):
    """The frames through planes_ahc_post_batch (host path, then device path) and planes_ahc_batch (device path) -> the device
    results; every comparison and every counter delta of the module's docstring is asserted here."""
    depth, K4 = np.stack([f.depth for f in frames]), frames[0].K4
    B = len(frames)
    _on_device(ctx, False)
    ref = ctx.planes_ahc_post_batch(depth, K4, S.INV, MAXD, TH, cap=cap, n_threads=n_threads, seg=True)
    _on_device(ctx, True)
    s0 = ctx.planes_ahc_stats()
    got = ctx.planes_ahc_post_batch(depth, K4, S.INV, MAXD, TH, cap=cap, n_threads=n_threads, seg=True)
    s1 = ctx.planes_ahc_stats()
    mem = ctx.planes_ahc_batch(depth, K4, S.INV, cap=cap, n_threads=n_threads, members=True)
    s2 = ctx.planes_ahc_stats()
    for name, a, b in zip(("planes", "n_planes", "post", "n_accepted", "plane_num", "seg"), ref, got):
        assert a.tobytes() == b.tobytes(), name
    planes, n = got[0], got[1]
    for f, fr in enumerate(frames):
        o = S.ahc_oracle(orc, fr)
        _equals_oracle(planes[f, :n[f]], got[5][f], o)
        _equals_oracle(mem[f]["planes"], mem[f]["seg"], o, mem[f]["members"])
    to_host = sum(fr.to_host for fr in frames)
    kept = sum(len(S.ahc_oracle(orc, fr)["planes"]) for fr in frames if not fr.to_host)
    d1, d2 = _delta(s0, s1), _delta(s1, s2)
    print(f"{[fr.name for fr in frames]}: post batch {d1}, extractor batch {d2}")
    assert d1["frames"] == B and d1["to_host"] == to_host and d1["voxel_grids"] == kept, (d1, to_host, kept)
    assert d2["frames"] == B and d2["to_host"] == to_host and d2["voxel_grids"] == 0 and d2["voxel_grids_to_host"] == 0, (d2, to_host)
    return got, mem


@pytest.mark.parametrize("name", [c.name for c in S.ahc_calls() if c.name != "mixed_640x480"])
def test_ahc_scenarios(ctx_of, oracle_mod, name):
    """One call of each batch entry per image size and K: the grid edges (block grids 1, 2 and 3 wide or tall, spare pixels, 49
    blocks), the kernel switch (3200 blocks in the small form, 3240 and 6000 in the big one), the long-list union and both list
    caps (376 at 640 x 480, 1024 at 1280 x 960), the three tie frames, the support threshold, the creases and the frames with 84
    and 165 planes.  to_host is 0 except for the full combs, the many-plane frames and the 640 x 480 mirrored-noise wall (an
    observed hand-back: see its builder), which count one each."""
    call = S.ahc_call(name)
    _run_ahc(ctx_of(call.frames[0].size), oracle_mod, call.frames, call.cap)


def test_ahc_mixed_batch(ctx_of, oracle_mod):
    """[scene, full comb, no depth, 84 facets, scene, full comb, tie wall, scene]: three hand-backs in the middle of a launch.
    As ordered, reversed and with one host thread: every frame equals the oracle's answer for it and the host path's, whatever
    its neighbours in the launch are, and to_host is 3 each time.  Then every frame goes through the device path on its own (sent
    twice, as every lone scenario is): what the mixed launch returned for it is what that call returns."""
    call = S.ahc_call("mixed_640x480")
    ctx = ctx_of(call.frames[0].size)
    assert [f.to_host for f in call.frames] == [0, 1, 0, 1, 0, 1, 0, 0]
    first, _ = _run_ahc(ctx, oracle_mod, call.frames, call.cap)
    back, _ = _run_ahc(ctx, oracle_mod, call.frames[::-1], call.cap)
    one, _ = _run_ahc(ctx, oracle_mod, call.frames, call.cap, n_threads=1)
    for a, b, c in zip(first, back, one):
        assert a.tobytes() == b[::-1].tobytes() and a.tobytes() == c.tobytes()
    alone = {}
    for f, fr in enumerate(call.frames):
        key = fr.depth.tobytes()
        if key not in alone:                                   # the two combs are one image
            s0 = ctx.planes_ahc_stats()
            alone[key] = ctx.planes_ahc_post_batch(np.stack([fr.depth, fr.depth]), fr.K4, S.INV, MAXD, TH, cap=call.cap, n_threads=THREADS, seg=True)
            d = _delta(s0, ctx.planes_ahc_stats())
            assert d["frames"] == 2 and d["to_host"] == 2 * fr.to_host, (fr.name, d)
        for name, a, b in zip(("planes", "n_planes", "post", "n_accepted", "plane_num", "seg"), first, alone[key]):
            assert a[f].tobytes() == b[0].tobytes() == b[1].tobytes(), (fr.name, name)


def test_ahc_refusals_are_alike(ctx_of, oracle_mod):
    """What the host extractor does at the cap, it does for the device path too (planes_ahc_core: DRFE_ERR_CAPACITY, nothing is
    truncated): 84 planes with cap = 64, 336 planes (more than a CV_8U label image holds) with any cap, and an image narrower
    than one block - each refused by both entries in both modes, with the same code and message."""
    from dr_slam_amd import lib
    many, scene = S.ahc_call("tele_640x480").frames[3], S.ahc_call("tele_640x480").frames[1]
    big = S.refused_frame()
    assert len(S.ahc_oracle(oracle_mod, many)["planes"]) == 84 and len(S.ahc_oracle(oracle_mod, big)["N"]) == 336
    # the return code (DRFE_ERR_CAPACITY = -3, DRFE_ERR_INVALID = -1) and planes_ahc_core's / run_blocks' own message: the same
    # refusal from both entries in both modes, not any error (an allocation or a HIP failure reads differently)
    cases = [(np.stack([scene.depth, many.depth]), many.K4, 64, r"\(-3\): planes_ahc: plane buffer too small"),
             (np.stack([big.depth, big.depth]), big.K4, 512, r"\(-3\): planes_ahc: more planes than a CV_8U label image holds"),
             (np.zeros((2, 400, 9), np.uint16), S.K_TUM3, 64, r"\(-1\): planes_ahc: invalid argument")]
    for depth, K4, cap, why in cases:
        ctx = ctx_of((depth.shape[2], depth.shape[1]))
        for on in (False, True):
            _on_device(ctx, on)
            with pytest.raises(lib.DrfeError, match=why):
                ctx.planes_ahc_post_batch(depth, K4, S.INV, MAXD, TH, cap=cap, n_threads=2, seg=True)
            with pytest.raises(lib.DrfeError, match=why):
                ctx.planes_ahc_batch(depth, K4, S.INV, cap=cap, n_threads=2, members=True)
    # the context still works after the refusals
    _run_ahc(ctx_of(scene.size), oracle_mod, [scene, scene], 64)


@pytest.mark.parametrize("name", [c.name for c in S.cape_calls()])
def test_cape_scenarios(ctx_of, oracle_mod, name):
    """planes_cape_batch with CAPE::process on the device against the oracle (normal, mean, d as uint64; mse, score as uint32;
    n_points; label image) and against the same call on the host pool.  `frames` counts the call only where it qualifies for the
    device (not the 3120-cell frames; the 645-wide ones are refused alike in both modes); to_host is the number of frames built to exceed 63 segments plus the
    frames whose histogram quotient the oracle-side recomputation shows within 1e-9 of an integer (cape_axis_wall_0)."""
    call = next(c for c in S.cape_calls() if c.name == name)
    ctx = ctx_of((call.depth.shape[2], call.depth.shape[1]))
    depth = call.depth
    if call.refused:
        from dr_slam_amd import lib
        s0 = ctx.planes_cape_stats()
        for on in (False, True):
            ctx.planes_configure_cape(on)
            with pytest.raises(lib.DrfeError):
                ctx.planes_cape_batch(depth, call.K4, patch=call.patch, cap=call.cap, n_threads=THREADS, seg=True)
        assert _delta(s0, ctx.planes_cape_stats()) == dict(frames=0, to_host=0)
        return
    ctx.planes_configure_cape(False)
    ref = ctx.planes_cape_batch(depth, call.K4, patch=call.patch, cap=call.cap, n_threads=THREADS, seg=True)
    ctx.planes_configure_cape(True)
    s0 = ctx.planes_cape_stats()
    got = ctx.planes_cape_batch(depth, call.K4, patch=call.patch, cap=call.cap, n_threads=THREADS, seg=True)
    d = _delta(s0, ctx.planes_cape_stats())
    for a, b in zip(ref, got):
        assert a.tobytes() == b.tobytes()
    planes, n, seg = got
    for f, fr in enumerate(call.frames):
        o = S.cape_oracle(oracle_mod, fr)
        p = planes[f, :n[f]]
        assert n[f] == len(o["planes"]), (fr.name, int(n[f]), len(o["planes"]))
        for field, want in (("normal", o["planes"][:, 0:3]), ("mean", o["planes"][:, 3:6]), ("d", o["planes"][:, 6]), ("mse", o["MSE"]),
                            ("score", o["score"]), ("n_points", o["nr_pts"])):
            assert np.ascontiguousarray(p[field]).tobytes() == np.ascontiguousarray(want).tobytes(), (fr.name, field)
        assert seg[f].tobytes() == o["seg"].tobytes(), fr.name
    want = sum(S.cape_expected_to_host(oracle_mod, fr) for fr in call.frames) if call.device else 0
    print(f"{name}: {d}")
    assert d["frames"] == (len(call.frames) if call.device else 0) and d["to_host"] == want, (d, want)
