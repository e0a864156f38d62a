"""GPU tests of the device ORB extractor on the hand-built images of tests/orb_edge_scenarios.py: k_pyr_*, k_fast_cells /
k_fast_cells_cols<8|12>, k_quadtree<...>, k_blur and k_orient_desc at their ties, seams, thresholds and spill paths.  Every
scenario's pyramid and blurred bytes, FAST candidates per level, keypoint fields (float bit patterns) and descriptors with their
order are compared bit for bit with the CPU oracle, and drfe_batch_check(ctx) must be 0 after each.  tests/test_orb_edges_cpu.py
proves the scenarios' preconditions without a device.  No comparison here has a tolerance.

FAST contexts: `generic` = DRFE_FAST_GENERIC=1, `screen0|1|2` = DRFE_FAST_SCREEN, `3 levels` = a 160 x 120 context whose level 2 has
40-wide cells, so the whole geometry runs k_fast_cells without any variable (asserted with fast_partition and fast_cells).
Quadtree: one frame of one level runs k_quadtree<512,16,256> up to a quota of 252 and <512,16,1024> above.

Scenario: branch aimed at | precondition proven with the oracle | FAST kernel(s), quadtree instantiation
  ladder d = 7, 8, 20, 21, 255 on 0, 0 on 255 (160x120, 160x92): score d - 1 against minTh / iniTh | closed-form candidate list,
      score 254 | k_fast_cells (generic, 3 levels), cols<12> (160x120) and cols<8> (160x92) under screen 0 / 1 / 2; <512,16,1024>
  fallback, plateau h / v / d / a: threshold 7 only in a cell empty at 20; strict NMS on equal neighbours | [[14,25,99],[51,25,11]],
      [[25,17,11]], the pair alone nothing | the same five contexts; <512,16,1024>
  border: first / last evaluated row and column | the four keypoints at (19|w-20, 19|h-20) | the same
  sweep right / down / down_right / down_left, 64 frames each as one batch: strict NMS at every lane seam (pixel-pair halves,
      lane +- ncp, masked last column, rows past iInv) and cell seam | strong always, weak iff the strong one lies outside the
      evaluated area of the weak one's cell; every position of every cell visited | the same five contexts; <512,16,1024>
  screen_* (12 cells): every way through k_fast_cells_cols - unsampled rows, 7|8 and 42|43 of 64 sampled lanes at iniTh, 15|16 at
      minTh, restart after NMS (to the screened and to the plain way), dense, survivors above the list capacity at iniTh and at
      both thresholds | the restated sampling decisions give exactly these ways; the layout restatement equals drfe_orb_fast_cells,
      list capacity 592 < 704 pair rows | cols<12> under screen 0 / 1 / 2, k_fast_cells; <512,16,1024>.  The same at 160x92 less the
      two overflow cells (the list of cols<8> holds all 480 pair rows) | cols<8> under screen 0 / 1 / 2, k_fast_cells
  qt_tie (3), qt_lattice (11 quotas), qt_sort_ties (2), qt_roots (2, 400x150), qt_mid (6) and qt_on_line (4) on 160x120 and
      135x101: response ties in a node, equal node sizes, N + 1 .. N + 3 overshoot, erased roots, fractional hX, x < mx with the
      ceil for odd extents | which key is kept, 7 / 22 / 34 keypoints, distribute() on the closed form = the extraction |
      cols<12> / cols<8>, <512,16,256> (quota <= 252; qt_lattice_q200: <512,16,1024>)
  noise 640x480, nfeatures 2000: keys in registers and in global memory | 11753 candidates on level 0 > 8192 | cols<8|12>,
      <512,16,1024>
  batch of 72 frames, 8 levels: the register-key spill of the small variant | noise in slots 5 and 41 with 5793 / 4301 / 2890
      candidates on levels 2 - 4 > 2048; the other slots stage frames and a flat one | cols<8|12>, <512,16,256> on levels 0 - 1,
      <256,8,256> on levels 2 - 7
  angle_* (9): fastAtan2 on its axes and diagonals, atan2(0, 0) | the stated angles exactly | cols<12>, <512,16,1024>
  levels_* (5, 333x250, 8 levels): level lookup of k_orient_desc with empty levels | keypoints on levels [4,7] .. [0,1,2,4,7] |
      k_fast_cells (rows per lane above 12), <512,16,256>
  wave_1 .. wave_9: 1, 2, 3, 4, 5, 7, 8, 9 keypoints (DESC_KPW = 4), alone and in one batch with flat frames between | counts, own
      descriptor per keypoint | cols<12>, <512,16,1024>
  stage_* (7 frames at 333x250 and 640x480): no saturation in k_pyr_resize_tile and the 8.8 blur, reflection at every border |
      constants stay constant on every level | k_fast_cells / cols<8|12>, <512,16,256>
  batch of every one-level 160x120 frame, in builder order and reversed | each slot = its single-frame result = the oracle |
      cols<12>, <512,16,1024>"""
import numpy as np
import pytest

import orb_edge_scenarios as S

pytestmark = pytest.mark.gpu

FAST_ENVS = {"generic": ("DRFE_FAST_GENERIC", "1"), "screen0": ("DRFE_FAST_SCREEN", "0"), "screen1": ("DRFE_FAST_SCREEN", "1"),
             "screen2": ("DRFE_FAST_SCREEN", "2")}
_REF = {}


def _ref(orc, params, img):
    """The oracle's answer for a frame, computed once: keypoints, descriptors, and per level pyramid, blurred image and candidates
    (the oracle blurs only levels with keypoints; the device blurs all of them: the others come from the oracle's own blur)."""
    key = (params[:3], img.shape, img.tobytes())
    if key not in _REF:
        o = orc.OrbOracle(params[0], params[1], params[2], S.INI_TH, S.MIN_TH)
        kps, desc = o(img)
        pyr = [o.pyramid(l) for l in range(params[2])]
        blur = [o.blurred(l) for l in range(params[2])]
        blur = [b if b is not None else orc.gaussian_blur(p[S.EDGE:-S.EDGE, S.EDGE:-S.EDGE]) for b, p in zip(blur, pyr)]
        _REF[key] = dict(kps=kps, desc=desc, pyr=pyr, blur=blur, cand=[o.candidates(l) for l in range(params[2])])
    return _REF[key]


def _ctx(params, max_batch=1):
    from dr_slam_amd import lib
    return lib.Context(nfeatures=params[0], scale_factor=params[1], nlevels=params[2], max_width=params[3], max_height=params[4],
                       max_batch=max_batch)


def _same_kps(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in ("x", "y", "size", "angle", "response"):
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), (what, f)
    for f in ("octave", "class_id"):
        assert np.array_equal(a[f], b[f]), (what, f)


def _check_slot(ctx, slot, kps, desc, r, what, stages=True):
    if stages:
        for l in range(len(r["pyr"])):
            assert np.array_equal(ctx.pyramid_level(slot, l), r["pyr"][l]), (what, "pyramid level", l)
            assert np.array_equal(ctx.blurred_level(slot, l), r["blur"][l]), (what, "blurred level", l)
            assert np.array_equal(ctx.candidates(slot, l), r["cand"][l]), (what, "FAST candidates level", l)
    _same_kps(kps, r["kps"], what)
    assert np.array_equal(desc, r["desc"]), (what, "descriptors")


def _single(ctx, orc, s):
    for i, img in enumerate(s.images):
        kps, desc = ctx.orb_extract(img)
        _check_slot(ctx, 0, kps, desc, _ref(orc, s.params, img), (s.name, i))
        assert ctx.L.drfe_batch_check(ctx.h) == 0


def _batch(ctx, orc, params, images, what, stages=True):
    """The frames through one orb_extract_batch_ptr launch -> [(kps, desc)] per slot, each compared with the oracle."""
    import torch
    w, h = params[3:]
    gray = torch.from_numpy(np.stack(images)).cuda()
    ctx.orb_extract_batch_ptr(gray.data_ptr(), w * h, w, w, h, len(images), torch.cuda.current_stream().cuda_stream)
    counts = ctx.orb_counts(len(images))
    out = []
    for f, img in enumerate(images):
        r = _ref(orc, params, img)
        kps, desc = ctx.orb_download(f)
        assert counts[f] == len(r["kps"]), (what, f)
        _check_slot(ctx, f, kps, desc, r, (what, f), stages)
        out.append((kps, desc))
    assert ctx.L.drfe_batch_check(ctx.h) == 0
    return out


def _assert_table(ctx, w, h, params, generic_env):
    """The numpy restatement of the cell table and lane layout equals the library's, and so does the list capacity."""
    got = ctx.fast_cells(w, h)
    want = S.cell_table(w, h, params[1], params[2], generic_env)
    assert len(got) == len(want)
    for f in ("level", "x0", "y0", "ww", "wh", "offX", "offY", "cellIdx", "ncp", "rpl", "nrb", "kernel"):
        assert got[f].tolist() == [c[f] for c in want], f
    assert got["list_cap"].tolist() == [S.fastc_list_cap(want, c["kernel"]) if c["kernel"] else 0 for c in want]
    cells, _ = ctx.fast_partition(w, h)
    n12 = sum(c["kernel"] == 12 for c in want)
    assert cells.tolist() == [len(want) - n12, n12]
    return {c["kernel"] for c in want}


@pytest.mark.parametrize("env,w,h", [(e, w, h) for w, h in S.FAST_SIZES for e in FAST_ENVS] + [("3 levels", 160, 120)])
def test_fast_scores_thresholds_fallback(oracle_mod, monkeypatch, env, w, h):
    """Ladder, per-cell fallback, plateaus, detection border and the four NMS sweeps (64 frames each, one batch per direction) under
    the generic kernel by variable, the three screen modes and the generic kernel by geometry.  Level 0's candidates are also the
    closed form."""
    if env in FAST_ENVS:
        monkeypatch.setenv(*FAST_ENVS[env])
    nl = 3 if env == "3 levels" else 1
    params = (1000, 1.2, nl, w, h)
    ctx = _ctx(params, max_batch=64)
    try:
        kernels = _assert_table(ctx, w, h, params, env == "generic")
        assert kernels == ({0} if env in ("generic", "3 levels") else {12} if h == 120 else {8})
        for s in S.fast_scenarios(w, h):
            s.params = params
            _single(ctx, oracle_mod, s)
            assert np.array_equal(ctx.candidates(0, 0), S.dot_candidates(w, h, s.dots[0], s.expect.get("bg", S.BG))), s.name
        for name, d in S.SWEEP_DIRS:
            s = S.sweep_scenario(w, h, name, d)
            _batch(ctx, oracle_mod, params, s.images, s.name)
            for f, dots in enumerate(s.dots):
                assert np.array_equal(ctx.candidates(f, 0), S.dot_candidates(w, h, dots)), (s.name, f)
    finally:
        ctx.close()


@pytest.mark.parametrize("env,w,h", [(e, w, h) for w, h in S.SCREEN_SIZES for e in FAST_ENVS])
def test_screen_branches(oracle_mod, monkeypatch, env, w, h):
    """One cell per way through k_fast_cells_cols.  The restated layout must equal the library's table before the restated branch
    is relied on; then every scenario alone and all of them in one batch."""
    monkeypatch.setenv(*FAST_ENVS[env])
    params = (1000, 1.2, 1, w, h)
    scns = S.screen_scenarios(w, h)
    ctx = _ctx(params, max_batch=len(scns))
    try:
        kernels = _assert_table(ctx, w, h, params, env == "generic")
        row = ctx.fast_cells(w, h)[0]
        if env != "generic":
            pair_rows = row["ncp"] * (row["wh"] - 6)
            assert (kernels, row["list_cap"], pair_rows) == (({12}, 592, 704) if h == 120 else ({8}, 512, 480))
            mode = int(FAST_ENVS[env][1])
            cell = S.level_cells(w, h)[0]
            for s in scns:
                has = S.cell_has_corner_at_ini(_ref(oracle_mod, params, s.images[0])["cand"][0], cell)
                path, _ = S.cell_path(s.images[0], cell, mode, int(row["list_cap"]), has)
                assert path == ("plain" if mode == 0 else s.expect[f"path{mode}"]), s.name
                if s.dots is not None:
                    assert np.array_equal(_ref(oracle_mod, params, s.images[0])["cand"][0], S.dot_candidates(w, h, s.dots[0])), s.name
        for s in scns:
            _single(ctx, oracle_mod, s)
        _batch(ctx, oracle_mod, params, [s.images[0] for s in scns], "screen batch")
    finally:
        ctx.close()


def test_quadtree_ties_roots_midpoints(oracle_mod):
    """One-level dot fields: response ties, lattice ties at eleven quotas, the sort's creation-order ties, three roots with a
    fractional hX, midpoints."""
    made = {}
    try:
        for s in S.quadtree_scenarios():
            if s.params not in made:
                made[s.params] = _ctx(s.params)
            ctx = made[s.params]
            _single(ctx, oracle_mod, s)
            kps, _ = ctx.orb_extract(s.images[0])
            xy = sorted((int(x), int(y)) for x, y in zip(kps["x"], kps["y"]))
            if "kept" in s.expect:
                assert xy == sorted([s.expect["kept"], s.expect["weak"]]), s.name
            if "kept_set" in s.expect:
                assert xy == sorted(s.expect["kept_set"]), s.name
    finally:
        for c in made.values():
            c.close()


def test_quadtree_global_key_path(oracle_mod):
    """nfeatures = 2000 on the noise frame: k_quadtree<512,16,1024> with 11753 candidates on level 0, more than the 8192 keys its
    threads hold in registers."""
    from dr_slam_amd import synth
    g = synth.noise_frame(7, 640, 480)
    params = (2000, 1.2, 8, 640, 480)
    r = _ref(oracle_mod, params, g)
    assert len(r["cand"][0]) == 11753
    ctx = _ctx(params)
    try:
        kps, desc = ctx.orb_extract(g)
        _check_slot(ctx, 0, kps, desc, r, "noise, 2000 features")
        assert ctx.L.drfe_batch_check(ctx.h) == 0
    finally:
        ctx.close()


def test_quadtree_small_variant_spills(oracle_mod):
    """72 frames at 8 levels: levels 2 - 7 run k_quadtree<256,8,256>.  The noise frame sits in slots 5 and 41; its levels 2, 3 and 4
    have 5793, 4301 and 2890 candidates, more than the 2048 keys that variant holds in registers.  The other slots hold the
    640 x 480 stage frames and a flat one."""
    from dr_slam_amd import synth
    params = (1000, 1.2, 8, 640, 480)
    noise = synth.noise_frame(7, 640, 480)
    others = [s.images[0] for s in S.stage_scenarios(640, 480)] + [np.full((480, 640), 77, np.uint8)]
    frames = [others[i % len(others)] for i in range(72)]
    frames[5] = frames[41] = noise
    assert [len(c) for c in _ref(oracle_mod, params, noise)["cand"][2:5]] == [5793, 4301, 2890]
    ctx = _ctx(params, max_batch=72)
    try:
        _batch(ctx, oracle_mod, params, frames, "spill batch", stages=False)
        for f in (5, 41):
            for l in range(8):
                assert np.array_equal(ctx.candidates(f, l), _ref(oracle_mod, params, noise)["cand"][l]), (f, l)
    finally:
        ctx.close()


def test_orientation_levels_waves(oracle_mod):
    """fastAtan2's axes (the stated angles, exactly), frames whose keypoints skip levels, and every keypoint count modulo the four a
    wavefront of k_orient_desc carries - each alone, then the wave frames in one batch with a flat frame between them."""
    made = {}
    try:
        for s in S.orientation_scenarios() + S.level_scenarios() + S.wave_scenarios():
            if s.params not in made:
                made[s.params] = _ctx(s.params, max_batch=2 * len(S.WAVE_COUNTS))
            ctx = made[s.params]
            _single(ctx, oracle_mod, s)
            kps, _ = ctx.orb_extract(s.images[0])
            if "angle" in s.expect:
                assert len(kps) == 1 and kps["angle"][0] == s.expect["angle"], s.name
            if "levels" in s.expect:
                assert sorted(set(kps["octave"].tolist())) == s.expect["levels"], s.name
            if "n_keypoints" in s.expect:
                assert len(kps) == s.expect["n_keypoints"], s.name
        waves = S.wave_scenarios()
        flat = np.full((120, 160), S.BG, np.uint8)
        frames = [f for s in waves for f in (s.images[0], flat)]
        got = _batch(made[waves[0].params], oracle_mod, waves[0].params, frames, "wave batch")
        assert [len(k) for k, _ in got] == [n for c in S.WAVE_COUNTS for n in (c, 0)]
    finally:
        for c in made.values():
            c.close()


@pytest.mark.parametrize("w,h", S.STAGE_SIZES)
def test_stage_images_at_the_extremes(oracle_mod, w, h):
    """Pyramid and blurred bytes of every level on constant 0 / 255, checkerboards, stripes and corner impulses."""
    scns = S.stage_scenarios(w, h)
    ctx = _ctx(scns[0].params)
    try:
        for s in scns:
            _single(ctx, oracle_mod, s)
            if s.expect["constant"] is not None:
                for l in range(8):
                    assert (ctx.pyramid_level(0, l) == s.expect["constant"]).all() and (ctx.blurred_level(0, l) == s.expect["constant"]).all()
    finally:
        ctx.close()


def test_batch_equals_single_and_oracle(oracle_mod):
    """Every one-level 160 x 120 scenario frame in one launch, in builder order and reversed: each slot equals the oracle (all
    stages), its single-frame result and its slot of the other order."""
    scns = S.all_dot_scenarios()
    params = scns[0].params
    frames = [s.images[0] for s in scns]
    ctx = _ctx(params, max_batch=len(frames))
    try:
        alone = [ctx.orb_extract(f) for f in frames]
        fwd = _batch(ctx, oracle_mod, params, frames, "batch")
        back = _batch(ctx, oracle_mod, params, frames[::-1], "batch reversed")
        for (k0, d0), (k1, d1), (k2, d2) in zip(alone, fwd, back[::-1]):
            assert k0.tobytes() == k1.tobytes() == k2.tobytes() and d0.tobytes() == d1.tobytes() == d2.tobytes()
    finally:
        ctx.close()
