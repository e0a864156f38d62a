"""CPU tests of the hand-built ORB scenarios (tests/orb_edge_scenarios.py): every scenario's precondition - the property its
builder claims, proven with the CPU oracle (OrbOracle, its candidates / geom / quota / distribute / ic_angle) -, the numpy
restatements of the geometry against the oracle's, and the oracle itself against the closed form wherever a scenario has one.
tests/test_gpu_orb_edges.py holds the device kernels to the same scenarios."""
import numpy as np
import pytest

import orb_edge_scenarios as S

GEOMETRIES = ((160, 120, 1), (160, 92, 1), (160, 122, 1), (160, 120, 3), (400, 150, 1), (135, 101, 1), (333, 250, 8), (640, 480, 8))


def _oracle(orc, s):
    return orc.OrbOracle(s.params[0], s.params[1], s.params[2], S.INI_TH, S.MIN_TH)


def _xy(kps):
    return [(int(x), int(y)) for x, y in zip(kps["x"], kps["y"])]


@pytest.mark.parametrize("w,h,nl", GEOMETRIES)
def test_geometry_restatement_equals_the_oracle(oracle_mod, w, h, nl):
    """Level sizes, quotas, borders, cell grid: the numpy restatement the builders aim with is the oracle's geometry."""
    o = oracle_mod.OrbOracle(1000, 1.2, nl, S.INI_TH, S.MIN_TH)
    g = o.geometry(w, h)
    sizes = S.level_sizes(w, h, 1.2, nl)
    assert [tuple(r[:2]) for r in g] == sizes
    assert list(o.quota) == S.quotas(1000, 1.2, nl) and list(g[:, 2]) == list(o.quota)
    for l, (lw, lh) in enumerate(sizes):
        G = S.level_geom(lw, lh)
        assert (G["minB"], G["minB"], G["maxBX"], G["maxBY"], G["nCols"], G["nRows"], G["wCell"], G["hCell"]) == tuple(g[l][3:11])


def test_kernel_choice_of_the_scenario_sizes():
    """Which FAST kernel each scenario size runs (asserted against the library's own table by the GPU test): 160 x 120 with one level
    only <12>, 160 x 92 only <8>, 160 x 120 with three levels the generic kernel through level 2's 40-wide cells, and 333 x 250 with
    eight levels the generic kernel through rows per lane above 12."""
    assert {c["kernel"] for c in S.cell_table(160, 120)} == {12}
    assert {c["kernel"] for c in S.cell_table(160, 92)} == {8}
    t = S.cell_table(160, 120, 1.2, 3)
    assert {c["kernel"] for c in t} == {0} and max(c["ww"] - 6 for c in t if c["level"] == 2) == 40 > S.FASTC_MAX_EW
    assert all(c["rpl"] <= S.FASTC_MAX_RPL for c in t if c["level"] < 2)
    assert {c["kernel"] for c in S.cell_table(640, 480, 1.2, 8)} == {8, 12}
    assert {c["kernel"] for c in S.cell_table(333, 250, 1.2, 8)} == {0}
    assert {c["kernel"] for c in S.cell_table(160, 120, generic_env=True)} == {0}
    # the detection area of 160 x 120: 4 x 2 cells, x in [19, 140], y in [19, 100]
    c = S.level_cells(160, 120)
    assert len(c) == 8 and (c[0]["x0"] + 3, c[0]["y0"] + 3) == (19, 19)
    assert (c[-1]["x0"] + c[-1]["ww"] - 4, c[-1]["y0"] + c[-1]["wh"] - 4) == (140, 100)


@pytest.mark.parametrize("w,h", S.FAST_SIZES)
def test_fast_closed_forms(oracle_mod, w, h):
    """Threshold ladder, per-cell fallback, plateaus, detection border: the oracle's candidate list is the closed form, and the closed
    form is what the scenario states."""
    for s in S.fast_scenarios(w, h):
        o = _oracle(oracle_mod, s)
        kps, _ = o(s.images[0])
        c = o.candidates(0)
        assert np.array_equal(c, S.dot_candidates(w, h, s.dots[0], s.expect.get("bg", S.BG))), s.name
        e = s.expect
        if "n_candidates" in e:
            assert len(c) == e["n_candidates"] and (c[:, 2] == e["score"]).all(), s.name
        if "scores" in e:
            assert c[:, 2].tolist() == e["scores"], s.name
        if "xy" in e:
            assert _xy(kps) and sorted(_xy(kps)) == sorted(e["xy"]), s.name
    # the ladder's statement: d = 7 and d = 20 give nothing at their threshold, d = 8 is found through the fallback
    lad = {s.name.split("_")[1]: s for s in S.fast_scenarios(w, h) if s.name.startswith("ladder_d")}
    assert len(S.dot_candidates(w, h, lad["d7"].dots[0])) == 0
    assert (S.dot_candidates(w, h, lad["d20"].dots[0])[:, 2] == 19).all() and (S.dot_candidates(w, h, lad["d21"].dots[0])[:, 2] == 20).all()


@pytest.mark.parametrize("w,h", S.FAST_SIZES)
@pytest.mark.parametrize("name,direction", S.SWEEP_DIRS)
def test_nms_sweep(oracle_mod, w, h, name, direction):
    """64 frames per direction.  The oracle equals the closed form on every frame, and the closed form is the stated rule: a strong
    dot is a candidate iff a cell evaluates it, its weak neighbour iff a cell evaluates it and that cell does not evaluate the strong
    one.  Every position of every cell's evaluated area is visited by a strong dot."""
    s = S.sweep_scenario(w, h, name, direction)
    o = _oracle(oracle_mod, s)
    cells = S.level_cells(w, h)
    owner = np.full((h, w), -1)
    for k, c in enumerate(cells):
        owner[c["y0"] + 3:c["y0"] + c["wh"] - 3, c["x0"] + 3:c["x0"] + c["ww"] - 3] = k
    visited = np.zeros((h, w), bool)
    n_weak = 0
    for img, dots in zip(s.images, s.dots):
        o(img)
        got = o.candidates(0)
        assert np.array_equal(got, S.dot_candidates(w, h, dots))
        have = {(x + 16, y + 16): r for x, y, r in got.tolist()}
        for (sx, sy, _), (wx, wy, _) in zip(dots[0::2], dots[1::2]):
            visited[sy, sx] = True
            assert ((sx, sy) in have) == (owner[sy, sx] >= 0)
            weak = owner[wy, wx] >= 0 and owner[wy, wx] != owner[sy, sx]
            assert ((wx, wy) in have) == weak, (sx, sy)
            n_weak += weak
    assert visited[owner >= 0].all() and n_weak > 0
    if (w, h, name) == (160, 120, "right"):
        # the seam between level columns 50 and 51: both are emitted there, one column to either side only the strong one
        seen = {}
        for img, dots in zip(s.images, s.dots):
            for (sx, sy, _) in dots[0::2]:
                if sy == 40 and sx in (49, 50, 51):
                    o(img)
                    seen[sx] = [r for r in o.candidates(0).tolist() if r[1] == 24 and sx - 16 <= r[0] <= sx - 15]
        assert seen == {49: [[33, 24, 99]], 50: [[34, 24, 99], [35, 24, 79]], 51: [[35, 24, 99]]}


def test_generic_geometry_scenarios(oracle_mod):
    """The 160 x 120 frames through a three-level context (the whole geometry runs k_fast_cells): level 0 still has the closed-form
    candidates."""
    for s in S.fast_scenarios(160, 120):
        o = oracle_mod.OrbOracle(1000, 1.2, 3, S.INI_TH, S.MIN_TH)
        o(s.images[0])
        assert np.array_equal(o.candidates(0), S.dot_candidates(160, 120, s.dots[0], s.expect.get("bg", S.BG))), s.name


@pytest.mark.parametrize("w,h", S.SCREEN_SIZES)
def test_screen_scenarios_take_the_way_they_are_built_for(oracle_mod, w, h):
    """One cell per way through k_fast_cells_cols: the restated sampling decisions say which way cell 0 goes under DRFE_FAST_SCREEN
    2 and 1, with the sampled counts printed.  Whether the cell has a corner at iniTh comes from the oracle.  At 160 x 120 the cell
    runs the 12-row instantiation and can overflow its list (592 entries for 704 pair rows); at 160 x 92 the 8-row one, whose list
    holds every pair row."""
    big = (w, h) == (160, 120)
    table = S.cell_table(w, h)
    cap = S.fastc_list_cap(table, 12 if big else 8)
    cell = S.level_cells(w, h)[0]
    pair_rows = cell["ncp"] * (cell["wh"] - 6)
    assert (cap, pair_rows) == ((592, 704) if big else (512, 480))
    scns = S.screen_scenarios(w, h)
    seen2, seen1 = set(), set()
    for s in scns:
        o = _oracle(oracle_mod, s)
        o(s.images[0])
        c = o.candidates(0)
        in0 = c[(c[:, 0] + 16 < cell["x0"] + cell["ww"] - 3) & (c[:, 1] + 16 < cell["y0"] + cell["wh"] - 3)]
        assert len(in0) == len(c) or s.dots is None                    # the other cells are flat
        has = S.cell_has_corner_at_ini(c, cell)
        assert has == bool((in0[:, 2] >= S.INI_TH).any())
        p2, f2 = S.cell_path(s.images[0], cell, 2, cap, has)
        p1, _ = S.cell_path(s.images[0], cell, 1, cap, has)
        p0, _ = S.cell_path(s.images[0], cell, 0, cap, has)
        print(f"{s.name}: screen 2 -> {p2}, screen 1 -> {p1}; (nS, nAll, survivors) {f2}; {len(in0)} candidates")
        assert (p2, p1, p0) == (s.expect["path2"], s.expect["path1"], "plain"), s.name
        if s.dots is not None:
            assert np.array_equal(c, S.dot_candidates(w, h, s.dots[0])), s.name
        seen2.add(p2)
        seen1.add(p1)
    over = {"ini_overflow>plain", "ini_overflow>min_overflow>plain"} if big else set()
    assert seen2 == {"ini", "min", "plain", "ini>min", "ini>plain"} | over
    assert seen1 == {"min", "plain"} | ({"min_overflow>plain"} if big else set())
    # the sampled fractions sit on either side of each bound by one lane
    by = {s.name[7:].replace(f"_{w}x{h}", ""): S.cell_path(s.images[0], cell, 2, cap, True)[1] for s in scns}
    assert by["ini_low_out"]["ini"][:2] == (7, 64) and by["ini_low_in"]["ini"][:2] == (8, 64)
    assert by["ini_high_in"]["ini"][:2] == (42, 64) and by["ini_high_out"]["ini"][:2] == (43, 64)
    assert by["min_in"]["min"][:2] == (15, 64) and by["min_out"]["min"][:2] == (16, 64)
    assert by["unsampled_rows"]["ini"][0] == 0 and by["unsampled_rows"]["ini"][2] > 0
    assert by["dense"]["ini"] == (64, 64, pair_rows)
    if big:
        assert by["overflow_ini"]["ini"][2] > cap and by["overflow_both"]["min"][2] > cap


def test_quadtree_scenarios(oracle_mod):
    """Every quadtree scenario: the candidate list is the closed form, OrbOracle.distribute on that list gives the keypoints of the
    full extraction in its order, and the stated outcomes hold: which of two equal responses is kept, the lattice's overshoot
    counts, the keys kept around a split line."""
    counts = {}
    for s in S.quadtree_scenarios():
        w, h = s.params[3:]
        o = _oracle(oracle_mod, s)
        kps, _ = o(s.images[0])
        cf = S.dot_candidates(w, h, s.dots[0])
        assert np.array_equal(o.candidates(0), cf), s.name
        g = S.level_geom(w, h)
        sel = o.distribute(cf, g["minB"], g["maxBX"], g["minB"], g["maxBY"], s.params[0])
        assert _xy(kps) == [(x + g["minB"], y + g["minB"]) for x, y in cf[sel][:, :2].tolist()], s.name
        assert kps["response"].tolist() == cf[sel][:, 2].tolist(), s.name
        e = s.expect
        if "kept" in e:
            assert sorted(_xy(kps)) == sorted([e["kept"], e["weak"]]), s.name
        if "kept_set" in e:
            assert sorted(_xy(kps)) == sorted(e["kept_set"]), s.name
        if "n_candidates" in e:
            assert len(cf) == e["n_candidates"]
            counts[s.params[0]] = len(kps)
    assert (counts[7], counts[20], counts[33]) == (7, 22, 34)
    assert counts[117] == counts[200] == 117 and all(counts[q] >= min(q, 4) for q in counts)
    # roots: one scenario has keys in the middle root only, the other on either side of both root seams and in the last column
    by = {s.name: s for s in S.quadtree_scenarios()}
    g = S.level_geom(400, 150)
    roots = lambda s: [int(np.float32(x - g["minB"]) / g["hX"]) for x, _, _ in s.dots[0]]
    assert set(roots(by["qt_roots_one"])) == {1}
    r = roots(by["qt_roots_seams"])
    # the column int(hX * i), where root i's corner is put, still bins to root i - 1 (x / hX with hX = 122.67): [xs - 1, xs, xs + 1]
    assert r[:6] == [0, 0, 1, 1, 1, 2] and r[6:9] == [2, 2, 2] and max(x for x, _, _ in by["qt_roots_seams"].dots[0]) == g["maxBX"] - 4
    # midpoints: a key on either side of each split line of the first three rounds, and one on the line
    for w, h in ((160, 120), (135, 101)):
        G = S.level_geom(w, h)
        W = G["maxBX"] - G["minB"]
        xs = {x - G["minB"] for x, _, _ in by[f"qt_mid_{w}x{h}_q5"].dots[0]}
        half = int(np.ceil(W / 2))
        assert {half - 1, half + 1, half} <= xs and (W % 2 == 1) == (w == 135)


def test_orientation_on_the_axes(oracle_mod):
    """Exact float equality with the stated angles; ic_angle on the level gives the keypoint's angle."""
    for s in S.orientation_scenarios():
        o = _oracle(oracle_mod, s)
        kps, _ = o(s.images[0])
        assert len(kps) == 1 and _xy(kps) == [(80, 60)], s.name
        assert kps["angle"][0] == s.expect["angle"], (s.name, kps["angle"][0])
        pyr = o.pyramid(0)
        assert np.float32(o.ic_angle(pyr, 80 + 19, 60 + 19)) == kps["angle"][0]
    assert len({float(s.expect["angle"]) for s in S.orientation_scenarios()}) == 8        # alone and (+8, 0) are both 0


def test_level_and_wave_scenarios(oracle_mod):
    lists = []
    for s in S.level_scenarios():
        kps, _ = _oracle(oracle_mod, s)(s.images[0])
        lv = sorted(set(kps["octave"].tolist()))
        assert lv == s.expect["levels"], (s.name, lv)
        lists.append(lv)
    gap = lambda lv: any(b - a > 1 for a, b in zip(lv, lv[1:]))
    assert any(gap(lv) and lv[0] == 0 for lv in lists) and any(lv[0] > 0 for lv in lists) and all(gap(lv) for lv in lists)
    angles = set()
    for s in S.wave_scenarios():
        kps, desc = _oracle(oracle_mod, s)(s.images[0])
        assert len(kps) == s.expect["n_keypoints"], s.name
        assert len({d.tobytes() for d in desc}) == len(kps)            # every keypoint has its own descriptor
        angles |= set(kps["angle"].tolist())
    assert [s.expect["n_keypoints"] % 4 for s in S.wave_scenarios()] == [1, 2, 3, 0, 1, 3, 0, 1] and len(angles) == 9


@pytest.mark.parametrize("w,h", S.STAGE_SIZES)
def test_stage_extremes(oracle_mod, w, h):
    """Constant 0 and 255 stay constant on every level and under the blur; the other frames hold 0 and 255 side by side."""
    for s in S.stage_scenarios(w, h):
        o = _oracle(oracle_mod, s)
        kps, _ = o(s.images[0])
        const = s.expect["constant"]
        if const is None:
            assert s.images[0].min() == 0 and s.images[0].max() == 255
            continue
        assert len(kps) == 0
        for l in range(8):
            p = o.pyramid(l)
            assert (p == const).all(), (s.name, l)
            assert (oracle_mod.gaussian_blur(p[19:-19, 19:-19]) == const).all(), (s.name, l)


def test_spill_preconditions(oracle_mod):
    """The noise frame's candidate counts against the key registers of the quadtree instantiations: level 0 above the 512 x 16 keys
    of k_quadtree<512,16,*>, levels 2 to 4 above the 256 x 8 keys of k_quadtree<256,8,256>."""
    from dr_slam_amd import synth
    g = synth.noise_frame(7, 640, 480)
    o = oracle_mod.OrbOracle(2000, 1.2, 8, S.INI_TH, S.MIN_TH)
    o(g)
    assert len(o.candidates(0)) == 11753 > 512 * 16 and max(o.quota) + 4 > 256
    o = oracle_mod.OrbOracle()
    o(g)
    assert [len(o.candidates(l)) for l in (2, 3, 4)] == [5793, 4301, 2890] and 2890 > 256 * 8
    sizes = S.level_sizes(640, 480, 1.2, 8)
    assert all(lw * lh <= 160000 for lw, lh in sizes[2:]) and sizes[1][0] * sizes[1][1] > 160000 and max(o.quota) + 4 <= 256
