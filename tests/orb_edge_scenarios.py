"""Hand-built images for the ORB extractor's decisions that rendered rooms and noise meet by chance or never: equal FAST scores
side by side, corners on cell seams and on the detection border, one cell per way through k_fast_cells_cols, equal responses in
one quadtree node, moments on the axes of fastAtan2, empty pyramid levels, every keypoint count modulo the descriptor kernel's
wave grouping, and stage images at 0 / 255.  numpy only: tests/test_orb_edges_cpu.py proves each scenario's precondition with the
CPU oracle, tests/test_gpu_orb_edges.py holds the device path to the oracle on the same images.

The building block is the DOT: one pixel of value BG + d on a flat background BG.  Its 16-pixel ring is all background, so it is a
FAST corner of score |d| - 1, and a corner at threshold t iff |d| - 1 >= t; no other pixel near it has a contiguous 9-arc.  Dots
whose offset is not a ring offset do not change each other's score (adjacent dots included), so a dot field fixes the candidate
list the quadtree sees.  `dot_candidates` is the closed form: the reference's per-cell FAST (threshold 20, strict 3x3 maximum inside
the cell's evaluated area, threshold 7 if the cell came out empty; ORBextractor.cc:789-829) restated on the sparse score map."""
from dataclasses import dataclass, field

import numpy as np

BG = 100
EDGE = 19
INI_TH, MIN_TH = 20, 7
FASTC_MAX_EW, FASTC_MAX_RPL = 38, 12
RING = {(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)}


@dataclass
class Scn:
    name: str
    images: list                       # uint8 [h, w] each
    params: tuple                      # (nfeatures, scale_factor, nlevels, w, h)
    branch: str
    dots: list = None                  # per image [(x, y, value)]: the closed form applies (level 0)
    expect: dict = field(default_factory=dict)


# ---------------------------------------------------------------------------------------------------------------------------
# geometry restated (orb_geometry.cpp: drfe_build_tables / drfe_build_geometry; ORBextractor.cc:410-446, :773-806)

def level_sizes(w, h, scale_factor=1.2, nlevels=1):
    sc = [np.float32(1)]
    for _ in range(1, nlevels):
        sc.append(np.float32(np.float64(sc[-1]) * np.float64(np.float32(scale_factor))))
    out = []
    for s in sc:
        inv = np.float32(1) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


def quotas(nfeatures, scale_factor=1.2, nlevels=1):
    factor = np.float32(1.0 / np.float64(np.float32(scale_factor)))
    want = np.float32(nfeatures) * (np.float32(1) - factor) / (np.float32(1) - np.float32(np.float64(factor) ** nlevels))
    q, total = [], 0
    for _ in range(nlevels - 1):
        q.append(int(np.rint(want)))
        total += q[-1]
        want = np.float32(want * factor)
    q.append(max(nfeatures - total, 0))
    return q


def level_geom(lw, lh):
    """-> dict(minB, maxBX, maxBY, nCols, nRows, wCell, hCell, nIni, hX) of a level of lw x lh pixels."""
    minB, maxBX, maxBY = EDGE - 3, lw - EDGE + 3, lh - EDGE + 3
    width, height = maxBX - minB, maxBY - minB
    nCols, nRows = int(np.float32(width) / np.float32(30)), int(np.float32(height) / np.float32(30))
    wCell, hCell = int(np.ceil(np.float32(width) / np.float32(nCols))), int(np.ceil(np.float32(height) / np.float32(nRows)))
    nIni = int(np.floor(np.float32(width) / np.float32(height) + np.float32(0.5)))        # std::round of a positive float
    return dict(minB=minB, maxBX=maxBX, maxBY=maxBY, nCols=nCols, nRows=nRows, wCell=wCell, hCell=hCell, nIni=nIni,
                hX=np.float32(width) / np.float32(nIni))


def level_cells(lw, lh, level=0):
    """The FAST cells of a level in the reference's loop order, with the lane layout of k_fast_cells_cols (orb_geometry.cpp:236-241):
    ncp column pairs, rpl rows per lane, nrb row blocks.  (x0, y0, ww, wh) is the cv::FAST window in level coordinates; its evaluated
    area is the window less 3 pixels on every side."""
    g = level_geom(lw, lh)
    cells = []
    for i in range(g["nRows"]):
        iniY = g["minB"] + i * g["hCell"]
        maxY = min(iniY + g["hCell"] + 6, g["maxBY"])
        if iniY >= g["maxBY"] - 3:
            continue
        for j in range(g["nCols"]):
            iniX = g["minB"] + j * g["wCell"]
            maxX = min(iniX + g["wCell"] + 6, g["maxBX"])
            if iniX >= g["maxBX"] - 6:
                continue
            ww, wh = maxX - iniX, maxY - iniY
            if ww < 7 or wh < 7:
                continue
            ew, eh = ww - 6, wh - 6
            ncp = (ew + 1) // 2
            nrb0 = min(64 // ncp, eh)
            rpl = (eh + nrb0 - 1) // nrb0
            nrb = (eh + rpl - 1) // rpl
            cells.append(dict(level=level, x0=iniX, y0=iniY, ww=ww, wh=wh, offX=j * g["wCell"], offY=i * g["hCell"],
                              cellIdx=i * g["nCols"] + j, ncp=ncp, rpl=rpl, nrb=nrb))
    return cells


def cell_table(w, h, scale_factor=1.2, nlevels=1, generic_env=False):
    """The launch-order cell table of a frame: cells of at most 8 rows per lane first (stable), `kernel` = 8 / 12 for the two
    k_fast_cells_cols instantiations or 0 for k_fast_cells, which takes the whole geometry as soon as one cell has an evaluated width
    above 38 or more than 12 rows per lane, or when DRFE_FAST_GENERIC=1."""
    cells = [c for l, (lw, lh) in enumerate(level_sizes(w, h, scale_factor, nlevels)) for c in level_cells(lw, lh, l)]
    cols = all(c["ww"] - 6 <= FASTC_MAX_EW and c["rpl"] <= FASTC_MAX_RPL for c in cells) and not generic_env
    cells = [c for c in cells if c["rpl"] <= 8] + [c for c in cells if c["rpl"] > 8]
    for c in cells:
        c["kernel"] = (8 if c["rpl"] <= 8 else 12) if cols else 0
    return cells


def fastc_list_cap(cells, kernel):
    """Survivor-list capacity of a k_fast_cells_cols launch (orb_kernels.hip: fastc_list_off / fastc_list_cap): at least 320 entries,
    and what the 1280-byte LDS granule leaves behind them, up to every pair row of a wavefront."""
    rows = max([7] + [max(c["nrb"] * c["rpl"] + 6, c["wh"]) for c in cells])
    off = (rows * 104 + 16 + 15) & ~15
    total = (off + 320 * 2 + 1279) // 1280 * 1280
    return max(320, min(kernel * 64, (total - off) // 2))


# ---------------------------------------------------------------------------------------------------------------------------
# the compass screen and the sampling decisions of k_fast_cells_cols, restated

def _screen(img, xs, ys, th):
    """fastc_screen: pixel passes iff two adjacent compass pixels (ring positions 0, 4, 8, 12) are both brighter than v + th or
    both darker than v - th.  img is the bordered level (reflect-101), xs / ys bordered coordinates."""
    v = img[ys, xs].astype(np.int32)
    d0, d4 = img[ys + 3, xs].astype(np.int32), img[ys, xs + 3].astype(np.int32)
    d8, d12 = img[ys - 3, xs].astype(np.int32), img[ys, xs - 3].astype(np.int32)
    M = np.minimum(np.maximum(d0, d8), np.maximum(d4, d12))
    m = np.maximum(np.minimum(d0, d8), np.minimum(d4, d12))
    return (M > v + th) | (m < v - th)


def cell_has_corner_at_ini(cands, cell):
    """Whether a level's candidate list [x - minB, y - minB, score] holds a corner at iniTh inside the cell's evaluated area."""
    mb = EDGE - 3
    x, y = cands[:, 0] + mb, cands[:, 1] + mb
    inside = (x >= cell["x0"] + 3) & (x < cell["x0"] + cell["ww"] - 3) & (y >= cell["y0"] + 3) & (y < cell["y0"] + cell["wh"] - 3)
    return bool((cands[inside, 2] >= INI_TH).any())


def cell_path(level_img, cell, screen_mode, list_cap, has_corner_at_ini):
    """Which way k_fast_cells_cols takes through a cell -> (path, figures).  path is one of
      'ini'              screened at iniTh, the cell has a corner there: done
      'ini>min' / 'ini>plain' / 'ini>min_overflow>plain'   screened at iniTh, no corner after NMS: starts again
      'ini_overflow>min', 'ini_overflow>plain', 'ini_overflow>min_overflow>plain'   survivors at iniTh exceed the list
      'min'              screened at minTh
      'min_overflow>plain', 'plain'
    has_corner_at_ini: whether the cell has a candidate at iniTh (from the oracle or the closed form)."""
    img = np.pad(level_img, 3, mode="reflect")
    ew, eh = cell["ww"] - 6, cell["wh"] - 6
    ncp, rpl, nrb = cell["ncp"], cell["rpl"], cell["nrb"]
    xs = cell["x0"] + 3 + np.arange(2 * ncp) + 3
    ys = cell["y0"] + 3 + np.arange(eh) + 3
    fig = {}

    def stage(th):
        p = _screen(img, np.minimum(xs, img.shape[1] - 4)[None, :], ys[:, None], th)
        p[:, ew:] = False                                            # the masked odd last column
        pair = p.reshape(eh, ncp, 2).any(axis=2)                     # a lane's pair row passes if either half does
        sample = pair[[rb * rpl for rb in range(nrb)]]               # every lane's first row of its row block
        return int(sample.sum()), ncp * nrb, int(pair.sum())

    path = []
    if screen_mode >= 2:
        nS, nAll, tot = stage(INI_TH)
        fig["ini"] = (nS, nAll, tot)
        if 8 * nS >= nAll and 3 * nS < 2 * nAll:
            if tot <= list_cap:
                if has_corner_at_ini:
                    return "ini", fig
                path.append("ini")
            else:
                path.append("ini_overflow")
    if screen_mode >= 1:
        nS, nAll, tot = stage(MIN_TH)
        fig["min"] = (nS, nAll, tot)
        if 4 * nS < nAll:
            if tot <= list_cap:
                return ">".join(path + ["min"]), fig
            path.append("min_overflow")
    return ">".join(path + ["plain"]), fig


# ---------------------------------------------------------------------------------------------------------------------------
# dots

def dot_image(w, h, dots, bg=BG):
    img = np.full((h, w), bg, np.uint8)
    for x, y, v in dots:
        img[y, x] = v
    return img


def dots_are_independent(dots):
    """No dot on another dot's ring: every dot keeps the score |d| - 1."""
    pos = {(x, y) for x, y, _ in dots}
    return all((x + dx, y + dy) not in pos for x, y, _ in dots for dx, dy in RING)


def dot_candidates(w, h, dots, bg=BG):
    """Closed form of level 0's candidate list [x - minB, y - minB, score] in emission order (cells row-major, raster inside)."""
    sc = np.zeros((h, w), np.int32)
    for x, y, v in dots:
        sc[y, x] = abs(int(v) - bg) - 1
    out = []
    for c in level_cells(w, h):
        ax, ay = c["x0"] + 3, c["y0"] + 3
        area = sc[ay:ay + c["wh"] - 6, ax:ax + c["ww"] - 6]
        for th in (INI_TH, MIN_TH):
            s = np.pad(np.where(area >= th, area, 0), 1)
            nb = np.max([s[1 + dy:s.shape[0] - 1 + dy, 1 + dx:s.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                         if (dx, dy) != (0, 0)], axis=0)
            core = s[1:-1, 1:-1]
            ys, xs = np.nonzero((core > 0) & (core > nb))
            if len(xs):
                out += [[ax + x - (EDGE - 3), ay + y - (EDGE - 3), core[y, x]] for y, x in zip(ys, xs)]
                break
    return np.array(out, np.int32).reshape(-1, 3)


def _one(name, w, h, dots, branch, nfeatures=1000, **expect):
    assert dots_are_independent(dots), name
    return Scn(name, [dot_image(w, h, dots)], (nfeatures, 1.2, 1, w, h), branch, dots=[dots], expect=expect)


def _cell_centres(w, h):
    """A pixel well inside every cell's evaluated area."""
    return [(c["x0"] + c["ww"] // 2, c["y0"] + c["wh"] // 2) for c in level_cells(w, h)]


# FAST scenarios: every builder works at any size; FAST_SIZES gives one whose full cells run k_fast_cells_cols<12> (11 rows per lane)
# and one whose cells run <8>
FAST_SIZES = ((160, 120), (160, 92))


def fast_scenarios(w, h):
    cc = _cell_centres(w, h)
    assert len(cc) >= 6
    tag = f"{w}x{h}"
    out = []
    # 1. threshold ladder: |d| - 1 against 20 and 7
    for d in (7, 8, 20, 21):
        dots = [(x, y, BG + (d if k % 2 == 0 else -d)) for k, (x, y) in enumerate(cc)]
        out.append(_one(f"ladder_d{d}_{tag}", w, h, dots, "score d - 1 against minTh / iniTh, bright and dark",
                        n_candidates={7: 0, 8: len(cc), 20: len(cc), 21: len(cc)}[d], score=d - 1))
    for bg, v in ((0, 255), (255, 0)):
        img = np.full((h, w), bg, np.uint8)
        dots = [(x, y, v) for x, y in cc]
        for x, y, _ in dots:
            img[y, x] = v
        out.append(Scn(f"ladder_{v}_on_{bg}_{tag}", [img], (1000, 1.2, 1, w, h), "score 254: the end of the f16-subnormal range",
                       dots=[dots], expect=dict(n_candidates=len(cc), score=254, bg=bg)))
    # 2. per-cell fallback: strong + weak in cell 0 -> strong only; weak alone in cell 1 -> the weak one
    (x0, y0), (x1, y1) = cc[0], cc[1]
    out.append(_one(f"fallback_{tag}", w, h, [(x0 - 5, y0, BG + 100), (x0 + 5, y0 + 4, BG + 12), (x1, y1, BG + 12)],
                    "threshold 7 only in a cell without a corner at 20", scores=[99, 11]))
    # 3. plateaus: two adjacent equal dots and a weak third in one cell -> only the weak one; the pair alone -> nothing
    for nm, (dx, dy) in (("h", (1, 0)), ("v", (0, 1)), ("d", (1, 1)), ("a", (-1, 1))):
        dots = [(x0, y0, BG + 100), (x0 + dx, y0 + dy, BG + 100), (x0 + 6, y0 - 8, BG + 12),
                (x1, y1, BG + 100), (x1 + dx, y1 + dy, BG + 100)]
        out.append(_one(f"plateau_{nm}_{tag}", w, h, dots, "strict NMS on equal neighbours, then the fallback", scores=[11]))
    # 5. detection border
    dots = [(x, y, BG + 100) for y in (18, 19, h - 20, h - 19) for x in (18, 19, w - 20, w - 19)]
    out.append(_one(f"border_{tag}", w, h, dots, "first / last evaluated row and column; patches reach the level's edge",
                    xy=[(19, 19), (w - 20, 19), (19, h - 20), (w - 20, h - 20)]))
    return out


SWEEP_DIRS = (("right", (1, 0)), ("down", (0, 1)), ("down_right", (1, 1)), ("down_left", (-1, 1)))


def sweep_dots(w, h, direction, ox, oy):
    """A lattice of strong dots (d = 100) every 8 pixels at phase (ox, oy), each with a weak neighbour (d = 80) in `direction`: over
    the 64 phases the strong pixel visits every position of every cell's evaluated area, of the seams between cells and of the
    rows and columns just outside the detection area."""
    dx, dy = direction
    dots = []
    for y in range(8 + oy, h - 8, 8):
        for x in range(8 + ox, w - 8, 8):
            dots += [(x, y, BG + 100), (x + dx, y + dy, BG + 80)]
    return dots


def sweep_scenario(w, h, name, direction):
    """4. NMS sweep: 64 frames per direction.  Closed form (dot_candidates): the strong pixel is a candidate wherever it is evaluated;
    the weak one exactly when the strong one lies outside the evaluated area of the weak one's cell."""
    frames = [sweep_dots(w, h, direction, ox, oy) for oy in range(8) for ox in range(8)]
    assert all(dots_are_independent(d) for d in frames)
    return Scn(f"sweep_{name}_{w}x{h}", [dot_image(w, h, d) for d in frames], (1000, 1.2, 1, w, h),
               "strict NMS across every lane seam, cell seam and the masked last column / rows", dots=frames)


# ---------------------------------------------------------------------------------------------------------------------------
# one cell per way through k_fast_cells_cols.  One level; cell 0 has 16 column pairs x 4 row blocks: of 11 rows at 160 x 120
# (k_fast_cells_cols<12>, list capacity 592 of 704 pair rows) and of 8 rows at 160 x 92 (<8>; its list holds all 480 pair rows, so the
# overflow scenarios exist at 160 x 120 only)

SCREEN_SIZE = (160, 120)
SCREEN_SIZES = ((160, 120), (160, 92))


def _stripes(w, h):
    """Diagonal 0 / 255 stripes of period 6: all four compass pixels of every pixel are its opposite - every pixel passes the screen
    at any threshold."""
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 6 < 3, 255, 0).astype(np.uint8)


def screen_scenarios(w=160, h=120):
    """Each scenario puts its texture into cell 0 (evaluated area x 19..50, y from 19) of a flat frame and names the way the
    restatement must say cell 0 takes with DRFE_FAST_SCREEN=2 (`path2`) and =1 (`path1`).  Sampled rows at 160 x 120: 19, 30, 41,
    52; at 160 x 92: 19, 27, 35, 43."""
    c = level_cells(w, h)[0]
    assert (c["ncp"], c["rpl"], c["nrb"], c["ww"], c["wh"]) == ((16, 11, 4, 38, 50) if h == 120 else (16, 8, 4, 38, 36))
    r = c["rpl"]
    ax, ay = c["x0"] + 3, c["y0"] + 3
    sampled = [ay + rb * c["rpl"] for rb in range(c["nrb"])]
    lanes = [(ax + 2 * cp, y) for y in sampled for cp in range(c["ncp"])]           # the 64 sampled pair rows (their even pixel)
    out = []

    def add(name, dots, branch, path2, path1, img=None):
        if img is None:
            assert dots_are_independent(dots), name
            img = dot_image(w, h, dots)
        out.append(Scn(f"screen_{name}" + ("" if (w, h) == SCREEN_SIZE else f"_{w}x{h}"), [img], (1000, 1.2, 1, w, h), branch, dots=None if dots is None else [dots],
                       expect=dict(path2=path2, path1=path1)))

    def on_lanes(n, d, odd=False):
        # odd: the second and fourth sampled rows carry the dot in the odd half of the pixel pair
        return [(x + ((k // 16) % 2 if odd else 0), y, BG + d) for k, (x, y) in enumerate(lanes[:n])]

    unsampled = [(ax + 4 * k + 1, ay + r // 2, BG + 100) for k in range(6)] + [(ax + 4 * k, ay + r + r // 2, BG + 12) for k in range(6)]
    add("unsampled_rows", unsampled, "corners only in rows the sample does not see", "min", "min")
    # the bounds at iniTh: 8 nS >= nAll (nS = 8 of 64) and 3 nS < 2 nAll (nS <= 42); alternate halves of the pixel pair
    add("ini_low_out", on_lanes(7, 100, odd=True) + unsampled, "8 nS >= nAll fails by one lane", "min", "min")
    add("ini_low_in", on_lanes(8, 100, odd=True) + unsampled, "8 nS >= nAll holds with equality", "ini", "min")
    add("ini_high_in", on_lanes(42, 100, odd=True), "3 nS < 2 nAll holds by one lane", "ini", "plain")
    add("ini_high_out", on_lanes(43, 100, odd=True), "3 nS < 2 nAll fails by one lane", "plain", "plain")
    # the bound at minTh: 4 nS < nAll (nS <= 15); dots of d = 12 never pass at iniTh and are emitted by the fallback
    add("min_in", on_lanes(15, 12), "4 nS < nAll holds by one lane; fallback after the screened fill", "min", "min")
    add("min_out", on_lanes(16, 12), "4 nS < nAll fails with equality; fallback on the plain path", "plain", "plain")
    # passes at iniTh, no corner at 20 after NMS: starts again
    third = [l for k, l in enumerate(lanes) if k % 16 % 3 == 0]             # every third lane: the pairs stay off each other's rings
    plate = [(x + k, y, BG + 100) for x, y in third[:8] for k in (0, 1)]
    add("restart", plate + [(ax + 9, ay + r // 2, BG + 12)], "screened at iniTh, plateaus only: no corner after NMS, starts again",
        "ini>min", "min")
    plate = [(x + k, y, BG + 100) for x, y in third[:20] for k in (0, 1)]
    add("restart_plain", plate + [(ax + 9, ay + r // 2, BG + 12)], "the same with 20 sampled lanes: starts again on the plain path",
        "ini>plain", "plain")
    # dense: every pixel passes the screen
    img = np.full((h, w), BG, np.uint8)
    img[c["y0"]:c["y0"] + c["wh"], c["x0"]:c["x0"] + c["ww"]] = _stripes(w, h)[c["y0"]:c["y0"] + c["wh"], c["x0"]:c["x0"] + c["ww"]]
    add("dense", None, "every sampled lane passes: the plain way", "plain", "plain", img=img)
    if fastc_list_cap(cell_table(w, h), 8 if r <= 8 else 12) >= c["ncp"] * (c["wh"] - 6):
        return out                                                # the list holds every pair row of the cell
    # survivors exceed the list: stripes, with a constant run on the sampled rows (a pixel whose row neighbours at +-3 equal it fails
    # the screen whatever is above and below)
    for name, run, p2, p1 in (("overflow_ini", 18, "ini_overflow>plain", "plain"),
                              ("overflow_both", 32, "ini_overflow>min_overflow>plain", "min_overflow>plain")):
        im2 = img.copy()
        for y in sampled:
            im2[y, c["x0"]:c["x0"] + run] = 128
        add(name, None, "survivors exceed the list capacity: screened_fill returns false", p2, p1, img=im2)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# quadtree: one-level dot fields

def quadtree_scenarios():
    out = []
    w, h = 160, 120
    # 1. equal responses in one node: emission order (cells row-major, then pixels) decides, not raster order
    # two cells of one cell row: (30, 50) lies in cell 0, (70, 30) in cell 1 - raster order would keep (70, 30).  One cell: raster
    # order inside the cell.  Two cell rows (160 x 122: three cell rows, the root's first split at y = 61 holds the first two):
    # emission and raster order agree there, an order by x would not
    for name, hh, a, b, weak, kept in (("one_cell_row", 120, (70, 30), (30, 50), (120, 80), (30, 50)),
                                       ("one_cell", 120, (45, 30), (25, 50), (120, 80), (45, 30)),
                                       ("two_cell_rows", 122, (70, 30), (30, 55), (120, 90), (70, 30))):
        out.append(_one(f"qt_tie_{name}", w, hh, [(a[0], a[1], BG + 100), (b[0], b[1], BG + 100), (weak[0], weak[1], BG + 50)],
                        "equal responses in one node: the first in emission order is kept", nfeatures=2, kept=kept, weak=weak))
    # 2. lattice ties
    lat = [(x, y, BG + 100) for y in range(20, 101, 10) for x in range(20, 141, 10)]
    for q in (1, 4, 7, 12, 20, 33, 50, 64, 100, 117, 200):
        out.append(_one(f"qt_lattice_q{q}", w, h, lat, "equal node sizes in the largest-first rounds, N + 1 .. N + 3 overshoot",
                        nfeatures=q, n_candidates=117))
    # closed form: two dots (d = 100, d = 60) in each quadrant of the root, so four nodes of two keys after the first round.  The
    # largest-first rounds split equal sizes latest-created first (BR, then BL, UR, UL) and stop at the quota: with N = 5 both keys of
    # BR are kept and the strong one of the others, with N = 6 both of BR and BL
    quads = [((30, 30), (60, 50)), ((100, 30), (130, 50)), ((30, 75), (60, 95)), ((100, 75), (130, 95))]
    qd = [(x, y, BG + d) for a, b in quads for (x, y), d in ((a, 100), (b, 60))]
    for q, both in ((5, [3]), (6, [3, 2])):
        out.append(_one(f"qt_sort_ties_q{q}", w, h, qd, "equal sizes in the largest-first sort: the node created last goes first",
                        nfeatures=q, kept_set=[quads[k][0] for k in range(4)] + [quads[k][1] for k in both]))
    # 3. roots: 400 x 150 gives three roots with a fractional hX
    w, h = 400, 150
    g = level_geom(w, h)
    assert g["nIni"] == 3 and float(g["hX"]) != int(g["hX"])
    mb = g["minB"]
    one_root = [(mb + 150 + 7 * k, 30 + 9 * (k % 10), BG + 100 - k) for k in range(14)]
    out.append(_one("qt_roots_one", w, h, one_root, "dots in the middle root only: the empty roots are erased", nfeatures=8))
    seams = []
    for i in (1, 2):
        xs = int(np.float32(g["hX"]) * np.float32(i))
        seams += [(mb + xs - 1, 40 + 20 * i, BG + 100), (mb + xs, 50 + 20 * i, BG + 90), (mb + xs + 1, 60 + 20 * i, BG + 80)]
    last = [(g["maxBX"] - 4, y, BG + 70 + y % 7) for y in (25, 60, 110)]       # the last evaluated column
    out.append(_one("qt_roots_seams", w, h, seams + last + [(mb + 40, 40, BG + 60)],
                    "candidate columns on either side of hX * i; the last column (min(..., nIni - 1))", nfeatures=6))
    # 4. midpoints of the first three rounds, in x and y (160 x 120: one root 128 x 88; 135 x 101: odd extents 103 x 69)
    for w, h in ((160, 120), (135, 101)):
        g = level_geom(w, h)
        assert g["nIni"] == 1
        W, H = g["maxBX"] - g["minB"], g["maxBY"] - g["minB"]
        xs, ys = {0, W}, {0, H}
        for _ in range(3):
            xs |= {a + int(np.ceil((b - a) / 2)) for a, b in zip(sorted(xs), sorted(xs)[1:])}
            ys |= {a + int(np.ceil((b - a) / 2)) for a, b in zip(sorted(ys), sorted(ys)[1:])}
        dots, k = [], 0
        for mx in sorted(xs - {0, W}):
            for dx in (-1, 1):                                    # candidate x = mx - 1 (left child) and mx + 1: two pixels apart
                cx = mx + dx
                if 3 <= cx < W - 3:
                    dots.append((cx + g["minB"], g["minB"] + 3 + (11 * k) % (H - 6), BG + 40 + k))
                    k += 1
        for my in sorted(ys - {0, H}):
            for dy in (-1, 1):
                cy = my + dy
                if 3 <= cy < H - 3:
                    dots.append((g["minB"] + 3 + (17 * k) % (W - 6), cy + g["minB"], BG + 40 + k))
                    k += 1
        on = [(mx + g["minB"], g["minB"] + 5 + 9 * i, BG + 90 + i) for i, mx in enumerate(sorted(xs - {0, W}))]   # x == mx: right child
        dots = on + dots
        keep = []
        for d in dots:                                            # drop the few that would sit on another dot's ring or beside it
            if all(max(abs(d[0] - e[0]), abs(d[1] - e[1])) > 3 for e in keep):
                keep.append(d)
        for q in (5, 12, 30):
            out.append(_one(f"qt_mid_{w}x{h}_q{q}", w, h, keep, "x < mx and the ceil in mx for odd extents", nfeatures=q))
        # closed form: the strongest dot P exactly on the first split line, Q (weaker) left of it, R (weakest) right of it, S in the
        # other half.  Three nodes after the first round = the quota: P shares its node with R (x < mx is false for x == mx), so P, Q
        # and S are kept and R is not.  `x <= mx` would keep P, R and S.  The same in y.
        mx, my, mb = int(np.ceil(W / 2)), int(np.ceil(H / 2)), g["minB"]
        px = [(mb + mx, mb + 10, BG + 100), (mb + mx - 9, mb + 20, BG + 95), (mb + mx + 9, mb + 15, BG + 90), (mb + 20, mb + my + 9, BG + 60)]
        out.append(_one(f"qt_on_line_x_{w}x{h}", w, h, px, "a key with x == mx goes to the right child", nfeatures=3,
                        kept_set=[px[0][:2], px[1][:2], px[3][:2]]))
        py = [(mb + 10, mb + my, BG + 100), (mb + 20, mb + my - 9, BG + 95), (mb + 15, mb + my + 9, BG + 90), (mb + mx + 9, mb + 20, BG + 60)]
        out.append(_one(f"qt_on_line_y_{w}x{h}", w, h, py, "a key with y == my goes to the lower child", nfeatures=3,
                        kept_set=[py[0][:2], py[1][:2], py[3][:2]]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# orientation, levels, wave grouping

ANGLES = {(0, 0): 0.0, (8, 0): 0.0, (-8, 0): 180.0, (0, 8): 90.0, (0, -8): 270.0, (8, 8): 44.990456, (-8, 8): 135.00955,
          (-8, -8): 224.99045, (8, -8): 315.00955}


def orientation_scenarios():
    """A dot alone has zero moments (the disc is symmetric and the flat background cancels): atan2(0, 0).  A second pixel of d = 5
    (no corner: score 4 < 7) eight pixels away puts the centroid on an axis or a diagonal of fastAtan2."""
    w, h = 160, 120
    out = []
    for (dx, dy), ang in ANGLES.items():
        dots = [(80, 60, BG + 100)] + ([(80 + dx, 60 + dy, BG + 5)] if (dx, dy) != (0, 0) else [])
        out.append(_one(f"angle_{dx:+d}_{dy:+d}", w, h, dots, "fastAtan2 on its axes and diagonals", angle=np.float32(ang)))
    return out


def bump_frame(w, h, amp, sigma, cx=None, cy=None, bg=BG):
    y, x = np.mgrid[0:h, 0:w]
    cx, cy = w // 2 if cx is None else cx, h // 2 if cy is None else cy
    return np.rint(bg + amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))).astype(np.uint8)


def level_scenarios():
    """333 x 250, 8 levels.  A rounded Gaussian bump of amplitude 40 is too smooth for a corner at level 0 (its ring differs from the
    centre by 4 at sigma 7) and becomes one only where the pyramid has shrunk it: keypoints on a few high levels with empty ones
    between, and an empty level 0.  A dot of d = 30 far from the bump adds a keypoint to the lowest levels until the resize has
    flattened it.  `levels` is what the oracle finds (asserted by the CPU test)."""
    p = (1000, 1.2, 8, 333, 250)
    why = "level lookup of the descriptor kernel with empty levels"
    out = []
    for s, dot, lv in ((7, False, [4, 7]), (6, False, [2, 4, 7]), (7, True, [0, 1, 4, 7]), (6, True, [0, 1, 2, 4, 7])):
        img = bump_frame(333, 250, 40, s)
        if dot:
            img[60, 60] = BG + 30
        out.append(Scn(f"levels_bump_s{s}{'_dot' if dot else ''}", [img], p, why, expect=dict(levels=lv)))
    out.append(Scn("levels_wide_bump", [bump_frame(333, 250, 60, 12)], p, why, expect=dict(levels=[4, 6, 7])))
    return out


WAVE_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9)


def wave_scenarios():
    w, h = 160, 120
    spots = [(30, 30), (130, 90), (130, 30), (30, 90), (80, 60), (80, 25), (80, 95), (25, 60), (135, 60)]
    # beside each dot a plateau (two adjacent equal pixels: never a candidate) in its own direction at its own distance 4 + k: every
    # keypoint has its own angle and, the distances differing, its own descriptor
    dirs = [(int(np.sign(ox)), int(np.sign(oy))) for ox, oy in ANGLES if (ox, oy) != (0, 0)] + [(1, 0)]

    def dots(n):
        out = []
        for k, (x, y) in enumerate(spots[:n]):
            out.append((x, y, BG + 60 + 3 * k))
            for i, r in enumerate(sorted({4 + k, 14 - k})):              # a second plateau a quarter turn on, at 14 - k
                sx, sy = dirs[k] if i == 0 else (-dirs[k][1], dirs[k][0])
                out += [(x + sx * r, y + sy * r, BG + 100), (x + sx * r + 1, y + sy * r, BG + 100)]
        return out
    return [_one(f"wave_{n}", w, h, dots(n), "keypoints modulo the four a wavefront of k_orient_desc carries", n_keypoints=n)
            for n in WAVE_COUNTS]


# ---------------------------------------------------------------------------------------------------------------------------
# stage images at the extremes

STAGE_SIZES = ((333, 250), (640, 480))


def stage_scenarios(w, h):
    y, x = np.mgrid[0:h, 0:w]
    u8 = lambda a: a.astype(np.uint8)
    imp = np.zeros((h, w), np.uint8)
    for px, py in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (1, 1)):
        imp[py, px] = 255
    frames = [("const0", np.zeros((h, w), np.uint8)), ("const255", np.full((h, w), 255, np.uint8)),
              ("checker1", u8(((x + y) & 1) * 255)), ("checker2", u8((((x >> 1) + (y >> 1)) & 1) * 255)),
              ("stripes_x", u8((x & 1) * 255)), ("stripes_y", u8((y & 1) * 255)), ("impulses", imp)]
    return [Scn(f"stage_{n}_{w}x{h}", [f], (1000, 1.2, 8, w, h), "no saturation in the resize and the 8.8 blur; reflection at every border",
                expect=dict(constant=int(f[0, 0]) if n.startswith("const") else None)) for n, f in frames]


def all_dot_scenarios():
    """Every one-level 160 x 120 scenario with default nfeatures, in builder order: the frames of the batch test."""
    s = fast_scenarios(160, 120) + screen_scenarios(160, 120) + orientation_scenarios() + wave_scenarios()
    return [x for x in s if x.params == (1000, 1.2, 1, 160, 120)]
