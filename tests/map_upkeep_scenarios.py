"""Hand-built items that put map-point and map-line upkeep on its decision points: medians that tie
(the first of the tied rows wins), N = 1..4, bad keyframes interleaved so that best_obs must point into the caller's list, all
keyframes bad, no observations, a bad item, a bad keyframe that still counts in the normal, the zero-length viewing ray; and,
for the device's rank selection and its minimum over a lane group, a wavefront or a workgroup, items of a chosen number of rows
whose winner is stated by construction: the last row strictly least, all rows identical, two tied rows at chosen positions, a
row and its complement (medians 256 and 0), fully random rows.

scene() builds one item; cases() lists the hand-built ones with the outcome stated by hand; medians() restates the lower median
of every row with np.sort (for the conditions on the inputs, at any size); merge() concatenates one-item scenes into one call,
shifting obs_kf and ref_kf.  Nothing here calls the library: tests/test_map_upkeep_cpu.py holds the host to these cases,
tests/test_gpu_map_upkeep_edges.py the device."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_upkeep_numpy as MU  # noqa: E402

f32, f64 = np.float32, np.float64
BASE = np.random.default_rng(3).integers(0, 256, 32, dtype=np.uint8)
# both sides of every bucket boundary (4, 16, 64), of the workgroup kernel's one row per thread (256) and the device cap (2048)
BUCKET_ROWS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 256, 257, 2048)


def flip(base, bits):
    b = np.unpackbits(base.copy())
    b[list(bits)] ^= 1
    return np.packbits(b)


def scene(rows, obs_kf=None, kf_bad=None, world=None, centers=None, ref_kf=0, ref_level=0, line=False, bad=0):
    """one item observed by len(rows) keyframes (keyframe q = observation q unless obs_kf says otherwise)"""
    n = len(rows)
    obs_kf = np.arange(n, dtype=np.int32) if obs_kf is None else np.asarray(obs_kf, np.int32)
    K = max(int(obs_kf.max()) + 1 if n else 1, ref_kf + 1)
    rng = np.random.default_rng(7)
    centers = rng.normal(0, 1, (K, 3)).astype(f32) if centers is None else np.asarray(centers, f32)
    if world is None:
        world = np.array([[0.5, 1.5, 4.0, 0.7, 1.1, 4.4]], f64) if line else np.array([[0.5, 1.5, 4.0]], f32)
    return dict(kf_center=centers, kf_bad=np.zeros(len(centers), np.uint8) if kf_bad is None else np.asarray(kf_bad, np.uint8),
                scale_factors=MU.scale_factors(), bad=np.array([bad], np.uint8), obs_offsets=np.array([0, n], np.int32),
                obs_kf=obs_kf, obs_desc=np.asarray(rows, np.uint8).reshape(-1, 32), world=world,
                ref_kf=np.array([ref_kf], np.int32), ref_level=np.array([ref_level], np.int32))


# --- the hand-built cases ---------------------------------------------------------------------------------------------------

def tie_rows():
    """a far row first, then three rows 8 apart: medians 40, 8, 8, 8 - the first of the tied rows (1) wins"""
    return [flip(BASE, range(100, 140)), flip(BASE, range(0, 4)), flip(BASE, range(4, 8)), flip(BASE, range(8, 12))]


def small_n_rows(N):
    """N = 1 and 2: the median index is 0, so row 0 wins.  N = 3: a far row, then B and B^{30,31}: medians 30, 2, 2, so
    row 1.  N = 4: B, B^{0,1}, B^{0..9}, B^{200..249}: the lower median (index 1) ties rows 0 and 1 at 2, so row 0; the
    upper median would have picked row 1 (8 against 10).  Returns (rows, the winner)."""
    if N == 1:
        return [BASE], 0
    if N == 2:
        return [flip(BASE, range(0, 30)), BASE], 0
    if N == 3:
        return [flip(BASE, range(0, 30)), BASE, flip(BASE, range(30, 32))], 1
    return [BASE, flip(BASE, [0, 1]), flip(BASE, range(0, 10)), flip(BASE, range(200, 250))], 0


def interleaved_rows():
    """observations of keyframes [bad, good, bad, good, good]: the rows are the three good ones (far, then two 6 apart), the
    first of the two close rows wins and best_obs points into the caller's list (3).  The bad keyframe's row B would have
    won (3 from both close rows) had it counted."""
    return [flip(BASE, range(50, 90)), flip(BASE, range(100, 120)), BASE, flip(BASE, range(0, 3)), flip(BASE, range(3, 6))]


def zero_ray_scene(line):
    """a keyframe centre at the point (the line's middle): norm 0, and the normal becomes NaN as in the reference"""
    centers = np.array([[0.5, 1.5, 4.0], [1.0, 0.0, 0.0]], f32)
    world = np.array([[0.25, 1.25, 3.5, 0.75, 1.75, 4.5]], f64) if line else np.array([[0.5, 1.5, 4.0]], f32)
    return scene([BASE, BASE], centers=centers, world=world, ref_kf=1, line=line)


def cases(line=False):
    """every hand-built case as (name, one-item scene, expectation); an expectation is a dict over the item: best_obs, desc (the
    winning row's bytes), status (with both halves asked for), nan_normal"""
    out = []

    def add(name, s, **expect):
        out.append((name, s, expect))
    rows = tie_rows()
    add("median_tie", scene(rows, line=line), best_obs=1, desc=rows[1].tobytes(), status=3)
    for N in (1, 2, 3, 4):
        rows, win = small_n_rows(N)
        add(f"n_{N}", scene(rows, line=line), best_obs=win, desc=rows[win].tobytes(), status=3)
    rows = interleaved_rows()
    add("bad_keyframes_interleaved", scene(rows, kf_bad=[1, 0, 1, 0, 0], line=line), best_obs=3, desc=rows[3].tobytes(), status=3)
    add("one_bad_keyframe", scene(rows, kf_bad=[1, 0, 0, 0, 0], line=line), best_obs=2, desc=rows[2].tobytes(), status=3)
    rows = [BASE, flip(BASE, [1, 2])]
    add("all_keyframes_bad", scene(rows, kf_bad=[1, 1], line=line), best_obs=-1, desc=bytes(32), status=2)
    add("no_observations", scene(np.zeros((0, 32), np.uint8), line=line), best_obs=-1, desc=bytes(32), status=0)
    add("bad_item", scene(rows, bad=1, line=line), best_obs=-1, desc=bytes(32), status=0)
    rows = [BASE, flip(BASE, [1]), flip(BASE, [2])]
    add("bad_keyframe_in_the_normal", scene(rows, kf_bad=[0, 1, 0], line=line), status=3)
    add("no_bad_keyframe", scene(rows, line=line), status=3)
    add("without_its_observation", scene([rows[0], rows[2]], obs_kf=[0, 2], line=line), status=3)
    add("zero_length_viewing_ray", zero_ray_scene(line), status=3, nan_normal=True, best_obs=0)
    return out


def holds(expect, r, i=0, what=3):
    """asserts a case's expectation on item i of a result computed with the halves `what`"""
    if what & 1:
        for key in ("best_obs", "desc"):
            if key in expect:
                got = r[key][i].tobytes() if key == "desc" else r[key][i]
                assert got == expect[key], (key, got)
    if "status" in expect:
        assert r["status"][i] == expect["status"] & what, ("status", r["status"][i])
    if expect.get("nan_normal") and what & 2:
        assert np.isnan(r["normal"][i]).all()


# --- items of a chosen number of rows -----------------------------------------------------------------------------------------

def medians(rows):
    """the lower median (index int(0.5 * (N - 1)) of the sorted row, src/MapPoint.cc:334) of every row's Hamming distances"""
    b = np.unpackbits(np.asarray(rows, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    D = (b @ (1 - b).T + (1 - b) @ b.T).astype(np.int32)
    return np.sort(D, axis=1)[:, int(0.5 * (len(b) - 1))]


def around(rng, centre, n, nflips, avoid=(), must=()):
    """n rows: centre with nflips random bits flipped, none of `avoid`; with `must`, one of its bits (row i takes must[i % len])
    is among them"""
    free = np.setdiff1d(np.arange(256), np.asarray(list(avoid) + list(must), np.int64))
    out = []
    for i in range(n):
        bits = list(rng.choice(free, nflips - (1 if must else 0), replace=False))
        if must:
            bits.append(must[i % len(must)])
        out.append(flip(centre, bits))
    return out


def rows_last_least(nr, seed=0):
    """the last row is the centre C of the others (C with 40 random bits flipped each): its distances are all 40, the others
    see 40 once and about 67 otherwise, so from five rows on (median index >= 2) the last row alone has the least median.
    With two to four rows no such item exists: the median index is 0 or 1, the nearest-neighbour distance at most, and the
    nearest neighbour of the winner has a median as small.  -> rows, or None"""
    if 2 <= nr <= 4:
        return None
    rng = np.random.default_rng(100 + seed)
    c = rng.integers(0, 256, 32, dtype=np.uint8)
    return around(rng, c, nr - 1, 40) + [c]


def rows_identical(nr):
    return [BASE] * nr


def tie_positions(nr):
    """where the two tied rows go: not row 0 where that is possible; above 64 rows in different wavefronts of the workgroup
    kernel; above 256 rows once in one thread's stride (rows r and r + 256) and once in different threads"""
    if nr < 2:
        return []
    if nr == 2:
        return [(0, 1)]
    if nr <= 256:
        return [(1, nr - 1)]
    return [(nr - 257, nr - 1), (1, nr - 2)]


def rows_two_tied(nr, lo, hi, seed=0):
    """exactly two rows, at lo < hi, tie for the least median.  A and B = A with bits 0, 1 flipped; every other row is A with 40
    bits flipped, exactly one of them bit 0 or 1, so it is 40 from A and from B and about 67 from the rest.  A and B see
    {0, 2, 40, ...}: the median is 2 with three or four rows and 40 from seven rows on, where the others' is about 67.  Five
    rows (median index 2) get a layout of their own: r1 = A with 10 bits flipped, r2 = B with 10 others, r3 far; A and B see
    {0, 2, 10, 12, far} and r1, r2 see {0, 10, 12, 22, far}: 10 against 12."""
    rng = np.random.default_rng(200 + seed)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = flip(a, [0, 1])
    if nr == 5:
        rest = [flip(a, range(10, 20)), flip(b, range(20, 30)), flip(a, range(100, 200))]
    elif nr == 6:
        raise ValueError("six rows are not among the cases")
    else:
        rest = around(rng, a, nr - 2, 40, must=(0, 1))
    rows = []
    for i in range(nr):
        rows.append(a if i == lo else b if i == hi else rest.pop())
    return rows


def rows_complement(nr):
    """nr = 2 k + 1: k copies of a row, then k + 1 of its complement: medians 256 and 0, row k wins"""
    assert nr % 2 == 1
    k = nr // 2
    return [BASE] * k + [np.bitwise_not(BASE)] * (k + 1)


def rows_random(nr, seed=0):
    return list(np.random.default_rng(300 + seed).integers(0, 256, (nr, 32), dtype=np.uint8))


def bucket_items(nr):
    """the items of nr rows as (name, rows, the winning row or None where only the reference says), each with its condition on
    the inputs asserted here on medians()"""
    out = []
    rows = rows_last_least(nr, nr)
    if rows is not None:
        m = medians(rows)
        assert nr == 1 or m[-1] < m[:-1].min()
        out.append(("last_least", rows, nr - 1))
    rows = rows_identical(nr)
    assert not medians(rows).any()
    out.append(("identical", rows, 0))
    for lo, hi in tie_positions(nr):
        rows = rows_two_tied(nr, lo, hi, nr)
        m = medians(rows)
        assert m[lo] == m[hi] == m.min() and (m == m.min()).sum() == 2 and rows[lo].tobytes() != rows[hi].tobytes()
        if nr > 64:
            assert (lo % 256) // 64 != (hi % 256) // 64 or lo % 256 == hi % 256
        out.append((f"tied_{lo}_{hi}", rows, lo))
    if nr % 2 == 1:
        rows = rows_complement(nr)
        m = medians(rows)
        assert (m[:nr // 2] == 256).all() and not m[nr // 2:].any()
        out.append(("complement", rows, nr // 2))
    rows = rows_random(nr, nr)
    if nr > 4:
        m = medians(rows)
        assert 100 < m.min() and m.max() < 156
    out.append(("random", rows, None))
    return out


def with_bad_keyframes(n_obs, n_good, seed=0, line=False):
    """one item of n_obs observations of which n_good, spread over the list, are on good keyframes; the good rows lie around
    one centre, the rows of bad keyframes around another, so a row of a bad keyframe would win had it counted"""
    rng = np.random.default_rng(400 + seed)
    good = np.sort(rng.choice(n_obs, n_good, replace=False))
    kf_bad = np.ones(n_obs, np.uint8)
    kf_bad[good] = 0
    c = rng.integers(0, 256, 32, dtype=np.uint8)
    rows = np.array(around(rng, np.bitwise_not(c), n_obs, 3))
    rows[good] = around(rng, c, n_good, 30)
    return scene(rows, kf_bad=kf_bad, line=line)


def merge(scenes, line=False):
    """one call of the scenes' items: keyframes, observations and items appended, obs_kf and ref_kf shifted"""
    cen, kfb, bad, off, okf, desc, world, rkf, rlv = [], [], [], [0], [], [], [], [], []
    nk = 0
    for s in scenes:
        K = len(s["kf_center"])
        cen.append(s["kf_center"])
        kfb.append(s["kf_bad"])
        bad.append(s["bad"])
        off += [off[-1] + int(o) for o in s["obs_offsets"][1:]]
        okf.append(np.asarray(s["obs_kf"], np.int32) + nk)
        desc.append(np.asarray(s["obs_desc"], np.uint8).reshape(-1, 32))
        world.append(s["world"])
        rkf.append(np.asarray(s["ref_kf"], np.int32) + nk)
        rlv.append(s["ref_level"])
        nk += K
    return dict(kf_center=np.concatenate(cen), kf_bad=np.concatenate(kfb), scale_factors=scenes[0]["scale_factors"],
                bad=np.concatenate(bad), obs_offsets=np.int32(off), obs_kf=np.concatenate(okf), obs_desc=np.concatenate(desc),
                world=np.concatenate(world), ref_kf=np.concatenate(rkf), ref_level=np.concatenate(rlv))
