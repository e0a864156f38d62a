"""Hand-built maps for LocalMapping::MapPlaneCulling: each scenario is a scene (plane_cull_numpy's dict),
the premise it exists for, and `needs`: a check of the numpy restatement's result (its paths() counters among them) that
proves the scene takes the path it was built for.  test_plane_cull_cpu.py asserts every `needs`; the host entry and the
device batch are then held to the restatement on every scene.

C is the chunk of the device distance pass and TILE its row tile (drfe_plane_map_cull_limits; the CPU test holds the two to the
library).  Scenes have at most 24 planes and clouds of 0 .. 2 C + 1 points.

Most scenes use the family of planes z = h, coefficients (0, 0, 1, -h): every pair of them has angle exactly 1, and the
distance of a point is |z - h| up to one float rounding.  Planes of the family x = h never gate with them (angle 0).

Not built: "ldTh narrowed to float between candidates, with a second candidate between (float)d1 and d1".  PointDistanceFromPlane
returns a widened float, so (float)d1 == d1 for every candidate and no such pair of float distances exists; the narrowing shows
only in float ldTh = dTh, where it cannot change a verdict either: no float lies between dTh and (float)dTh."""
import numpy as np

import map_plane_numpy as mpn
import plane_cull_numpy as un
import plane_match_numpy as pmn

f32, f64 = np.float32, np.float64
C = 1024
TILE = 16


def zplane(h):
    return np.array([0, 0, 1, -h], f32)


def patch(rng, n, h, extent=0.5, axis=2, center=(0.0, 0.0)):
    """n points of the plane (axis) = h, on the voxel lattice's scale so that a voxel grid keeps them apart"""
    p = np.empty((n, 3), f32)
    others = [a for a in range(3) if a != axis]
    p[:, others[0]] = center[0] + rng.uniform(-extent, extent, n)
    p[:, others[1]] = center[1] + rng.uniform(-extent, extent, n)
    p[:, axis] = h
    return p


class Builder:
    """planes in vpMapPlanes order; key frames at translated identity poses unless given"""

    def __init__(self, seed, n_kfs=6, dTh=0.1, aTh=0.985, current=10):
        self.rng = np.random.default_rng(seed)
        self.s = dict(coefs=[], bad=[], clouds=[], found=[], visible=[], n_obs=[], first_kf_id=[], obs=[],
                      kf_clouds=[[] for _ in range(n_kfs)], Twc=np.stack([np.eye(4, dtype=f32)] * n_kfs), dTh=dTh, aTh=aTh,
                      current_kf_id=current, recent=[])
        for k in range(n_kfs):
            self.s["Twc"][k, :3, 3] = (0.25 * k, -0.125 * k, 0.0)

    def plane(self, coef, cloud, obs, found=10, visible=10, first=9, bad=0, n_obs=None):
        """obs: list of (key frame, world cloud seen from it); the key frame's cloud is the world cloud moved into its frame"""
        s = self.s
        s["coefs"].append(np.asarray(coef, f32))
        s["bad"].append(bad)
        s["clouds"].append(np.asarray(cloud, f32).reshape(-1, 3))
        s["found"].append(found)
        s["visible"].append(visible)
        s["first_kf_id"].append(first)
        o = []
        for kf, world in sorted(obs, key=lambda e: e[0]):
            local = (np.asarray(world, f32).reshape(-1, 3) - s["Twc"][kf, :3, 3]).astype(f32)
            s["kf_clouds"][kf].append(local)
            o.append((kf, len(s["kf_clouds"][kf]) - 1))
        s["obs"].append(o)
        s["n_obs"].append(len(o) if n_obs is None else n_obs)
        return len(s["coefs"]) - 1

    def zp(self, h, cloud_h=None, n=40, kfs=(0,), obs_h=None, **kw):
        """plane z = h with a resident cloud at z = cloud_h and observations at z = obs_h (both default to h)"""
        cloud_h = h if cloud_h is None else cloud_h
        obs_h = cloud_h if obs_h is None else obs_h
        return self.plane(zplane(h), patch(self.rng, n, cloud_h), [(k, patch(self.rng, 30, obs_h)) for k in kfs], **kw)

    def done(self):
        s = self.s
        s["coefs"] = np.stack(s["coefs"]).astype(f32) if s["coefs"] else np.zeros((0, 4), f32)
        s["bad"] = np.array(s["bad"], np.uint8)
        for k in ("found", "visible", "n_obs", "first_kf_id"):
            s[k] = np.array(s[k], np.int32)
        return s


def _events(r):
    return [tuple(e) for e in r["events"].tolist()]


def same(got, ref):
    """events, flags, counts, counters, verdicts, and the rebuilt clouds as u32 views"""
    assert np.array_equal(got["events"], ref["events"]), (got["events"].tolist(), ref["events"].tolist())
    for k in ("bad", "n_obs", "found", "visible", "verdicts"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["counters"] == ref["counters"]
    assert got["rebuilt"] == ref["rebuilt"]
    for j in ref["rebuilt"]:
        assert np.array_equal(got["clouds"][j].view(np.uint32), ref["clouds"][j].view(np.uint32)), j


def cloud_sizes():
    b = Builder(1)
    b.zp(0.0)
    for k, n in enumerate((0, 1, C - 1, C, C + 1, 2 * C + 1)):
        i = b.zp(2.0 + k, n=n)
        if n:                                  # the minimum sits in the cloud's last point, alone in its chunk where n = k C + 1
            b.s["clouds"][i][n - 1, 2] = 1.5 + k if n < 2 * C + 1 else 0.0625
    return dict(scene=b.done(), premise="clouds of 0, 1, C-1, C, C+1 and 2C+1 points; the last one's last point is the match",
                needs=lambda r, s: _events(r) == [(0, 6)] and r["paths"]["empty_cloud_scans"] >= 1)


def row_tiles():
    b = Builder(2)
    for k in range(18):
        b.zp(float(k))
    b.s["clouds"][16][5, 2] = 0.03125          # row 0 of column 16's one full tile
    b.s["clouds"][17][7, 2] = 16.0625          # row 16 of column 17: the only row of its second tile
    return dict(scene=b.done(), premise="columns with TILE and TILE + 1 gated rows; the match is in the last row of each",
                needs=lambda r, s: _events(r) == [(0, 16), (16, 17)] and TILE == 16)


def z_zero_minimum():
    b = Builder(3)
    x0 = np.array([1, 0, 0, 0], f32)
    far = patch(b.rng, 20, 0.5, axis=0)
    far[:, 2] += 1.0
    near = np.array([[0.015625, 0.25, 0.0]], f32)
    b.plane(x0, far, [(0, far)])
    b.plane(np.array([1, 0, 0, -0.5], f32), np.vstack([far, near]), [(1, far)])
    s = b.done()
    return dict(scene=s, premise="the minimum is a point with z == 0: Map::PointDistanceFromPlane has no z skip, PlaneMatcher's has",
                needs=lambda r, s: _events(r) == [(0, 1)] and un.point_distance_from_plane(s["coefs"][0], s["clouds"][1]) == 0.015625
                and pmn.point_distance_from_plane(s["coefs"][0], s["clouds"][1]) == 0.5)


def nan_and_inf():
    b = Builder(4)
    b.zp(0.0)
    i = b.zp(3.0)                              # NaN and inf points around a real minimum
    b.s["clouds"][i][0] = (np.nan, 0, 0.001)
    b.s["clouds"][i][1] = (np.inf, 0, 0.001)   # 0 * inf is NaN: the distance is NaN and never wins
    b.s["clouds"][i][2] = (0, 0, np.nan)
    b.s["clouds"][i][3] = (0, 0, -np.inf)      # distance +inf
    b.s["clouds"][i][9, 2] = 0.046875
    j = b.zp(5.0, n=6)                         # nothing but NaN: the start value 100 stands
    b.s["clouds"][j][:] = np.nan
    return dict(scene=b.done(), premise="NaN and inf distances never win; an all-NaN cloud gives 100",
                needs=lambda r, s: _events(r) == [(0, 1)] and un.point_distance_from_plane(s["coefs"][0], s["clouds"][2]) == 100.0)


def empty_cloud_wide():
    b = Builder(5, dTh=200.0)
    b.zp(0.0, n=30, cloud_h=150.0)
    b.zp(1.0, n=0, kfs=(1, 2))
    return dict(scene=b.done(), premise="dTh = 200: the empty cloud's 100 is below the threshold and matches",
                needs=lambda r, s: _events(r) == [(0, 1)] and r["paths"]["empty_cloud_scans"] == 1)


def gate_float_edge():
    b = Builder(6)
    a = f32(0.985)
    y = f32(np.sqrt(1 - f64(a) ** 2))
    near = patch(b.rng, 30, 0.0, axis=0)
    b.plane(np.array([1, 0, 0, 0], f32), near, [(0, near)])
    b.plane(np.array([a, y, 0, 0], f32), near, [(1, near)])
    return dict(scene=b.done(), premise="angle == (float)0.985 with aTh = 0.985: passes the double compare, would fail a float one",
                needs=lambda r, s: _events(r) == [(0, 1)] and un.angle_of(s["coefs"][0], s["coefs"][1]) == f32(0.985)
                and f64(f32(0.985)) > 0.985 and not f32(0.985) > f32(0.985))


def gate_negative():
    b = Builder(7)
    near = patch(b.rng, 30, 0.03125)
    b.plane(zplane(0.0), near, [(0, near)])
    b.plane(np.array([0, 0, -1, 0.03125], f32), near, [(1, near)])
    return dict(scene=b.done(), premise="angle < -aTh",
                needs=lambda r, s: _events(r) == [(0, 1)] and r["paths"]["negative_gate"] == 1)


def gate_equal():
    b = Builder(8, aTh=0.5)
    near = patch(b.rng, 30, 0.0, axis=0)
    b.plane(np.array([1, 0, 0, 0], f32), near, [(0, near)])
    b.plane(np.array([0.5, 0.8660254, 0, 0], f32), near, [(1, near)])
    b.plane(np.array([-0.5, 0, 0.8660254, 0], f32), near, [(2, near)])
    return dict(scene=b.done(), premise="angle == aTh and angle == -aTh, both exact in double: the compares are strict, nothing gates",
                needs=lambda r, s: _events(r) == [] and r["counters"]["gated_pairs"] == 0)


def equal_distances():
    b = Builder(9)
    b.zp(0.0)
    b.zp(3.0, cloud_h=0.0625)
    b.zp(5.0, cloud_h=0.0625)
    b.zp(7.0, cloud_h=-0.0625)
    return dict(scene=b.done(), premise="three columns at the same distance: the first wins",
                needs=lambda r, s: _events(r)[0] == (0, 1))


def distance_equals_threshold():
    b = Builder(10, dTh=0.125)
    b.zp(0.0)
    b.zp(3.0, cloud_h=0.125)
    b.zp(5.0, cloud_h=0.1875)
    return dict(scene=b.done(), premise="dis == dTh: strict, fails",
                needs=lambda r, s: _events(r) == [] and un.point_distance_from_plane(s["coefs"][0], s["clouds"][1]) == 0.125)


def more_observations_first():
    b = Builder(11)
    b.zp(0.0, kfs=(0, 1, 2))
    b.zp(3.0, cloud_h=0.03125, kfs=(3, 4))
    return dict(scene=b.done(), premise="pMP1 has more observations: pMP2 is replaced",
                needs=lambda r, s: _events(r) == [(1, 0)] and r["paths"]["replaced_second"] == 1 and r["n_obs"][0] == 5)


def shared_keyframe_chain():
    b = Builder(12)
    b.zp(0.0, kfs=(0, 1, 2))
    b.zp(0.015625, kfs=(1, 2, 3))
    b.zp(0.03125, cloud_h=0.0625, kfs=(0, 1, 2, 4, 5))
    # equal counts: plane 0 goes into plane 1, which shares two key frames with it and ends at 4 observations, not 6; against
    # plane 2's 5 that flips who is replaced in row 1
    return dict(scene=b.done(), premise="a shared key frame keeps the union below the sum and flips the next comparison; a chain",
                needs=lambda r, s: _events(r) == [(0, 1), (1, 2)] and r["paths"]["shared_keyframe"] >= 2 and r["paths"]["chain"] == 1
                and r["paths"]["replaced_first"] == 2)


def found_and_visible_reach_the_list():
    b = Builder(13)
    b.zp(0.0, found=8, visible=10)
    b.zp(0.03125, found=2, visible=10)
    s = b.done()
    s["recent"] = [1, 0]
    return dict(scene=s, premise="the survivor alone is below 0.25; with the replaced plane's counts it is kept; the replaced one is erased",
                needs=lambda r, s: _events(r) == [(0, 1)] and r["verdicts"].tolist() == [un.KEPT, un.ERASED_BAD]
                and un.found_ratio(2, 10) < f32(0.25))


def dead_row_and_column():
    b = Builder(14)
    b.zp(0.0, kfs=(0, 1, 2, 3, 4))
    b.zp(0.5)
    i = b.zp(0.5625, cloud_h=0.03125, kfs=(0, 1))
    b.s["clouds"][i][:10, 2] = 0.515625        # nearest to plane 1, but plane 2 dies in row 0
    b.zp(9.0, cloud_h=0.5625)
    return dict(scene=b.done(), premise="row 0 replaces column 2: row 1 takes the next best, row 2 has no candidates; the survivor is "
                                        "never read again (end-of-call batch)",
                needs=lambda r, s: _events(r) == [(2, 0), (1, 3)] and r["paths"]["dead_row"] == 1 and r["paths"]["dead_column"] >= 1
                and r["paths"]["unread_rebuilds"] >= 1 and un.point_distance_from_plane(s["coefs"][1], s["clouds"][2]) == 0.015625)


def stale_column_shrinks():
    b = Builder(15)
    b.zp(0.0)
    b.zp(0.5)
    i = b.zp(0.03125, kfs=(1,))
    b.s["clouds"][i][:5, 2] = 0.53125          # resident points none of the observations has: lost by the rebuild
    return dict(scene=b.done(), premise="the survivor's resident cloud holds points its observations lack; row 1 would match the stale cloud",
                needs=lambda r, s: _events(r) == [(0, 2)] and r["counters"]["stale_columns"] == 1
                and un.point_distance_from_plane(s["coefs"][1], s["clouds"][2]) < 0.1
                and un.point_distance_from_plane(s["coefs"][1], r["all_clouds"][2]) > 0.1)


def stale_column_grows():
    b = Builder(16)
    far = patch(np.random.default_rng(160), 30, 0.53125)
    b.plane(zplane(0.0), patch(b.rng, 40, 0.0), [(0, far)])
    b.zp(0.5)
    b.zp(0.03125, kfs=(1,))
    return dict(scene=b.done(), premise="the merged observations bring a point that row 1 matches; the stale cloud has none",
                needs=lambda r, s: _events(r) == [(0, 2), (1, 2)] and r["counters"]["stale_columns"] == 1
                and un.point_distance_from_plane(s["coefs"][1], s["clouds"][2]) > 0.1)


def rebuilt_twice_with_a_read_between():
    b = Builder(17)
    b.zp(0.0)
    b.zp(1.0)
    b.zp(0.03125, cloud_h=0.5, obs_h=0.0625, kfs=(1,))
    b.zp(2.0)
    b.zp(0.046875, cloud_h=0.0625, kfs=(2,))
    return dict(scene=b.done(), premise="plane 4 survives row 0, is read by row 1, survives row 2 and is read by row 3",
                needs=lambda r, s: _events(r) == [(0, 4), (2, 4)] and r["counters"]["stale_columns"] == 2
                and r["counters"]["rebuilds"] == 2 and r["paths"]["rebuilt_twice"] == 1)


def handed_back_voxel_job():
    b = Builder(18)
    wide = np.random.default_rng(180).uniform(-800, 800, (60, 3)).astype(f32)      # overflows the voxel grid's int32 leaf index
    b.plane(zplane(0.0), patch(b.rng, 40, 0.0), [(0, wide)])
    b.zp(1.0)
    b.zp(0.03125, kfs=(1,))
    return dict(scene=b.done(), premise="the survivor's merged cloud overflows the voxel grid: PCL returns the input, the device hands the job back",
                needs=lambda r, s: _events(r) == [(0, 2)] and len(r["all_clouds"][2]) == 90, host_jobs=1)


def recent_list():
    b = Builder(19, current=10)
    rows = [(1, 4, 9, 3), (8388607, 33554432, 9, 3),                         # ratio exactly 0.25; just below it in float
            (5, 10, 9, 2), (5, 10, 9, 3), (5, 10, 8, 2), (5, 10, 8, 3), (5, 10, 7, 2), (5, 10, 7, 3),   # ages 1, 2, 3 x 2, 3 observations
            (0, 0, 9, 3), (3, 0, 9, 3)]                                      # 0 / 0 is NaN (kept by that rule), 3 / 0 is +inf
    for k, (fo, vi, first, n) in enumerate(rows):
        b.zp(2.0 * k, found=fo, visible=vi, first=first, n_obs=n, kfs=(0, 1, 2)[:min(n, 3)])
    b.zp(30.0, bad=1)
    s = b.done()
    s["recent"] = [0, -1, 1, 2, 3, 4, 5, 6, 7, 10, 8, 9, 4, -1]
    K, EB, BR, BO, EA = un.KEPT, un.ERASED_BAD, un.BAD_BY_RATIO, un.BAD_BY_OBSERVATIONS, un.ERASED_BY_AGE
    return dict(scene=s, premise="every rule of the recent list at its edge; -1 entries; a plane listed twice",
                needs=lambda r, s: r["verdicts"].tolist() == [K, EB, BR, K, K, BO, K, BO, EA, EB, K, K, EB, EB] and _events(r) == []
                and un.found_ratio(1, 4) == f32(0.25) and un.found_ratio(8388607, 33554432) < f32(0.25))


def no_planes():
    s = Builder(20, n_kfs=1).done()
    s["recent"] = [-1]
    return dict(scene=s, premise="an empty map", needs=lambda r, s: _events(r) == [] and r["verdicts"].tolist() == [un.ERASED_BAD])


def random_map(seed, n_planes=24, n_kfs=40):
    """A Manhattan-style map: walls of the three axes at five offsets, several map planes per wall, clouds of 200 to 700 points,
    each plane seen from two to six of 40 randomly posed key frames; per-frame updates have left stray points in the resident
    clouds; the last planes are the recent ones."""
    rng = np.random.default_rng(seed)
    b = Builder(seed, n_kfs=n_kfs, current=50)
    for k in range(n_kfs):
        b.s["Twc"][k] = mpn.random_pose(rng, 0.3)
    walls = [(axis, h) for axis in range(3) for h in (-3.0, -1.5, 0.0, 1.5, 3.0)]
    for p in range(n_planes):
        axis, h = walls[rng.integers(len(walls))]
        sign = -1.0 if rng.random() < 0.3 else 1.0
        n = np.zeros(3)
        n[axis] = 1
        n = n + rng.normal(0, 0.01, 3)
        n = sign * n / np.linalg.norm(n)
        off = h + rng.normal(0, 0.02)
        coef = np.array([n[0], n[1], n[2], -sign * off], f32)
        center = rng.uniform(-1, 1, 2)
        recent = p >= n_planes - 10
        kfs = sorted(rng.choice(n_kfs, int(rng.integers(2, 4 if recent else 7)), replace=False).tolist())
        obs = []
        for kf in kfs:
            world = patch(rng, int(rng.integers(60, 160)), off, extent=0.8, axis=axis, center=center)
            world[:, axis] += rng.normal(0, 0.004, len(world)).astype(f32)
            obs.append((kf, world))
        cloud = patch(rng, int(rng.integers(200, 701)), off, extent=0.9, axis=axis, center=center)
        cloud[:, axis] += rng.normal(0, 0.004, len(cloud)).astype(f32)
        if rng.random() < 0.5:                  # strays that only the resident cloud has
            cloud[:8, axis] += rng.choice([-0.3, 0.3])
        b.plane(coef, cloud, obs, found=int(rng.integers(1, 6 if recent else 12)), visible=int(rng.integers(8, 14)),
                first=int(50 - rng.integers(0, 5)) if recent else 20, bad=int(rng.random() < 0.08))
    s = b.done()
    # key-frame clouds: the builder moved them by the translation alone; these poses rotate, so move them properly
    for p in range(n_planes):
        for kf, idx in s["obs"][p]:
            T = np.linalg.inv(s["Twc"][kf].astype(f64))
            world = s["kf_clouds"][kf][idx].astype(f64) + s["Twc"][kf][:3, 3].astype(f64)
            s["kf_clouds"][kf][idx] = (world @ T[:3, :3].T + T[:3, 3]).astype(f32)
    s["recent"] = list(range(n_planes - 10, n_planes)) + [-1]
    return s


RANDOM_SEEDS = (4, 5, 7)          # the first three seeds whose maps meet _random's condition on the numpy restatement


def _random(seed):
    def needs(r, s):
        v = r["paths"]["verdicts"]
        return len(r["events"]) >= 3 and r["counters"]["stale_columns"] >= 1 and all(n >= 1 for n in v)
    return dict(scene=random_map(seed), premise="a Manhattan-style map of 24 planes: at least 3 events, a stale column and every list verdict",
                needs=needs)


def all_scenarios():
    out = {f.__name__: f() for f in (
        cloud_sizes, row_tiles, z_zero_minimum, nan_and_inf, empty_cloud_wide, gate_float_edge, gate_negative, gate_equal,
        equal_distances, distance_equals_threshold, more_observations_first, shared_keyframe_chain, found_and_visible_reach_the_list,
        dead_row_and_column, stale_column_shrinks, stale_column_grows, rebuilt_twice_with_a_read_between, handed_back_voxel_job,
        recent_list, no_planes)}
    for seed in RANDOM_SEEDS:
        out[f"random_{seed}"] = _random(seed)
    return out
