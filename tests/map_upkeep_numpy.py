"""Independent numpy restatement of map-point / map-line upkeep: MapPoint::ComputeDistinctiveDescriptors
and UpdateNormalAndDepth (reference src/MapPoint.cc:288-411), MapLine::ComputeDistinctiveDescriptors and UpdateAverageDir
(src/MapLine.cpp:241-362).  Written from the reference text with np.sort and explicit float32 / float64 steps, not from the
C++ core; plus the random scenes the tests share.

A scene is a dict: kf_center [K, 3] float32, kf_bad [K] uint8, scale_factors [L] float32, bad [n] uint8, obs_offsets [n + 1]
int32, obs_kf [T] int32, obs_desc [T, 32] uint8, world [n, 3] float32 (points) or [n, 6] float64 (lines), ref_kf [n] int32,
ref_level [n] int32."""
import numpy as np

f32, f64 = np.float32, np.float64


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def distinctive(rows, full_matrix=False):
    """index of the row with the least median distance (first at ties); rows [N, 32].  Points fill the upper triangle and
    mirror it, lines the full matrix (src/MapLine.cpp:281-291): the values are the same."""
    N = len(rows)
    D = np.zeros((N, N), f32)
    for i in range(N):
        D[i, i] = 0
        for j in (range(N) if full_matrix else range(i + 1, N)):
            d = hamming(rows[i], rows[j])
            D[i, j] = d
            D[j, i] = d
    best_median, best = 2 ** 31 - 1, 0
    for i in range(N):
        v = np.sort(D[i].astype(np.int64))
        median = int(v[int(0.5 * (N - 1))])
        if median < best_median:
            best_median, best = median, i
    return best


def _norm_f32(v):
    """cv::norm of a float 3-vector: the double sum of squares in order, then sqrt"""
    s = f64(0.0)
    for k in range(3):
        s = s + f64(v[k]) * f64(v[k])
    return np.sqrt(s)


def _item(scene, i, what, line):
    off = scene["obs_offsets"]
    o0, o1 = int(off[i]), int(off[i + 1])
    kf_bad = scene.get("kf_bad")
    bad = scene.get("bad")
    r = dict(best_obs=-1, desc=np.zeros(32, np.uint8), normal=np.zeros(3, f64 if line else f32), max_distance=f32(0),
             min_distance=f32(0), status=0)
    if (bad is not None and bad[i]) or o1 == o0:
        return r
    if what & 1:
        idx = [q - o0 for q in range(o0, o1) if kf_bad is None or not kf_bad[scene["obs_kf"][q]]]
        if idx:
            rows = np.array([scene["obs_desc"][o0 + q] for q in idx], np.uint8)
            b = distinctive(rows, full_matrix=line)
            r["best_obs"], r["desc"] = idx[b], rows[b].copy()
            r["status"] |= 1
    if what & 2:
        C = scene["kf_center"]
        sc = scene["scale_factors"]
        Owr = C[scene["ref_kf"][i]]
        n = o1 - o0
        with np.errstate(all="ignore"):
            if not line:
                X = scene["world"][i].astype(f32)
                normal = np.zeros(3, f32)
                for q in range(o0, o1):
                    normali = (X - C[scene["obs_kf"][q]]).astype(f32)
                    s = _norm_f32(normali)
                    alpha = f32(f64(1.0) / s)                          # scaleAdd's float alpha
                    normal = (normali * alpha).astype(f32) + normal   # src1 * alpha + src2, no FMA
                dist = f32(_norm_f32((X - Owr).astype(f32)))
                normal = (normal * f32(f64(1.0) / f64(n))).astype(f32)
            else:
                P = scene["world"][i].astype(f64)
                normal = np.zeros(3, f64)
                mid = f64(0.5) * (P[:3] + P[3:])
                for q in range(o0, o1):
                    v = mid - C[scene["obs_kf"][q]].astype(f64)
                    s = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
                    normal = normal + v / s
                SP, EP = P[:3].astype(f32), P[3:].astype(f32)
                MP = ((SP + EP) * f32(0.5)).astype(f32)
                dist = f32(_norm_f32((MP - Owr).astype(f32)))
                normal = normal / f64(n)
            mx = f32(dist * sc[scene["ref_level"][i]])
            mn = f32(mx / sc[len(sc) - 1])
        r.update(normal=normal, max_distance=mx, min_distance=mn)
        r["status"] |= 2
    return r


def upkeep(scene, what=3, line=False):
    """all items of a scene: dict of arrays as the host entry returns them (frustum included)"""
    n = len(scene["obs_offsets"]) - 1
    rs = [_item(scene, i, what, line) for i in range(n)]
    out = dict(best_obs=np.array([r["best_obs"] for r in rs], np.int32).reshape(n),
               desc=np.array([r["desc"] for r in rs], np.uint8).reshape(n, 32),
               normal=np.array([r["normal"] for r in rs], f64 if line else f32).reshape(n, 3),
               max_distance=np.array([r["max_distance"] for r in rs], f32).reshape(n),
               min_distance=np.array([r["min_distance"] for r in rs], f32).reshape(n),
               status=np.array([r["status"] for r in rs], np.uint8).reshape(n))
    on = (out["status"] & 2) != 0
    if line:
        fr = np.zeros(n, [("world", "<f8", (6,)), ("normal", "<f8", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4")])
    else:
        fr = np.zeros(n, [("world", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4")])
    if n:
        fr["world"][on] = np.asarray(scene["world"])[on]
        fr["normal"] = out["normal"]
        fr["min_distance"] = (f32(0.8) * out["min_distance"]).astype(f32)
        fr["max_distance"] = (f32(1.2) * out["max_distance"]).astype(f32)
    out["frustum"] = fr
    return out


def scale_factors(nlevels=8, factor=1.2):
    """ORBextractor's mvScaleFactor: scale[i] = scale[i - 1] * factor in float"""
    s = [f32(1.0)]
    for _ in range(1, nlevels):
        s.append(f32(s[-1] * f32(factor)))
    return np.array(s, f32)


def random_scene(rng, counts, line=False, n_kf=64, p_bad_kf=0.1, p_bad_item=0.03, flips=(0, 24), nlevels=8):
    """items with the given observation counts: descriptors a per-item base row plus a few random bit flips (medians tie
    often), keyframe centres around the items, ref keyframe usually among the observations"""
    counts = np.asarray(counts, np.int64)
    n, T = len(counts), int(counts.sum())
    C = rng.normal(0, 2, (n_kf, 3)).astype(f32)
    kf_bad = (rng.random(n_kf) < p_bad_kf).astype(np.uint8)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(counts)
    obs_kf = np.zeros(T, np.int32)
    desc = np.zeros((T, 32), np.uint8)
    ref_kf = np.zeros(n, np.int32)
    for i in range(n):
        o0, o1 = off[i], off[i + 1]
        k = o1 - o0
        obs_kf[o0:o1] = rng.integers(0, n_kf, k) if k > n_kf else np.sort(rng.choice(n_kf, k, replace=False))
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        bits = np.unpackbits(np.tile(base, (k, 1)), axis=1)
        nf = rng.integers(flips[0], flips[1] + 1, k)
        for q in range(k):
            bits[q, rng.choice(256, int(nf[q]), replace=False)] ^= 1
        desc[o0:o1] = np.packbits(bits, axis=1)
        ref_kf[i] = obs_kf[o0 + rng.integers(0, k)] if k and rng.random() < 0.9 else rng.integers(0, n_kf)
    if line:
        mid = rng.normal(0, 3, (n, 3))
        d = rng.normal(0, 0.5, (n, 3))
        world = np.hstack([mid - d, mid + d]).astype(f64)
    else:
        world = rng.normal(0, 3, (n, 3)).astype(f32)
    return dict(kf_center=C, kf_bad=kf_bad, scale_factors=scale_factors(nlevels), bad=(rng.random(n) < p_bad_item).astype(np.uint8),
                obs_offsets=off, obs_kf=obs_kf, obs_desc=desc, world=world, ref_kf=ref_kf,
                ref_level=rng.integers(0, nlevels, n).astype(np.int32))
