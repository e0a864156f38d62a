"""A literal restatement of the Sim3 propagation of LoopClosing::CorrectLoop (reference src/LoopClosing.cc:480-562) on Python
objects, with KeyFrame::SetPose, MapPoint::UpdateNormalAndDepth, g2o::Sim3 and Eigen's Quaterniond pieces written out in numpy
float32 / float64 scalars.  It is a sequential pointer-order walk that mutates its objects as the reference does: a key frame's
SetPose happens when the loop reaches it, and a later UpdateNormalAndDepth simply reads whatever centre a key frame has at that
moment.  It shares nothing with dr_slam_amd/csrc/correct_core.h: no slots, no positions, no claims, no "is the centre new" rule.
It extends conn_numpy.Store and has lib.LocalMap's interface, so a script (tests/loop_correct_scenarios.py) plays on either."""
import numpy as np

import conn_numpy as cn
import lmap_numpy as ln

f32, f64 = np.float32, np.float64
NORMAL = 2                      # DRFE_UPKEEP_NORMAL


# ---- Eigen / g2o ---------------------------------------------------------------------------------------------------------------

def quat_from_matrix(m):
    """Eigen 3.3.7 Quaterniond(Matrix3d); returns [x, y, z, w]"""
    q = [f64(0)] * 4
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        t = np.sqrt(t + f64(1.0))
        q[3] = f64(0.5) * t
        t = f64(0.5) / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i][i] - m[j][j] - m[k][k] + f64(1.0))
        q[i] = f64(0.5) * t
        t = f64(0.5) / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def quat_to_matrix(q):
    x, y, z, w = q
    tx, ty, tz = f64(2.0) * x, f64(2.0) * y, f64(2.0) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = f64(1.0)
    return [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def rotate(q, v):
    """Quaternion::_transformVector"""
    uv = cross(q[:3], v)
    uv = [c + c for c in uv]
    c = cross(q[:3], uv)
    return [(v[k] + q[3] * uv[k]) + c[k] for k in range(3)]


class Sim3:
    def __init__(self, q, t, s):
        self.q, self.t, self.s = [f64(v) for v in q], [f64(v) for v in t], f64(s)

    @staticmethod
    def from_pose(R, t):
        """g2o::Sim3(toMatrix3d(R), toVector3d(t), 1.0) of float32 arrays"""
        return Sim3(quat_from_matrix([[f64(R[r][c]) for c in range(3)] for r in range(3)]), [f64(v) for v in t], 1.0)

    def map(self, v):
        r = rotate(self.q, v)
        return [self.s * r[k] + self.t[k] for k in range(3)]

    def inverse(self):
        conj = [-self.q[0], -self.q[1], -self.q[2], self.q[3]]
        m = f64(-1.0) / self.s
        return Sim3(conj, rotate(conj, [m * v for v in self.t]), f64(1.0) / self.s)

    def __mul__(self, o):
        ax, ay, az, aw = self.q
        bx, by, bz, bw = o.q
        q = [((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz,
             ((aw * bz + az * bw) + ax * by) - ay * bx, ((aw * bw - ax * bx) - ay * by) - az * bz]
        return Sim3(q, self.map(o.t), self.s * o.s)

    def coeffs8(self):
        return np.array(self.q + self.t + [self.s], f64)


# ---- OpenCV --------------------------------------------------------------------------------------------------------------------

def gemm4(A, B):
    """cv::Mat C = A * B of two CV_32F 4x4: the small-matrix path"""
    C = np.zeros((4, 4), f32)
    for r in range(4):
        for c in range(4):
            t = A[r][0] * B[0][c] + A[r][1] * B[1][c] + A[r][2] * B[2][c] + A[r][3] * B[3][c]
            C[r][c] = f32(f64(t) * f64(1.0))
    return C


def norm3(v):
    """cv::norm of a CV_32F 3-vector: the double sum of squares in order, then sqrt"""
    s = f64(0.0)
    for k in range(3):
        s += f64(v[k]) * f64(v[k])
    return np.sqrt(s)


class Pose:
    """what KeyFrame::SetPose keeps"""

    def __init__(self, Tcw):
        self.Tcw = np.array(Tcw, f32).reshape(4, 4).copy()
        R, t = self.Tcw[:3, :3], self.Tcw[:3, 3]
        self.Ow = np.zeros(3, f32)
        for i in range(3):
            d = R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]          # Rwc = Rcw.t() stored, then gemm without a flag
            self.Ow[i] = f32(f64(d) * f64(-1.0))
        self.Twc = np.eye(4, dtype=f32)
        self.Twc[:3, :3] = R.T
        self.Twc[:3, 3] = self.Ow


class Geometry:
    def __init__(self, row):
        self.world = np.array(row["world"], f32).reshape(3).copy()
        self.ref_kf = int(row["ref_kf"])
        self.ref_level = int(row.get("ref_level", 0))
        self.mnCorrectedByKF = int(row.get("corrected_by", 0))
        self.mnCorrectedReference = int(row.get("corrected_ref", 0))


class Store(cn.Store):
    def __init__(self):
        super().__init__()
        self.scales = np.zeros(0, f32)
        self.pose, self.geo = {}, {}
        self.rcounts = dict(calls=0, keyframes=0, moved=0, moved_without_obs=0, entries_walked=0)

    # -- the store's interface --------------------------------------------------------------------------------------------------
    def set_scales(self, sf):
        self.scales = np.array(sf, f32)

    def get_scales(self):
        return self.scales.copy()

    def set_poses(self, handles, Tcw):
        T = np.asarray(Tcw, f32).reshape(len(handles), 4, 4)
        for h, t in zip(handles, T):
            self.pose[int(h)] = Pose(t)

    def get_poses(self, handles):
        return {"Tcw": np.stack([self.pose[int(h)].Tcw for h in handles]).reshape(-1, 4, 4),
                "Ow": np.stack([self.pose[int(h)].Ow for h in handles]).reshape(-1, 3),
                "Twc": np.stack([self.pose[int(h)].Twc for h in handles]).reshape(-1, 4, 4)}

    def set_point_geometry(self, rows):
        for r in rows:
            self.geo[int(r["handle"])] = Geometry(r)

    def get_point_geometry(self, handles):
        g = [self.geo[int(h)] for h in handles]
        return {"world": np.stack([p.world for p in g]).reshape(-1, 3), "ref_kf": np.array([p.ref_kf for p in g], np.int32),
                "ref_level": np.array([p.ref_level for p in g], np.int32),
                "corrected_by": np.array([p.mnCorrectedByKF for p in g], np.int32),
                "corrected_ref": np.array([p.mnCorrectedReference for p in g], np.int32)}

    def remove(self, kind, handle):
        super().remove(kind, handle)
        (self.pose if kind == ln.KEYFRAME else self.geo if kind == ln.POINT else {}).pop(int(handle), None)

    # -- MapPoint::UpdateNormalAndDepth -------------------------------------------------------------------------------------------
    def _update_normal_and_depth(self, h):
        pMP, g = self.mp[h], self.geo[h]
        if pMP.bad or not pMP.observations:
            return None
        Pos = g.world.copy()
        normal = np.zeros(3, f32)
        n = 0
        for kh in pMP.observations:
            Owi = self.pose[kh].Ow
            normali = g.world - Owi
            scale = f32(f64(1.0) / norm3(normali))
            normal = normali * scale + normal
            n += 1
        PC = Pos - self.pose[g.ref_kf].Ow
        dist = f32(norm3(PC))
        mx = dist * self.scales[g.ref_level]
        mn = mx / self.scales[len(self.scales) - 1]
        return normal * f32(f64(1.0) / f64(n)), mx, mn

    # -- LoopClosing::CorrectLoop :480-562 --------------------------------------------------------------------------------------
    def correct(self, cur, Scw, handles, mode=None, capacity=None):
        cur = int(cur)
        S = np.asarray(Scw, f64).reshape(8)
        mg2oScw = Sim3(S[:4], S[4:7], S[7])
        connected = [int(h) for h in handles]
        rank = lambda h: self.kf[h].rank
        Corrected, NonCorrected = {cur: mg2oScw}, {}
        Twc = self.pose[cur].Twc.copy()
        for h in connected:
            Tiw = self.pose[h].Tcw
            if h != cur:
                Tic = gemm4(Tiw, Twc)
                Corrected[h] = Sim3.from_pose(Tic[:3, :3], Tic[:3, 3]) * mg2oScw
            NonCorrected[h] = Sim3.from_pose(Tiw[:3, :3], Tiw[:3, 3])
        walk = sorted(Corrected, key=rank)
        poses = {}
        moved = dict(points=[], claimed_by=[], world=[], normal=[], max_distance=[], min_distance=[], status=[])
        with np.errstate(all="ignore"):
            for h in walk:
                Siw_c = Corrected[h]
                Swi_c = Siw_c.inverse()
                Siw = NonCorrected[h]
                self.rcounts["entries_walked"] += len(self.kf[h].mvpMapPoints)
                for ph in self.kf[h].mvpMapPoints:
                    if ph == -1:
                        continue
                    pMP = self.mp[ph]
                    if pMP.bad:
                        continue
                    g = self.geo[ph]
                    if g.mnCorrectedByKF == cur:
                        continue
                    X = Swi_c.map(Siw.map([f64(v) for v in g.world]))
                    g.world = np.array([f32(v) for v in X], f32)
                    g.mnCorrectedByKF = cur
                    g.mnCorrectedReference = h
                    und = self._update_normal_and_depth(ph)
                    moved["points"].append(ph)
                    moved["claimed_by"].append(h)
                    moved["world"].append(g.world.copy())
                    if und is None:
                        und = (np.zeros(3, f32), f32(0), f32(0))
                        self.rcounts["moved_without_obs"] += 1
                        moved["status"].append(0)
                    else:
                        moved["status"].append(NORMAL)
                    moved["normal"].append(und[0])
                    moved["max_distance"].append(und[1])
                    moved["min_distance"].append(und[2])
                R = quat_to_matrix(Siw_c.q)
                inv = f64(1.0) / Siw_c.s
                T = np.eye(4, dtype=f32)
                for r in range(3):
                    for c in range(3):
                        T[r][c] = f32(R[r][c])
                    T[r][3] = f32(Siw_c.t[r] * inv)
                self.pose[h] = Pose(T)
                poses[h] = T
        self.rcounts["calls"] += 1
        self.rcounts["keyframes"] += len(connected)
        self.rcounts["moved"] += len(moved["points"])
        m = len(moved["points"])
        return {"walk_pos": np.array([walk.index(h) for h in connected], np.int32),
                "corrected": np.stack([Corrected[h].coeffs8() for h in connected]),
                "non_corrected": np.stack([NonCorrected[h].coeffs8() for h in connected]),
                "Tiw": np.stack([poses[h] for h in connected]),
                "points": np.array(moved["points"], np.int32), "claimed_by": np.array(moved["claimed_by"], np.int32),
                "world": np.array(moved["world"], f32).reshape(m, 3), "normal": np.array(moved["normal"], f32).reshape(m, 3),
                "max_distance": np.array(moved["max_distance"], f32), "min_distance": np.array(moved["min_distance"], f32),
                "status": np.array(moved["status"], np.uint8)}


CORRECT_KEYS = ("walk_pos", "corrected", "non_corrected", "Tiw", "points", "claimed_by", "world", "normal", "max_distance",
                "min_distance", "status")


def same_correct(a, b):
    """equal bytes"""
    for k in CORRECT_KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (k, x, y)


def same_geometry(a, b, kfs, pts):
    """the stores hold the same poses, derived members, positions, references and stamps, byte for byte"""
    if len(kfs):
        pa, pb = a.get_poses(kfs), b.get_poses(kfs)
        for k in ("Tcw", "Ow", "Twc"):
            assert np.ascontiguousarray(pa[k]).tobytes() == np.ascontiguousarray(pb[k]).tobytes(), k
    if len(pts):
        ga, gb = a.get_point_geometry(pts), b.get_point_geometry(pts)
        for k in ("world", "ref_kf", "ref_level", "corrected_by", "corrected_ref"):
            assert np.ascontiguousarray(ga[k]).tobytes() == np.ascontiguousarray(gb[k]).tobytes(), k
    assert a.get_scales().tobytes() == b.get_scales().tobytes()
