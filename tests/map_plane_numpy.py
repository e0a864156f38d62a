"""An independent numpy restatement of MapPlane::UpdateCoefficientsAndPoints (reference src/MapPlane.cc:298-371; DESIGN.md
section 13) for the host tests: the two pose paths (g2o::SE3Quat's quaternion round trip of Eigen 3.3.7, and the widened
Twc), pcl::transformPointCloud in float64 with the association written out (no FMA: numpy multiplies and adds separately),
the concatenation order, and oracle.post_voxel_grid for the voxel step."""
import numpy as np

f32, f64 = np.float32, np.float64


def quaternion_of(R):
    """Eigen 3.3.7 quaternion_assign_impl<3, 3>: (x, y, z, w) of a float64 3x3, scalar by scalar"""
    m = [[f64(R[r][c]) for c in range(3)] for r in range(3)]
    q = [f64(0)] * 4
    t = (m[0][0] + m[1][1]) + m[2][2]
    if t > 0:
        t = np.sqrt(t + f64(1))
        q[3] = f64(0.5) * t
        t = f64(0.5) / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
        return q, "trace"
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + f64(1))
    q[i] = f64(0.5) * t
    t = f64(0.5) / t
    q[3] = (m[k][j] - m[j][k]) * t
    q[j] = (m[j][i] + m[i][j]) * t
    q[k] = (m[k][i] + m[i][k]) * t
    return q, f"i={i}"


def se3quat_rotation(R):
    """g2o::SE3Quat(R, t)'s normalizeRotation then toRotationMatrix: (rotation float64 3x3, branch, flipped)"""
    q, branch = quaternion_of(R)
    flipped = bool(q[3] < 0)
    if flipped:
        q = [-v for v in q]
    z = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    if z > 0:
        s = np.sqrt(z)
        q = [v / s for v in q]
    x, y, zq, w = q
    tx, ty, tz = f64(2) * x, f64(2) * y, f64(2) * zq
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * zq
    Rq = np.array([[f64(1) - (tyy + tzz), txy - twz, txz + twy],
                   [txy + twz, f64(1) - (txx + tzz), tyz - twx],
                   [txz - twy, tyz + twx, f64(1) - (txx + tyy)]], f64)
    return Rq, branch, flipped


def pose_update(Tcw):
    """Isometry3d(toSE3Quat(Tcw)).inverse().matrix() as a float64 4x4"""
    Tcw = np.asarray(Tcw, f32).reshape(4, 4)
    Rq, _, _ = se3quat_rotation(Tcw[:3, :3].astype(f64))
    t = Tcw[:3, 3].astype(f64)
    T = np.zeros((4, 4), f64)
    T[3, 3] = 1
    for r in range(3):
        for c in range(3):
            T[r, c] = Rq[c, r]
        T[r, 3] = -((Rq[0, r] * t[0] + Rq[1, r] * t[1]) + Rq[2, r] * t[2])
    return T


def pose_rebuild(Twc):
    """Converter::toMatrix4d(Twc): widened element by element"""
    return np.asarray(Twc, f32).reshape(4, 4).astype(f64)


def transform(T, xyz):
    """pcl::transformPointCloud with a Matrix4d: (float)(((T00 x + T01 y) + T02 z) + T03) per row"""
    p = np.asarray(xyz, f32).reshape(-1, 3).astype(f64)
    out = np.empty((len(p), 3), f32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]).astype(f32)
    return out


def voxel(xyz):
    from oracle import oracle as orc
    p = np.asarray(xyz, f32).reshape(-1, 3)
    return orc.post_voxel_grid(p, 0.05) if len(p) else np.zeros((0, 3), f32)


def update(Tcw, frame_xyz, map_xyz):
    """UpdateCoefficientsAndPoints(F, i): the transformed frame points first, then the plane's current cloud"""
    combined = np.vstack([transform(pose_update(Tcw), frame_xyz), np.asarray(map_xyz, f32).reshape(-1, 3)])
    return voxel(combined)


def rebuild(Twcs, clouds):
    """UpdateCoefficientsAndPoints(): every observation's cloud moved by its Twc, in the order given"""
    parts = [transform(pose_rebuild(T), c) for T, c in zip(Twcs, clouds)]
    return voxel(np.vstack(parts) if parts else np.zeros((0, 3), f32))


def rotation(axis, angle):
    a = np.asarray(axis, f64)
    k = a / np.linalg.norm(a)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def random_pose(rng, scale=0.6):
    T = np.eye(4)
    T[:3, :3] = rotation(rng.normal(0, 1, 3), rng.uniform(-scale * np.pi, scale * np.pi))
    T[:3, 3] = rng.normal(0, 1, 3)
    return T.astype(f32)


def plane_cloud(rng, n, center=(0, 0, 2), normal=(0, 0, 1), extent=1.0, noise=0.004):
    """n points on a plane patch, float32"""
    nrm = np.asarray(normal, f64) / np.linalg.norm(normal)
    u = np.cross(nrm, [1, 0, 0] if abs(nrm[0]) < 0.9 else [0, 1, 0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    a, b = rng.uniform(-extent, extent, (2, n))
    p = np.asarray(center, f64) + a[:, None] * u + b[:, None] * v + rng.normal(0, noise, n)[:, None] * nrm
    return p.astype(f32)
