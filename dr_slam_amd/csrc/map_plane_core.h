/* map_plane_core.h — the arithmetic of MapPlane::UpdateCoefficientsAndPoints (reference src/MapPlane.cc:298-371) in front of
 * its voxel grid: the pose of each form as a double 4x4 and pcl::transformPointCloud's per-point product.  Shared by the host
 * entries (map_plane.cpp) and the device gather (map_plane_kernels.hip) so that both produce the same bits; plain IEEE
 * add / mul / div / sqrt in double, compiled with -ffp-contract=off on both sides.  DESIGN.md section 13.
 *
 * Matrices are row-major: the float poses are 4x4 (16 floats), the results 4x4 doubles of which rows 0..2 are read. */
#ifndef DRFE_MAP_PLANE_CORE_H
#define DRFE_MAP_PLANE_CORE_H

#include "../../include/drfe.h"
#include "../../include/drfe_math.h"

/* The per-frame form: Eigen::Isometry3d(Converter::toSE3Quat(Tcw)).inverse().matrix().
 *   toSE3Quat (src/Converter.cc:37-47) widens R and t to double; g2o::SE3Quat(R, t) takes Quaterniond(R) (Eigen 3.3.7
 *   quaternion_assign_impl<3, 3>), negates the four coefficients when w < 0 and normalises (z = squaredNorm; if z > 0 each
 *   coefficient / sqrt(z)); the Isometry3d cast sets linear = q.toRotationMatrix(), translation = t; inverse() of an isometry
 *   is linear^T and (-linear^T) * t.
 * Eigen leaves the association of the trace, the 4-term squaredNorm and the 3-term products open: they are read left to right
 * here (canonical, as DESIGN.md section 9 does for Eigen's reductions).  -(a * t0) - ... equals -(a * t0 + ...) exactly.
 * The quaternion pieces stand alone because pose_opt_core.h runs the same ones. */

/* Eigen 3.3.7's Quaterniond(Matrix3d) (quaternion_assign_impl<3, 3>): q is x y z w, Eigen's coeffs() order */
DRFE_HD void mp_quat_from_matrix(const double m[3][3], double q[4])
{
    double tr = m[0][0] + m[1][1] + m[2][2];
    if (tr > 0.0) {
        tr = sqrt(tr + 1.0);
        q[3] = 0.5 * tr;
        tr = 0.5 / tr;
        q[0] = (m[2][1] - m[1][2]) * tr;
        q[1] = (m[0][2] - m[2][0]) * tr;
        q[2] = (m[1][0] - m[0][1]) * tr;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        tr = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[i] = 0.5 * tr;
        tr = 0.5 / tr;
        q[3] = (m[k][j] - m[j][k]) * tr;
        q[j] = (m[j][i] + m[i][j]) * tr;
        q[k] = (m[k][i] + m[i][k]) * tr;
    }
}

/* g2o::SE3Quat::normalizeRotation: the four coefficients negated when w < 0, then Quaternion::normalize */
DRFE_HD void mp_quat_normalize_rotation(double q[4])
{
    if (q[3] < 0.0)
        for (int c = 0; c < 4; c++) q[c] = -q[c];
    const double z = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (z > 0.0) {
        const double s = sqrt(z);
        for (int c = 0; c < 4; c++) q[c] = q[c] / s;
    }
}

/* Quaternion::toRotationMatrix */
DRFE_HD void mp_quat_to_matrix(const double q[4], double R[3][3])
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0][0] = 1.0 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1.0 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1.0 - (txx + tyy);
}

/* Converter::toSE3Quat(Tcw): the quaternion (x y z w) and translation of g2o::SE3Quat(R, t) over the widened float pose */
DRFE_HD void mp_to_se3quat(const float Tcw[16], double q[4], double t[3])
{
    double m[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[r][c] = (double)Tcw[r * 4 + c];
    t[0] = (double)Tcw[3]; t[1] = (double)Tcw[7]; t[2] = (double)Tcw[11];
    mp_quat_from_matrix(m, q);
    mp_quat_normalize_rotation(q);
}

DRFE_HD void mp_pose_update(const float Tcw[16], double T[16])
{
    double q[4], t[3], R[3][3];                   /* x y z w, Eigen's coeffs() order */
    mp_to_se3quat(Tcw, q, t);
    mp_quat_to_matrix(q, R);
    const double t0 = t[0], t1 = t[1], t2 = t[2];
    /* inverse: R^T and -(R^T t) */
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[r * 4 + c] = R[c][r];
        T[r * 4 + 3] = -(R[0][r] * t0 + R[1][r] * t1 + R[2][r] * t2);
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

/* The observation form: Converter::toMatrix4d(KF->GetPoseInverse()) (src/Converter.cc:156-166), the float Twc widened element
 * by element. */
DRFE_HD void mp_pose_rebuild(const float Twc[16], double T[16])
{
    for (int k = 0; k < 16; k++) T[k] = (double)Twc[k];
}

/* pcl::transformPointCloud(cloud, out, Matrix4d) of PCL 1.9.1 (common/impl/transforms.hpp), one point of a dense cloud:
 * the point widened to double, (float)(((T00 x + T01 y) + T02 z) + T03) per row. */
DRFE_HD void mp_transform_point(const double T[16], float x, float y, float z, float o[3])
{
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    for (int r = 0; r < 3; r++) o[r] = (float)(((T[r * 4 + 0] * dx + T[r * 4 + 1] * dy) + T[r * 4 + 2] * dz) + T[r * 4 + 3]);
}

#endif
