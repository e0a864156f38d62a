/* trans_opt_core.h — the arithmetic of Optimizer::TranslationOptimization (reference src/Optimizer.cc:3211-3980) where it differs
 * from PoseOptimization's (pose_opt_core.h, which this includes and whose chi2, Huber kernel, LDLT, step control and oplusImpl
 * it uses unchanged): the map geometry rotated once by the float R_cw of the input pose, the *OnlyTranslation edges, whose
 * computeError reads only the estimate's translation and whose Jacobians have zero rotation columns, and an edge's nine terms
 * of the translation block of H and b.  Shared by the host entry (trans_opt.cpp) and the device kernel
 * (trans_opt_kernels.hip), both compiled with -ffp-contract=off.  DESIGN.md section 21.
 *
 * An edge is formed from the caller's arrays by whoever evaluates it (to_make_edge): nothing is widened into records ahead of
 * the launch. */
#ifndef DRFE_TRANS_OPT_CORE_H
#define DRFE_TRANS_OPT_CORE_H

#include "pose_opt_core.h"
#include "sim3_core.h"

enum { TO_H_TERMS = 6, TO_TERMS = 9 };          /* the lower triangle of H's translation block, row by row, then b[3..5] */

/* a call as both entries see it: the caller's arrays (on the device, their staged copies), the outlier flags in the caller's
 * layout, and the plane constants of src/Optimizer.cc:3449-3461 */
struct ToView {
    const float *Tcw, *K, *bf;
    const uint8_t* b_struct;
    const int32_t *point_offsets, *line_offsets, *plane_offsets;
    const float *obs, *u_right, *inv_sigma2, *Xw;
    const double *line_fn, *line_ends;
    const float *plane_meas, *plane_world;
    const uint8_t* plane_mask;
    uint8_t *point_outlier, *line_outlier, *plane_outlier[3];   /* the matched, the parallel and the vertical planes' flags */
    double planeInfo[3], disInfo, planeChi[3], planeDelta[3];    /* per pass: matched, parallel, vertical */
};

/* one frame of the view: R_cw, the camera, where its features start and how many edges they make.  Beside it goes the table
 * planeAt (to_plane_table): planeAt[j] = pass * 64 + slot of the frame's j-th plane edge, in the reference's order: the matched
 * planes of every slot, then with bStruct the parallel ones, then the vertical ones */
struct ToFrame {
    float R[9];
    PoCam cam;
    int32_t point0, line0, slot0;
    int32_t nPoints, nLines, nSlots, nPlaneEdges, nEdges;
};

DRFE_HD void to_view_settings(ToView& V, const double ps[7])
{
    V.planeInfo[0] = 3282.8 / (ps[0] * ps[0]);
    V.disInfo = ps[1] * ps[1];
    V.planeInfo[1] = 3282.8 / (ps[2] * ps[2]);
    V.planeInfo[2] = 3282.8 / (ps[3] * ps[3]);
    V.planeChi[0] = ps[4]; V.planeChi[1] = ps[5]; V.planeChi[2] = ps[5];
    for (int k = 0; k < 3; k++) V.planeDelta[k] = (double)(float)sqrt(V.planeChi[k]);
}

/* everything of ToFrame but nPlaneEdges / nEdges, which need planeAt (to_plane_table) */
DRFE_HD void to_frame(const ToView& V, int f, ToFrame& F)
{
    const float* T = V.Tcw + 16 * (size_t)f;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) F.R[r * 3 + c] = T[r * 4 + c];
    const float* K = V.K + 4 * (size_t)f;
    F.cam.fx = (double)K[0]; F.cam.fy = (double)K[1]; F.cam.cx = (double)K[2]; F.cam.cy = (double)K[3];
    F.cam.bf = (double)V.bf[f];
    F.point0 = V.point_offsets[f]; F.nPoints = V.point_offsets[f + 1] - F.point0;
    F.line0 = V.line_offsets[f]; F.nLines = V.line_offsets[f + 1] - F.line0;
    F.slot0 = V.plane_offsets[f]; F.nSlots = V.plane_offsets[f + 1] - F.slot0;
    F.nPlaneEdges = 0;
    F.nEdges = F.nPoints + 2 * F.nLines;
}

/* the frame's plane edges; planeAt has room for 3 * DRFE_POSE_OPT_MAX_PLANES */
DRFE_HD int to_plane_table(const ToView& V, int f, const ToFrame& F, uint8_t* planeAt)
{
    int n = 0;
    for (int pass = 0; pass < (V.b_struct[f] ? 3 : 1); pass++)
        for (int i = 0; i < F.nSlots; i++)
            if (V.plane_mask[F.slot0 + i] & (1 << pass)) planeAt[n++] = (uint8_t)(pass * 64 + i);
    return n;
}

/* cv::Mat Xc = R_cw * Xw: gemm's small-matrix path on floats, the result widened by `e->Xc[k] = Xc.at<float>(k)` */
DRFE_HD void to_rotate(const float R[9], const float x[3], double Xc[4])
{
    for (int r = 0; r < 3; r++) Xc[r] = (double)s3_gemm_row(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], x, 1.0, 0.f, 0.0);
    Xc[3] = 0.0;
}

/* edge k of the frame (points, then start and end of every line, then the plane edges) as the reference sets it up */
DRFE_HD void to_make_edge(const ToView& V, const ToFrame& F, const uint8_t* planeAt, int k, PoEdge& E)
{
    E.pad = 0;
    E.obs[3] = 0.0;
    if (k < F.nPoints) {
        const size_t i = (size_t)F.point0 + k;
        const float ur = V.u_right[i];
        E.kind = ur < 0 ? PO_MONO : PO_STEREO;
        E.obs[0] = (double)V.obs[2 * i];
        E.obs[1] = (double)V.obs[2 * i + 1];
        E.obs[2] = ur < 0 ? 0.0 : (double)ur;
        to_rotate(F.R, V.Xw + 3 * i, E.X);
        for (int c = 0; c < 3; c++) E.info[c] = (double)V.inv_sigma2[i];
        E.delta = ur < 0 ? po_delta_mono() : po_delta_stereo();
        E.th = ur < 0 ? po_th_mono() : po_th_stereo();
    } else if (k < F.nPoints + 2 * F.nLines) {
        const int j = k - F.nPoints;
        const size_t i = (size_t)F.line0 + (j >> 1);
        E.kind = PO_LINE;
        float x[3];                                 /* Converter::toCvVec of mWorldPos.head(3) / .tail(3) */
        for (int c = 0; c < 3; c++) {
            E.obs[c] = V.line_fn[3 * i + c];
            x[c] = (float)V.line_ends[6 * i + 3 * (j & 1) + c];
            E.info[c] = 1.0;
        }
        to_rotate(F.R, x, E.X);
        E.delta = po_delta_stereo();
        E.th = po_th_line();
    } else {
        const int at = planeAt[k - F.nPoints - 2 * F.nLines];
        const int pass = at >> 6;
        const size_t i = (size_t)F.slot0 + (at & 63);
        E.kind = PO_PLANE + pass;
        po_to_plane3d(V.plane_meas + 4 * i, E.obs);
        /* Xw.rotateNormal(Converter::toMatrix3d(R_cw)): the floats widened, a double product on the normal alone */
        double w[4];
        po_to_plane3d(V.plane_world + 12 * i + 4 * pass, w);
        for (int r = 0; r < 3; r++)
            E.X[r] = ((double)F.R[r * 3] * w[0] + (double)F.R[r * 3 + 1] * w[1]) + (double)F.R[r * 3 + 2] * w[2];
        E.X[3] = w[3];
        E.info[0] = V.planeInfo[pass]; E.info[1] = V.planeInfo[pass]; E.info[2] = pass == 0 ? V.disInfo : 0.0;
        E.delta = V.planeDelta[pass];
        E.th = V.planeChi[pass];
    }
}

/* where edge k's outlier flag lives in the caller's arrays (a line's two ends share their line's) */
DRFE_HD uint8_t* to_flag(const ToView& V, const ToFrame& F, const uint8_t* planeAt, int k)
{
    if (k < F.nPoints) return V.point_outlier + F.point0 + k;
    if (k < F.nPoints + 2 * F.nLines) return V.line_outlier + F.line0 + ((k - F.nPoints) >> 1);
    const int at = planeAt[k - F.nPoints - 2 * F.nLines];
    return V.plane_outlier[at >> 6] + F.slot0 + (at & 63);
}

/* computeError of the *OnlyTranslation edges: estimate().mapTrans(Xc) = Xc + t, or localPlane = w2n + Xc (Plane3D.h:204-212) */
DRFE_HD void to_edge_error(LmCtx& ctx, const PoEdge& E, const PoCam& C, const double t[3], double e[3])
{
    if (po_is_plane(E.kind)) {
        double l[4] = {E.X[0], E.X[1], E.X[2], 0.0};
        po_plane_ominus(ctx, E, l, t, e);
        return;
    }
    const double p[3] = {E.X[0] + t[0], E.X[1] + t[1], E.X[2] + t[2]};
    po_project_error(E, C, p, e);
}

/* linearizeOplus of the point and line edges, columns 3..5 (0..2 are zero): J[r][c] is _jacobianOplusXi(r, 3 + c) */
DRFE_HD void to_edge_jacobian(const PoEdge& E, const PoCam& C, const double t[3], double J[3][3])
{
    const double x = E.X[0] + t[0], y = E.X[1] + t[1];
    const double invz = 1.0 / (E.X[2] + t[2]);
    const double invz_2 = invz * invz;
    const double fx = C.fx, fy = C.fy;
    for (int r = 1; r < 3; r++)
        for (int c = 0; c < 3; c++) J[r][c] = 0.0;
    if (E.kind == PO_LINE) {
        const double lx = E.obs[0], ly = E.obs[1];
        J[0][0] = (fx * lx) * invz;
        J[0][1] = (fy * ly) * invz;
        J[0][2] = (-(((fx * lx) * x) + ((fy * ly) * y))) * invz_2;
        return;
    }
    J[0][0] = (-invz) * fx;
    J[0][1] = 0.0;
    J[0][2] = (x * invz_2) * fx;
    J[1][1] = (-invz) * fy;
    J[1][2] = (y * invz_2) * fy;
    if (E.kind == PO_STEREO) {
        J[2][0] = J[0][0];
        J[2][2] = J[0][2] - C.bf * invz_2;
    }
}

/* one perturbed error of a plane edge's numeric Jacobian, dimension 3 + d: computeError at exp(+-1e-9 e_(3 + d)) * estimate,
 * through the whole of oplusImpl as BaseUnaryEdge::linearizeOplus does (a translation that is not finite spreads there) */
DRFE_HD void to_plane_perturbed(LmCtx& ctx, const PoEdge& E, const double q[4], const double t[3], int d, int side, double e[3])
{
    double u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, pq[4], pt[3];
    u[3 + d] = side ? -1e-9 : 1e-9;
    for (int k = 0; k < 4; k++) pq[k] = q[k];
    for (int k = 0; k < 3; k++) pt[k] = t[k];
    (void)po_oplus(ctx, pq, pt, u);
    double l[4] = {E.X[0], E.X[1], E.X[2], 0.0};
    po_plane_ominus(ctx, E, l, pt, e);
}
/* the plane Jacobian: columns 3..5 of BaseUnaryEdge::linearizeOplus(); what it computes for 0..2 is overwritten with 0 */
DRFE_HD void to_plane_jacobian(LmCtx& ctx, const PoEdge& E, const double q[4], const double t[3], double J[3][3])
{
    const double scalar = lm_numeric_scalar();
    for (int d = 0; d < 3; d++) {
        double e1[3], e2[3];
        to_plane_perturbed(ctx, E, q, t, d, 0, e1);
        to_plane_perturbed(ctx, E, q, t, d, 1, e2);
        for (int r = 0; r < 3; r++) J[r][d] = scalar * (e1[r] - e2[r]);
    }
}

/* the translation columns widened to the D x 6 Jacobian constructQuadraticForm reads */
DRFE_HD void to_full_jacobian(const double J3[3][3], double J[3][6])
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { J[r][c] = 0.0; J[r][3 + c] = J3[r][c]; }
}

/* po_edge_terms for rows and columns 3..5 only, the same expressions in the same order: term[c (c + 1) / 2 + j] is what the
 * edge adds to H(3 + c, 3 + j), term[6 + c] what it takes from b(3 + c).  Returns 1 when the 18 terms left out are certain to
 * be +-0, as they are while everything that multiplies a zero column is finite: the error, rho1 Omega and A^T W.  Where it
 * returns 0 (a term 0 * inf) the caller needs the full form. */
template <int D>
DRFE_HD int to_edge_terms_dim(const PoEdge& E, const double J[3][3], const double e[3], int robust, double term[TO_TERMS])
{
    double rho1 = 1.0;
    if (robust) {
        double r0;
        po_huber(po_chi2(E, e), E.delta, &r0, &rho1);
    }
    int fin = isfinite(rho1) ? 1 : 0;
    double T[3][3], Tb[3][3];
    for (int k = 0; k < D; k++) fin &= (isfinite(e[k]) && isfinite(rho1 * E.info[k])) ? 1 : 0;
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < D; k++) {
            double s = 0.0, sb = 0.0;
            for (int m = 0; m < D; m++) {
                const double om = m == k ? E.info[m] : 0.0;
                const double w = robust ? rho1 * om : om;
                const double a = J[m][i] * w;
                const double ab = robust ? (rho1 * J[m][i]) * om : J[m][i] * om;
                s = m == 0 ? a : s + a;
                sb = m == 0 ? ab : sb + ab;
            }
            T[i][k] = s;
            Tb[i][k] = sb;
            fin &= (isfinite(s) && isfinite(sb) && isfinite(J[k][i])) ? 1 : 0;
        }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j <= i; j++) {
            double s = 0.0;
            for (int k = 0; k < D; k++) {
                const double a = T[i][k] * J[k][j];
                s = k == 0 ? a : s + a;
            }
            term[i * (i + 1) / 2 + j] = s;
        }
        double s = 0.0;
        for (int k = 0; k < D; k++) {
            const double a = Tb[i][k] * e[k];
            s = k == 0 ? a : s + a;
        }
        term[TO_H_TERMS + i] = s;
    }
    return fin;
}
/* the dimension is a template argument so that every loop unrolls and T, Tb and the terms stay in registers */
DRFE_HD int to_edge_terms(const PoEdge& E, const double J[3][3], const double e[3], int robust, double term[TO_TERMS])
{
    return po_dim(E.kind) == 2 ? to_edge_terms_dim<2>(E, J, e, robust, term) : to_edge_terms_dim<3>(E, J, e, robust, term);
}

/* where the nine land in PoLM's H (lower triangle, row by row) and b */
DRFE_HD int to_h_index(int r) { const int i = r < 1 ? 0 : r < 3 ? 1 : 2; const int j = r - i * (i + 1) / 2; return (3 + i) * (4 + i) / 2 + 3 + j; }

#endif
