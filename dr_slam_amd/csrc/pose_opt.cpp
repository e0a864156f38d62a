/* pose_opt.cpp — Optimizer::PoseOptimization (reference src/Optimizer.cc:601-1338) behind the C-ABI of include/drfe.h: the host
 * entry (no context), the batch entry (pose_opt_kernels.hip) and its counters.  Both sides evaluate pose_opt_core.h; here are the
 * argument checks and caps, the edge list of a call, the frame's rounds on the host, and the hand-back of a frame whose sin / cos
 * or cube the device could not certify.  DESIGN.md section 20. */
#include "pose_opt_internal.h"
#include "batch_entry.h"
#include "stage_layout.h"
#include "../../include/drfe_debug.h"

#include <cstring>
#include <vector>

struct PoseOptBuffers : BatchBuffers {};   /* scratch: _error of every edge; the hand-back counts frames */

void drfe_pose_opt_free(drfe_ctx* c) { batch_free(c->pose_opt); }

namespace {

struct Plan {
    std::vector<PoFrameRec> frame;
    std::vector<PoEdge> edge;
};

/* all-or-nothing validation of a call, then its frames and edges */
int make_plan(const drfe_pose_opt_problems* p, const drfe_pose_opt_out* o, Plan& P, std::string& err)
{
    err = "pose_opt: invalid argument";
    if (!p || !o || p->n < 0) return DRFE_ERR_INVALID;
    if (p->n > DRFE_POSE_OPT_MAX_FRAMES) { err = "pose_opt: more than DRFE_POSE_OPT_MAX_FRAMES frames in a call"; return DRFE_ERR_INVALID; }
    const int n = p->n;
    if (n == 0) return DRFE_OK;
    if (!p->Tcw || !p->K || !p->bf || !p->b_struct || !p->point_offsets || !p->line_offsets || !p->plane_offsets) return DRFE_ERR_INVALID;
    if (!o->Tcw || !o->returns || !o->rounds || !o->iterations || !o->trials) return DRFE_ERR_INVALID;
    if (!batch_offsets_ok("pose_opt", p->point_offsets, n, DRFE_POSE_OPT_MAX_POINTS, "point", "DRFE_POSE_OPT_MAX_POINTS points", err) ||
        !batch_offsets_ok("pose_opt", p->line_offsets, n, DRFE_POSE_OPT_MAX_LINES, "line", "DRFE_POSE_OPT_MAX_LINES lines", err) ||
        !batch_offsets_ok("pose_opt", p->plane_offsets, n, DRFE_POSE_OPT_MAX_PLANES, "plane", "DRFE_POSE_OPT_MAX_PLANES plane slots", err))
        return DRFE_ERR_INVALID;
    const int nP = p->point_offsets[n], nL = p->line_offsets[n], nS = p->plane_offsets[n];
    if (nS > 0 && (!p->plane_meas || !p->plane_world || !p->plane_mask || !o->plane_outlier || !o->par_plane_outlier ||
                   !o->ver_plane_outlier))
        return DRFE_ERR_INVALID;
    /* src/Optimizer.cc:822-834 */
    const double* ps = p->plane_settings;
    const double angleInfo = 3282.8 / (ps[0] * ps[0]), disInfo = ps[1] * ps[1];
    const double parInfo = 3282.8 / (ps[2] * ps[2]), verInfo = 3282.8 / (ps[3] * ps[3]);
    const double planeChi = ps[4], vpChi = ps[5];
    const double deltaPlane = (double)(float)sqrt(planeChi), deltaVP = (double)(float)sqrt(vpChi);
    size_t nPlaneEdges = 0;
    for (int f = 0; f < n; f++)
        for (int i = p->plane_offsets[f]; i < p->plane_offsets[f + 1]; i++) {
            const int m = p->plane_mask[i];
            nPlaneEdges += (m & DRFE_POSE_OPT_PLANE_MATCHED) ? 1 : 0;
            if (p->b_struct[f]) nPlaneEdges += ((m & DRFE_POSE_OPT_PLANE_PARALLEL) ? 1 : 0) + ((m & DRFE_POSE_OPT_PLANE_VERTICAL) ? 1 : 0);
        }
    if (nP > 0 && (!p->obs || !p->u_right || !p->inv_sigma2 || !p->Xw || !o->point_outlier)) return DRFE_ERR_INVALID;
    if (nL > 0 && (!p->line_fn || !p->line_ends || !o->line_outlier)) return DRFE_ERR_INVALID;
    P.frame.resize((size_t)n);
    P.edge.resize((size_t)nP + 2 * (size_t)nL + nPlaneEdges);
    size_t at = 0;
    for (int f = 0; f < n; f++) {
        PoFrameRec& F = P.frame[(size_t)f];
        std::memcpy(F.Tcw, p->Tcw + 16 * (size_t)f, sizeof(F.Tcw));
        const float* K = p->K + 4 * (size_t)f;
        F.cam = PoCam{(double)K[0], (double)K[1], (double)K[2], (double)K[3], (double)p->bf[f]};
        F.edge0 = (int32_t)at;
        F.nPoints = p->point_offsets[f + 1] - p->point_offsets[f];
        F.nLines = p->line_offsets[f + 1] - p->line_offsets[f];
        F.pad[0] = F.pad[1] = F.pad[2] = 0;
        for (int i = p->point_offsets[f]; i < p->point_offsets[f + 1]; i++) {
            PoEdge& E = P.edge[at++];
            const float ur = p->u_right[i];
            E = PoEdge{};
            E.kind = ur < 0 ? PO_MONO : PO_STEREO;
            E.obs[0] = (double)p->obs[2 * (size_t)i];
            E.obs[1] = (double)p->obs[2 * (size_t)i + 1];
            E.obs[2] = ur < 0 ? 0.0 : (double)ur;
            for (int k = 0; k < 3; k++) E.X[k] = (double)p->Xw[3 * (size_t)i + k];
            for (int k = 0; k < 3; k++) E.info[k] = (double)p->inv_sigma2[i];
            E.delta = ur < 0 ? po_delta_mono() : po_delta_stereo();
            E.th = ur < 0 ? po_th_mono() : po_th_stereo();
        }
        for (int i = p->line_offsets[f]; i < p->line_offsets[f + 1]; i++)
            for (int end = 0; end < 2; end++) {
                PoEdge& E = P.edge[at++];
                E = PoEdge{};
                E.kind = PO_LINE;
                for (int k = 0; k < 3; k++) {
                    E.obs[k] = p->line_fn[3 * (size_t)i + k];
                    E.X[k] = p->line_ends[6 * (size_t)i + 3 * end + k];
                    E.info[k] = 1.0;
                }
                E.delta = po_delta_stereo();
                E.th = po_th_line();
            }
        /* the matched planes of every slot, then with bStruct the parallel ones, then the vertical ones */
        const size_t plane0 = at;
        for (int pass = 0; pass < (p->b_struct[f] ? 3 : 1); pass++)
            for (int i = p->plane_offsets[f]; i < p->plane_offsets[f + 1]; i++) {
                if (!(p->plane_mask[i] & (1 << pass))) continue;
                PoEdge& E = P.edge[at++];
                E = PoEdge{};
                E.kind = PO_PLANE + pass;
                po_to_plane3d(p->plane_meas + 4 * (size_t)i, E.obs);
                po_to_plane3d(p->plane_world + 12 * (size_t)i + 4 * pass, E.X);
                const double w = pass == 0 ? angleInfo : pass == 1 ? parInfo : verInfo;
                E.info[0] = w; E.info[1] = w; E.info[2] = pass == 0 ? disInfo : 0.0;
                E.delta = pass == 0 ? deltaPlane : deltaVP;
                E.th = pass == 0 ? planeChi : vpChi;
            }
        F.nPlaneEdges = (int32_t)(at - plane0);
        F.nEdges = F.nPoints + 2 * F.nLines + F.nPlaneEdges;
    }
    return DRFE_OK;
}

/* computeActiveErrors and activeRobustChi2: the active edges in order */
double host_errors(const PoFrameRec& F, const PoEdge* E, const uint8_t* flag, PoLM& S, int robust, double* err)
{
    double chi = 0.0;
    for (int k = 0; k < F.nEdges; k++) {
        if (flag[k]) continue;
        po_edge_error(S.lm.ctx, E[k], F.cam, S.q, S.t, err + 3 * (size_t)k);
        chi += po_chi_term(E[k], err + 3 * (size_t)k, robust);
    }
    return chi;
}

/* one frame on the host: the four rounds (src/Optimizer.cc:1049-1330) */
void host_frame(const PoFrameRec& F, const PoEdge* E, uint8_t* flag, PoFrameOut& O)
{
    std::memset(&O, 0, sizeof(O));
    std::memcpy(O.Tcw, F.Tcw, sizeof(O.Tcw));
    std::memset(flag, 0, (size_t)F.nEdges);
    const int nInitial = F.nPoints + F.nLines + F.nPlaneEdges;
    if (nInitial < 3) return;
    std::vector<double> err(3 * (size_t)F.nEdges, 0.0);
    PoLM S;
    lm_init(S.lm, 1);
    int robust = 1, nBad = 0;
    for (int it = 0; it < 4; it++) {
        mp_to_se3quat(F.Tcw, S.q, S.t);
        S.lm.lastRejected = 0;
        int nActive = 0;
        for (int k = 0; k < F.nEdges; k++) nActive += flag[k] ? 0 : 1;
        if (nActive == 0) O.diag[PO_DIAG_EMPTY_ROUNDS]++;       /* optimize() returns before its first iteration: no active vertex */
        for (int i = 0; i < 10 && nActive > 0; i++) {
            const double chi = host_errors(F, E, flag, S, robust, err.data());
            for (int r = 0; r < PO_H_TERMS; r++) S.lm.H[r] = 0.0;
            for (int r = 0; r < 6; r++) S.lm.b[r] = 0.0;
            for (int k = 0; k < F.nEdges; k++) {
                if (flag[k]) continue;
                double J[3][6], term[PO_TERMS];
                if (po_is_plane(E[k].kind)) po_plane_jacobian(S.lm.ctx, E[k], S.q, S.t, J);
                else po_edge_jacobian(E[k], F.cam, S.q, S.t, J);
                po_edge_terms(E[k], J, err.data() + 3 * (size_t)k, robust, term);
                for (int r = 0; r < PO_H_TERMS; r++) S.lm.H[r] += term[r];
                for (int r = 0; r < 6; r++) S.lm.b[r] -= term[PO_H_TERMS + r];
            }
            lm_begin(S.lm, i, chi);
            int more;
            do {
                lm_step(S);
                more = lm_judge(S, host_errors(F, E, flag, S, robust, err.data()));
            } while (more);
            if (!lm_end(S.lm)) break;
        }
        O.rounds++;
        if (S.lm.lastRejected) O.diag[PO_DIAG_LAST_REJECTED]++;
        nBad = 0;
        const int line0 = F.nPoints, plane0 = F.nPoints + 2 * F.nLines;
        for (int k = 0; k < F.nEdges; k++) {
            if (k >= line0 && k < plane0) continue;
            if (flag[k]) po_edge_error(S.lm.ctx, E[k], F.cam, S.q, S.t, err.data() + 3 * (size_t)k);
            flag[k] = (uint8_t)po_outlier(E[k], err.data() + 3 * (size_t)k);
            nBad += flag[k];
        }
        for (int l = 0; l < F.nLines; l++) {
            const int k = line0 + 2 * l;
            po_edge_error(S.lm.ctx, E[k], F.cam, S.q, S.t, err.data() + 3 * (size_t)k);
            po_edge_error(S.lm.ctx, E[k + 1], F.cam, S.q, S.t, err.data() + 3 * (size_t)(k + 1));
            const int out = po_outlier(E[k], err.data() + 3 * (size_t)k) || po_outlier(E[k + 1], err.data() + 3 * (size_t)(k + 1));
            flag[k] = flag[k + 1] = (uint8_t)out;
            nBad += out;
        }
        if (it == 2) robust = 0;
        if (F.nEdges < 10) break;
    }
    po_pose_out(S.q, S.t, O.Tcw);
    O.ret = nInitial - nBad;
    O.iterations = S.lm.iterations;
    O.trials = S.lm.trials;
    O.diag[PO_DIAG_REJECTED] = S.lm.rejected;
    O.diag[PO_DIAG_NBAD_STOPS] = S.lm.nBadStops;
    O.diag[PO_DIAG_SMALL_THETA] = S.lm.smallTheta;
    O.diag[PO_DIAG_BIG_THETA] = S.lm.bigTheta;
}

/* a frame's record and per-edge flags into the caller's arrays */
void write_frame(const drfe_pose_opt_problems* p, int f, const PoFrameRec& F, const PoFrameOut& O, const uint8_t* flag,
                 drfe_pose_opt_out* o)
{
    std::memcpy(o->Tcw + 16 * (size_t)f, O.Tcw, sizeof(O.Tcw));
    o->returns[f] = O.ret;
    o->rounds[f] = O.rounds;
    o->iterations[f] = O.iterations;
    o->trials[f] = O.trials;
    if (o->diag) std::memcpy(o->diag + PO_DIAG_N * (size_t)f, O.diag, sizeof(O.diag));
    if (F.nPoints) std::memcpy(o->point_outlier + p->point_offsets[f], flag, (size_t)F.nPoints);
    for (int l = 0; l < F.nLines; l++) o->line_outlier[p->line_offsets[f] + l] = flag[F.nPoints + 2 * l];
    int k = F.nPoints + 2 * F.nLines;
    uint8_t* const planeOut[3] = {o->plane_outlier, o->par_plane_outlier, o->ver_plane_outlier};
    for (int pass = 0; pass < 3; pass++)
        for (int i = p->plane_offsets[f]; i < p->plane_offsets[f + 1]; i++) {
            const bool edge = (pass == 0 || p->b_struct[f]) && (p->plane_mask[i] & (1 << pass));
            planeOut[pass][i] = edge ? flag[k++] : 0;
        }
}

}  // namespace

extern "C" {

int drfe_pose_opt_host(const drfe_pose_opt_problems* p, drfe_pose_opt_out* o)
{
    Plan P;
    std::string err;
    const int rc = make_plan(p, o, P, err);
    if (rc || p->n == 0) return rc;
    std::vector<uint8_t> flag;
    for (int f = 0; f < p->n; f++) {
        const PoFrameRec& F = P.frame[(size_t)f];
        flag.assign((size_t)F.nEdges + 1, 0);
        PoFrameOut O;
        host_frame(F, P.edge.data() + F.edge0, flag.data(), O);
        write_frame(p, f, F, O, flag.data(), o);
    }
    return DRFE_OK;
}

int drfe_pose_opt_batch(drfe_ctx* c, const drfe_pose_opt_problems* p, drfe_pose_opt_out* o, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    Plan P;
    const int rc = make_plan(p, o, P, c->err);
    if (rc) return rc;
    PoseOptBuffers* b = batch_buffers(c->pose_opt);
    b->stats[0]++;
    if (p->n == 0) return DRFE_OK;
    const int n = p->n;
    const size_t nE = P.edge.size();
    StageLayout<16> in, out, scr;
    const auto sFrame = in.add<PoFrameRec>((size_t)n);
    const auto sEdge = in.add<PoEdge>(nE);
    const auto sOut = out.add<PoFrameOut>((size_t)n);
    const auto sFlag = out.add<uint8_t>(nE);
    const auto sErr = scr.add<double>(3 * nE);
    hipStream_t st;
    if (const int e = batch_begin(c, b, stream, in.bytes(), out.bytes(), scr.bytes(), &st)) return e;
    char* h = b->io.hin;
    sFrame.put(h, P.frame.data());
    sEdge.put(h, P.edge.data());
    const char* d = b->io.din;
    char* dO = b->io.dout;
    char* dS = b->scratch;
    if (const int e = batch_upload(c, b, in.bytes(), out.bytes(), st)) return e;
    PoLaunch L{};
    L.nFrames = n;
    L.frame = sFrame.at(d);
    L.edge = sEdge.at(d);
    L.err = sErr.at(dS);
    L.flag = sFlag.at(dO);
    L.out = sOut.at(dO);
    if (const int e = batch_finish(c, "pose_opt", drfe_launch_pose_opt(L, st), b, out.bytes(), st)) return e;
    const char* ho = b->io.hout;
    std::vector<uint8_t> flag;
    for (int f = 0; f < n; f++) {
        const PoFrameRec& F = P.frame[(size_t)f];
        const PoFrameOut* O = sOut.at(ho) + f;
        const uint8_t* fl = sFlag.at(ho) + F.edge0;
        PoFrameOut redo;
        if (O->handBack || (b->handBackEvery > 0 && f % b->handBackEvery == 0)) {
            /* what the device could not certify: the host core runs the frame again, with the host's libm where it is needed */
            flag.assign((size_t)F.nEdges + 1, 0);
            host_frame(F, P.edge.data() + F.edge0, flag.data(), redo);
            O = &redo;
            fl = flag.data();
            b->stats[6]++;
        }
        write_frame(p, f, F, *O, fl, o);
        b->stats[1]++;
        b->stats[2] += F.nPoints;
        b->stats[3] += 2 * (int64_t)F.nLines + F.nPlaneEdges;
        b->stats[4] += O->iterations;
        b->stats[5] += O->trials;
        if (F.nPoints + F.nLines + F.nPlaneEdges < 3) b->stats[7]++;
    }
    return DRFE_OK;
}

int drfe_pose_opt_stats(drfe_ctx* c, int64_t* stats) { return batch_stats(c, &drfe_ctx::pose_opt, stats); }

int drfe_debug_pose_opt_hand_back(drfe_ctx* c, int every) { return batch_hand_back(c, &drfe_ctx::pose_opt, every); }

int drfe_debug_cr_cube(const double* x, int n, double* out, uint8_t* ok)
{
    if (n < 0 || (n > 0 && (!x || !out || !ok))) return DRFE_ERR_INVALID;
    for (int i = 0; i < n; i++) {
        out[i] = 0.0;
        ok[i] = (uint8_t)drfe_cr_cube(x[i], out + i);
    }
    return DRFE_OK;
}

int drfe_debug_pose_opt_plane_error(int kind, const float* meas, const float* world, const float* Tcw, double* e)
{
    if (kind < PO_PLANE || kind > PO_VER_PLANE || !meas || !world || !Tcw || !e) return DRFE_ERR_INVALID;
    PoEdge E{};
    E.kind = kind;
    po_to_plane3d(meas, E.obs);
    po_to_plane3d(world, E.X);
    double q[4], t[3];
    mp_to_se3quat(Tcw, q, t);
    LmCtx ctx = {0, 1};
    po_plane_error(ctx, E, q, t, e);
    return DRFE_OK;
}

int drfe_debug_pose_opt_ldlt(const double* A, const double* b, double* x, int32_t* positive)
{
    if (!A || !b || !x || !positive) return DRFE_ERR_INVALID;
    double M[6][6];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) M[i][j] = A[6 * i + j];
    *positive = lm_ldlt_solve<6>(M, b, x);
    return DRFE_OK;
}

}  // extern "C"
