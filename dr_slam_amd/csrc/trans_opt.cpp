/* trans_opt.cpp — Optimizer::TranslationOptimization (reference src/Optimizer.cc:3211-3980) behind the C-ABI of include/drfe.h:
 * the host entry (no context), the batch entry (trans_opt_kernels.hip) and its counters.  Both sides evaluate trans_opt_core.h
 * over the caller's arrays as they are; here are the argument checks and caps, the frame's rounds on the host in the full 6x6
 * form, and the hand-back of a frame the device could not certify or that met a term that is not finite.  DESIGN.md section 21. */
#include "trans_opt_internal.h"
#include "batch_entry.h"
#include "stage_layout.h"
#include "../../include/drfe_debug.h"

#include <cstring>
#include <vector>

struct TransOptBuffers : BatchBuffers {};  /* scratch: _error of every edge; the hand-back counts frames */

void drfe_trans_opt_free(drfe_ctx* c) { batch_free(c->trans_opt); }

namespace {

/* all-or-nothing validation of a call, then its view over the caller's arrays */
int check_call(const drfe_pose_opt_problems* p, const drfe_pose_opt_out* o, ToView& V, std::string& err)
{
    err = "trans_opt: invalid argument";
    if (!p || !o || p->n < 0) return DRFE_ERR_INVALID;
    if (p->n > DRFE_POSE_OPT_MAX_FRAMES) { err = "trans_opt: more than DRFE_POSE_OPT_MAX_FRAMES frames in a call"; return DRFE_ERR_INVALID; }
    const int n = p->n;
    if (n == 0) return DRFE_OK;
    if (!p->Tcw || !p->K || !p->bf || !p->b_struct || !p->point_offsets || !p->line_offsets || !p->plane_offsets) return DRFE_ERR_INVALID;
    if (!o->Tcw || !o->returns || !o->rounds || !o->iterations || !o->trials) return DRFE_ERR_INVALID;
    if (!batch_offsets_ok("trans_opt", p->point_offsets, n, DRFE_POSE_OPT_MAX_POINTS, "point", "DRFE_POSE_OPT_MAX_POINTS points", err) ||
        !batch_offsets_ok("trans_opt", p->line_offsets, n, DRFE_POSE_OPT_MAX_LINES, "line", "DRFE_POSE_OPT_MAX_LINES lines", err) ||
        !batch_offsets_ok("trans_opt", p->plane_offsets, n, DRFE_POSE_OPT_MAX_PLANES, "plane", "DRFE_POSE_OPT_MAX_PLANES plane slots", err))
        return DRFE_ERR_INVALID;
    const int nP = p->point_offsets[n], nL = p->line_offsets[n], nS = p->plane_offsets[n];
    if (nS > 0 && (!p->plane_meas || !p->plane_world || !p->plane_mask || !o->plane_outlier || !o->par_plane_outlier ||
                   !o->ver_plane_outlier))
        return DRFE_ERR_INVALID;
    if (nP > 0 && (!p->obs || !p->u_right || !p->inv_sigma2 || !p->Xw || !o->point_outlier)) return DRFE_ERR_INVALID;
    if (nL > 0 && (!p->line_fn || !p->line_ends || !o->line_outlier)) return DRFE_ERR_INVALID;
    V = ToView{};
    V.Tcw = p->Tcw; V.K = p->K; V.bf = p->bf; V.b_struct = p->b_struct;
    V.point_offsets = p->point_offsets; V.line_offsets = p->line_offsets; V.plane_offsets = p->plane_offsets;
    V.obs = p->obs; V.u_right = p->u_right; V.inv_sigma2 = p->inv_sigma2; V.Xw = p->Xw;
    V.line_fn = p->line_fn; V.line_ends = p->line_ends;
    V.plane_meas = p->plane_meas; V.plane_world = p->plane_world; V.plane_mask = p->plane_mask;
    V.point_outlier = o->point_outlier; V.line_outlier = o->line_outlier;
    V.plane_outlier[0] = o->plane_outlier; V.plane_outlier[1] = o->par_plane_outlier; V.plane_outlier[2] = o->ver_plane_outlier;
    to_view_settings(V, p->plane_settings);
    return DRFE_OK;
}

struct HostFrame {
    const ToView& V;
    ToFrame F;
    uint8_t planeAt[3 * DRFE_POSE_OPT_MAX_PLANES];
    std::vector<PoEdge> E;             /* the frame's edges, formed once: the host entry is a plain loop */
    std::vector<double> err;

    HostFrame(const ToView& v, int f) : V(v)
    {
        to_frame(V, f, F);
        F.nPlaneEdges = to_plane_table(V, f, F, planeAt);
    }
    uint8_t& flag(int k) { return *to_flag(V, F, planeAt, k); }

    /* computeActiveErrors and activeRobustChi2: the active edges in order */
    double errors(PoLM& S, int robust)
    {
        double chi = 0.0;
        for (int k = 0; k < F.nEdges; k++) {
            if (flag(k)) continue;
            to_edge_error(S.lm.ctx, E[(size_t)k], F.cam, S.t, &err[3 * (size_t)k]);
            chi += po_chi_term(E[(size_t)k], &err[3 * (size_t)k], robust);
        }
        return chi;
    }

    /* the frame as the reference runs it (src/Optimizer.cc:3420, :3687-3979); the flags of its features are zero on entry */
    void run(PoFrameOut& O, const float* Tcw)
    {
        std::memset(&O, 0, sizeof(O));
        std::memcpy(O.Tcw, Tcw, sizeof(O.Tcw));
        const int nInitial = F.nPoints;                          /* lines and planes do not count */
        if (nInitial < 3) return;                                /* before the plane edges exist */
        F.nEdges = F.nPoints + 2 * F.nLines + F.nPlaneEdges;
        E.resize((size_t)F.nEdges);
        for (int k = 0; k < F.nEdges; k++) to_make_edge(V, F, planeAt, k, E[(size_t)k]);
        err.assign(3 * (size_t)F.nEdges, 0.0);
        PoLM S;
        lm_init(S.lm, 1);
        int robust = 1, nBad = 0;
        for (int it = 0; it < 4; it++) {
            mp_to_se3quat(Tcw, S.q, S.t);
            S.lm.lastRejected = 0;
            int nActive = 0;
            for (int k = 0; k < F.nEdges; k++) nActive += flag(k) ? 0 : 1;
            if (nActive == 0) O.diag[PO_DIAG_EMPTY_ROUNDS]++;
            for (int i = 0; i < 10 && nActive > 0; i++) {
                const double chi = errors(S, robust);
                for (int r = 0; r < PO_H_TERMS; r++) S.lm.H[r] = 0.0;
                for (int r = 0; r < 6; r++) S.lm.b[r] = 0.0;
                for (int k = 0; k < F.nEdges; k++) {
                    if (flag(k)) continue;
                    const PoEdge& Ek = E[(size_t)k];
                    double J3[3][3], J[3][6], term[PO_TERMS];
                    if (po_is_plane(Ek.kind)) to_plane_jacobian(S.lm.ctx, Ek, S.q, S.t, J3);
                    else to_edge_jacobian(Ek, F.cam, S.t, J3);
                    to_full_jacobian(J3, J);
                    po_edge_terms(Ek, J, &err[3 * (size_t)k], robust, term);
                    for (int r = 0; r < PO_H_TERMS; r++) S.lm.H[r] += term[r];
                    for (int r = 0; r < 6; r++) S.lm.b[r] -= term[PO_H_TERMS + r];
                }
                lm_begin(S.lm, i, chi);
                int more;
                do {
                    lm_step(S);
                    more = lm_judge(S, errors(S, robust));
                } while (more);
                if (!lm_end(S.lm)) break;
            }
            O.rounds++;
            if (S.lm.lastRejected) O.diag[PO_DIAG_LAST_REJECTED]++;
            nBad = 0;                                            /* nLineBad is counted by the reference and not returned */
            const int line0 = F.nPoints, plane0 = F.nPoints + 2 * F.nLines;
            for (int k = 0; k < F.nEdges; k++) {
                if (k >= line0 && k < plane0) continue;
                if (flag(k)) to_edge_error(S.lm.ctx, E[(size_t)k], F.cam, S.t, &err[3 * (size_t)k]);
                flag(k) = (uint8_t)po_outlier(E[(size_t)k], &err[3 * (size_t)k]);
                nBad += flag(k);
            }
            for (int l = 0; l < F.nLines; l++) {
                const int k = line0 + 2 * l;
                if (flag(k)) {
                    to_edge_error(S.lm.ctx, E[(size_t)k], F.cam, S.t, &err[3 * (size_t)k]);
                    to_edge_error(S.lm.ctx, E[(size_t)k + 1], F.cam, S.t, &err[3 * (size_t)(k + 1)]);
                }
                flag(k) = (uint8_t)(po_outlier(E[(size_t)k], &err[3 * (size_t)k]) || po_outlier(E[(size_t)k + 1], &err[3 * (size_t)(k + 1)]));
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
};

void zero_flags(const ToView& V, int f)
{
    ToFrame F;
    to_frame(V, f, F);
    if (F.nPoints) std::memset(V.point_outlier + F.point0, 0, (size_t)F.nPoints);
    if (F.nLines) std::memset(V.line_outlier + F.line0, 0, (size_t)F.nLines);
    for (int pass = 0; pass < 3 && F.nSlots; pass++) std::memset(V.plane_outlier[pass] + F.slot0, 0, (size_t)F.nSlots);
}

void write_record(int f, const PoFrameOut& O, drfe_pose_opt_out* o)
{
    std::memcpy(o->Tcw + 16 * (size_t)f, O.Tcw, sizeof(O.Tcw));
    o->returns[f] = O.ret;
    o->rounds[f] = O.rounds;
    o->iterations[f] = O.iterations;
    o->trials[f] = O.trials;
    if (o->diag) std::memcpy(o->diag + PO_DIAG_N * (size_t)f, O.diag, sizeof(O.diag));
}

void host_frame(const ToView& V, int f, PoFrameOut& O)
{
    zero_flags(V, f);
    HostFrame H(V, f);
    H.run(O, V.Tcw + 16 * (size_t)f);
}

}  // namespace

extern "C" {

int drfe_trans_opt_host(const drfe_pose_opt_problems* p, drfe_pose_opt_out* o)
{
    ToView V;
    std::string err;
    const int rc = check_call(p, o, V, err);
    if (rc || p->n == 0) return rc;
    for (int f = 0; f < p->n; f++) {
        PoFrameOut O;
        host_frame(V, f, O);
        write_record(f, O, o);
    }
    return DRFE_OK;
}

int drfe_trans_opt_batch(drfe_ctx* c, const drfe_pose_opt_problems* p, drfe_pose_opt_out* o, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    ToView V;
    const int rc = check_call(p, o, V, c->err);
    if (rc) return rc;
    TransOptBuffers* b = batch_buffers(c->trans_opt);
    b->stats[0]++;
    if (p->n == 0) return DRFE_OK;
    const size_t n = (size_t)p->n;
    const size_t nP = (size_t)p->point_offsets[n], nL = (size_t)p->line_offsets[n], nS = (size_t)p->plane_offsets[n];
    /* the caller's arrays as they are: one block, one copy */
    StageLayout<16> in, out, scr;
    const auto sTcw = in.add<float>(16 * n);
    const auto sK = in.add<float>(4 * n);
    const auto sBf = in.add<float>(n);
    const auto sStruct = in.add<uint8_t>(n);
    const auto sPointOff = in.add<int32_t>(n + 1);
    const auto sLineOff = in.add<int32_t>(n + 1);
    const auto sPlaneOff = in.add<int32_t>(n + 1);
    const auto sObs = in.add<float>(2 * nP);
    const auto sUr = in.add<float>(nP);
    const auto sInv = in.add<float>(nP);
    const auto sXw = in.add<float>(3 * nP);
    const auto sLineFn = in.add<double>(3 * nL);
    const auto sLineEnds = in.add<double>(6 * nL);
    const auto sMeas = in.add<float>(4 * nS);
    const auto sWorld = in.add<float>(12 * nS);
    const auto sMask = in.add<uint8_t>(nS);
    const auto sOut = out.add<PoFrameOut>(n);
    const auto sPointFlag = out.add<uint8_t>(nP);
    const auto sLineFlag = out.add<uint8_t>(nL);
    const auto sPlaneFlag = out.add<uint8_t>(3 * nS);
    const auto sErr = scr.add<double>(3 * (nP + 2 * nL + 3 * nS));
    hipStream_t st;
    if (const int e = batch_begin(c, b, stream, in.bytes(), out.bytes(), scr.bytes(), &st)) return e;
    char* h = b->io.hin;
    sTcw.put(h, p->Tcw); sK.put(h, p->K); sBf.put(h, p->bf); sStruct.put(h, p->b_struct);
    sPointOff.put(h, p->point_offsets); sLineOff.put(h, p->line_offsets); sPlaneOff.put(h, p->plane_offsets);
    sObs.put(h, p->obs); sUr.put(h, p->u_right); sInv.put(h, p->inv_sigma2); sXw.put(h, p->Xw);
    sLineFn.put(h, p->line_fn); sLineEnds.put(h, p->line_ends);
    sMeas.put(h, p->plane_meas); sWorld.put(h, p->plane_world); sMask.put(h, p->plane_mask);
    const char* d = b->io.din;
    char* dO = b->io.dout;
    if (const int e = batch_upload(c, b, in.bytes(), out.bytes(), st)) return e;
    ToLaunch L{};
    L.nFrames = p->n;
    L.view = V;                                    /* the settings; every pointer is replaced */
    L.view.Tcw = sTcw.at(d); L.view.K = sK.at(d); L.view.bf = sBf.at(d); L.view.b_struct = sStruct.at(d);
    L.view.point_offsets = sPointOff.at(d); L.view.line_offsets = sLineOff.at(d); L.view.plane_offsets = sPlaneOff.at(d);
    L.view.obs = sObs.at(d); L.view.u_right = sUr.at(d); L.view.inv_sigma2 = sInv.at(d); L.view.Xw = sXw.at(d);
    L.view.line_fn = sLineFn.at(d); L.view.line_ends = sLineEnds.at(d);
    L.view.plane_meas = sMeas.at(d); L.view.plane_world = sWorld.at(d); L.view.plane_mask = sMask.at(d);
    L.view.point_outlier = sPointFlag.at(dO); L.view.line_outlier = sLineFlag.at(dO);
    for (int pass = 0; pass < 3; pass++) L.view.plane_outlier[pass] = sPlaneFlag.at(dO) + pass * nS;
    char* dS = b->scratch;
    L.err = sErr.at(dS);
    L.lineErr0 = (int64_t)nP;
    L.planeErr0 = (int64_t)(nP + 2 * nL);
    L.out = sOut.at(dO);
    if (const int e = batch_finish(c, "trans_opt", drfe_launch_trans_opt(L, st), b, out.bytes(), st)) return e;
    const char* ho = b->io.hout;
    /* the flags are in the caller's layout already */
    sPointFlag.get(ho, o->point_outlier);
    sLineFlag.get(ho, o->line_outlier);
    if (nS) {
        std::memcpy(o->plane_outlier, sPlaneFlag.at(ho), nS);
        std::memcpy(o->par_plane_outlier, sPlaneFlag.at(ho) + nS, nS);
        std::memcpy(o->ver_plane_outlier, sPlaneFlag.at(ho) + 2 * nS, nS);
    }
    for (int f = 0; f < p->n; f++) {
        const PoFrameOut* O = sOut.at(ho) + f;
        PoFrameOut redo;
        if (O->handBack || (b->handBackEvery > 0 && f % b->handBackEvery == 0)) {
            /* a transcendental the device could not certify, or a term that is not finite, which the nine sums do not carry:
             * the host runs the frame again in the full form */
            host_frame(V, f, redo);
            O = &redo;
            b->stats[6]++;
        }
        write_record(f, *O, o);
        const int nPf = p->point_offsets[f + 1] - p->point_offsets[f], nLf = p->line_offsets[f + 1] - p->line_offsets[f];
        int nPlaneEdges = 0;
        for (int i = p->plane_offsets[f]; nPf >= 3 && i < p->plane_offsets[f + 1]; i++)
            for (int pass = 0; pass < (p->b_struct[f] ? 3 : 1); pass++) nPlaneEdges += (p->plane_mask[i] >> pass) & 1;
        b->stats[1]++;
        b->stats[2] += nPf;
        b->stats[3] += 2 * (int64_t)nLf + nPlaneEdges;
        b->stats[4] += O->iterations;
        b->stats[5] += O->trials;
        if (nPf < 3) b->stats[7]++;
    }
    return DRFE_OK;
}

int drfe_trans_opt_stats(drfe_ctx* c, int64_t* stats) { return batch_stats(c, &drfe_ctx::trans_opt, stats); }

int drfe_debug_trans_opt_hand_back(drfe_ctx* c, int every) { return batch_hand_back(c, &drfe_ctx::trans_opt, every); }

int drfe_debug_trans_opt_plane_error(int kind, const float* meas, const float* world, const float* Tcw, double* e)
{
    if (kind < PO_PLANE || kind > PO_VER_PLANE || !meas || !world || !Tcw || !e) return DRFE_ERR_INVALID;
    /* one slot of one frame whose only map plane is of this kind */
    const int pass = kind - PO_PLANE;
    float w[12] = {0};
    std::memcpy(w + 4 * pass, world, 4 * sizeof(float));
    const uint8_t mask = (uint8_t)(1 << pass), bStruct = 1;
    const int32_t none[2] = {0, 0}, one[2] = {0, 1};
    const float K[4] = {1, 1, 0, 0}, bf = 0;
    ToView V{};
    V.Tcw = Tcw; V.K = K; V.bf = &bf; V.b_struct = &bStruct;
    V.point_offsets = none; V.line_offsets = none; V.plane_offsets = one;
    V.plane_meas = meas; V.plane_world = w; V.plane_mask = &mask;
    ToFrame F;
    to_frame(V, 0, F);
    uint8_t planeAt[3];
    F.nPlaneEdges = to_plane_table(V, 0, F, planeAt);
    PoEdge E;
    to_make_edge(V, F, planeAt, 0, E);
    double q[4], t[3];
    mp_to_se3quat(Tcw, q, t);
    LmCtx ctx = {0, 1};
    to_edge_error(ctx, E, F.cam, t, e);
    return DRFE_OK;
}

}  // extern "C"
