/* sim3_opt.cpp — Optimizer::OptimizeSim3 (reference src/Optimizer.cc:3982-4177) behind the C-ABI of include/drfe.h: the host
 * entry (no context), the batch entry (sim3_opt_kernels.hip) and its counters.  Both sides evaluate sim3_opt_core.h; here are the
 * argument checks and caps, the match list of a call, a problem's two optimize() calls on the host, the free-scale problems the
 * batch entry keeps on the host, and the hand-back of a problem whose sin / cos or cube the device could not certify.  DESIGN.md
 * section 22. */
#include "sim3_opt_internal.h"
#include "batch_entry.h"
#include "stage_layout.h"
#include "../../include/drfe_debug.h"

#include <cstring>
#include <vector>

struct Sim3OptBuffers : BatchBuffers {};   /* scratch: _error of every edge; the hand-back counts problems */

void drfe_sim3_opt_free(drfe_ctx* c) { batch_free(c->sim3_opt); }

namespace {

struct Plan {
    std::vector<SoProbRec> prob;
    std::vector<SoMatch> match;
};

/* all-or-nothing validation of a call, then its problems and matches */
int make_plan(const drfe_sim3_opt_problems* p, const drfe_sim3_opt_out* o, Plan& P, std::string& err)
{
    err = "sim3_opt: invalid argument";
    if (!p || !o || p->n < 0) return DRFE_ERR_INVALID;
    if (p->n > DRFE_SIM3_OPT_MAX_PROBLEMS) { err = "sim3_opt: more than DRFE_SIM3_OPT_MAX_PROBLEMS problems in a call"; return DRFE_ERR_INVALID; }
    const int n = p->n;
    if (n == 0) return DRFE_OK;
    if (!p->S12 || !p->K1 || !p->K2 || !p->R1w || !p->t1w || !p->R2w || !p->t2w || !p->th2 || !p->fix_scale || !p->match_offsets)
        return DRFE_ERR_INVALID;
    if (!o->S12 || !o->T12 || !o->Scw || !o->returns || !o->n_bad || !o->iterations || !o->trials) return DRFE_ERR_INVALID;
    const int32_t* off = p->match_offsets;
    if (off[0] != 0) { err = "sim3_opt: match_offsets[0] is not 0"; return DRFE_ERR_INVALID; }
    for (int f = 0; f < n; f++) {
        if (off[f + 1] < off[f]) { err = "sim3_opt: decreasing match_offsets"; return DRFE_ERR_INVALID; }
        if (off[f + 1] - off[f] > DRFE_SIM3_OPT_MAX_MATCHES) {
            err = "sim3_opt: more than DRFE_SIM3_OPT_MAX_MATCHES matches in a problem";
            return DRFE_ERR_INVALID;
        }
    }
    const int nM = off[n];
    if (nM > 0 && (!p->P3D1w || !p->P3D2w || !p->obs1 || !p->obs2 || !p->inv_sigma2_1 || !p->inv_sigma2_2 || !o->outlier))
        return DRFE_ERR_INVALID;
    if (p->index)
        for (int f = 0; f < n; f++)
            for (int i = off[f]; i < off[f + 1]; i++)
                if (p->index[i] < 0 || (i > off[f] && p->index[i] <= p->index[i - 1])) {
                    err = "sim3_opt: index is not increasing within a problem";
                    return DRFE_ERR_INVALID;
                }
    P.prob.resize((size_t)n);
    P.match.resize((size_t)nM);
    for (int f = 0; f < n; f++) {
        SoProbRec& R = P.prob[(size_t)f];
        std::memcpy(R.S12, p->S12 + 8 * (size_t)f, sizeof(R.S12));
        for (int k = 0; k < 4; k++) {
            R.cam.K1[k] = (double)p->K1[4 * (size_t)f + k];
            R.cam.K2[k] = (double)p->K2[4 * (size_t)f + k];
        }
        const float th2 = p->th2[f];
        R.cam.delta = (double)sqrtf(th2);
        R.cam.th2 = (double)th2;
        std::memcpy(R.R2w, p->R2w + 9 * (size_t)f, sizeof(R.R2w));
        std::memcpy(R.t2w, p->t2w + 3 * (size_t)f, sizeof(R.t2w));
        R.match0 = off[f];
        R.nMatches = off[f + 1] - off[f];
        R.fixScale = p->fix_scale[f] ? 1 : 0;
        R.pad = 0;
        for (int i = off[f]; i < off[f + 1]; i++) {
            SoMatch& M = P.match[(size_t)i];
            so_camera_point(p->R1w + 9 * (size_t)f, p->t1w + 3 * (size_t)f, p->P3D1w + 3 * (size_t)i, M.P1c);
            so_camera_point(p->R2w + 9 * (size_t)f, p->t2w + 3 * (size_t)f, p->P3D2w + 3 * (size_t)i, M.P2c);
            for (int k = 0; k < 2; k++) {
                M.obs1[k] = (double)p->obs1[2 * (size_t)i + k];
                M.obs2[k] = (double)p->obs2[2 * (size_t)i + k];
            }
            M.info1 = (double)p->inv_sigma2_1[i];
            M.info2 = (double)p->inv_sigma2_2[i];
        }
    }
    return DRFE_OK;
}

/* computeActiveErrors and activeRobustChi2: the active edges in order, e12 then e21 of every kept match */
double host_errors(const SoProbRec& P, const SoMatch* M, const uint8_t* flag, const SoSim3& S, double* err)
{
    SoSim3 Sinv;
    so_inverse(S, Sinv);
    double chi = 0.0;
    for (int m = 0; m < P.nMatches; m++) {
        if (flag[m]) continue;
        for (int kind = 0; kind < 2; kind++) {
            double* e = err + 4 * (size_t)m + 2 * kind;
            so_edge_error(M[m], P.cam, kind, S, Sinv, e);
            chi += so_chi_term(kind ? M[m].info2 : M[m].info1, P.cam.delta, e);
        }
    }
    return chi;
}

/* one problem on the host: optimize(5), the first classification, optimize(5 or 10), the second (src/Optimizer.cc:4116-4176) */
void host_problem(const SoProbRec& P, const SoMatch* M, uint8_t* flag, SoProbOut& O)
{
    std::memset(&O, 0, sizeof(O));
    std::memset(flag, 0, (size_t)P.nMatches);
    std::vector<double> err(4 * (size_t)P.nMatches + 1, 0.0);
    SoLM L;
    so_lm_init(L, P.S12, P.fixScale, 1);
    const SoSim3 S0 = L.S;
    int nBad = 0, early = 0;
    for (int phase = 0; phase < 2; phase++) {
        const int iters = phase == 0 ? 5 : (nBad > 0 ? 10 : 5);
        const int it0 = L.lm.iterations, tr0 = L.lm.trials;
        L.lm.lastRejected = 0;
        int nActive = 0;
        for (int m = 0; m < P.nMatches; m++) nActive += flag[m] ? 0 : 1;
        for (int i = 0; i < iters && nActive > 0; i++) {
            const double chi = host_errors(P, M, flag, L.S, err.data());
            SoSim3 pert[14], pinv[14];
            for (int j = 0; j < 14; j++) so_perturbed(L.lm.ctx, L.S, P.fixScale, j, pert[j], pinv[j]);
            for (int r = 0; r < SO_H_TERMS; r++) L.lm.H[r] = 0.0;
            for (int r = 0; r < 7; r++) L.lm.b[r] = 0.0;
            const double scalar = lm_numeric_scalar();
            for (int m = 0; m < P.nMatches; m++) {
                if (flag[m]) continue;
                for (int kind = 0; kind < 2; kind++) {
                    double J[2][7], term[SO_TERMS];
                    for (int d = 0; d < 7; d++) {
                        double e1[2], e2[2];
                        so_edge_error(M[m], P.cam, kind, pert[2 * d], pinv[2 * d], e1);
                        so_edge_error(M[m], P.cam, kind, pert[2 * d + 1], pinv[2 * d + 1], e2);
                        for (int r = 0; r < 2; r++) J[r][d] = scalar * (e1[r] - e2[r]);
                    }
                    so_edge_terms(kind ? M[m].info2 : M[m].info1, P.cam.delta, J, err.data() + 4 * (size_t)m + 2 * kind, term);
                    for (int r = 0; r < SO_H_TERMS; r++) L.lm.H[r] += term[r];
                    for (int r = 0; r < 7; r++) L.lm.b[r] += term[SO_H_TERMS + r];
                }
            }
            lm_begin(L.lm, i, chi);
            int more;
            do {
                lm_step(L);
                const double tempChi = host_errors(P, M, flag, L.S, err.data());
                more = lm_judge(L, tempChi);
            } while (more);
            if (!lm_end(L.lm)) break;
        }
        O.iterations[phase] = L.lm.iterations - it0;
        O.trials[phase] = L.lm.trials - tr0;
        if (L.lm.lastRejected) O.diag[SO_DIAG_LAST_REJECTED]++;
        /* no computeError() precedes the classification: _error is what the last trial left, also a rejected one */
        SoSim3 Sinv;
        so_inverse(L.S, Sinv);
        int count = 0;
        for (int m = 0; m < P.nMatches; m++) {
            if (flag[m]) continue;
            const int out = so_outlier(M[m], P.cam.th2, err.data() + 4 * (size_t)m);
            if (L.lm.lastRejected) {
                double e[4];
                so_edge_error(M[m], P.cam, 0, L.S, Sinv, e);
                so_edge_error(M[m], P.cam, 1, L.S, Sinv, e + 2);
                if (so_outlier(M[m], P.cam.th2, e) != out) O.diag[SO_DIAG_STALE_DECIDED]++;
            }
            flag[m] = (uint8_t)out;
            count += out;
        }
        if (phase == 0) {
            nBad = count;
            if (P.nMatches - nBad < 10) { early = 1; break; }
        } else {
            O.ret = nActive - count;
        }
    }
    O.nBad = nBad;
    O.diag[SO_DIAG_REJECTED] = L.lm.rejected;
    O.diag[SO_DIAG_NBAD_STOPS] = L.lm.nBadStops;
    O.diag[SO_DIAG_SMALL_THETA] = L.lm.smallTheta;
    O.diag[SO_DIAG_BIG_THETA] = L.lm.bigTheta;
    O.diag[SO_DIAG_EARLY_RETURN] = early;
    so_finish(P, early ? S0 : L.S, O);
}

/* a problem's record and per-match flags into the caller's arrays */
void write_problem(int f, const SoProbRec& P, const SoProbOut& O, const uint8_t* flag, drfe_sim3_opt_out* o)
{
    std::memcpy(o->S12 + 8 * (size_t)f, O.S12, sizeof(O.S12));
    std::memcpy(o->T12 + 16 * (size_t)f, O.T12, sizeof(O.T12));
    std::memcpy(o->Scw + 16 * (size_t)f, O.Scw, sizeof(O.Scw));
    o->returns[f] = O.ret;
    o->n_bad[f] = O.nBad;
    for (int k = 0; k < 2; k++) {
        o->iterations[2 * (size_t)f + k] = O.iterations[k];
        o->trials[2 * (size_t)f + k] = O.trials[k];
    }
    if (o->diag) std::memcpy(o->diag + SO_DIAG_N * (size_t)f, O.diag, sizeof(O.diag));
    if (P.nMatches) std::memcpy(o->outlier + P.match0, flag, (size_t)P.nMatches);
}

}  // namespace

extern "C" {

int drfe_sim3_opt_host(const drfe_sim3_opt_problems* p, drfe_sim3_opt_out* o)
{
    Plan P;
    std::string err;
    const int rc = make_plan(p, o, P, err);
    if (rc || p->n == 0) return rc;
    std::vector<uint8_t> flag;
    for (int f = 0; f < p->n; f++) {
        const SoProbRec& R = P.prob[(size_t)f];
        flag.assign((size_t)R.nMatches + 1, 0);
        SoProbOut O;
        host_problem(R, P.match.data() + R.match0, flag.data(), O);
        write_problem(f, R, O, flag.data(), o);
    }
    return DRFE_OK;
}

int drfe_sim3_opt_batch(drfe_ctx* c, const drfe_sim3_opt_problems* p, drfe_sim3_opt_out* o, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    Plan P;
    const int rc = make_plan(p, o, P, c->err);
    if (rc) return rc;
    Sim3OptBuffers* b = batch_buffers(c->sim3_opt);
    b->stats[0]++;
    if (p->n == 0) return DRFE_OK;
    const int n = p->n;
    const size_t nM = P.match.size();
    StageLayout<16> in, out, scr;
    const auto sProb = in.add<SoProbRec>((size_t)n);
    const auto sMatch = in.add<SoMatch>(nM);
    const auto sOut = out.add<SoProbOut>((size_t)n);
    const auto sFlag = out.add<uint8_t>(nM);
    const auto sErr = scr.add<double>(4 * nM);
    hipStream_t st;
    if (const int e = batch_begin(c, b, stream, in.bytes(), out.bytes(), scr.bytes(), &st)) return e;
    char* h = b->io.hin;
    sProb.put(h, P.prob.data());
    sMatch.put(h, P.match.data());
    const char* d = b->io.din;
    char* dO = b->io.dout;
    char* dS = b->scratch;
    if (const int e = batch_upload(c, b, in.bytes(), out.bytes(), st)) return e;
    SoLaunch L{};
    L.nProblems = n;
    L.prob = sProb.at(d);
    L.match = sMatch.at(d);
    L.err = sErr.at(dS);
    L.flag = sFlag.at(dO);
    L.out = sOut.at(dO);
    if (const int e = batch_copy_back(c, "sim3_opt", drfe_launch_sim3_opt(L, st), b, out.bytes(), st)) return e;
    /* the free-scale problems need exp: the host core runs them while the launch is in flight (their workgroups return at once) */
    std::vector<uint8_t> flag;
    for (int f = 0; f < n; f++) {
        const SoProbRec& R = P.prob[(size_t)f];
        if (R.fixScale) continue;
        flag.assign((size_t)R.nMatches + 1, 0);
        SoProbOut O;
        host_problem(R, P.match.data() + R.match0, flag.data(), O);
        write_problem(f, R, O, flag.data(), o);
        b->stats[3]++;
        b->stats[4] += O.iterations[0] + O.iterations[1];
        b->stats[5] += O.trials[0] + O.trials[1];
        if (O.diag[SO_DIAG_EARLY_RETURN]) b->stats[7]++;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    const char* ho = b->io.hout;
    for (int f = 0; f < n; f++) {
        const SoProbRec& R = P.prob[(size_t)f];
        b->stats[1]++;
        b->stats[2] += R.nMatches;
        if (!R.fixScale) continue;
        const SoProbOut* O = sOut.at(ho) + f;
        const uint8_t* fl = sFlag.at(ho) + R.match0;
        SoProbOut redo;
        if (O->handBack || (b->handBackEvery > 0 && f % b->handBackEvery == 0)) {
            /* what the device could not certify: the host core runs the problem again, with the host's libm where it is needed */
            flag.assign((size_t)R.nMatches + 1, 0);
            host_problem(R, P.match.data() + R.match0, flag.data(), redo);
            O = &redo;
            fl = flag.data();
            b->stats[6]++;
        }
        write_problem(f, R, *O, fl, o);
        b->stats[4] += O->iterations[0] + O->iterations[1];
        b->stats[5] += O->trials[0] + O->trials[1];
        if (O->diag[SO_DIAG_EARLY_RETURN]) b->stats[7]++;
    }
    return DRFE_OK;
}

int drfe_sim3_opt_stats(drfe_ctx* c, int64_t* stats) { return batch_stats(c, &drfe_ctx::sim3_opt, stats); }

int drfe_debug_sim3_opt_hand_back(drfe_ctx* c, int every) { return batch_hand_back(c, &drfe_ctx::sim3_opt, every); }

int drfe_debug_sim3_opt_ldlt(const double* A, const double* b, double* x, int32_t* positive)
{
    if (!A || !b || !x || !positive) return DRFE_ERR_INVALID;
    double M[7][7];
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) M[i][j] = A[7 * i + j];
    *positive = lm_ldlt_solve<7>(M, b, x);
    return DRFE_OK;
}

int drfe_debug_sim3_opt_step(const double* S12, const double* x, int fix_scale, int read_before, double* S12_out, double* scale)
{
    if (!S12 || !x || !S12_out || !scale) return DRFE_ERR_INVALID;
    SoLM L;
    so_lm_init(L, S12, fix_scale, 1);
    for (int k = 0; k < 7; k++) { L.lm.x[k] = x[k]; L.lm.b[k] = x[7 + k]; }
    L.lm.lambda = x[14];
    /* the core's own update and computeScale, in the order lm_step and lm_judge run them, or the other way round */
    const double before = lm_scale(L.lm);
    so_lm_update(L);
    *scale = read_before ? before : lm_scale(L.lm);
    for (int k = 0; k < 4; k++) S12_out[k] = L.S.q[k];
    for (int k = 0; k < 3; k++) S12_out[4 + k] = L.S.t[k];
    S12_out[7] = L.S.s;
    return DRFE_OK;
}

}  // extern "C"
