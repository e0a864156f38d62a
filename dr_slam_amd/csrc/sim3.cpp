/* sim3.cpp — Sim3Solver (reference src/Sim3Solver.cc) behind the C-ABI of include/drfe.h: the host entry (no context), the batch
 * entry (sim3_kernels.hip) and its counters.  Both sides evaluate sim3_core.h; what is sequential and cheap — SetRansacParameters'
 * iteration count (the host's libm, :118-142) and the sampling (a glibc rand() stream per solver, :167-181) — runs once, on the
 * host, for both.  The table's scaffold (plan, sampling, scatter, common counters) is ransac_table.h, shared with pnp.cpp; here are
 * the argument checks, the records, the rows on the host and the hand-back path.  DESIGN.md section 16. */
#include "sim3_internal.h"
#include "stage_layout.h"
#include "../../include/drfe_debug.h"

struct Sim3Buffers : BatchBuffers {};  /* scratch: Sim3Corr per correspondence, T21 per hypothesis; the hand-back counts hypotheses */

void drfe_sim3_free(drfe_ctx* c) { batch_free(c->sim3); }

namespace {

enum { SIM3_MAX_SOLVERS = 65535 };     /* the counting kernel's grid has one row per solver */

using Plan = RansacPlan<3, DRFE_SIM3_MAX_CORR>;

int cap_of(const drfe_sim3_problems* p, int s) { return p->max_iterations[s] > 1 ? p->max_iterations[s] : 1; }

/* all-or-nothing validation of a call, then the plan of its table */
int make_plan(const drfe_sim3_problems* p, const drfe_sim3_out* o, Plan& P, std::string& err)
{
    err = "sim3: invalid argument";
    if (!p || !o || p->n < 0 || p->n > SIM3_MAX_SOLVERS) return DRFE_ERR_INVALID;
    const int n = p->n;
    if (n == 0) return DRFE_OK;
    if (!p->Tcw1 || !p->Tcw2 || !p->K1 || !p->K2 || !p->fix_scale || !p->probability || !p->min_inliers || !p->max_iterations ||
        !p->seed || !p->offsets)
        return DRFE_ERR_INVALID;
    if (!o->iterations || !o->hypotheses || !o->sample || !o->R12 || !o->t12 || !o->s12 || !o->T12 || !o->inliers || !o->returns ||
        !o->best || !o->mask)
        return DRFE_ERR_INVALID;
    for (int s = 0; s < n; s++) {
        if (!ransac_offsets_ok(p->offsets, s, DRFE_SIM3_MAX_CORR, "sim3", "DRFE_SIM3_MAX_CORR", err)) return DRFE_ERR_INVALID;
        if (p->max_iterations[s] > DRFE_SIM3_MAX_ITERATIONS) { err = "sim3: max_iterations above DRFE_SIM3_MAX_ITERATIONS"; return DRFE_ERR_INVALID; }
        if (p->min_inliers[s] < 0) { err = "sim3: negative min_inliers"; return DRFE_ERR_INVALID; }
    }
    const int M = p->offsets[n];
    if (M > 0 && (!p->Xw1 || !p->Xw2 || !p->sigma2_1 || !p->sigma2_2)) return DRFE_ERR_INVALID;
    for (int i = 0; i < M; i++)
        for (const float* sg : {p->sigma2_1, p->sigma2_2}) {
            const double b = 9.210 * (double)sg[i];
            if (!(b >= 0.0 && b < 9223372036854775808.0)) { err = "sim3: 9.210 * sigma2 outside [0, 2^63)"; return DRFE_ERR_INVALID; }
        }
    for (int s = 0; s < n; s++) {
        /* SetRansacParameters (:118-142): float epsilon */
        const int N = p->offsets[s + 1] - p->offsets[s], minInliers = p->min_inliers[s];
        const bool single = minInliers == N;
        const int it = ransac_iteration_count(single, single ? 0.f : (float)minInliers / N, p->probability[s], p->max_iterations[s]);
        P.add_solver(N, it, (N < minInliers || N < 3) ? 0 : it, cap_of(p, s), p->seed[s]);
    }
    return DRFE_OK;
}

/* the per-solver outputs, the zeroed table and the samples */
void begin_out(const drfe_sim3_problems* p, const Plan& P, drfe_sim3_out* o)
{
    const size_t rows = (size_t)P.rows;
    std::memset(o->sample, 0, rows * 3 * sizeof(int32_t));
    std::memset(o->R12, 0, rows * 9 * sizeof(float));
    std::memset(o->t12, 0, rows * 3 * sizeof(float));
    std::memset(o->s12, 0, rows * sizeof(float));
    std::memset(o->T12, 0, rows * 12 * sizeof(float));
    std::memset(o->inliers, 0, rows * sizeof(int32_t));
    std::memset(o->returns, 0, rows);
    std::memset(o->best, 0, rows * sizeof(int32_t));
    std::memset(o->mask, 0, (size_t)P.maskWordsOut * sizeof(uint64_t));
    for (int s = 0; s < p->n; s++) {
        o->iterations[s] = P.iterations[(size_t)s];
        o->hypotheses[s] = P.hyp[(size_t)s];
        P.scatter(s, o->sample, P.sample.data(), 3);
    }
}

void solver_corrs(const drfe_sim3_problems* p, int s, std::vector<Sim3Corr>& corr)
{
    const int c0 = p->offsets[s], N = p->offsets[s + 1] - c0;
    corr.resize((size_t)N);
    for (int i = 0; i < N; i++) {
        const size_t g = (size_t)c0 + i;
        corr[(size_t)i] = s3_corr(p->Tcw1 + 12 * (size_t)s, p->Tcw2 + 12 * (size_t)s, p->K1 + 4 * (size_t)s, p->K2 + 4 * (size_t)s,
                                  p->Xw1 + 3 * g, p->Xw2 + 3 * g, p->sigma2_1[g], p->sigma2_2[g]);
    }
}

/* row h of solver s on the host, into the caller's table; a hypothesis the core cannot certify is finished with libm */
void host_row(const drfe_sim3_problems* p, const Plan& P, int s, int h, const std::vector<Sim3Corr>& corr, drfe_sim3_out* o)
{
    const size_t row = (size_t)P.row0[(size_t)s] + h;
    const int32_t* smp = P.sample_of(s, h);
    float P1[9], P2[9];
    for (int q = 0; q < 3; q++)
        for (int r = 0; r < 3; r++) {
            P1[r * 3 + q] = corr[(size_t)smp[q]].c1[r];
            P2[r * 3 + q] = corr[(size_t)smp[q]].c2[r];
        }
    float R[9], t[3], sc, T12[12], T21[12];
    if (!s3_horn(P1, P2, p->fix_scale[s], 0, R, t, &sc, T12, T21)) (void)s3_horn(P1, P2, p->fix_scale[s], 1, R, t, &sc, T12, T21);
    for (int k = 0; k < 9; k++) o->R12[9 * row + k] = s3_canon(R[k]);
    for (int k = 0; k < 3; k++) o->t12[3 * row + k] = s3_canon(t[k]);
    o->s12[row] = s3_canon(sc);
    for (int k = 0; k < 12; k++) o->T12[12 * row + k] = s3_canon(T12[k]);
    const int N = (int)corr.size(), words = P.words[(size_t)s];
    uint64_t* mask = o->mask + P.mask0Out[(size_t)s] + (size_t)h * words;
    int count = 0;
    for (int w = 0; w < words; w++) mask[w] = 0;
    for (int i = 0; i < N; i++)
        if (s3_inlier(corr[(size_t)i], T12, T21, p->K1 + 4 * (size_t)s, p->K2 + 4 * (size_t)s)) {
            mask[i >> 6] |= 1ull << (i & 63);
            count++;
        }
    o->inliers[row] = count;
}

void host_walk(const drfe_sim3_problems* p, const Plan& P, int s, drfe_sim3_out* o)
{
    const size_t row0 = (size_t)P.row0[(size_t)s];
    s3_walk(o->inliers + row0, P.hyp[(size_t)s], p->min_inliers[s], o->returns + row0, o->best + row0);
}

}  // namespace

extern "C" {

int drfe_sim3_ransac_host(const drfe_sim3_problems* p, drfe_sim3_out* o)
{
    Plan P;
    std::string err;
    const int rc = make_plan(p, o, P, err);
    if (rc || p->n == 0) return rc;
    begin_out(p, P, o);
    std::vector<Sim3Corr> corr;
    for (int s = 0; s < p->n; s++) {
        if (!P.hyp[(size_t)s]) continue;
        solver_corrs(p, s, corr);
        for (int h = 0; h < P.hyp[(size_t)s]; h++) host_row(p, P, s, h, corr, o);
        host_walk(p, P, s, o);
    }
    return DRFE_OK;
}

int drfe_sim3_ransac_batch(drfe_ctx* c, const drfe_sim3_problems* p, drfe_sim3_out* o, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    Plan P;
    const int rc = make_plan(p, o, P, c->err);
    if (rc) return rc;
    Sim3Buffers* b = batch_buffers(c->sim3);
    P.count_call(b->stats, p->offsets);
    if (p->n == 0) return DRFE_OK;
    const int n = p->n, M = p->offsets[n], H = P.nHyp;
    for (int s = 0; s < n; s++)
        if (P.hyp[(size_t)s]) b->stats[p->offsets[s + 1] - p->offsets[s] <= DRFE_SIM3_LDS_CORR ? 4 : 5]++;
    begin_out(p, P, o);
    if (H == 0) return DRFE_OK;
    const size_t nM = (size_t)M, nH = (size_t)H;
    StageLayout<16> in, out, scr;
    const auto sSolver = in.add<Sim3Solver>((size_t)n);
    const auto sCorrSolver = in.add<int32_t>(nM);
    const auto sXw1 = in.add<float>(nM * 3), sXw2 = in.add<float>(nM * 3), sSig1 = in.add<float>(nM), sSig2 = in.add<float>(nM);
    const auto sHypSolver = in.add<int32_t>(nH), sSample = in.add<int32_t>(nH * 3);
    const auto sR = out.add<float>(nH * 9), sT = out.add<float>(nH * 3), sS = out.add<float>(nH), sT12 = out.add<float>(nH * 12);
    const auto sInl = out.add<int32_t>(nH), sBest = out.add<int32_t>(nH);
    const auto sRet = out.add<uint8_t>(nH), sUnc = out.add<uint8_t>(nH);
    const auto sMask = out.add<uint64_t>((size_t)P.maskWords);
    const auto sCorr = scr.add<Sim3Corr>(nM);
    const auto sT21 = scr.add<float>(nH * 12);
    hipStream_t st;
    if (const int e = batch_begin(c, b, stream, in.bytes(), out.bytes(), scr.bytes(), &st)) return e;
    char* h = b->io.hin;
    Sim3Solver* sol = sSolver.at(h);
    int32_t* corrSolver = sCorrSolver.at(h);
    for (int s = 0; s < n; s++) {
        Sim3Solver& S = sol[s];
        std::memcpy(S.Tcw1, p->Tcw1 + 12 * (size_t)s, sizeof(S.Tcw1));
        std::memcpy(S.Tcw2, p->Tcw2 + 12 * (size_t)s, sizeof(S.Tcw2));
        std::memcpy(S.K1, p->K1 + 4 * (size_t)s, sizeof(S.K1));
        std::memcpy(S.K2, p->K2 + 4 * (size_t)s, sizeof(S.K2));
        S.fixScale = p->fix_scale[s] ? 1 : 0;
        S.pad = 0;
        S.head = P.head(s, p->offsets, p->min_inliers[s]);
        for (int i = p->offsets[s]; i < p->offsets[s + 1]; i++) corrSolver[i] = s;
    }
    P.fill_hyp_solver(sHypSolver.at(h));
    sXw1.put(h, p->Xw1);
    sXw2.put(h, p->Xw2);
    sSig1.put(h, p->sigma2_1);
    sSig2.put(h, p->sigma2_2);
    sSample.put(h, P.sample.data());
    const char* d = b->io.din;
    char* dO = b->io.dout;
    char* dS = b->scratch;
    if (const int e = batch_upload(c, b, in.bytes(), 0, st)) return e;    /* this entry does not clear its out block */
    Sim3Launch L{};
    L.solver = sSolver.at(d);
    L.nSolvers = n; L.nCorr = M; L.nHyp = H; L.maxHyp = P.maxHyp;
    L.corrSolver = sCorrSolver.at(d);
    L.Xw1 = sXw1.at(d); L.Xw2 = sXw2.at(d); L.sig1 = sSig1.at(d); L.sig2 = sSig2.at(d);
    L.hypSolver = sHypSolver.at(d);
    L.sample = sSample.at(d);
    L.corr = sCorr.at(dS);
    L.T21 = sT21.at(dS);
    L.R12 = sR.at(dO); L.t12 = sT.at(dO); L.s12 = sS.at(dO); L.T12 = sT12.at(dO);
    L.inliers = sInl.at(dO); L.best = sBest.at(dO); L.returns = sRet.at(dO); L.uncertified = sUnc.at(dO);
    L.mask = sMask.at(dO);
    if (const int e = batch_finish(c, "sim3", drfe_launch_sim3(L, st), b, out.bytes(), st)) return e;
    const char* ho = b->io.hout;
    const uint8_t* unc = sUnc.at(ho);
    std::vector<Sim3Corr> corr;
    for (int s = 0; s < n; s++) {
        const size_t hy = (size_t)P.hyp[(size_t)s], h0 = (size_t)P.hyp0[(size_t)s];
        P.scatter(s, o->R12, sR.at(ho), 9);
        P.scatter(s, o->t12, sT.at(ho), 3);
        P.scatter(s, o->s12, sS.at(ho));
        P.scatter(s, o->T12, sT12.at(ho), 12);
        P.scatter(s, o->inliers, sInl.at(ho));
        P.scatter(s, o->best, sBest.at(ho));
        P.scatter(s, o->returns, sRet.at(ho));
        P.scatter_mask(s, o->mask, sMask.at(ho));
        /* what the device could not certify: the host core finishes the row, then redoes the solver's bookkeeping */
        int handed = 0;
        for (size_t q = 0; q < hy; q++)
            if (unc[h0 + q] || (b->handBackEvery > 0 && (h0 + q) % (size_t)b->handBackEvery == 0)) {
                if (!handed) solver_corrs(p, s, corr);
                host_row(p, P, s, (int)q, corr, o);
                handed++;
            }
        if (handed) {
            host_walk(p, P, s, o);
            b->stats[6] += handed;
        }
    }
    return DRFE_OK;
}

int drfe_sim3_stats(drfe_ctx* c, int64_t* stats) { return batch_stats(c, &drfe_ctx::sim3, stats); }

int drfe_debug_sim3_atan2(const double* y, const double* x, int n, double* out, int32_t* ok)
{
    if (n < 0 || (n > 0 && (!y || !x || !out || !ok))) return DRFE_ERR_INVALID;
    for (int i = 0; i < n; i++) ok[i] = drfe_cr_atan2(y[i], x[i], &out[i]);
    return DRFE_OK;
}

int drfe_debug_sim3_hand_back(drfe_ctx* c, int every) { return batch_hand_back(c, &drfe_ctx::sim3, every); }

int drfe_debug_sim3_horn(const float* P1, const float* P2, int n, int fix_scale, int libm, float* out, int32_t* ok)
{
    if (n < 0 || (n > 0 && (!P1 || !P2 || !out || !ok))) return DRFE_ERR_INVALID;
    for (int i = 0; i < n; i++) {
        float* o = out + 37 * (size_t)i;
        ok[i] = s3_horn(P1 + 9 * (size_t)i, P2 + 9 * (size_t)i, fix_scale, libm ? 1 : 0, o, o + 9, o + 12, o + 13, o + 25);
    }
    return DRFE_OK;
}

int drfe_debug_sim3_rand(uint32_t seed, int n, int32_t* out)
{
    if (n < 0 || (n > 0 && !out)) return DRFE_ERR_INVALID;
    GlibcRand rng(seed);
    for (int i = 0; i < n; i++) out[i] = rng.next();
    return DRFE_OK;
}

}  // extern "C"
