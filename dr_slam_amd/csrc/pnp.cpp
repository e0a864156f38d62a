/* pnp.cpp — PnPsolver (reference src/PnPsolver.cc) behind the C-ABI of include/drfe.h: the host entry (no context), the batch
 * entry (pnp_kernels.hip) and its counters.  Both sides evaluate pnp_core.h; what is sequential and cheap — SetRansacParameters
 * (the host's libm, :121-157) and the sampling (a glibc rand() stream per solver, :188-201) — runs once, on the host, for both.
 * The table's scaffold (plan, sampling, scatter, common counters) is ransac_table.h, shared with sim3.cpp; here are the argument
 * checks and caps, the adjusted mRansacMinInliers, the records and the rows on the host.  DESIGN.md section 17. */
#include "pnp_internal.h"
#include "stage_layout.h"
#include "../../include/drfe_debug.h"

struct PnpBuffers : BatchBuffers {};   /* scratch: the refine jobs of every solver */

void drfe_pnp_free(drfe_ctx* c) { batch_free(c->pnp); }

namespace {

enum { PNP_MAX_SOLVERS = 65535 };      /* the counting kernel's grid has one row per solver */

struct Plan : RansacPlan<4, DRFE_PNP_MAX_CORR> {
    std::vector<int32_t> minInliers;       /* per solver, after SetRansacParameters */
    std::vector<PnpCorr> corr;             /* per correspondence of the call */
};

/* SetRansacParameters (:121-152) with minSet = 4: the adjusted mRansacMinInliers and mRansacMaxIts.  float products and
 * quotients, the int conversion as cvttss2si (NaN and out-of-range give INT_MIN) */
void ransac_parameters(int N, double probability, int minInliers, int maxIterations, float epsilon, int* minOut, int* itOut)
{
    const float prod = (float)N * epsilon;
    int nMinInliers = (prod >= -2147483648.0f && prod < 2147483648.0f) ? (int)prod : INT_MIN;
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < 4) nMinInliers = 4;
    if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
    *minOut = nMinInliers;
    *itOut = ransac_iteration_count(nMinInliers == N, epsilon, probability, maxIterations);
}

int cap_of(const drfe_pnp_problems* p, int s) { return (p->max_iterations[s] > 1 ? p->max_iterations[s] : 1) + p->tail[s]; }

/* all-or-nothing validation of a call, then the plan of its table */
int make_plan(const drfe_pnp_problems* p, const drfe_pnp_out* o, Plan& P, std::string& err)
{
    err = "pnp: invalid argument";
    if (!p || !o || p->n < 0 || p->n > PNP_MAX_SOLVERS) return DRFE_ERR_INVALID;
    const int n = p->n;
    if (n == 0) return DRFE_OK;
    if (!p->K || !p->probability || !p->min_inliers || !p->max_iterations || !p->epsilon || !p->th2 || !p->tail || !p->seed ||
        !p->offsets)
        return DRFE_ERR_INVALID;
    if (!o->iterations || !o->min_inliers || !o->hypotheses || !o->refines || !o->sample || !o->R || !o->t || !o->inliers ||
        !o->mask || !o->best || !o->returns || !o->refined_R || !o->refined_t || !o->refined_inliers || !o->refined_mask)
        return DRFE_ERR_INVALID;
    for (int s = 0; s < n; s++) {
        if (!ransac_offsets_ok(p->offsets, s, DRFE_PNP_MAX_CORR, "pnp", "DRFE_PNP_MAX_CORR", err)) return DRFE_ERR_INVALID;
        if (p->max_iterations[s] > DRFE_PNP_MAX_ITERATIONS) { err = "pnp: max_iterations above DRFE_PNP_MAX_ITERATIONS"; return DRFE_ERR_INVALID; }
        if (p->tail[s] < 0 || p->tail[s] > DRFE_PNP_MAX_TAIL) { err = "pnp: tail outside [0, DRFE_PNP_MAX_TAIL]"; return DRFE_ERR_INVALID; }
        if (p->min_inliers[s] < 0) { err = "pnp: negative min_inliers"; return DRFE_ERR_INVALID; }
    }
    {
        int64_t rows = 0, words = 0;
        for (int s = 0; s < n; s++) {
            rows += cap_of(p, s);
            words += (int64_t)cap_of(p, s) * (((int64_t)p->offsets[s + 1] - p->offsets[s] + 63) / 64);
        }
        if (rows > DRFE_PNP_MAX_ROWS) { err = "pnp: more than DRFE_PNP_MAX_ROWS rows in a call"; return DRFE_ERR_INVALID; }
        if (words > DRFE_PNP_MAX_MASK_WORDS) { err = "pnp: more than DRFE_PNP_MAX_MASK_WORDS mask words in a call"; return DRFE_ERR_INVALID; }
    }
    const int M = p->offsets[n];
    if (M > 0 && (!p->p2d || !p->Xw || !p->sigma2)) return DRFE_ERR_INVALID;
    P.corr.resize((size_t)M);
    for (int s = 0; s < n; s++)
        for (int i = p->offsets[s]; i < p->offsets[s + 1]; i++) {
            PnpCorr& c = P.corr[(size_t)i];
            c.u = p->p2d[2 * (size_t)i];
            c.v = p->p2d[2 * (size_t)i + 1];
            for (int k = 0; k < 3; k++) c.X[k] = p->Xw[3 * (size_t)i + k];
            c.maxErr = p->sigma2[i] * p->th2[s];
            if (!std::isfinite(c.maxErr)) { err = "pnp: sigma2 * th2 is not finite"; return DRFE_ERR_INVALID; }
        }
    for (int s = 0; s < n; s++) {
        const int N = p->offsets[s + 1] - p->offsets[s];
        int it, mi;
        ransac_parameters(N, p->probability[s], p->min_inliers[s], p->max_iterations[s], p->epsilon[s], &mi, &it);
        P.minInliers.push_back(mi);
        P.add_solver(N, it, N < mi ? 0 : it + p->tail[s], cap_of(p, s), p->seed[s]);
    }
    return DRFE_OK;
}

/* the per-solver outputs, the zeroed table and the samples */
void begin_out(const drfe_pnp_problems* p, const Plan& P, drfe_pnp_out* o)
{
    const size_t rows = (size_t)P.rows;
    std::memset(o->sample, 0, rows * 4 * sizeof(int32_t));
    std::memset(o->R, 0, rows * 9 * sizeof(double));
    std::memset(o->t, 0, rows * 3 * sizeof(double));
    std::memset(o->refined_R, 0, rows * 9 * sizeof(double));
    std::memset(o->refined_t, 0, rows * 3 * sizeof(double));
    std::memset(o->inliers, 0, rows * sizeof(int32_t));
    std::memset(o->refined_inliers, 0, rows * sizeof(int32_t));
    std::memset(o->best, 0, rows * sizeof(int32_t));
    std::memset(o->returns, 0, rows);
    std::memset(o->mask, 0, (size_t)P.maskWordsOut * sizeof(uint64_t));
    std::memset(o->refined_mask, 0, (size_t)P.maskWordsOut * sizeof(uint64_t));
    for (int s = 0; s < p->n; s++) {
        o->iterations[s] = P.iterations[(size_t)s];
        o->min_inliers[s] = P.minInliers[(size_t)s];
        o->hypotheses[s] = P.hyp[(size_t)s];
        o->refines[s] = 0;
        P.scatter(s, o->sample, P.sample.data(), 4);
    }
}

void solver_K(const drfe_pnp_problems* p, int s, double K[4])
{
    for (int k = 0; k < 4; k++) K[k] = (double)p->K[4 * (size_t)s + k];
}

/* compute_pose over sel, CheckInliers over all N: R, t canonical into Rout / tout, the mask and its count */
int host_pose_and_count(const PnpSel& sel, int N, const double K[4], double* Rout, double* tout, uint64_t* mask, int words)
{
    double big[144], R[9], t[3];
    pnp_compute_pose(PnpSerial(), sel, K, PnpStrided{big, 1}, R, t);
    for (int k = 0; k < 9; k++) Rout[k] = pnp_canon(R[k]);
    for (int k = 0; k < 3; k++) tout[k] = pnp_canon(t[k]);
    int count = 0;
    for (int w = 0; w < words; w++) mask[w] = 0;
    for (int i = 0; i < N; i++)
        if (pnp_inlier(sel.corr[i], R, t, K)) {
            mask[i >> 6] |= 1ull << (i & 63);
            count++;
        }
    return count;
}

void host_solver(const drfe_pnp_problems* p, const Plan& P, int s, drfe_pnp_out* o)
{
    const int hyp = P.hyp[(size_t)s], N = p->offsets[s + 1] - p->offsets[s], words = P.words[(size_t)s];
    const size_t row0 = (size_t)P.row0[(size_t)s];
    const PnpCorr* corr = P.corr.data() + p->offsets[s];
    double K[4];
    solver_K(p, s, K);
    for (int h = 0; h < hyp; h++) {
        const int32_t* smp = P.sample_of(s, h);
        const PnpSel sel{corr, smp, nullptr, 4, 4, smp[0]};
        o->inliers[row0 + h] = host_pose_and_count(sel, N, K, o->R + 9 * (row0 + h), o->t + 3 * (row0 + h),
                                                   o->mask + P.mask0Out[(size_t)s] + (size_t)h * words, words);
    }
    std::vector<int32_t> jobs((size_t)hyp);
    const int nj = pnp_walk_best(o->inliers + row0, hyp, P.minInliers[(size_t)s], o->best + row0, jobs.data());
    o->refines[s] = nj;
    for (int j = 0; j < nj; j++) {
        const int h = jobs[(size_t)j];
        const uint64_t* rowMask = o->mask + P.mask0Out[(size_t)s] + (size_t)h * words;
        int first = 0;
        while (!((rowMask[first >> 6] >> (first & 63)) & 1)) first++;
        const PnpSel sel{corr, nullptr, rowMask, N, o->inliers[row0 + h], first};
        o->refined_inliers[row0 + h] = host_pose_and_count(sel, N, K, o->refined_R + 9 * (row0 + h), o->refined_t + 3 * (row0 + h),
                                                           o->refined_mask + P.mask0Out[(size_t)s] + (size_t)h * words, words);
    }
    pnp_walk_returns(o->inliers + row0, o->best + row0, o->refined_inliers + row0, hyp, P.minInliers[(size_t)s], o->returns + row0);
}

}  // namespace

extern "C" {

int drfe_pnp_ransac_host(const drfe_pnp_problems* p, drfe_pnp_out* o)
{
    Plan P;
    std::string err;
    const int rc = make_plan(p, o, P, err);
    if (rc || p->n == 0) return rc;
    begin_out(p, P, o);
    for (int s = 0; s < p->n; s++)
        if (P.hyp[(size_t)s]) host_solver(p, P, s, o);
    return DRFE_OK;
}

int drfe_pnp_ransac_batch(drfe_ctx* c, const drfe_pnp_problems* p, drfe_pnp_out* o, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    Plan P;
    const int rc = make_plan(p, o, P, c->err);
    if (rc) return rc;
    PnpBuffers* b = batch_buffers(c->pnp);
    P.count_call(b->stats, p->offsets);
    if (p->n == 0) return DRFE_OK;
    const int n = p->n, M = p->offsets[n], H = P.nHyp;
    for (int s = 0; s < n; s++)
        if (P.hyp[(size_t)s] && p->offsets[s + 1] - p->offsets[s] > DRFE_PNP_LDS_CORR) b->stats[6]++;
    begin_out(p, P, o);
    if (H == 0) return DRFE_OK;
    const size_t nM = (size_t)M, nH = (size_t)H, nW = (size_t)P.maskWords;
    StageLayout<16> in, out, scr;
    const auto sSolver = in.add<PnpSolverRec>((size_t)n);
    const auto sCorr = in.add<PnpCorr>(nM);
    const auto sHypSolver = in.add<int32_t>(nH), sSample = in.add<int32_t>(nH * 4);
    const auto sR = out.add<double>(nH * 9), sT = out.add<double>(nH * 3), sRefR = out.add<double>(nH * 9), sRefT = out.add<double>(nH * 3);
    const auto sInl = out.add<int32_t>(nH), sBest = out.add<int32_t>(nH), sRefInl = out.add<int32_t>(nH);
    const auto sJobsN = out.add<int32_t>((size_t)n);
    const auto sRet = out.add<uint8_t>(nH);
    const auto sMask = out.add<uint64_t>(nW), sRefMask = out.add<uint64_t>(nW);
    const auto sJobs = scr.add<int32_t>(nH), sJobSolver = scr.add<int32_t>(nH), sJobRow = scr.add<int32_t>(nH), sTotal = scr.add<int32_t>(1);
    hipStream_t st;
    if (const int e = batch_begin(c, b, stream, in.bytes(), out.bytes(), scr.bytes(), &st)) return e;
    char* h = b->io.hin;
    PnpSolverRec* sol = sSolver.at(h);
    for (int s = 0; s < n; s++) {
        solver_K(p, s, sol[s].K);
        sol[s].head = P.head(s, p->offsets, P.minInliers[(size_t)s]);
    }
    P.fill_hyp_solver(sHypSolver.at(h));
    sCorr.put(h, P.corr.data());
    sSample.put(h, P.sample.data());
    const char* d = b->io.din;
    char* dO = b->io.dout;
    char* dS = b->scratch;
    if (const int e = batch_upload(c, b, in.bytes(), out.bytes(), st)) return e;
    PnpLaunch L{};
    L.solver = sSolver.at(d);
    L.nSolvers = n; L.nCorr = M; L.nHyp = H; L.maxHyp = P.maxHyp;
    L.corr = sCorr.at(d);
    L.hypSolver = sHypSolver.at(d);
    L.sample = sSample.at(d);
    L.jobs = sJobs.at(dS); L.jobSolver = sJobSolver.at(dS); L.jobRow = sJobRow.at(dS); L.totalJobs = sTotal.at(dS);
    L.R = sR.at(dO); L.t = sT.at(dO); L.refR = sRefR.at(dO); L.refT = sRefT.at(dO);
    L.inliers = sInl.at(dO); L.best = sBest.at(dO); L.refInliers = sRefInl.at(dO); L.nJobs = sJobsN.at(dO);
    L.returns = sRet.at(dO);
    L.mask = sMask.at(dO); L.refMask = sRefMask.at(dO);
    if (const int e = batch_finish(c, "pnp", drfe_launch_pnp(L, st), b, out.bytes(), st)) return e;
    const char* ho = b->io.hout;
    for (int s = 0; s < n; s++) {
        const size_t hy = (size_t)P.hyp[(size_t)s], r0 = (size_t)P.row0[(size_t)s];
        if (!hy) continue;
        P.scatter(s, o->R, sR.at(ho), 9);
        P.scatter(s, o->t, sT.at(ho), 3);
        P.scatter(s, o->refined_R, sRefR.at(ho), 9);
        P.scatter(s, o->refined_t, sRefT.at(ho), 3);
        P.scatter(s, o->inliers, sInl.at(ho));
        P.scatter(s, o->refined_inliers, sRefInl.at(ho));
        P.scatter(s, o->best, sBest.at(ho));
        P.scatter(s, o->returns, sRet.at(ho));
        P.scatter_mask(s, o->mask, sMask.at(ho));
        P.scatter_mask(s, o->refined_mask, sRefMask.at(ho));
        o->refines[s] = sJobsN.at(ho)[s];
        b->stats[4] += o->refines[s];
        /* a refine job's points: the count of every row that became the best one */
        int last = -1;
        for (size_t q = 0; q < hy; q++) {
            const int bq = o->best[r0 + q];
            if (bq >= 0 && bq != last) { b->stats[5] += o->inliers[r0 + (size_t)bq]; last = bq; }
        }
    }
    return DRFE_OK;
}

int drfe_pnp_stats(drfe_ctx* c, int64_t* stats) { return batch_stats(c, &drfe_ctx::pnp, stats); }

int drfe_debug_pnp_svd(const double* A, int m, int n, double* w, double* ut, double* vt)
{
    if (!A || !w || !ut || !vt || n < 1 || m < n || m > 12) return DRFE_ERR_INVALID;
    double At[144];
    for (int i = 0; i < n; i++)
        for (int k = 0; k < m; k++) At[i * m + k] = A[k * n + i];
    pnp_jacobi_svd(At, m, n, w, vt);
    std::memcpy(ut, At, sizeof(double) * (size_t)m * n);
    return DRFE_OK;
}

int drfe_debug_pnp_inliers(const double* R, const double* t, const float* K, const float* p2d, const float* Xw, const float* max_err,
                           int n, uint8_t* out)
{
    if (n < 0 || !R || !t || !K || (n > 0 && (!p2d || !Xw || !max_err || !out))) return DRFE_ERR_INVALID;
    const double Kd[4] = {(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
    for (int i = 0; i < n; i++) {
        const PnpCorr c{p2d[2 * (size_t)i], p2d[2 * (size_t)i + 1], {Xw[3 * (size_t)i], Xw[3 * (size_t)i + 1], Xw[3 * (size_t)i + 2]}, max_err[i]};
        out[i] = pnp_inlier(c, R, t, Kd) ? 1 : 0;
    }
    return DRFE_OK;
}

int drfe_debug_pnp_inliers_device(drfe_ctx* c, const double* R, const double* t, const float* K, const float* p2d, const float* Xw,
                                  const float* max_err, int n, uint8_t* out)
{
    if (!c || n < 0 || n > DRFE_PNP_MAX_CORR || !R || !t || !K || (n > 0 && (!p2d || !Xw || !max_err || !out))) return DRFE_ERR_INVALID;
    if (n == 0) return DRFE_OK;
    const size_t words = ((size_t)n + 63) / 64;
    StageLayout<16> in, out_;
    const auto sCorr = in.add<PnpCorr>((size_t)n);
    const auto sRt = in.add<double>(12), sK = in.add<double>(4);
    const auto sMask = out_.add<uint64_t>(words);
    const auto sCount = out_.add<int32_t>(1);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<char> din, dout;
    std::vector<char> hin(in.bytes()), hout(out_.bytes());
    HIPCHK(c, din.alloc(in.bytes()));
    HIPCHK(c, dout.alloc(out_.bytes()));
    PnpCorr* corr = sCorr.at(hin.data());
    for (int i = 0; i < n; i++)
        corr[i] = PnpCorr{p2d[2 * (size_t)i], p2d[2 * (size_t)i + 1], {Xw[3 * (size_t)i], Xw[3 * (size_t)i + 1], Xw[3 * (size_t)i + 2]}, max_err[i]};
    for (int k = 0; k < 9; k++) sRt.at(hin.data())[k] = R[k];
    for (int k = 0; k < 3; k++) sRt.at(hin.data())[9 + k] = t[k];
    for (int k = 0; k < 4; k++) sK.at(hin.data())[k] = (double)K[k];
    HIPCHK(c, hipMemcpyAsync(din, hin.data(), in.bytes(), hipMemcpyHostToDevice, c->stream));
    const char* d = din;
    char* dO = dout;
    HIPCHK(c, drfe_launch_pnp_sweep_one(sCorr.at(d), n, sRt.at(d), sK.at(d), sMask.at(dO), sCount.at(dO), c->stream));
    HIPCHK(c, hipMemcpyAsync(hout.data(), dO, out_.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t* m = sMask.at(hout.data());
    int count = 0;
    for (int i = 0; i < n; i++) {
        out[i] = (uint8_t)((m[i >> 6] >> (i & 63)) & 1);
        count += out[i];
    }
    if (count != *sCount.at(hout.data())) { c->err = "pnp sweep: the count is not the mask's popcount"; return DRFE_ERR_HIP; }
    return DRFE_OK;
}

}  // extern "C"
