/* init.cpp — Initializer (reference src/Initializer.cc) behind the C-ABI of include/drfe.h: the host entry (no context), the batch
 * entry (init_kernels.hip) and its counters.  Both sides evaluate init_core.h.  What is sequential and cheap runs once, on the
 * host, for both: the match list, Normalize's four ordered float sums per frame (while packing), the sampling (a glibc rand()
 * stream per solver) and the tail - the parallax through the host's acosf and the reference's choice among the 4 or 8 motion
 * hypotheses.  The table's scaffold is ransac_table.h.  DESIGN.md section 19. */
#include "init_internal.h"
#include "stage_layout.h"

#include <algorithm>

struct InitBuffers : BatchBuffers {};

void drfe_init_free(drfe_ctx* c) { batch_free(c->init); }

namespace {

struct Plan : RansacPlan<8, DRFE_INIT_MAX_KEYS> {
    std::vector<int32_t> matchOff;         /* n + 1: a solver's matches in the call's list */
    std::vector<InitMatch> match;
    std::vector<InitNorm> norm;
    std::vector<int32_t> first;
    std::vector<InitSolverRec> rec;
};

/* Normalize (:754-800): meanX, meanY, meanDevX, meanDevY are float sums in index order over every key of the frame; the normalised
 * points into pn, T into T */
void normalize(const float* keys, int N, std::vector<float>& pn, float T[9])
{
    float meanX = 0, meanY = 0;
    pn.resize(2 * (size_t)N);
    for (int i = 0; i < N; i++) {
        meanX += keys[2 * i];
        meanY += keys[2 * i + 1];
    }
    meanX = meanX / N;
    meanY = meanY / N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; i++) {
        pn[2 * (size_t)i] = keys[2 * i] - meanX;
        pn[2 * (size_t)i + 1] = keys[2 * i + 1] - meanY;
        meanDevX += fabsf(pn[2 * (size_t)i]);
        meanDevY += fabsf(pn[2 * (size_t)i + 1]);
    }
    meanDevX = meanDevX / N;
    meanDevY = meanDevY / N;
    const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
    for (int i = 0; i < N; i++) {
        pn[2 * (size_t)i] = pn[2 * (size_t)i] * sX;
        pn[2 * (size_t)i + 1] = pn[2 * (size_t)i + 1] * sY;
    }
    init_T(meanX, meanY, sX, sY, T);
}

/* all-or-nothing validation of a call, then the plan of its table and the records both entries work on */
int make_plan(const drfe_init_problems* p, const drfe_init_out* o, Plan& P, std::string& err)
{
    err = "init: invalid argument";
    if (!p || !o || p->n < 0) return DRFE_ERR_INVALID;
    if (p->n > DRFE_INIT_MAX_SOLVERS) { err = "init: more than DRFE_INIT_MAX_SOLVERS solvers"; return DRFE_ERR_INVALID; }
    const int n = p->n;
    if (n == 0) return DRFE_OK;
    if (!p->K || !p->sigma || !p->max_iterations || !p->seed || !p->key1_offsets || !p->key2_offsets) return DRFE_ERR_INVALID;
    if (!o->N || !o->iterations || !o->hypotheses || !o->SH || !o->SF || !o->RH || !o->branch || !o->motions || !o->ok || !o->flags ||
        !o->R21 || !o->t21 || !o->vP3D || !o->vbTriangulated || !o->sample || !o->H21 || !o->F21 || !o->score_h || !o->score_f ||
        !o->best_h || !o->best_f || !o->mask_h || !o->mask_f || !o->motion_R || !o->motion_t || !o->motion_good || !o->motion_cos ||
        !o->motion_parallax || !o->motion_status || !o->motion_vbGood || !o->motion_vP3D)
        return DRFE_ERR_INVALID;
    for (int s = 0; s < n; s++) {
        if (!ransac_offsets_ok(p->key1_offsets, s, DRFE_INIT_MAX_KEYS, "init", "DRFE_INIT_MAX_KEYS", err)) return DRFE_ERR_INVALID;
        if (!ransac_offsets_ok(p->key2_offsets, s, DRFE_INIT_MAX_KEYS, "init", "DRFE_INIT_MAX_KEYS", err)) return DRFE_ERR_INVALID;
        if (p->max_iterations[s] < 0) { err = "init: negative max_iterations"; return DRFE_ERR_INVALID; }
        if (p->max_iterations[s] > DRFE_INIT_MAX_ITERATIONS) { err = "init: max_iterations above DRFE_INIT_MAX_ITERATIONS"; return DRFE_ERR_INVALID; }
    }
    const int M1 = p->key1_offsets[n], M2 = p->key2_offsets[n];
    if ((M1 > 0 && (!p->keys1 || !p->matches12)) || (M2 > 0 && !p->keys2)) return DRFE_ERR_INVALID;
    P.matchOff.assign(1, 0);
    {
        int64_t rows = 0, words = 0;
        for (int s = 0; s < n; s++) {
            const int k1 = p->key1_offsets[s], n1 = p->key1_offsets[s + 1] - k1, n2 = p->key2_offsets[s + 1] - p->key2_offsets[s];
            int N = 0;
            for (int i = 0; i < n1; i++) {
                const int32_t m = p->matches12[k1 + i];
                if (m >= n2 || m < -1) { err = "init: a match is neither -1 nor a key of the current frame"; return DRFE_ERR_INVALID; }
                if (m >= 0) N++;
            }
            P.matchOff.push_back(P.matchOff.back() + N);
            rows += p->max_iterations[s];
            words += (int64_t)p->max_iterations[s] * ((N + 63) / 64);
        }
        if (rows > DRFE_INIT_MAX_ROWS) { err = "init: more than DRFE_INIT_MAX_ROWS rows in a call"; return DRFE_ERR_INVALID; }
        if (words > DRFE_INIT_MAX_MASK_WORDS) { err = "init: more than DRFE_INIT_MAX_MASK_WORDS mask words in a call"; return DRFE_ERR_INVALID; }
    }
    const size_t M = (size_t)P.matchOff[(size_t)n];
    P.match.resize(M);
    P.norm.resize(M);
    P.first.resize(M);
    P.rec.resize((size_t)n);
    std::vector<float> pn1, pn2;
    for (int s = 0; s < n; s++) {
        const int k1 = p->key1_offsets[s], k2 = p->key2_offsets[s];
        const int n1 = p->key1_offsets[s + 1] - k1, n2 = p->key2_offsets[s + 1] - k2;
        const float *keys1 = p->keys1 + 2 * (size_t)k1, *keys2 = p->keys2 + 2 * (size_t)k2;
        InitSolverRec& S = P.rec[(size_t)s];
        float T2[9];
        normalize(keys1, n1, pn1, S.T1);
        normalize(keys2, n2, pn2, T2);
        init_inv3(T2, S.T2inv);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) S.T2t[r * 3 + c] = T2[c * 3 + r];
        for (int k = 0; k < 9; k++) S.K[k] = p->K[9 * (size_t)s + k];
        S.sigma = p->sigma[s];
        S.invSigma2 = init_inv_sigma2(S.sigma);
        S.nKeys1 = n1;
        S.key10 = k1;
        size_t at = (size_t)P.matchOff[(size_t)s];
        for (int i = 0; i < n1; i++) {
            const int32_t j = p->matches12[k1 + i];
            if (j < 0) continue;
            P.match[at] = InitMatch{keys1[2 * i], keys1[2 * i + 1], keys2[2 * j], keys2[2 * j + 1]};
            P.norm[at] = InitNorm{pn1[2 * (size_t)i], pn1[2 * (size_t)i + 1], pn2[2 * (size_t)j], pn2[2 * (size_t)j + 1]};
            P.first[at] = i;
            at++;
        }
        const int N = P.matchOff[(size_t)s + 1] - P.matchOff[(size_t)s], it = p->max_iterations[s];
        P.add_solver(N, it, N < 8 ? 0 : it, it, p->seed[s]);
        S.head = P.head(s, P.matchOff.data(), 0);
    }
    return DRFE_OK;
}

/* the per-solver outputs, the zeroed tables and the samples */
void begin_out(const drfe_init_problems* p, const Plan& P, drfe_init_out* o)
{
    const size_t rows = (size_t)P.rows, n = (size_t)p->n, M1 = (size_t)p->key1_offsets[p->n];
    std::memset(o->sample, 0, rows * 8 * sizeof(int32_t));
    std::memset(o->H21, 0, rows * 9 * sizeof(float));
    std::memset(o->F21, 0, rows * 9 * sizeof(float));
    std::memset(o->score_h, 0, rows * sizeof(float));
    std::memset(o->score_f, 0, rows * sizeof(float));
    std::memset(o->best_h, 0, rows * sizeof(int32_t));
    std::memset(o->best_f, 0, rows * sizeof(int32_t));
    std::memset(o->mask_h, 0, (size_t)P.maskWordsOut * sizeof(uint64_t));
    std::memset(o->mask_f, 0, (size_t)P.maskWordsOut * sizeof(uint64_t));
    std::memset(o->SH, 0, n * sizeof(float));
    std::memset(o->SF, 0, n * sizeof(float));
    std::memset(o->RH, 0, n * sizeof(float));
    std::memset(o->branch, 0, n * sizeof(int32_t));
    std::memset(o->motions, 0, n * sizeof(int32_t));
    std::memset(o->ok, 0, n * sizeof(int32_t));
    std::memset(o->flags, 0, n * sizeof(int32_t));
    std::memset(o->R21, 0, n * 9 * sizeof(float));
    std::memset(o->t21, 0, n * 3 * sizeof(float));
    std::memset(o->vP3D, 0, M1 * 3 * sizeof(float));
    std::memset(o->vbTriangulated, 0, M1);
    std::memset(o->motion_R, 0, n * 72 * sizeof(float));
    std::memset(o->motion_t, 0, n * 24 * sizeof(float));
    std::memset(o->motion_good, 0, n * 8 * sizeof(int32_t));
    std::memset(o->motion_cos, 0, n * 8 * sizeof(float));
    std::memset(o->motion_parallax, 0, n * 8 * sizeof(float));
    std::memset(o->motion_status, 0, n * 8 * sizeof(int32_t));
    std::memset(o->motion_vbGood, 0, M1 * 8);
    std::memset(o->motion_vP3D, 0, M1 * 24 * sizeof(float));
    for (int s = 0; s < p->n; s++) {
        o->N[s] = P.matchOff[(size_t)s + 1] - P.matchOff[(size_t)s];
        o->iterations[s] = P.iterations[(size_t)s];
        o->hypotheses[s] = P.hyp[(size_t)s];
        P.scatter(s, o->sample, P.sample.data(), 8);
    }
}

/* the row that holds solver s's best model of the branch taken, and its mask in the caller's table */
const uint64_t* best_mask(const Plan& P, int s, const drfe_init_out* o, int* row)
{
    const size_t i = (size_t)s, last = (size_t)P.row0[i] + (size_t)P.hyp[i] - 1;
    const bool H = o->branch[s] == DRFE_INIT_BRANCH_H;
    *row = H ? o->best_h[last] : o->best_f[last];
    return (H ? o->mask_h : o->mask_f) + P.mask0Out[i] + (size_t)*row * (size_t)P.words[i];
}

/* CheckRT's parallax (:901-909) from the selected cosine: acos(float) of the host's libm, * 180 in float, / CV_PI in double */
float parallax_of(int nGood, float cosSel)
{
    if (nGood <= 0) return 0.f;
    return init_canon((float)((double)(acosf(cosSel) * 180.0f) / 3.1415926535897932384626433832795));
}

/* the ends of ReconstructF (:504-574) and ReconstructH (:694-736) over the finished CheckRT results of solver s, minParallax 1.0,
 * minTriangulated 50 */
void finish_solver(const drfe_init_problems* p, const Plan& P, int s, drfe_init_out* o)
{
    const int nm = o->motions[s];
    if (nm == 0) return;
    const size_t i = (size_t)s;
    int32_t* good = o->motion_good + 8 * i;
    float* par = o->motion_parallax + 8 * i;
    for (int m = 0; m < nm; m++) par[m] = parallax_of(good[m], o->motion_cos[8 * i + m]);
    int row;
    const uint64_t* mask = best_mask(P, s, o, &row);
    int N = 0;
    for (int w = 0; w < P.words[i]; w++) N += __builtin_popcountll(mask[w]);
    int pick = -1;
    if (o->branch[s] == DRFE_INIT_BRANCH_F) {
        const int maxGood = std::max(good[0], std::max(good[1], std::max(good[2], good[3])));
        const int nMinGood = std::max((int)(0.9 * N), 50);
        int nsimilar = 0;
        for (int m = 0; m < 4; m++)
            if (good[m] > 0.7 * maxGood) nsimilar++;
        if (maxGood < nMinGood || nsimilar > 1) return;
        for (int m = 0; m < 4; m++)
            if (maxGood == good[m]) {
                if (par[m] > 1.0f) pick = m;
                break;
            }
    } else {
        int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
        float bestParallax = -1;
        for (int m = 0; m < 8; m++) {
            if (good[m] > bestGood) {
                secondBestGood = bestGood;
                bestGood = good[m];
                bestSolutionIdx = m;
                bestParallax = par[m];
            } else if (good[m] > secondBestGood)
                secondBestGood = good[m];
        }
        if (secondBestGood < 0.75 * bestGood && bestParallax >= 1.0f && bestGood > 50 && bestGood > 0.9 * N) pick = bestSolutionIdx;
    }
    if (pick < 0) return;
    const size_t k1 = (size_t)p->key1_offsets[s], n1 = (size_t)p->key1_offsets[s + 1] - k1, at = 8 * k1 + (size_t)pick * n1;
    o->ok[s] = 1;
    std::memcpy(o->R21 + 9 * i, o->motion_R + 72 * i + 9 * (size_t)pick, 9 * sizeof(float));
    std::memcpy(o->t21 + 3 * i, o->motion_t + 24 * i + 3 * (size_t)pick, 3 * sizeof(float));
    std::memcpy(o->vP3D + 3 * k1, o->motion_vP3D + 3 * at, 3 * n1 * sizeof(float));
    std::memcpy(o->vbTriangulated + k1, o->motion_vbGood + at, n1);
}

/* CheckRT (:803-912) of one motion hypothesis over the inliers of `mask`, up to the selected cosine */
void host_check_rt(const InitSolverRec& S, const InitMatch* match, const int32_t* first, const uint64_t* mask, const float* R,
                   const float* t, uint8_t* vbGood, float* vP3D, int32_t* nGoodOut, float* cosOut, int32_t* statusOut)
{
    InitCheck C;
    init_check_setup(S.K, R, t, S.sigma, &C);
    std::vector<uint32_t> keys;
    for (int i = 0; i < S.head.n; i++) {
        if (!((mask[i >> 6] >> (i & 63)) & 1)) continue;
        float X[3], c;
        const int code = init_check_point(C, match[i], X, &c);
        if (!(code & INIT_PT_COUNTED)) continue;
        keys.push_back(init_cos_key(c));
        for (int k = 0; k < 3; k++) vP3D[3 * (size_t)first[i] + k] = init_canon(X[k]);
        if (code & INIT_PT_GOOD) vbGood[first[i]] = 1;
    }
    *nGoodOut = (int32_t)keys.size();
    if (keys.empty()) return;
    std::sort(keys.begin(), keys.end());
    *cosOut = init_cos_value(keys[std::min((size_t)50, keys.size() - 1)]);
    if (keys.back() == 0xFFFFFFFFu) *statusOut = DRFE_INIT_MOTION_NAN_COS;
}

void host_solver(const drfe_init_problems* p, const Plan& P, int s, drfe_init_out* o)
{
    const size_t i = (size_t)s, row0 = (size_t)P.row0[i];
    const int hyp = P.hyp[i], N = P.rec[i].head.n, words = P.words[i];
    const InitSolverRec& S = P.rec[i];
    const InitMatch* match = P.match.data() + P.matchOff[i];
    const InitNorm* norm = P.norm.data() + P.matchOff[i];
    float big[225];
    for (int h = 0; h < hyp; h++) {
        const int32_t* smp = P.sample_of(s, h);
        InitNorm pts[8];
        for (int q = 0; q < 8; q++) pts[q] = norm[smp[q]];
        float H21[9], H12[9], F21[9];
        init_row_h(pts, S.T1, S.T2inv, big, H21, H12);
        init_row_f(pts, S.T1, S.T2t, big, F21);
        float sh = 0, sf = 0;
        uint64_t* mh = o->mask_h + P.mask0Out[i] + (size_t)h * words;
        uint64_t* mf = o->mask_f + P.mask0Out[i] + (size_t)h * words;
        for (int q = 0; q < N; q++) {
            float chi[2];
            bool in[2];
            init_chi_h(H21, H12, match[q], S.invSigma2, chi, in);
            sh = init_score_add(sh, chi, in);
            if (in[0] && in[1]) mh[q >> 6] |= 1ull << (q & 63);
            init_chi_f(F21, match[q], S.invSigma2, chi, in);
            sf = init_score_add(sf, chi, in);
            if (in[0] && in[1]) mf[q >> 6] |= 1ull << (q & 63);
        }
        for (int k = 0; k < 9; k++) {
            o->H21[9 * (row0 + h) + k] = init_canon(H21[k]);
            o->F21[9 * (row0 + h) + k] = init_canon(F21[k]);
        }
        o->score_h[row0 + h] = init_canon(sh);
        o->score_f[row0 + h] = init_canon(sf);
    }
    const int bh = init_walk_best(o->score_h + row0, hyp, o->best_h + row0);
    const int bf = init_walk_best(o->score_f + row0, hyp, o->best_f + row0);
    o->SH[s] = bh >= 0 ? o->score_h[row0 + bh] : 0.f;
    o->SF[s] = bf >= 0 ? o->score_f[row0 + bf] : 0.f;
    init_pick_branch(o->SH[s], o->SF[s], N, o->RH + s, o->branch + s, o->flags + s);
    if (o->branch[s] == DRFE_INIT_BRANCH_NONE) return;
    const bool H = o->branch[s] == DRFE_INIT_BRANCH_H;
    const float* model = H ? o->H21 + 9 * (row0 + bh) : o->F21 + 9 * (row0 + bf);
    o->motions[s] = init_solver_motions(S.K, o->branch[s], model, o->motion_R + 72 * i, o->motion_t + 24 * i, o->flags + s);
    int row;
    const uint64_t* mask = best_mask(P, s, o, &row);
    const size_t k1 = (size_t)S.key10, n1 = (size_t)S.nKeys1;
    for (int m = 0; m < o->motions[s]; m++)
        host_check_rt(S, match, P.first.data() + P.matchOff[i], mask, o->motion_R + 72 * i + 9 * m, o->motion_t + 24 * i + 3 * m,
                      o->motion_vbGood + 8 * k1 + m * n1, o->motion_vP3D + 3 * (8 * k1 + m * n1), o->motion_good + 8 * i + m,
                      o->motion_cos + 8 * i + m, o->motion_status + 8 * i + m);
}

}  // namespace

extern "C" {

int drfe_init_ransac_host(const drfe_init_problems* p, drfe_init_out* o)
{
    Plan P;
    std::string err;
    const int rc = make_plan(p, o, P, err);
    if (rc || p->n == 0) return rc;
    begin_out(p, P, o);
    for (int s = 0; s < p->n; s++) {
        if (P.hyp[(size_t)s]) host_solver(p, P, s, o);
        else init_pick_branch(0.f, 0.f, o->N[s], o->RH + s, o->branch + s, o->flags + s);
        finish_solver(p, P, s, o);
    }
    return DRFE_OK;
}

int drfe_init_ransac_batch(drfe_ctx* c, const drfe_init_problems* p, drfe_init_out* o, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    Plan P;
    const int rc = make_plan(p, o, P, c->err);
    if (rc) return rc;
    InitBuffers* b = batch_buffers(c->init);
    P.count_call(b->stats, P.matchOff.data());
    if (p->n == 0) return DRFE_OK;
    const int n = p->n, H = P.nHyp;
    begin_out(p, P, o);
    for (int s = 0; s < n; s++)
        if (!P.hyp[(size_t)s]) init_pick_branch(0.f, 0.f, o->N[s], o->RH + s, o->branch + s, o->flags + s);
    if (H == 0) return DRFE_OK;
    const size_t nS = (size_t)n, nM = P.match.size(), nH = (size_t)H, nW = (size_t)P.maskWords, nK1 = (size_t)p->key1_offsets[n];
    StageLayout<16> in, out, scr;
    const auto sSolver = in.add<InitSolverRec>(nS);
    const auto sMatch = in.add<InitMatch>(nM);
    const auto sNorm = in.add<InitNorm>(nM);
    const auto sFirst = in.add<int32_t>(nM), sHypSolver = in.add<int32_t>(nH), sSample = in.add<int32_t>(nH * 8);
    const auto sH21 = out.add<float>(nH * 9), sF21 = out.add<float>(nH * 9), sScoreH = out.add<float>(nH), sScoreF = out.add<float>(nH);
    const auto sBestH = out.add<int32_t>(nH), sBestF = out.add<int32_t>(nH);
    const auto sMaskH = out.add<uint64_t>(nW), sMaskF = out.add<uint64_t>(nW);
    const auto sSH = out.add<float>(nS), sSF = out.add<float>(nS), sRH = out.add<float>(nS);
    const auto sBranch = out.add<int32_t>(nS), sMotions = out.add<int32_t>(nS), sFlags = out.add<int32_t>(nS);
    const auto sMR = out.add<float>(nS * 72), sMt = out.add<float>(nS * 24), sMCos = out.add<float>(nS * 8);
    const auto sMGood = out.add<int32_t>(nS * 8), sMStatus = out.add<int32_t>(nS * 8);
    const auto sMVb = out.add<uint8_t>(nK1 * 8);
    const auto sMP3D = out.add<float>(nK1 * 24);
    const auto sH12 = scr.add<float>(nH * 9);
    const auto sLastH = scr.add<int32_t>(nS), sLastF = scr.add<int32_t>(nS);
    hipStream_t st;
    if (const int e = batch_begin(c, b, stream, in.bytes(), out.bytes(), scr.bytes(), &st)) return e;
    char* h = b->io.hin;
    sSolver.put(h, P.rec.data());
    sMatch.put(h, P.match.data());
    sNorm.put(h, P.norm.data());
    sFirst.put(h, P.first.data());
    P.fill_hyp_solver(sHypSolver.at(h));
    sSample.put(h, P.sample.data());
    const char* d = b->io.din;
    char* dO = b->io.dout;
    char* dS = b->scratch;
    if (const int e = batch_upload(c, b, in.bytes(), out.bytes(), st)) return e;
    InitLaunch L{};
    L.solver = sSolver.at(d);
    L.nSolvers = n; L.nHyp = H; L.maxHyp = P.maxHyp;
    L.match = sMatch.at(d); L.norm = sNorm.at(d); L.first = sFirst.at(d);
    L.hypSolver = sHypSolver.at(d); L.sample = sSample.at(d);
    L.H12 = sH12.at(dS); L.lastH = sLastH.at(dS); L.lastF = sLastF.at(dS);
    L.H21 = sH21.at(dO); L.F21 = sF21.at(dO); L.scoreH = sScoreH.at(dO); L.scoreF = sScoreF.at(dO);
    L.bestH = sBestH.at(dO); L.bestF = sBestF.at(dO); L.maskH = sMaskH.at(dO); L.maskF = sMaskF.at(dO);
    L.SH = sSH.at(dO); L.SF = sSF.at(dO); L.RH = sRH.at(dO);
    L.branch = sBranch.at(dO); L.motions = sMotions.at(dO); L.flags = sFlags.at(dO);
    L.mR = sMR.at(dO); L.mt = sMt.at(dO); L.mCos = sMCos.at(dO); L.mGood = sMGood.at(dO); L.mStatus = sMStatus.at(dO);
    L.mVbGood = sMVb.at(dO); L.mP3D = sMP3D.at(dO);
    if (const int e = batch_finish(c, "init", drfe_launch_init(L, st), b, out.bytes(), st)) return e;
    const char* ho = b->io.hout;
    sMR.get(ho, o->motion_R);
    sMt.get(ho, o->motion_t);
    sMCos.get(ho, o->motion_cos);
    sMGood.get(ho, o->motion_good);
    sMStatus.get(ho, o->motion_status);
    sMVb.get(ho, o->motion_vbGood);
    sMP3D.get(ho, o->motion_vP3D);
    for (int s = 0; s < n; s++) {
        if (!P.hyp[(size_t)s]) continue;
        P.scatter(s, o->H21, sH21.at(ho), 9);
        P.scatter(s, o->F21, sF21.at(ho), 9);
        P.scatter(s, o->score_h, sScoreH.at(ho));
        P.scatter(s, o->score_f, sScoreF.at(ho));
        P.scatter(s, o->best_h, sBestH.at(ho));
        P.scatter(s, o->best_f, sBestF.at(ho));
        P.scatter_mask(s, o->mask_h, sMaskH.at(ho));
        P.scatter_mask(s, o->mask_f, sMaskF.at(ho));
        o->SH[s] = sSH.at(ho)[s];
        o->SF[s] = sSF.at(ho)[s];
        o->RH[s] = sRH.at(ho)[s];
        o->branch[s] = sBranch.at(ho)[s];
        o->motions[s] = sMotions.at(ho)[s];
        o->flags[s] = sFlags.at(ho)[s];
        finish_solver(p, P, s, o);
        if (o->branch[s] == DRFE_INIT_BRANCH_H) b->stats[4]++;
        if (o->branch[s] == DRFE_INIT_BRANCH_F) b->stats[5]++;
        if (o->ok[s]) b->stats[6]++;
    }
    return DRFE_OK;
}

int drfe_debug_init_cos_keys(const float* c, int n, uint32_t* key, float* value)
{
    if (n < 0 || (n > 0 && (!c || !key || !value))) return DRFE_ERR_INVALID;
    for (int i = 0; i < n; i++) {
        key[i] = init_cos_key(c[i]);
        value[i] = init_cos_value(key[i]);
    }
    return DRFE_OK;
}

int drfe_debug_init_null_vectors(const float* points, int n, float* h, float* fpre)
{
    if (n < 0 || (n > 0 && (!points || !h || !fpre))) return DRFE_ERR_INVALID;
    float big[225];
    for (int i = 0; i < n; i++) {
        InitNorm P[8];
        for (int q = 0; q < 8; q++) {
            const float* v = points + 32 * (size_t)i + 4 * q;
            P[q] = InitNorm{v[0], v[1], v[2], v[3]};
        }
        init_compute_h21(P, big, h + 9 * (size_t)i);
        init_compute_fpre(P, big, fpre + 9 * (size_t)i);
    }
    return DRFE_OK;
}

int drfe_debug_init_check_rt(drfe_ctx* c, const float* K, const float* R, const float* t, float sigma, const float* matches, int n,
                             int32_t* good, float* cosSel, float* parallax, int32_t* status, uint8_t* vbGood, float* vP3D)
{
    if (!K || !R || !t || !good || !cosSel || !parallax || !status || n < 0 || n > DRFE_INIT_MAX_KEYS) return DRFE_ERR_INVALID;
    if (n > 0 && (!matches || !vbGood || !vP3D)) return DRFE_ERR_INVALID;
    *good = 0;
    *cosSel = 0.f;
    *parallax = 0.f;
    *status = 0;
    if (n == 0) return DRFE_OK;
    const size_t N = (size_t)n, words = (N + 63) / 64;
    std::memset(vbGood, 0, N);
    std::memset(vP3D, 0, 3 * N * sizeof(float));
    InitSolverRec S{};
    for (int k = 0; k < 9; k++) S.K[k] = K[k];
    S.sigma = sigma;
    S.invSigma2 = init_inv_sigma2(sigma);
    S.nKeys1 = n;
    S.head.n = n;
    S.head.hyp = 1;
    S.head.words = (int32_t)words;
    std::vector<InitMatch> match(N);
    std::vector<int32_t> first(N);
    std::vector<uint64_t> mask(words, 0);
    for (int i = 0; i < n; i++) {
        match[(size_t)i] = InitMatch{matches[4 * i], matches[4 * i + 1], matches[4 * i + 2], matches[4 * i + 3]};
        first[(size_t)i] = i;
        mask[(size_t)i >> 6] |= 1ull << (i & 63);
    }
    if (!c) {
        host_check_rt(S, match.data(), first.data(), mask.data(), R, t, vbGood, vP3D, good, cosSel, status);
        *parallax = parallax_of(*good, *cosSel);
        return DRFE_OK;
    }
    InitBuffers* b = batch_buffers(c->init);
    StageLayout<16> in, out;
    const auto sSolver = in.add<InitSolverRec>(1);
    const auto sMatch = in.add<InitMatch>(N);
    const auto sFirst = in.add<int32_t>(N);
    const auto sMask = in.add<uint64_t>(words);
    const auto sMR = in.add<float>(72), sMt = in.add<float>(24);
    const auto sBranch = in.add<int32_t>(1), sMotions = in.add<int32_t>(1), sLast = in.add<int32_t>(1);
    const auto sMCos = out.add<float>(8);
    const auto sMGood = out.add<int32_t>(8), sMStatus = out.add<int32_t>(8);
    const auto sMVb = out.add<uint8_t>(N * 8);
    const auto sMP3D = out.add<float>(N * 24);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(c, b->io.grow(in.bytes(), out.bytes()));
    char* h = b->io.hin;
    std::memset(h, 0, in.bytes());
    sSolver.put(h, &S);
    sMatch.put(h, match.data());
    sFirst.put(h, first.data());
    sMask.put(h, mask.data());
    for (int k = 0; k < 9; k++) sMR.at(h)[k] = R[k];
    for (int k = 0; k < 3; k++) sMt.at(h)[k] = t[k];
    *sBranch.at(h) = DRFE_INIT_BRANCH_H;
    *sMotions.at(h) = 1;
    *sLast.at(h) = 0;
    char* d = b->io.din;
    char* dO = b->io.dout;
    HIPCHK(c, hipMemcpyAsync(d, h, in.bytes(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(dO, 0, out.bytes(), st));
    InitLaunch L{};
    L.solver = sSolver.at(d);
    L.nSolvers = 1; L.nHyp = 1; L.maxHyp = 1;
    L.match = sMatch.at(d); L.first = sFirst.at(d);
    L.maskH = sMask.at(d); L.lastH = sLast.at(d); L.branch = sBranch.at(d); L.motions = sMotions.at(d);
    L.mR = sMR.at(d); L.mt = sMt.at(d);
    L.mCos = sMCos.at(dO); L.mGood = sMGood.at(dO); L.mStatus = sMStatus.at(dO); L.mVbGood = sMVb.at(dO); L.mP3D = sMP3D.at(dO);
    if (const int e = batch_finish(c, "init check", drfe_launch_init_check(L, st), b, out.bytes(), st)) return e;
    const char* ho = b->io.hout;
    *good = sMGood.at(ho)[0];
    *cosSel = sMCos.at(ho)[0];
    *status = sMStatus.at(ho)[0];
    *parallax = parallax_of(*good, *cosSel);
    std::memcpy(vbGood, sMVb.at(ho), N);
    std::memcpy(vP3D, sMP3D.at(ho), 3 * N * sizeof(float));
    return DRFE_OK;
}

int drfe_init_stats(drfe_ctx* c, int64_t* stats) { return batch_stats(c, &drfe_ctx::init, stats); }

}  // extern "C"
