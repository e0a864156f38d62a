/* triangulate.cpp — the per-match body of LocalMapping::CreateNewMapPoints / CreateNewMapLines2 (reference
 * src/LocalMapping.cc:383-538, 875-1026) behind the C-ABI of include/drfe.h: the two host entries (no context), the two batch
 * entries (triangulate_kernels.hip) and their counters.  Both sides evaluate triangulate_core.h; DESIGN.md section 15. */
#include "triangulate_internal.h"
#include "hip_buf.h"
#include "stage_layout.h"

#include <cstring>
#include <string>
#include <vector>

struct TriBuffers {
    StagePair io;                      /* staging: one copy each way */
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

void drfe_triangulate_free(drfe_ctx* c)
{
    delete c->tri;
    c->tri = nullptr;
}

namespace {

/* the feature arrays of either kind, for validation and staging */
struct Feats {
    const int32_t *off, *octave;
    const float *a, *b, *c, *d;        /* points: un, raw, u_right, depth; lines: ends, depth */
    const double* l3;
};
Feats feats_of(const drfe_tri_keypoints* k) { return Feats{k->offsets, k->octave, k->un, k->raw, k->u_right, k->depth, nullptr}; }
Feats feats_of(const drfe_tri_keylines* k) { return Feats{k->offsets, k->octave, k->ends, k->depth, nullptr, nullptr, k->lines3d}; }

TriView view_of(const drfe_tri_keyframes* k, const Feats& f, bool line)
{
    TriView V{};
    V.kf = k->kf;
    V.scale = k->scale_factors;
    V.sigma2 = k->level_sigma2;
    V.nLevels = k->n_levels;
    V.off = f.off;
    V.octave = f.octave;
    if (line) { V.ends = f.a; V.depthLine = f.b; V.lines3d = f.l3; }
    else { V.un = f.a; V.raw = f.b; V.uRight = f.c; V.depth = f.d; }
    return V;
}

/* all-or-nothing validation of a call */
int check_args(int monocular, const drfe_tri_keyframes* k, const Feats* f, const drfe_tri_pairs* p, const drfe_tri_out* o, bool line,
               std::string& err)
{
    err = "triangulate: invalid argument";
    if (monocular) { err = "triangulate: the monocular branch is not supported"; return DRFE_ERR_INVALID; }
    if (!k || !p || !o || k->n < 0 || p->n < 0) return DRFE_ERR_INVALID;
    if (p->n == 0) return DRFE_OK;
    if (!p->kf1 || !p->kf2 || !p->match_offsets || p->match_offsets[0] != 0 || !o->status) return DRFE_ERR_INVALID;
    if (k->n < 1 || !k->kf || k->n_levels < 1 || !k->scale_factors || !k->level_sigma2 || !f->off || f->off[0] < 0)
        return DRFE_ERR_INVALID;
    for (int q = 0; q < k->n; q++)
        if (f->off[q + 1] < f->off[q]) { err = "triangulate: decreasing feature offsets"; return DRFE_ERR_INVALID; }
    for (int i = 0; i < p->n; i++) {
        if (p->match_offsets[i + 1] < p->match_offsets[i]) { err = "triangulate: decreasing match_offsets"; return DRFE_ERR_INVALID; }
        if (p->kf1[i] < 0 || p->kf1[i] >= k->n || p->kf2[i] < 0 || p->kf2[i] >= k->n) {
            err = "triangulate: keyframe index out of range";
            return DRFE_ERR_INVALID;
        }
    }
    const int M = p->match_offsets[p->n];
    if (M > 0 && (!p->matches || !f->octave || !f->a || !f->b || (line ? !f->l3 : (!f->c || !f->d)))) return DRFE_ERR_INVALID;
    for (int i = 0; i < p->n; i++) {
        const int f1 = p->kf1[i], f2 = p->kf2[i];
        for (int m = p->match_offsets[i]; m < p->match_offsets[i + 1]; m++) {
            const int i1 = p->matches[2 * (size_t)m], i2 = p->matches[2 * (size_t)m + 1];
            if (i1 < 0 || i1 >= f->off[f1 + 1] - f->off[f1] || i2 < 0 || i2 >= f->off[f2 + 1] - f->off[f2]) {
                err = "triangulate: feature index out of range";
                return DRFE_ERR_INVALID;
            }
            const int g[2] = {f->off[f1] + i1, f->off[f2] + i2};
            for (int s = 0; s < 2; s++) {
                if (f->octave[g[s]] < 0 || f->octave[g[s]] >= k->n_levels) { err = "triangulate: octave out of range"; return DRFE_ERR_INVALID; }
                if (!line && f->c[g[s]] >= 0 && !(f->d[g[s]] > 0)) {
                    err = "triangulate: a stereo keypoint (u_right >= 0) without depth";
                    return DRFE_ERR_INVALID;
                }
            }
        }
    }
    return DRFE_OK;
}

/* the per-pair outputs and the counters from the per-match statuses */
void finish_pairs(const drfe_tri_pairs* p, const std::vector<uint8_t>& skip, const uint8_t* status, const uint8_t* branch,
                  drfe_tri_out* o, int64_t* stats)
{
    for (int i = 0; i < p->n; i++) {
        int acc = 0;
        for (int m = p->match_offsets[i]; m < p->match_offsets[i + 1]; m++) {
            acc += (status[m] & 0x7F) == DRFE_TRI_ACCEPTED ? 1 : 0;
            if (stats && branch[m] >= DRFE_TRI_BRANCH_SVD) stats[3 + branch[m]]++;
        }
        if (o->pair_skipped) o->pair_skipped[i] = skip[(size_t)i];
        if (o->accepted) o->accepted[i] = acc;
        if (stats) { stats[2] += skip[(size_t)i]; stats[7] += acc; }
    }
}

template <bool Line>
int tri_host(int monocular, const drfe_tri_keyframes* k, const Feats& f, const drfe_tri_pairs* p, drfe_tri_out* o)
{
    std::string err;
    const int rc = check_args(monocular, k, &f, p, o, Line, err);
    if (rc || p->n == 0) return rc;
    const TriView V = view_of(k, f, Line);
    const int M = p->match_offsets[p->n];
    std::vector<uint8_t> skip((size_t)p->n), br((size_t)M);
    const int w = Line ? 6 : 3;
    for (int i = 0; i < p->n; i++) {
        const int f1 = p->kf1[i], f2 = p->kf2[i];
        skip[(size_t)i] = tr_pair_skipped(k->kf[f1], k->kf[f2]) ? 1 : 0;
        for (int m = p->match_offsets[i]; m < p->match_offsets[i + 1]; m++) {
            const int i1 = p->matches[2 * (size_t)m], i2 = p->matches[2 * (size_t)m + 1];
            const int g1 = f.off[f1] + i1, g2 = f.off[f2] + i2;
            float X[6] = {0, 0, 0, 0, 0, 0};
            int b = DRFE_TRI_BRANCH_NONE, st;
            if (skip[(size_t)i]) st = DRFE_TRI_BASELINE;
            else if (Line) st = tr_line(V, f1, f2, g1, g2, i2 < f.off[f1 + 1] - f.off[f1] ? f.off[f1] + i2 : -1, X, X + 3, &b);
            else st = tr_point(V, f1, f2, g1, g2, X, &b);
            o->status[m] = (uint8_t)st;
            br[(size_t)m] = (uint8_t)b;
            if (o->branch) o->branch[m] = (uint8_t)b;
            if (o->x3d)
                for (int q = 0; q < w; q++) o->x3d[(size_t)w * m + q] = (st & 0x7F) == DRFE_TRI_ACCEPTED ? X[q] : 0.f;
        }
    }
    finish_pairs(p, skip, o->status, br.data(), o, nullptr);
    return DRFE_OK;
}

/* the device path: one staging copy, one launch, one copy back */
template <bool Line>
int tri_batch(drfe_ctx* c, int monocular, const drfe_tri_keyframes* k, const Feats& f, const drfe_tri_pairs* p, drfe_tri_out* o,
              void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    const int rc = check_args(monocular, k, &f, p, o, Line, c->err);
    if (rc) return rc;
    TriBuffers* b = c->tri;
    if (!b) { b = new TriBuffers(); c->tri = b; }
    b->stats[0]++;
    if (p->n == 0) return DRFE_OK;
    b->stats[1] += p->n;
    const int M = p->match_offsets[p->n], K = k->n, L = k->n_levels, F = f.off[K];
    b->stats[3] += M;
    std::vector<uint8_t> skip((size_t)p->n);
    for (int i = 0; i < p->n; i++) skip[(size_t)i] = tr_pair_skipped(k->kf[p->kf1[i]], k->kf[p->kf2[i]]) ? 1 : 0;
    const size_t nF = (size_t)F;
    StageLayout<16> in, out;
    const auto sKf = in.add<drfe_tri_keyframe>((size_t)K);
    const auto sScale = in.add<float>((size_t)K * L), sSig = in.add<float>((size_t)K * L);
    const auto sOff = in.add<int32_t>((size_t)K + 1), sOct = in.add<int32_t>(nF);
    const auto sA = in.add<float>(nF * (Line ? 4 : 2)), sB = in.add<float>(nF * (Line ? 1 : 2));   /* points: un, raw; lines: ends, depth */
    const auto sRight = in.add<float>(Line ? 0 : nF), sDepth = in.add<float>(Line ? 0 : nF);
    const auto sL3 = in.add<double>(Line ? nF * 6 : 0);
    const auto sMatch = in.add<TriMatch>((size_t)M);
    const auto sStatus = out.add<uint8_t>((size_t)M), sBranch = out.add<uint8_t>((size_t)M);
    const auto sX = out.add<float>((size_t)M * (Line ? 6 : 3));
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, b->io.grow(in.bytes(), out.bytes()));
    char* h = b->io.hin;
    sKf.put(h, k->kf);
    sScale.put(h, k->scale_factors);
    sSig.put(h, k->level_sigma2);
    sOff.put(h, f.off);
    sOct.put(h, f.octave);
    sA.put(h, f.a);
    sB.put(h, f.b);
    sRight.put(h, f.c);
    sDepth.put(h, f.d);
    sL3.put(h, f.l3);
    TriMatch* rec = sMatch.at(h);
    for (int i = 0; i < p->n; i++)
        for (int m = p->match_offsets[i]; m < p->match_offsets[i + 1]; m++)
            rec[m] = TriMatch{skip[(size_t)i] ? -1 : p->kf1[i], p->kf2[i], p->matches[2 * (size_t)m], p->matches[2 * (size_t)m + 1]};
    const char* d = b->io.din;
    char* dO = b->io.dout;
    HIPCHK(c, hipMemcpyAsync(b->io.din, h, in.bytes(), hipMemcpyHostToDevice, s));
    TriLaunch Lc{};
    Lc.V.kf = sKf.at(d);
    Lc.V.scale = sScale.at(d);
    Lc.V.sigma2 = sSig.at(d);
    Lc.V.nLevels = L;
    Lc.V.off = sOff.at(d);
    Lc.V.octave = sOct.at(d);
    if (Line) {
        Lc.V.ends = sA.at(d);
        Lc.V.depthLine = sB.at(d);
        Lc.V.lines3d = sL3.at(d);
    } else {
        Lc.V.un = sA.at(d);
        Lc.V.raw = sB.at(d);
        Lc.V.uRight = sRight.at(d);
        Lc.V.depth = sDepth.at(d);
    }
    Lc.match = sMatch.at(d);
    Lc.n = M;
    Lc.line = Line ? 1 : 0;
    Lc.status = sStatus.at(dO);
    Lc.branch = sBranch.at(dO);
    Lc.x3d = sX.at(dO);
    hipError_t e = drfe_launch_triangulate(Lc, s);
    if (e == hipSuccess && M > 0) e = hipMemcpyAsync(b->io.hout, dO, out.bytes(), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { c->err = std::string("triangulate batch: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
    HIPCHK(c, hipStreamSynchronize(s));
    const char* ho = b->io.hout;
    const uint8_t* st = sStatus.at(ho);
    const uint8_t* br = sBranch.at(ho);
    sStatus.get(ho, o->status);
    sBranch.get(ho, o->branch);
    sX.get(ho, o->x3d);
    finish_pairs(p, skip, st, br, o, b->stats);
    return DRFE_OK;
}

}  // namespace

extern "C" {

int drfe_triangulate_points_host(int monocular, const drfe_tri_keyframes* kfs, const drfe_tri_keypoints* kps,
                                 const drfe_tri_pairs* pairs, drfe_tri_out* out)
{
    if (!kps) return DRFE_ERR_INVALID;
    return tri_host<false>(monocular, kfs, feats_of(kps), pairs, out);
}

int drfe_triangulate_lines_host(int monocular, const drfe_tri_keyframes* kfs, const drfe_tri_keylines* kls,
                                const drfe_tri_pairs* pairs, drfe_tri_out* out)
{
    if (!kls) return DRFE_ERR_INVALID;
    return tri_host<true>(monocular, kfs, feats_of(kls), pairs, out);
}

int drfe_triangulate_points_batch(drfe_ctx* ctx, int monocular, const drfe_tri_keyframes* kfs, const drfe_tri_keypoints* kps,
                                  const drfe_tri_pairs* pairs, drfe_tri_out* out, void* stream)
{
    if (!kps) return DRFE_ERR_INVALID;
    return tri_batch<false>(ctx, monocular, kfs, feats_of(kps), pairs, out, stream);
}

int drfe_triangulate_lines_batch(drfe_ctx* ctx, int monocular, const drfe_tri_keyframes* kfs, const drfe_tri_keylines* kls,
                                 const drfe_tri_pairs* pairs, drfe_tri_out* out, void* stream)
{
    if (!kls) return DRFE_ERR_INVALID;
    return tri_batch<true>(ctx, monocular, kfs, feats_of(kls), pairs, out, stream);
}

int drfe_triangulate_stats(drfe_ctx* c, int64_t* stats)
{
    if (!c || !stats) return DRFE_ERR_INVALID;
    if (c->tri) std::memcpy(stats, c->tri->stats, sizeof(c->tri->stats));
    else std::memset(stats, 0, 8 * sizeof(int64_t));
    return DRFE_OK;
}

int drfe_debug_triangulate_math(int which, const float* y, const float* x, int n, float* out)
{
    if (which < 0 || which > 2 || n < 0 || (n > 0 && (!y || !out || (which != 1 && !x)))) return DRFE_ERR_INVALID;
    for (int i = 0; i < n; i++)
        out[i] = which == 0 ? drfe_atan2f(y[i], x[i]) : which == 1 ? drfe_cosf(y[i]) : drfe_cosf(2 * drfe_atan2f(y[i] / 2, x[i]));
    return DRFE_OK;
}

int drfe_debug_triangulate_math_device(drfe_ctx* c, int which, const float* y, const float* x, int n, float* out)
{
    if (!c || which < 0 || which > 2 || n < 0 || (n > 0 && (!y || !out || (which != 1 && !x)))) return DRFE_ERR_INVALID;
    if (n == 0) return DRFE_OK;
    const size_t bytes = (size_t)n * sizeof(float);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> dy, dx, dout;
    HIPCHK(c, dy.alloc((size_t)n));
    HIPCHK(c, dout.alloc((size_t)n));
    HIPCHK(c, hipMemcpyAsync(dy, y, bytes, hipMemcpyHostToDevice, c->stream));
    if (which != 1) {
        HIPCHK(c, dx.alloc((size_t)n));
        HIPCHK(c, hipMemcpyAsync(dx, x, bytes, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, drfe_launch_triangulate_math(which, dy, which != 1 ? (const float*)dx : (const float*)dy, n, dout, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DRFE_OK;
}

}  // extern "C"
