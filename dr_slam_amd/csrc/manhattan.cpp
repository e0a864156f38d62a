/* manhattan.cpp — Manhattan-frame tracking (Tracking::TrackManhattanFrame, reference src/Tracking.cc:1336-1527) behind the
 * C-ABI of include/drfe.h: the single-frame host entry, and the batch entry over the device-resident records of the most
 * recent drfe_surface_normals_batch (manhattan_kernels.hip).  Both evaluate manhattan_core.h; DESIGN.md section 11. */
#include "post_internal.h"
#include "manhattan_core.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

/* One TrackManhattanFrame call on the host: the conic pass over all three axes, the threshold, then the mean-shift pass
 * axis by axis on the R it keeps updating (R_cm aliases R_cm_update), then the assembly. */
void track_once(float R[9], const drfe_surface_normal* recs, int n, const double* dirs, int nl, int call,
                std::vector<uint8_t>& cone, drfe_manhattan_call* ci, uint16_t* rb, uint16_t* lb)
{
    std::memset(ci, 0, sizeof(*ci));
    cone.assign((size_t)n + nl, 0);
    float M[9], o[3];
    for (int a = 1; a <= 3; a++) {
        mf_axis_rows(R, a, M);
        for (int i = 0; i < n; i++) {
            mf_nini_normal(M, recs[i].normal, o);
            if (mf_lambda(o) < DRFE_MF_SIN_NORMAL_CONE) {
                cone[i] |= (uint8_t)(1 << (a - 1));
                ci->in_cone[a - 1]++;
                if (rb) rb[i] |= DRFE_MANHATTAN_INLINE_BIT;
            }
        }
        for (int l = 0; l < nl; l++) {
            mf_nini_line(M, dirs + 3 * l, o);
            if (mf_lambda(o) < DRFE_MF_SIN_LINE_CONE) {
                cone[(size_t)n + l] |= (uint8_t)(1 << (a - 1));
                if (lb) lb[l] |= DRFE_MANHATTAN_INLINE_BIT;
            }
        }
    }
    int thr = n / 20;
    int s0 = ci->in_cone[0], s1 = ci->in_cone[1], s2 = ci->in_cone[2], t;
    if (s0 > s1) t = s0, s0 = s1, s1 = t;
    if (s1 > s2) t = s1, s1 = s2, s2 = t;
    if (s0 > s1) t = s0, s0 = s1, s1 = t;
    if (s1 < thr) { thr = (s1 + s0) / 2; ci->deficient = 1; }
    ci->threshold = thr;
    for (int a = 1; a <= 3; a++) {
        mf_axis_rows(R, a, M);
        const uint8_t bit = (uint8_t)(1 << (a - 1));
        const uint16_t pushed = (uint16_t)(1u << (3 * call + a - 1));
        double sx = 0, sy = 0, sk = 0, w[3], mx, my;
        int sel = 0;
        for (int i = 0; i < n + nl; i++) {
            if (!(cone[i] & bit)) continue;
            if (i < n) mf_nini_normal(M, recs[i].normal, o);
            else mf_nini_line(M, dirs + 3 * (i - n), o);
            const double lam = mf_lambda(o);
            if (!(lam < DRFE_MF_SIN_MS_CONE)) continue;
            if (i < n) { if (rb) rb[i] |= pushed; }
            else if (lb) lb[i - n] |= pushed;
            if (!mf_mj(lam, o, &mx, &my)) continue;
            mf_weight(mx, my, w);
            sx += w[0]; sy += w[1]; sk += w[2];
            sel++;
        }
        ci->n_selected[a - 1] = sel;
        if (sel > thr) {
            float col[3];
            if (mf_axis_tail(M, sx, sy, sk, sel, col, &ci->density[a - 1])) {
                ci->found |= bit;
                for (int r = 0; r < 3; r++) R[r * 3 + a - 1] = col[r];
            }
        }
    }
    ci->svd = mf_assemble(R, ci->found) ? 1 : 0;
}

}  // namespace

struct MfBuffers {                 /* drfe_manhattan_track_batch's buffers */
    DevBuf<float> R0, R;
    DevBuf<drfe_manhattan_info> info;
    DevBuf<uint16_t> rbits, lbits;
    DevBuf<double> dirs, sums;
    DevBuf<int32_t> loff;
    DevBuf<uint8_t> cone;
    PinnedBuf<float> hR0;          /* pinned staging of the host inputs */
    PinnedBuf<double> hDirs;
    PinnedBuf<int32_t> hLoff;
    hipEvent_t staged = nullptr;   /* the staging copies of the previous batch are done */
    int frames = 0, nrec = 0;      /* the most recent batch */
    std::vector<int32_t> lineOff;  /* its line offsets */
};

void drfe_manhattan_free(drfe_ctx* c)
{
    MfBuffers* b = c->mf;
    if (!b) return;
    if (b->staged) {
        (void)hipEventSynchronize(b->staged);
        (void)hipEventDestroy(b->staged);
    }
    delete b;
    c->mf = nullptr;
}

extern "C" {

int drfe_manhattan_track_host(const float* R_in, const drfe_surface_normal* recs, int n, const double* line_dirs, int n_lines,
                              int n_calls, float* R_out, drfe_manhattan_info* info, uint16_t* rec_bits, uint16_t* line_bits)
{
    if (!R_in || !R_out || n < 0 || n_lines < 0 || (n > 0 && !recs) || (n_lines > 0 && !line_dirs) || n_calls < 1 ||
        n_calls > DRFE_MANHATTAN_MAX_CALLS)
        return DRFE_ERR_INVALID;
    float R[9];
    std::memcpy(R, R_in, sizeof(R));
    drfe_manhattan_info inf;
    std::memset(&inf, 0, sizeof(inf));
    inf.n_calls = n_calls;
    if (rec_bits) std::memset(rec_bits, 0, (size_t)n * sizeof(uint16_t));
    if (line_bits) std::memset(line_bits, 0, (size_t)n_lines * sizeof(uint16_t));
    std::vector<uint8_t> cone;
    for (int k = 0; k < n_calls; k++) track_once(R, recs, n, line_dirs, n_lines, k, cone, &inf.call[k], rec_bits, line_bits);
    std::memcpy(R_out, R, sizeof(R));
    if (info) *info = inf;
    return DRFE_OK;
}

int drfe_manhattan_track_batch(drfe_ctx* c, const float* R0, int nseq, int seq_len, const double* line_dirs,
                               const int32_t* line_offsets, int n_calls, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    if (!R0 || nseq < 1 || seq_len < 1 || n_calls < 1 || n_calls > DRFE_MANHATTAN_MAX_CALLS || (!line_dirs) != (!line_offsets)) {
        c->err = "manhattan_track_batch: invalid argument";
        return DRFE_ERR_INVALID;
    }
    SnBuffers* sn = c->sn;
    const size_t frames = (size_t)nseq * seq_len;
    if (!sn || !sn->d_recs || frames > (size_t)sn->lastFrames) {
        c->err = "manhattan_track_batch: the most recent drfe_surface_normals_batch holds fewer frames";
        return DRFE_ERR_STATE;
    }
    const int nrec = (drfe_sn_w((int)sn->w) / 2) * (drfe_sn_h((int)sn->h) / 2);
    std::vector<int32_t> loff(frames + 1, 0);
    int maxLines = 0;
    if (line_offsets) {
        if (line_offsets[0] != 0) { c->err = "manhattan_track_batch: line_offsets[0] != 0"; return DRFE_ERR_INVALID; }
        for (size_t f = 0; f < frames; f++) {
            if (line_offsets[f + 1] < line_offsets[f]) { c->err = "manhattan_track_batch: line_offsets decrease"; return DRFE_ERR_INVALID; }
            maxLines = std::max(maxLines, line_offsets[f + 1] - line_offsets[f]);
        }
        std::memcpy(loff.data(), line_offsets, loff.size() * sizeof(int32_t));
    }
    const size_t nLines = (size_t)loff[frames];
    HIPCHK(c, hipSetDevice(c->device));
    MfBuffers* b = c->mf;
    if (!b) { b = new MfBuffers(); c->mf = b; }
    if (!b->staged) HIPCHK(c, hipEventCreateWithFlags(&b->staged, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(b->staged));         /* the previous batch's staging is free again */
    const size_t scratch = (size_t)nrec + maxLines;     /* entries per sequence: the frame's records, then its lines */
    const size_t nDirs = std::max<size_t>(nLines, 1);
    HIPCHK(c, b->R0.grow((size_t)nseq * 9));
    HIPCHK(c, b->R.grow(frames * 9));
    HIPCHK(c, b->info.grow(frames));
    HIPCHK(c, b->loff.grow(frames + 1));
    HIPCHK(c, b->rbits.grow(frames * (size_t)nrec));
    HIPCHK(c, b->dirs.grow(nDirs * 3));
    HIPCHK(c, b->lbits.grow(nDirs));
    HIPCHK(c, b->cone.grow((size_t)nseq * scratch));
    HIPCHK(c, b->sums.grow((size_t)nseq * scratch * 3));
    HIPCHK(c, b->hR0.grow((size_t)nseq * 9));
    HIPCHK(c, b->hLoff.grow(frames + 1));
    HIPCHK(c, b->hDirs.grow(nDirs * 3));
    std::memcpy(b->hR0, R0, (size_t)nseq * 9 * sizeof(float));
    std::memcpy(b->hLoff, loff.data(), loff.size() * sizeof(int32_t));
    if (nLines) std::memcpy(b->hDirs, line_dirs, nLines * 3 * sizeof(double));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, hipMemcpyAsync(b->R0, b->hR0, (size_t)nseq * 9 * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(b->loff, b->hLoff, loff.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (nLines) HIPCHK(c, hipMemcpyAsync(b->dirs, b->hDirs, nLines * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(b->staged, s));
    hipError_t e = drfe_launch_manhattan(sn->d_recs, nrec, b->R0, nseq, seq_len, b->dirs, b->loff, n_calls, b->cone, b->sums,
                                         scratch, b->R, b->info, b->rbits, b->lbits, s);
    if (e != hipSuccess) { c->err = std::string("manhattan_track_batch: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
    b->frames = (int)frames;
    b->nrec = nrec;
    b->lineOff.swap(loff);
    return DRFE_OK;
}

int drfe_manhattan_download(drfe_ctx* c, int frame, float* R, drfe_manhattan_info* info, uint16_t* rec_bits, uint16_t* line_bits)
{
    if (!c) return DRFE_ERR_INVALID;
    MfBuffers* b = c->mf;
    if (!b || frame < 0 || frame >= b->frames) { c->err = "manhattan_download: no such frame"; return DRFE_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (R) HIPCHK(c, hipMemcpy(R, b->R + (size_t)frame * 9, 9 * sizeof(float), hipMemcpyDeviceToHost));
    if (info) HIPCHK(c, hipMemcpy(info, b->info + frame, sizeof(*info), hipMemcpyDeviceToHost));
    if (rec_bits)
        HIPCHK(c, hipMemcpy(rec_bits, b->rbits + (size_t)frame * b->nrec, (size_t)b->nrec * sizeof(uint16_t), hipMemcpyDeviceToHost));
    const int l0 = b->lineOff[frame], nl = b->lineOff[frame + 1] - l0;
    if (line_bits && nl > 0) HIPCHK(c, hipMemcpy(line_bits, b->lbits + l0, (size_t)nl * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return DRFE_OK;
}

int drfe_debug_manhattan_math(int which, const double* x, int n, double* out)
{
    if (!x || !out || n < 0 || which < 0 || which > 2) return DRFE_ERR_INVALID;
    for (int i = 0; i < n; i++)
        out[i] = which == 0 ? drfe_asin(x[i]) : which == 1 ? drfe_exp(x[i]) : (double)drfe_tanf((float)x[i]);
    return DRFE_OK;
}

}  // extern "C"
