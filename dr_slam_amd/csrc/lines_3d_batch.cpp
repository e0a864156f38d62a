/* lines_3d_batch.cpp — Frame::isLineGood for the key lines of many frames in one device call (lines_3d_kernels.hip) and its
 * counters; the single-frame host entry is lines_3d.cpp, the arithmetic of both line3d_core.h.  What is sequential and cheap -
 * a frame's glibc rand() stream, at most DRFE_LINE3D_DRAWS draws a key line - is drawn here into a table; the kernels only advance
 * an offset into it.  DESIGN.md section 18. */
#include "line3d_internal.h"
#include "glibc_rand.h"
#include "stage_layout.h"

#include <algorithm>
#include <cstring>

struct Line3dBuffers {
    StagePair io;                      /* staging: one copy each way */
    DevBuf<char> scratch;              /* the lifted samples and the RANSAC's result per key line */
    DevBuf<float> depth;               /* a chunk's depth images, when they come from the host */
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

void drfe_line3d_free(drfe_ctx* c)
{
    delete c->line3d;
    c->line3d = nullptr;
}

namespace {

int check(const drfe_line3d_frames* p, const drfe_line3d_out* o, std::string& err)
{
    err = "line3d: invalid argument";
    if (!p || !o || p->nframes < 0 || p->cap < 0) return DRFE_ERR_INVALID;
    if (p->nframes == 0) return DRFE_OK;
    if (p->cap > DRFE_LINE3D_MAX_CAP) { err = "line3d: cap above DRFE_LINE3D_MAX_CAP"; return DRFE_ERR_INVALID; }
    if (!p->n_lines || !p->depth || p->w < 1 || p->h < 1) return DRFE_ERR_INVALID;
    if (p->stride < (size_t)p->w) { err = "line3d: row stride below the width"; return DRFE_ERR_INVALID; }
    if (!o->n_good) return DRFE_ERR_INVALID;
    bool any = false;
    for (int f = 0; f < p->nframes; f++) {
        if (p->n_lines[f] < 0 || p->n_lines[f] > p->cap) { err = "line3d: n_lines outside [0, cap]"; return DRFE_ERR_INVALID; }
        any = any || p->n_lines[f] > 0;
    }
    if (any && (!p->lines || !o->depth_line || !o->lines3d)) return DRFE_ERR_INVALID;
    return DRFE_OK;
}

}  // namespace

extern "C" {

int drfe_line3d_chunk_frames(int cap)
{
    return cap > 0 ? std::max(1, DRFE_LINE3D_SCRATCH_LINES / cap) : DRFE_LINE3D_SCRATCH_LINES;
}

int drfe_lines_is_good_batch(drfe_ctx* c, const drfe_line3d_frames* p, drfe_line3d_out* o, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    if (const int rc = check(p, o, c->err)) return rc;
    Line3dBuffers* b = c->line3d;
    if (!b) { b = new Line3dBuffers(); c->line3d = b; }
    b->stats[0]++;
    if (p->nframes == 0) return DRFE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t cap = (size_t)p->cap;
    const size_t span = (size_t)(p->h - 1) * p->stride + (size_t)p->w;     /* floats of a frame's depth image */
    const int chunk = drfe_line3d_chunk_frames(p->cap);
    for (int f0 = 0; f0 < p->nframes; f0 += chunk) {
        const int nf = std::min(chunk, p->nframes - f0);
        const size_t slots = (size_t)nf * cap;
        const int32_t* nLines = p->n_lines + f0;
        StageLayout<16> in, out, scr;
        const auto sLines = in.add<drfe_keyline>(slots);
        const auto sNLines = in.add<int32_t>((size_t)nf);
        const auto sDraws = in.add<int32_t>(slots * DRFE_LINE3D_DRAWS);
        const auto sL3 = out.add<double>(slots * 6);
        const auto sDepthLine = out.add<float>(slots);
        const auto sInl = out.add<int32_t>(slots);
        const auto sGood = out.add<int32_t>((size_t)nf);
        const auto sStats = out.add<L3FrameStats>((size_t)nf);
        const auto sPts = scr.add<L3Point>(slots * L3_MAX_SAMPLES);
        const auto sBest = scr.add<L3Best>(slots);
        const auto sNPts = scr.add<int32_t>(slots);
        HIPCHK(c, b->io.grow(in.bytes(), out.bytes()));
        HIPCHK(c, b->scratch.grow(scr.bytes()));
        char* h = b->io.hin;
        int maxLines = 0;
        for (int f = 0; f < nf; f++) {
            const int n = nLines[f];
            maxLines = std::max(maxLines, n);
            if (n) std::memcpy(sLines.at(h) + (size_t)f * cap, p->lines + (size_t)(f0 + f) * cap, (size_t)n * sizeof(drfe_keyline));
            GlibcRand rng(p->seeds ? p->seeds[f0 + f] : 1u);
            int32_t* d = sDraws.at(h) + (size_t)f * cap * DRFE_LINE3D_DRAWS;
            for (int k = 0; k < n * DRFE_LINE3D_DRAWS; k++) d[k] = rng.next();
        }
        sNLines.put(h, nLines);
        Line3dLaunch L{};
        L.nframes = nf; L.cap = p->cap; L.w = p->w; L.h = p->h; L.maxLines = maxLines;
        L.stride = p->stride;
        L.cx = p->cx; L.cy = p->cy; L.invfx = p->invfx; L.invfy = p->invfy;
        L.f = l3_focal(p->K, p->k_as_f64);
        if (p->depth_on_device) {
            L.depth = p->depth + (size_t)f0 * p->frame_stride;
            L.frameStride = p->frame_stride;
        } else {
            HIPCHK(c, b->depth.grow((size_t)nf * span));
            L.depth = b->depth;
            L.frameStride = span;
            const float* src = p->depth + (size_t)f0 * p->frame_stride;
            if (p->frame_stride == span || nf == 1)
                HIPCHK(c, hipMemcpyAsync(b->depth, src, (size_t)nf * span * sizeof(float), hipMemcpyHostToDevice, st));
            else
                for (int f = 0; f < nf; f++)
                    HIPCHK(c, hipMemcpyAsync(b->depth + (size_t)f * span, src + (size_t)f * p->frame_stride, span * sizeof(float),
                                             hipMemcpyHostToDevice, st));
        }
        const char* d = b->io.din;
        char* dO = b->io.dout;
        char* dS = b->scratch;
        HIPCHK(c, hipMemcpyAsync(b->io.din, h, in.bytes(), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(dO, 0, out.bytes(), st));
        L.lines = sLines.at(d); L.nLines = sNLines.at(d); L.draws = sDraws.at(d);
        L.pts = sPts.at(dS); L.best = sBest.at(dS); L.nPts = sNPts.at(dS);
        L.lines3d = sL3.at(dO); L.depthLine = sDepthLine.at(dO); L.nInliers = sInl.at(dO); L.nGood = sGood.at(dO);
        L.frameStats = sStats.at(dO);
        hipError_t e = drfe_launch_line3d(L, st);
        if (e == hipSuccess) e = hipMemcpyAsync(b->io.hout, dO, out.bytes(), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) { c->err = std::string("line3d batch: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
        HIPCHK(c, hipStreamSynchronize(st));
        const char* ho = b->io.hout;
        b->stats[1] += nf;
        for (int f = 0; f < nf; f++) {
            const size_t n = (size_t)nLines[f], at = (size_t)f * cap, to = (size_t)(f0 + f) * cap;
            if (n) {
                std::memcpy(o->depth_line + to, sDepthLine.at(ho) + at, n * sizeof(float));
                std::memcpy(o->lines3d + 6 * to, sL3.at(ho) + 6 * at, n * 6 * sizeof(double));
                if (o->n_inliers) std::memcpy(o->n_inliers + to, sInl.at(ho) + at, n * sizeof(int32_t));
            }
            o->n_good[f0 + f] = sGood.at(ho)[f];
            const L3FrameStats& fs = sStats.at(ho)[f];
            b->stats[2] += (int64_t)n;
            b->stats[3] += fs.ransacLines;
            b->stats[4] += fs.iterations;
            b->stats[5] += fs.coincident;
            b->stats[6] += fs.rejected;
            b->stats[7] += sGood.at(ho)[f];
        }
    }
    return DRFE_OK;
}

int drfe_line3d_stats(drfe_ctx* c, int64_t* stats)
{
    if (!c || !stats) return DRFE_ERR_INVALID;
    if (c->line3d) std::memcpy(stats, c->line3d->stats, sizeof(c->line3d->stats));
    else std::memset(stats, 0, 8 * sizeof(int64_t));
    return DRFE_OK;
}

}  // extern "C"
