/* orb_geometry.cpp — host-side constants of the ORB path: everything the reference computes once in
 * ORBextractor::ORBextractor (src/ORBextractor.cc:410-470) and the per-level geometry it derives per
 * frame in ComputePyramid (:1111-1113) / ComputeKeyPointsOctTree (:773-806), flattened into device
 * tables so the kernels contain no float geometry of their own. */
#include "drfe_internal.h"
#include "../../include/drfe_math.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

int drfe_build_tables(drfe_ctx* c)
{
    const int nl = c->cfg.nlevels;
    /* the reference stores scaleFactor in a double member initialised from the float argument
     * (include/ORBextractor.h:98) and multiplies float tables by it (:419-431) */
    const double sfd = (double)c->cfg.scale_factor;
    c->scale.assign(nl, 1.f); c->sigma2.assign(nl, 1.f);
    c->invScale.assign(nl, 1.f); c->invSigma2.assign(nl, 1.f);
    for (int i = 1; i < nl; i++) {
        c->scale[i] = (float)(c->scale[i - 1] * sfd);
        c->sigma2[i] = c->scale[i] * c->scale[i];
    }
    for (int i = 0; i < nl; i++) {
        c->invScale[i] = 1.0f / c->scale[i];
        c->invSigma2[i] = 1.0f / c->sigma2[i];
    }
    /* per-level quotas, :434-446 */
    c->quota.assign(nl, 0);
    const float factor = (float)(1.0f / sfd);
    float want = c->cfg.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; l++) {
        c->quota[l] = drfe_round_half_even(want);
        sum += c->quota[l];
        want *= factor;
    }
    c->quota[nl - 1] = std::max(c->cfg.nfeatures - sum, 0);
    /* umax, :454-469 */
    const int hp = DRFE_HALF_PATCH;
    for (int v = 0; v <= hp; v++) c->umax[v] = 0;
    const int vmax = (int)std::floor(hp * std::sqrt(2.f) / 2 + 1);
    const int vmin = (int)std::ceil(hp * std::sqrt(2.f) / 2);
    const double hp2 = hp * hp;
    for (int v = 0; v <= vmax; ++v) c->umax[v] = drfe_round_half_even_d(std::sqrt(hp2 - v * v));
    for (int v = hp, v0 = 0; v >= vmin; --v) {
        while (c->umax[v0] == c->umax[v0 + 1]) ++v0;
        c->umax[v] = v0;
        ++v0;
    }
    return DRFE_OK;
}

/* cv::resize(INTER_LINEAR) coefficient generation for one axis: source index pair
 * and the two 11-bit weights per destination index. */
static void build_taps_axis(int src, int dst, std::vector<ResizeTap>* out)
{
    const double inv = (double)dst / src;
    const double scale = 1. / inv;
    for (int d = 0; d < dst; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (s < 0) { s = 0; f = 0; }
        if (s >= src - 1) { s = src - 1; f = 0; }
        ResizeTap t;
        t.s0 = (uint16_t)s;
        t.s1 = (uint16_t)std::min(s + 1, src - 1);
        int w0 = drfe_round_half_even((1.f - f) * 2048.f), w1 = drfe_round_half_even(f * 2048.f);
        t.w0 = (int16_t)std::min(32767, std::max(-32768, w0));
        t.w1 = (int16_t)std::min(32767, std::max(-32768, w1));
        out->push_back(t);
    }
}

/* The table the kernel reads is indexed by the BORDERED destination coordinate (copyMakeBorder
 * REFLECT_101 of the resized interior, :1122-1123, folded into the lookup), starts 16-byte aligned and
 * is padded to `padded` entries with zero-weight taps (-> output 0 in the pitch padding) that keep the
 * last source position, so the source window of a thread's four taps stays <= 9 pixels wide. */
static void build_taps(int src, int dst, int padded, std::vector<ResizeTap>* out)
{
    std::vector<ResizeTap> axis;
    build_taps_axis(src, dst, &axis);
    if (out->size() & 1) out->push_back(ResizeTap{0, 0, 0, 0});
    const int bordered = dst + 2 * DRFE_EDGE;
    for (int b = 0; b < padded; b++) {
        if (b >= bordered) { ResizeTap z = out->back(); z.w0 = z.w1 = 0; out->push_back(z); continue; }
        int p = b - DRFE_EDGE;
        if (p < 0) p = -p;
        if (p >= dst) p = 2 * (dst - 1) - p;
        out->push_back(axis[p]);
    }
}

/* Item layout and source tiles of k_pyr_resize_tile for level L resized from P (see DevLevel).  Lanes go to bordered columns
 * only (rzCols = ceil((w + 38) / 4) per row group), and the rows computed directly are chosen among [h, h + 38] so that the
 * frame's last block is as full as possible.  Each block's tile is the union of the source windows of its items; all blocks
 * of a level load the same rzRows x rzWq quads (origins pulled back inside the source level where needed), so the fill is a
 * fixed count per thread. */
static void plan_resize_tile(DevLevel& L, const DevLevel& P, std::vector<ResizeTap>* taps)
{
    const int bw = L.w + 2 * DRFE_EDGE, bh = L.h + 2 * DRFE_EDGE, B = DRFE_RESIZE_BLOCK;
    const int cols = (bw + 3) / 4;
    int groups = 0, blocks = 0;
    for (int ng = (L.h + 3) / 4; 4 * ng <= bh; ng++) {
        const int nb = (ng * cols + B - 1) / B;
        /* fill = ng * cols / (nb * B); ties keep the fewer rows */
        if (!groups || (long long)ng * cols * blocks > (long long)groups * cols * nb) { groups = ng; blocks = nb; }
    }
    const int extra = 4 * groups - L.h;
    L.rzCols = cols; L.rzGroups = groups; L.rzBlocks = blocks;
    L.rzRow0 = DRFE_EDGE - std::max(0, extra - DRFE_EDGE);
    L.rzColsMagic = drfe_div_magic((uint32_t)cols);
    /* the kernel serves both taps of a column with one 8-byte window per column pair: the pair's first taps must lie within
     * 3 pixels of each other; scale factors up to 2 give at most 2, and that is what is checked */
    bool ok = true;
    const ResizeTap* xt = taps->data() + L.xtabOff;
    const ResizeTap* yt = taps->data() + L.ytabOff;
    for (int x = 0; x < 4 * cols; x += 2)
        if (std::abs((int)xt[x].s0 - (int)xt[x + 1].s0) > 2) ok = false;
    /* per block: bordered source rows [r0, r1] and columns [c0, c1] its taps read (the kernel reads s0 + 1 for the second tap) */
    std::vector<int> r0v(blocks), c0v(blocks);
    int rows = 0, quads = 0;
    for (int b = 0; b < blocks; b++) {
        const int i0 = b * B, i1 = std::min(groups * cols, i0 + B);
        int r0 = 1 << 30, r1 = -1, c0 = 1 << 30, c1 = -1;
        for (int g = i0 / cols; g <= (i1 - 1) / cols; g++) {
            for (int y = L.rzRow0 + 4 * g; y < L.rzRow0 + 4 * g + 4; y++) {
                r0 = std::min(r0, (int)yt[y].s0 + DRFE_EDGE); r1 = std::max(r1, (int)yt[y].s1 + DRFE_EDGE);
            }
            const int ca = std::max(i0 - g * cols, 0), cb = std::min(i1 - g * cols, cols);
            for (int x = 4 * ca; x < 4 * cb; x++) {
                c0 = std::min(c0, (int)xt[x].s0 + DRFE_EDGE); c1 = std::max(c1, (int)xt[x].s0 + 1 + DRFE_EDGE);
            }
        }
        r0v[b] = r0; c0v[b] = c0 & ~15;
        rows = std::max(rows, r1 - r0 + 1);
        quads = std::max(quads, (c1 - c0v[b]) / 16 + 1);
    }
    const int pbh = P.h + 2 * DRFE_EDGE;
    if (rows > pbh || 16 * quads > P.pyrPitch) ok = false;
    quads = std::max(quads, 2);                 /* divisors of the kernel's multiply-high quotients must be >= 2 */
    L.rzRows = rows; L.rzWq = quads;
    L.rzWqMagic = drfe_div_magic((uint32_t)quads);
    L.rzFill = (rows * quads + B - 1) / B;
    if (L.rzFill > DRFE_RESIZE_MAX_FILL || rows * quads * 16 + 16 > DRFE_RESIZE_TILE_BYTES) ok = false;
    L.resizeLds = ok ? 1 : 0;
    L.rzWinOff = (int)taps->size();
    for (int b = 0; b < blocks; b++) {
        /* pulled back so that every block's rows x quads stay inside the source level (P.pyrPitch is a multiple of 64) */
        const int r0 = std::max(0, std::min(r0v[b], pbh - rows)), c0 = std::max(0, std::min(c0v[b], P.pyrPitch - 16 * quads));
        taps->push_back(ResizeTap{(uint16_t)r0, (uint16_t)c0, 0, 0});
    }
}

/* The same tile plan for level 1 when level 0 is the caller's image (level0_view.h): the items and their taps are those of
 * plan_resize_tile, the source has no border.  Window rows and columns are interior coordinates, the column origin is 16-byte
 * aligned in the caller's rows (w is a multiple of 16, so pulling a window back from the row's end keeps it aligned), and a
 * window never starts before column 0 or ends past w: only bytes a tap with a non-zero weight reads are counted (the last
 * column's second tap has weight 0 and may fall on the tile's spare bytes).  Appended behind every other table: the offsets
 * of the bordered plan do not move.  false: level 1 cannot run the tile kernel on an unbordered source. */
static bool plan_resize_tile_raw(DevGeom* g, std::vector<ResizeTap>* taps)
{
    const DevLevel& L = g->lv[1];
    const DevLevel& P = g->lv[0];
    g->rz0Rows = g->rz0Wq = g->rz0Fill = g->rz0WinOff = 0;
    g->rz0WqMagic = 0;
    if (!L.resizeLds || (P.w & 15)) return false;
    const int B = DRFE_RESIZE_BLOCK, cols = L.rzCols, groups = L.rzGroups, blocks = L.rzBlocks;
    const ResizeTap* xt = taps->data() + L.xtabOff;
    const ResizeTap* yt = taps->data() + L.ytabOff;
    std::vector<int> r0v(blocks), c0v(blocks);
    int rows = 0, quads = 0;
    for (int b = 0; b < blocks; b++) {
        const int i0 = b * B, i1 = std::min(groups * cols, i0 + B);
        int r0 = 1 << 30, r1 = -1, c0 = 1 << 30, c1 = -1;
        for (int gi = i0 / cols; gi <= (i1 - 1) / cols; gi++) {
            for (int y = L.rzRow0 + 4 * gi; y < L.rzRow0 + 4 * gi + 4; y++) {
                r0 = std::min(r0, (int)yt[y].s0); r1 = std::max(r1, (int)yt[y].s1);
            }
            const int ca = std::max(i0 - gi * cols, 0), cb = std::min(i1 - gi * cols, cols);
            for (int x = 4 * ca; x < 4 * cb; x++) {
                c0 = std::min(c0, (int)xt[x].s0); c1 = std::max(c1, (int)xt[x].s1);
            }
        }
        r0v[b] = r0; c0v[b] = c0 & ~15;
        rows = std::max(rows, r1 - r0 + 1);
        quads = std::max(quads, (c1 - c0v[b]) / 16 + 1);
    }
    quads = std::max(quads, 2);
    if (rows > P.h || 16 * quads > P.w) return false;
    const int fill = (rows * quads + B - 1) / B;
    if (fill > DRFE_RESIZE_MAX_FILL || rows * quads * 16 + 16 > DRFE_RESIZE_TILE_BYTES) return false;
    g->rz0Rows = rows; g->rz0Wq = quads; g->rz0Fill = fill;
    g->rz0WqMagic = drfe_div_magic((uint32_t)quads);
    g->rz0WinOff = (int)taps->size();
    for (int b = 0; b < blocks; b++) {
        const int r0 = std::max(0, std::min(r0v[b], P.h - rows)), c0 = std::max(0, std::min(c0v[b], P.w - 16 * quads));
        taps->push_back(ResizeTap{(uint16_t)r0, (uint16_t)c0, 0, 0});
    }
    return true;
}

int drfe_build_geometry(drfe_ctx* c, int w, int h, DevGeom* g, std::vector<FastCell>* cells,
                        std::vector<BlurTile>* tiles, std::vector<ResizeTap>* taps)
{
    const int nl = c->cfg.nlevels;
    g->nlevels = nl;
    g->iniTh = c->cfg.ini_th_fast;
    g->minTh = c->cfg.min_th_fast;
    g->imgW = w; g->imgH = h;
    g->fastMaxWh = 7;
    g->fastCols = 1;
    g->fastColsRows = 7;
    int pyrOff = 0, blurOff = 0, candOff = 0, kpOff = 0;
    if (cells) cells->clear();
    if (tiles) tiles->clear();
    if (taps) taps->clear();
    for (int l = 0; l < nl; l++) {
        DevLevel& L = g->lv[l];
        L.w = drfe_round_half_even((float)w * c->invScale[l]);
        L.h = drfe_round_half_even((float)h * c->invScale[l]);
        L.quota = c->quota[l];
        L.scale = c->scale[l];
        L.kpSize = (float)(int)(31 * c->scale[l]);
        L.minBX = DRFE_EDGE - 3; L.minBY = DRFE_EDGE - 3;
        L.maxBX = L.w - DRFE_EDGE + 3; L.maxBY = L.h - DRFE_EDGE + 3;
        const float width = (float)(L.maxBX - L.minBX), height = (float)(L.maxBY - L.minBY);
        L.nCols = (int)(width / 30.f);
        L.nRows = (int)(height / 30.f);
        if (L.nCols <= 0 || L.nRows <= 0) {
            c->err = "pyramid level " + std::to_string(l) + " is smaller than one 30-px FAST cell";
            return DRFE_ERR_INVALID;
        }
        L.wCell = (int)std::ceil(width / L.nCols);
        L.hCell = (int)std::ceil(height / L.nRows);
        if (L.wCell + 6 > DRFE_FAST_MAX_WIN || L.hCell + 6 > DRFE_FAST_MAX_WIN) {
            c->err = "FAST cell window exceeds the LDS tile";
            return DRFE_ERR_INVALID;
        }
        /* DistributeOctTree root nodes, :543-545 */
        L.nIni = (int)std::round((float)(L.maxBX - L.minBX) / (L.maxBY - L.minBY));
        if (L.nIni < 1) {
            c->err = "frame aspect ratio gives zero quadtree root nodes (reference divides by zero)";
            return DRFE_ERR_INVALID;
        }
        L.hX = (float)(L.maxBX - L.minBX) / L.nIni;
        L.pyrPitch = align_up(L.w + 2 * DRFE_EDGE, 64);
        L.pyrOff = pyrOff;
        pyrOff += align_up(L.pyrPitch * (L.h + 2 * DRFE_EDGE), 256);
        /* blurred level: 32 x 4-pixel tiles of 128 bytes (DRFE_BLUR_TILE_*), blurPitch = tiles per tile row.  Its only
         * reader gathers 37 x 37 patches: ~23 lines per patch instead of ~48 with row-major rows. */
        L.blurPitch = (L.w + DRFE_BTILE_W - 1) / DRFE_BTILE_W;
        L.blurOff = blurOff;
        blurOff += align_up(L.blurPitch * ((L.h + DRFE_BTILE_H - 1) / DRFE_BTILE_H) * 128, 256);
        /* FAST cells in the reference's loop order with its skip rules, :789-806 */
        L.cellBegin = cells ? (int)cells->size() : 0;
        int candCap = 0;
        for (int i = 0; i < L.nRows; i++) {
            const float iniY = (float)(L.minBY + i * L.hCell);
            float maxY = iniY + L.hCell + 6;
            if (iniY >= L.maxBY - 3) continue;
            if (maxY > L.maxBY) maxY = (float)L.maxBY;
            for (int j = 0; j < L.nCols; j++) {
                const float iniX = (float)(L.minBX + j * L.wCell);
                float maxX = iniX + L.wCell + 6;
                if (iniX >= L.maxBX - 6) continue;
                if (maxX > L.maxBX) maxX = (float)L.maxBX;
                FastCell fc;
                fc.x0 = (uint16_t)iniX; fc.y0 = (uint16_t)iniY;
                const int ww = (int)maxX - (int)iniX, wh = (int)maxY - (int)iniY;
                if (ww < 7 || wh < 7) continue; /* cv::FAST evaluates nothing */
                fc.ww = (uint8_t)ww; fc.wh = (uint8_t)wh;
                fc.level = (uint8_t)l;
                fc.off = (uint8_t)((fc.x0 + DRFE_EDGE) & 3);
                fc.srcOff = (uint32_t)(L.pyrOff + (fc.y0 + DRFE_EDGE) * L.pyrPitch + (fc.x0 + DRFE_EDGE - fc.off));
                fc.pitch = (uint32_t)L.pyrPitch;
                fc.candOff = 0; fc.candCap = 0;   /* filled once the level's capacity is known */
                fc.offX = (uint16_t)(j * L.wCell); fc.offY = (uint16_t)(i * L.hCell);
                fc.cellIdx = (uint32_t)(i * L.nCols + j);
                {
                    const int ew = ww - 6, eh = wh - 6;
                    const int ncp = (ew + 1) / 2, nrb0 = std::min(64 / ncp, eh);
                    const int rpl = (eh + nrb0 - 1) / nrb0;
                    const int nrb = (eh + rpl - 1) / rpl;      /* every block but the last one is full, the last one not empty */
                    fc.ncp = (uint8_t)ncp; fc.nrb = (uint8_t)nrb; fc.rpl = (uint8_t)rpl; fc.pad = 0;
                    fc.ncpMagic = (uint32_t)((65536 + ncp - 1) / ncp);
                    g->fastColsRows = std::max(g->fastColsRows, std::max(nrb * rpl + 6, wh));
                    if (ew > DRFE_FASTC_MAX_EW || rpl > DRFE_FASTC_MAX_RPL) g->fastCols = 0;
                }
                if (cells) cells->push_back(fc);
                if (wh > g->fastMaxWh) g->fastMaxWh = wh;
                /* strict 3x3 maxima: at most one per 2x2 block of the evaluated area */
                candCap += ((ww - 6 + 1) / 2) * ((wh - 6 + 1) / 2);
            }
        }
        L.cellEnd = cells ? (int)cells->size() : 0;
        L.candCap = align_up(std::max(candCap, 64), 64);
        L.candOff = candOff;
        if (cells)
            for (int k = L.cellBegin; k < L.cellEnd; k++) { (*cells)[k].candOff = (uint32_t)L.candOff; (*cells)[k].candCap = (uint32_t)L.candCap; }
        candOff += L.candCap;
        L.kpCap = std::max(L.quota, 4 * L.nIni) + 4;
        if (L.kpCap > DRFE_QT_MAX_NODES) {
            c->err = "nfeatures too large for the quadtree node pool";
            return DRFE_ERR_CAPACITY;
        }
        L.kpOff = kpOff;
        kpOff += L.kpCap;
        /* blur tiles */
        L.tileBegin = tiles ? (int)tiles->size() : 0;
        for (int ty = 0; ty < (L.h + DRFE_BLUR_TH - 1) / DRFE_BLUR_TH; ty++)
            for (int tx = 0; tx < (L.w + DRFE_BLUR_TW - 1) / DRFE_BLUR_TW; tx++) {
                BlurTile t; t.tx = (uint16_t)tx; t.ty = (uint16_t)ty; t.level = (uint16_t)l; t.pad = 0;
                if (tiles) tiles->push_back(t);
            }
        L.tileEnd = tiles ? (int)tiles->size() : 0;
        /* resize taps from level l-1 (cascade, :1120) */
        L.xtabOff = L.ytabOff = 0;
        L.resizeLds = 0;
        L.rzRow0 = L.rzGroups = L.rzCols = L.rzBlocks = L.rzRows = L.rzWq = L.rzFill = L.rzWinOff = 0;
        L.rzColsMagic = L.rzWqMagic = 0;
        if (l > 0 && taps) {
            if (taps->size() & 1) taps->push_back(ResizeTap{0, 0, 0, 0});
            L.xtabOff = (int)taps->size();
            build_taps(g->lv[l - 1].w, L.w, L.pyrPitch, taps);
            if (taps->size() & 1) taps->push_back(ResizeTap{0, 0, 0, 0});
            L.ytabOff = (int)taps->size();
            build_taps(g->lv[l - 1].h, L.h, align_up(L.h + 2 * DRFE_EDGE, 4), taps);   /* 4 rows per thread */
            plan_resize_tile(L, g->lv[l - 1], taps);
            {
                /* the register-only kernel reads a 12-byte window per four output columns: the supported scale factors are
                 * those it can run, whichever kernel a level takes */
                for (int x = 0; x + 3 < L.pyrPitch; x += 4) {
                    int lo = 1 << 30, hi = -1;
                    for (int k = 0; k < 4; k++) {
                        const ResizeTap& t = (*taps)[L.xtabOff + x + k];
                        lo = std::min(lo, (int)t.s0); hi = std::max(hi, (int)t.s1);
                    }
                    if (hi + DRFE_EDGE - ((lo + DRFE_EDGE) & ~3) > 11) {
                        c->err = "pyramid scale factor too large for the resize kernels (supported: up to 2.0)";
                        return DRFE_ERR_INVALID;
                    }
                }
            }
        }
    }
    /* k_fast_cells_cols keeps a lane's row scores in registers: the cells of at most 8 rows per lane (the four large levels
     * at 640x480) come first and run the 8-row instantiation, the rest the DRFE_FASTC_MAX_RPL one.  The table's order is
     * free: FastCell::cellIdx carries the emission order. */
    g->fastColsSmall = 0;
    if (cells) {
        std::stable_partition(cells->begin(), cells->end(), [](const FastCell& f) { return f.rpl <= 8; });
        for (const FastCell& f : *cells) g->fastColsSmall += f.rpl <= 8 ? 1 : 0;
    }
    /* level 0 in place (level0_view.h): the geometry's part of the eligibility */
    g->l0InPlace = 0;
    g->rz0Rows = g->rz0Wq = g->rz0Fill = g->rz0WinOff = 0;
    g->rz0WqMagic = 0;
    if (cells && taps && nl >= 2 && (w & 15) == 0) {
        bool fit = g->fastCols != 0;
        /* k_fast_cells_cols' tile row holds three 16-byte chunks: window width + its start inside the first aligned dword */
        for (const FastCell& f : *cells)
            if (f.level == 0 && f.ww + drfe_l0_fast_off(f.x0) > 48) fit = false;
        if (plan_resize_tile_raw(g, taps) && fit) g->l0InPlace = 1;
    }
    g->pyrSlotBytes = pyrOff;
    g->blurSlotBytes = blurOff;
    g->candSlotElems = candOff;
    g->kpSlotElems = kpOff;
    g->totalCells = cells ? (int)cells->size() : 0;
    g->totalTiles = tiles ? (int)tiles->size() : 0;
    return DRFE_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* k_quadtree: which instantiation a level runs                                                      */

#define X(T, K, M) {T, K, M},
const QtInstance drfe_qt_instances[] = {DRFE_QT_INSTANCES(X)};
#undef X
const int drfe_qt_ninstances = (int)(sizeof(drfe_qt_instances) / sizeof(drfe_qt_instances[0]));

/* FAST candidates per pixel fall with the level's size: on rendered indoor frames at 640x480 / 1.2 / 8 levels from 2.4 % of
 * 307 k pixels on level 0 to 0.8 % of 24 k on level 7 (7286 / 4070 / 2454 / 1489 / 947 / 587 / 363 / 202 candidates at most).
 * load = 2.66 % * pixels * (pixels / 307200)^0.36 lies 12 - 25 % above every one of them; a level that has more keeps the
 * rest in the global arrays. */
int drfe_quadtree_design_load(int pixels)
{
    return (int)std::ceil(0.0266 * (double)pixels * std::pow((double)pixels / 307200.0, 0.36));
}

/* DRFE_QT_FORCE: "<threads>,<kpt>" pairs separated by ';' -> out[2 * pairs]; anything malformed gives no pairs */
int drfe_quadtree_parse_force(const char* s, int* out)
{
    int n = 0;
    while (s && *s && n < DRFE_MAX_LEVELS) {
        char* e = nullptr;
        const long t = std::strtol(s, &e, 10);
        if (e == s || *e != ',') return 0;
        s = e + 1;
        const long k = std::strtol(s, &e, 10);
        if (e == s || (*e && *e != ';') || t <= 0 || k <= 0) return 0;
        out[2 * n] = (int)t; out[2 * n + 1] = (int)k;
        n++;
        s = *e ? e + 1 : e;
    }
    return n;
}

int drfe_orb_quadtree_plan(const drfe_config* cfg, int width, int height, int nframes, const char* force, int32_t* out)
{
    if (!cfg || !out || cfg->nlevels < 1 || cfg->nlevels > DRFE_MAX_LEVELS || width <= 0 || height <= 0 || nframes < 1) return DRFE_ERR_INVALID;
    drfe_ctx* c = new drfe_ctx();
    c->cfg = *cfg;
    drfe_build_tables(c);
    DevGeom g;
    int rc = drfe_build_geometry(c, width, height, &g, nullptr, nullptr, nullptr);
    if (rc == DRFE_OK) {
        int pairs[2 * DRFE_MAX_LEVELS];
        QtPlan plan;
        drfe_quadtree_plan(g, nframes, pairs, drfe_quadtree_parse_force(force, pairs), &plan);
        for (int i = 0; i < plan.nlaunch; i++)
            for (int l = plan.launch[i].level0; l < plan.launch[i].level0 + plan.launch[i].nlevels; l++) {
                const QtInstance& q = drfe_qt_instances[plan.inst[l]];
                int32_t* o = out + 5 * l;
                o[0] = q.threads; o[1] = q.kpt; o[2] = q.maxn; o[3] = g.lv[l].kpCap; o[4] = i;
            }
        rc = plan.nlaunch;
    }
    delete c;
    return rc;
}

void drfe_quadtree_plan(const DevGeom& g, int nframes, const int* force, int nforce, QtPlan* plan)
{
    const int nl = g.nlevels;
    /* a batch whose workgroups are all resident at once (2 x 512 threads per CU) finishes soonest as ONE launch of the
     * 512-thread kernel: it is latency-bound and a second launch would only queue behind the first */
    const bool small = nl * nframes <= 2 * 256;
    int capMax = 0;
    for (int l = 0; l < nl; l++) capMax = std::max(capMax, g.lv[l].kpCap);
    for (int l = 0; l < nl; l++) {
        const DevLevel& L = g.lv[l];
        int pick = -1;
        if (nforce > 0) {
            const int* f = force + 2 * std::min(l, nforce - 1);
            for (int i = 0; i < drfe_qt_ninstances && pick < 0; i++) {
                const QtInstance& q = drfe_qt_instances[i];
                /* of the 512-thread kernel's two node capacities the small one where it holds the level */
                if (q.threads == f[0] && q.kpt == f[1] && q.maxn >= L.kpCap && !(q.maxn > 256 && L.kpCap <= 256)) pick = i;
            }
        }
        if (pick < 0 && small) pick = capMax > 256 ? 0 : 1;
        if (pick < 0) {
            /* the smallest instantiation whose registers hold the design load; none does: the largest */
            const int load = drfe_quadtree_design_load(L.w * L.h);
            pick = L.kpCap > 256 ? 0 : 1;
            for (int i = drfe_qt_ninstances - 1; i >= 1; i--) {
                const QtInstance& q = drfe_qt_instances[i];
                if (q.maxn >= L.kpCap && q.threads * q.kpt >= load) { pick = i; break; }
            }
        }
        plan->inst[l] = pick;
    }
    plan->nlaunch = 0;
    for (int l = 0; l < nl; l++) {
        if (l > 0 && plan->inst[l] == plan->inst[l - 1]) { plan->launch[plan->nlaunch - 1].nlevels++; continue; }
        plan->launch[plan->nlaunch++] = QtLaunch{l, 1, plan->inst[l]};
    }
}
