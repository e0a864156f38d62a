/* Host-side replay of every level-0 load of the in-place path (dr_slam_amd/csrc/level0_view.h) without a device: builds a
 * context's geometry through orb_geometry.cpp and walks, block by block and thread by thread, the source addresses the four
 * readers of level 0 compute with the helpers the kernels call.
 *   level0_view <w> <h> <row_stride> <nlevels> [pointer offset in bytes]
 * prints one line:  eligible <0|1> loads <n> outside <n> padding <n> plan <0|1> reflect <0|1>
 *   eligible  drfe_level0_in_place_ok for a 16-byte aligned pointer plus the offset, frames align16(h * row_stride) apart
 *   loads     loads replayed: whenever the frame width gives level 1 a window plan for an unbordered source, eligible or not
 *             (a batch that is not eligible takes the copy path and reads nothing in place)
 *   outside   loads with a byte outside [frame, frame + (h - 1) * row_stride + w)
 *   padding   loads with a byte in a row's padding, columns [w, row_stride)
 *   plan      level 1's window origins are 16-byte aligned, every window lies inside the image and holds every tap of its block
 *   reflect   the blur's three dwords, after the edge permutes, are columns reflect101(x - 4 + k) wherever a tap is non-zero
 * A geometry the context refuses prints "error <code> <text>" and exits with 1. */
#include "../../dr_slam_amd/csrc/drfe_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Walk {
    long long w, h, rs, loads = 0, outside = 0, padding = 0;
    void read(long long off, int len)
    {
        loads++;
        const long long end = (h - 1) * rs + w;
        if (off < 0 || off + len > end) { outside++; return; }
        const long long c0 = off % rs, c1 = (off + len - 1) % rs;
        if (c0 >= w || c1 >= w || c1 < c0) padding++;
    }
};

/* v_perm_b32 D, S0 = hi, S1 = lo: selector bytes 0-3 pick from lo, 4-7 from hi (the selectors used here go no further) */
static void perm_cols(const int hi[4], const int lo[4], uint32_t sel, int out[4])
{
    for (int i = 0; i < 4; i++) {
        const int s = (int)((sel >> (8 * i)) & 0xFF);
        out[i] = s < 4 ? lo[s] : hi[s - 4];
    }
}

int main(int argc, char** argv)
{
    if (argc != 5 && argc != 6) return 2;
    const int w = atoi(argv[1]), h = atoi(argv[2]);
    const size_t rs = (size_t)atoll(argv[3]);
    const size_t ptrOff = argc == 6 ? (size_t)atoll(argv[5]) : 0;
    drfe_ctx* c = new drfe_ctx();
    c->cfg.nfeatures = 1000;
    c->cfg.scale_factor = 1.2f;
    c->cfg.nlevels = atoi(argv[4]);
    c->cfg.ini_th_fast = 20;
    c->cfg.min_th_fast = 7;
    drfe_build_tables(c);
    DevGeom g;
    std::vector<FastCell> cells;
    std::vector<BlurTile> tiles;
    std::vector<ResizeTap> taps;
    const int rc = drfe_build_geometry(c, w, h, &g, &cells, &tiles, &taps);
    if (rc != DRFE_OK) { printf("error %d %s\n", rc, c->err.c_str()); return 1; }
    const size_t frameStride = ((size_t)h * rs + 15) & ~(size_t)15;
    const bool eligible = drfe_level0_in_place_ok(g, reinterpret_cast<const void*>((uintptr_t)0x10000 + ptrOff), frameStride, rs);
    Walk W;
    W.w = w; W.h = h; W.rs = (long long)rs;
    bool plan = true, reflect = true;
    if (g.rz0Rows > 0 && rs % 16 == 0) {
        const uint32_t pitch = (uint32_t)rs;
        /* k_pyr_resize_tile, level 1: the fill of every block, then every item's taps against its block's window */
        {
            const DevLevel& L = g.lv[1];
            const uint32_t nq = (uint32_t)(g.rz0Rows * g.rz0Wq);
            for (int bx = 0; bx < L.rzBlocks; bx++) {
                const ResizeTap win = taps[(size_t)(g.rz0WinOff + bx)];
                const uint32_t origin = drfe_rz_window_origin(win.s0, win.s1, pitch);
                if ((win.s1 & 15) || (int)win.s1 + 16 * g.rz0Wq > w || (int)win.s0 + g.rz0Rows > h) plan = false;
                for (int tid = 0; tid < DRFE_RESIZE_BLOCK; tid++)
                    for (int k = 0; k < g.rz0Fill; k++) {
                        const uint32_t j = (uint32_t)(tid + k * DRFE_RESIZE_BLOCK), jc = j < nq ? j : 0u;
                        uint32_t r, q;
                        const uint32_t so = drfe_rz_fill_offset(jc, (uint32_t)g.rz0Wq, g.rz0WqMagic, pitch, &r, &q);
                        if (r != jc / (uint32_t)g.rz0Wq || q != jc % (uint32_t)g.rz0Wq || ((origin + so) & 15)) plan = false;
                        W.read((long long)origin + so, 16);
                    }
            }
            const int nItems = L.rzGroups * L.rzCols;
            for (int item = 0; item < nItems; item++) {
                const int gi = item / L.rzCols, x4 = 4 * (item - gi * L.rzCols), y0 = L.rzRow0 + 4 * gi;
                const ResizeTap win = taps[(size_t)(g.rz0WinOff + item / DRFE_RESIZE_BLOCK)];
                int o[4];
                for (int k = 0; k < 4; k++) {
                    const ResizeTap t = taps[(size_t)(L.xtabOff + x4 + k)];
                    o[k] = (int)t.s0 - (int)win.s1;
                    /* the second tap is the next byte; past the window only with weight 0 (the level's last column) */
                    if (o[k] < 0 || o[k] >= 16 * g.rz0Wq || (o[k] + 1 >= 16 * g.rz0Wq && t.w1 != 0)) plan = false;
                }
                for (int pr = 0; pr < 2; pr++) {
                    const int lo = std::min(o[2 * pr], o[2 * pr + 1]) & ~3;
                    for (int k = 2 * pr; k < 2 * pr + 2; k++)
                        if (o[k] + 1 - lo > 7) plan = false;
                    if (lo + 8 > 16 * g.rz0Wq + 16) plan = false;         /* the tile has 16 spare bytes */
                }
                for (int r = 0; r < 4; r++) {
                    const ResizeTap ty = taps[(size_t)(L.ytabOff + y0 + r)];
                    const int a = (int)ty.s0 - (int)win.s0, b = (int)ty.s1 - (int)win.s0;
                    if (a < 0 || b >= g.rz0Rows) plan = false;
                }
            }
        }
        /* k_fast_cells_cols: the window fill of every level-0 cell */
        for (const FastCell& fc : cells) {
            if (fc.level != 0) continue;
            const int off = drfe_l0_fast_off(fc.x0), need = fc.ww + off, nch = (need + 15) >> 4, sh = off & 1;
            if (need > 48 && eligible) plan = false;
            const uint32_t origin = drfe_l0_fast_origin(fc.x0, fc.y0, pitch);
            for (int i = 0; i < fc.wh * nch; i++) {
                int r, cc;
                const uint32_t so = drfe_fastc_fill_offset(i, nch, pitch, &r, &cc);
                if (r != i / nch || cc != i % nch) plan = false;
                W.read((long long)origin + so, 16);
                if (sh && cc * 16 + 16 < need) W.read((long long)origin + so + 16, 4);
            }
        }
        /* k_blur: the horizontal pass of every level-0 tile, 256 threads = 32 column groups x 8 row pairs per trip */
        for (const BlurTile& t : tiles) {
            if (t.level != 0) continue;
            const int x0 = t.tx * DRFE_BLUR_TW, y0 = t.ty * DRFE_BLUR_TH, colg = DRFE_BLUR_TW / 4, rowl = 256 / colg;
            const int pEnd = std::min((DRFE_BLUR_TH + 6) / 2, (std::min(DRFE_BLUR_TH, h - y0) + 7) >> 1);
            for (int tid = 0; tid < 256; tid++) {
                const int cg = tid & (colg - 1), rr = tid / colg, x = x0 + cg * 4;
                const L0BlurCols bc = drfe_l0_blur_cols(x, w);
                if (x < w) {
                    int L[4], M[4], R[4], l[4], r[4];
                    for (int k = 0; k < 4; k++) { L[k] = (int)bc.l + k; M[k] = (int)bc.m + k; R[k] = (int)bc.r + k; }
                    perm_cols(M, L, bc.selL, l);
                    perm_cols(R, M, bc.selR, r);
                    for (int k = 1; k <= 10; k++) {                    /* bytes 1..10 carry taps */
                        const int col = k < 4 ? l[k] : k < 8 ? M[k - 4] : r[k - 8];
                        int want = x - 4 + k;
                        if (want < 0) want = -want;
                        if (want >= w) want = 2 * (w - 1) - want;
                        if (col != want) reflect = false;
                    }
                }
                for (int p = rr; p < pEnd; p += rowl)
                    for (int tr = 2 * p; tr <= 2 * p + 1; tr++) {
                        const uint32_t ro = drfe_l0_blur_row(y0, tr, h, pitch);
                        int wantRow = y0 + tr - 3;
                        if (wantRow < 0) wantRow = -wantRow;
                        if (wantRow >= h) wantRow = 2 * (h - 1) - wantRow;
                        /* rows up to h + 2 reach an output row; what lies beyond only has to stay inside the image */
                        if (y0 + tr - 3 <= h + 2 && ro != (uint32_t)wantRow * pitch) reflect = false;
                        W.read((long long)ro + bc.l, 4); W.read((long long)ro + bc.m, 4); W.read((long long)ro + bc.r, 4);
                    }
            }
        }
        /* k_orient_desc: the raw patch of keypoints along the rim of where a keypoint can lie, 19 px inside the level */
        for (int y : {19, 20, h - 21, h - 20})
            for (int x = 19; x <= w - 20; x++) {
                const uint32_t o0 = drfe_l0_patch_origin(x, y, pitch), base = o0 & ~3u;
                for (int t = 0; t < 31 * 9; t++) {
                    int row, col;
                    drfe_desc_raw_dword(t, &row, &col);
                    if (row != t / 9 || col != (t % 9) * 4) plan = false;
                    W.read((long long)base + (long long)row * pitch + col, 4);
                }
                /* the patch's 31 columns lie inside the 36 bytes fetched */
                if ((int)(o0 & 3u) + 31 > 36) plan = false;
            }
        for (int x : {19, w - 20})
            for (int y = 19; y <= h - 20; y++) {
                const uint32_t base = drfe_l0_patch_origin(x, y, pitch) & ~3u;
                for (int row = 0; row < 31; row += 30) { W.read((long long)base + (long long)row * pitch, 4); W.read((long long)base + (long long)row * pitch + 32, 4); }
            }
    }
    printf("eligible %d loads %lld outside %lld padding %lld plan %d reflect %d\n", eligible ? 1 : 0, W.loads, W.outside, W.padding,
           plan ? 1 : 0, reflect ? 1 : 0);
    delete c;
    return 0;
}
