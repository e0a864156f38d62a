/* Host-side check of the k_pyr_resize_tile item layout (DevLevel rz*) without a device: builds a context's tables and
 * geometry through orb_geometry.cpp and, for every level >= 1, replays the kernel's mapping of items to pixels.
 *   resize_plan <w> <h> <scale_factor> <nlevels>
 * prints one line per level: level w h lds fill coverage exact windows, where lds = 1 if the level takes the tile kernel,
 * coverage = bordered pixels computed / lane pixels launched, exact = 1 if every bordered pixel is stored exactly once
 * (directly or as a mirror image), windows = 1 if every tap the items read lies inside their block's LDS tile. */
#include "../../dr_slam_amd/csrc/drfe_internal.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    drfe_ctx* c = new drfe_ctx();
    c->cfg.nfeatures = 1000;
    c->cfg.scale_factor = (float)atof(argv[3]);
    c->cfg.nlevels = atoi(argv[4]);
    c->cfg.ini_th_fast = 20;
    c->cfg.min_th_fast = 7;
    const int w = atoi(argv[1]), h = atoi(argv[2]);
    drfe_build_tables(c);
    DevGeom g;
    std::vector<FastCell> cells;
    std::vector<BlurTile> tiles;
    std::vector<ResizeTap> taps;
    const int rc = drfe_build_geometry(c, w, h, &g, &cells, &tiles, &taps);
    if (rc != DRFE_OK) { printf("error %d %s\n", rc, c->err.c_str()); return 1; }
    for (int l = 1; l < g.nlevels; l++) {
        const DevLevel& L = g.lv[l];
        const DevLevel& P = g.lv[l - 1];
        const int bw = L.w + 2 * DRFE_EDGE, bh = L.h + 2 * DRFE_EDGE;
        const int rowEnd = L.rzRow0 + 4 * L.rzGroups, nItems = L.rzGroups * L.rzCols;
        std::vector<int> hits((size_t)bw * bh, 0);
        long long useful = 0;
        bool windows = true, inside = true;
        for (int item = 0; item < nItems; item++) {
            const int gi = item / L.rzCols, x4 = 4 * (item - gi * L.rzCols), y0 = L.rzRow0 + 4 * gi;
            const ResizeTap win = taps[L.rzWinOff + item / DRFE_RESIZE_BLOCK];
            int o[4];
            for (int k = 0; k < 4; k++) o[k] = (int)taps[L.xtabOff + x4 + k].s0 + DRFE_EDGE - (int)win.s1;
            /* bytes read: two dwords from each column pair's lower aligned dword */
            for (int pr = 0; pr < 2; pr++) {
                const int lo = std::min(o[2 * pr], o[2 * pr + 1]) & ~3;
                for (int k = 2 * pr; k < 2 * pr + 2; k++)
                    if (o[k] < 0 || o[k] + 1 - lo > 7) windows = false;
                if (lo + 8 > 16 * L.rzWq + 16) windows = false;
            }
            for (int k = 0; k < 4; k++)
                if (o[k] + 1 >= 16 * L.rzWq) windows = false;
            for (int r = 0; r < 4; r++) {
                const int y = y0 + r, p = y - DRFE_EDGE;
                if (y < 0 || y >= bh) { inside = false; continue; }
                const ResizeTap ty = taps[L.ytabOff + y];
                const int a = (int)ty.s0 + DRFE_EDGE - (int)win.s0, b = (int)ty.s1 + DRFE_EDGE - (int)win.s0;
                if (a < 0 || b >= L.rzRows) windows = false;
                std::vector<int> rows = {y};
                if (p >= 1 && p <= DRFE_EDGE && DRFE_EDGE - p < L.rzRow0) rows.push_back(DRFE_EDGE - p);
                const int yb = DRFE_EDGE + 2 * (L.h - 1) - p;
                if (p >= L.h - 1 - DRFE_EDGE && p <= L.h - 2 && yb >= rowEnd) rows.push_back(yb);
                for (int x = x4; x < x4 + 4; x++) {
                    if (x >= L.pyrPitch) { inside = false; continue; }
                    if (x >= bw) continue;                               /* pitch padding */
                    useful++;
                    for (int yy : rows) hits[(size_t)yy * bw + x]++;
                }
            }
        }
        /* the tile of every block stays inside the source level */
        for (int b = 0; b < L.rzBlocks; b++) {
            const ResizeTap win = taps[L.rzWinOff + b];
            if ((int)win.s0 + L.rzRows > P.h + 2 * DRFE_EDGE || (int)win.s1 + 16 * L.rzWq > P.pyrPitch || (win.s1 & 15)) windows = false;
        }
        bool exact = inside;
        for (int v : hits) exact = exact && v == 1;
        const double cover = (double)useful / ((double)L.rzBlocks * DRFE_RESIZE_BLOCK * 16);
        printf("%d %d %d %d %d %.4f %d %d\n", l, L.w, L.h, L.resizeLds, L.rzFill, cover, exact ? 1 : 0, windows ? 1 : 0);
    }
    delete c;
    return 0;
}
