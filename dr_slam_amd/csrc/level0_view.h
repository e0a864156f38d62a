/* level0_view.h — pyramid level 0 read in place from the caller's image.
 *
 * copyMakeBorder(REFLECT_101) of the input into the arena is a pass none of level 0's readers needs: level 1's resize reads
 * interior pixels only, the FAST windows and the descriptor's raw patch lie inside the image, and the blur needs 3 px of
 * reflection which it can build itself.  Where drfe_level0_in_place_ok holds, drfe_launch_orb skips the two level-0 kernels
 * and the four readers address level 0 through a Level0Src.
 *
 * Every source address of those readers comes out of the helpers below, as a byte offset from the frame's first byte, so that
 * tests/native/level0_view.cpp can replay each block and thread on the host and check that nothing outside
 * [frame, frame + (h - 1) * rowStride + w) is read.  Host and device compile the same expressions. */
#ifndef DRFE_LEVEL0_VIEW_H
#define DRFE_LEVEL0_VIEW_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DRFE_L0_HD static __host__ __device__ inline
#else
#define DRFE_L0_HD static inline
#endif

/* the caller's frames as level 0; base == nullptr: level 0 is the bordered copy in the arena */
struct Level0Src {
    const uint8_t* base;
    size_t frameStride;
    uint32_t rowStride;
};

DRFE_L0_HD uint32_t drfe_umulhi32(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
/* n / d through the host's drfe_div_magic(d), d >= 2 */
DRFE_L0_HD uint32_t drfe_divm(uint32_t n, uint32_t d, uint32_t magic)
{
    const uint32_t q = drfe_umulhi32(n, magic);
    return q * d > n ? q - 1 : q;
}

/* ---- k_pyr_resize_tile: quad j of a block's source window (rows of wq 16-byte quads from the block's origin) ---- */
DRFE_L0_HD uint32_t drfe_rz_window_origin(uint32_t s0, uint32_t s1, uint32_t srcPitch) { return s0 * srcPitch + s1; }
DRFE_L0_HD uint32_t drfe_rz_fill_offset(uint32_t j, uint32_t wq, uint32_t wqMagic, uint32_t srcPitch, uint32_t* r, uint32_t* q)
{
    *r = drfe_divm(j, wq, wqMagic);
    *q = j - *r * wq;
    return *r * srcPitch + *q * 16u;
}

/* ---- k_fast_cells_cols: the window of a level-0 cell starts at interior (x0, y0) of the caller's rows ---- */
DRFE_L0_HD int drfe_l0_fast_off(int x0) { return x0 & 3; }                      /* window start inside its first aligned dword */
DRFE_L0_HD uint32_t drfe_l0_fast_origin(int x0, int y0, uint32_t rowStride) { return (uint32_t)y0 * rowStride + (uint32_t)(x0 & ~3); }
/* fill item i of a window whose rows take nch (<= 3) 16-byte chunks: row r, chunk c, byte offset from the window's origin */
DRFE_L0_HD uint32_t drfe_fastc_fill_offset(int i, int nch, uint32_t pitch, int* r, int* c)
{
    *r = nch == 1 ? i : nch == 2 ? (i >> 1) : (int)(((uint32_t)i * 21846u) >> 16);
    *c = i - *r * nch;
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24((uint32_t)*r, pitch) + (uint32_t)*c * 16u;
#else
    return (uint32_t)*r * pitch + (uint32_t)*c * 16u;
#endif
}

/* ---- k_blur, level-0 tiles ---- */
DRFE_L0_HD int drfe_l0_reflect(int p, int n)
{
    if (p < 0) p = -p;
    if (p >= n) p = 2 * (n - 1) - p;
    return p < 0 ? 0 : (p > n - 1 ? n - 1 : p);              /* rows past the reflection are never used: kept inside the image */
}
/* The thread of pixels x..x+3 (x a multiple of 4) reads the aligned dwords [x-4..x-1] [x..x+3] [x+4..x+7].  At the image's
 * first dword column the left one, at its last the right one lies outside the row: it is not loaded (the address falls back
 * on the middle dword) and one v_perm_b32 builds it from the middle one - columns -3..-1 are columns 3..1, columns w..w+2 are
 * columns w-2..w-4.  selL / selR = that permute's selector over (middle : left) / (right : middle); elsewhere the identity.
 * A thread past the row (a tile that overhangs the image) takes the last in-row thread's addresses and stores nothing. */
struct L0BlurCols { uint32_t l, m, r, selL, selR; };
DRFE_L0_HD L0BlurCols drfe_l0_blur_cols(int x, int w)
{
    const int xc = x < w - 4 ? x : w - 4;
    L0BlurCols c;
    c.m = (uint32_t)xc;
    c.l = xc == 0 ? (uint32_t)xc : (uint32_t)(xc - 4);
    c.r = xc == w - 4 ? (uint32_t)xc : (uint32_t)(xc + 4);
    c.selL = xc == 0 ? 0x05060704u : 0x03020100u;
    c.selR = xc == w - 4 ? 0x00000102u : 0x07060504u;
    return c;
}
/* source row of tile row t (0 = three rows above the tile's first output row) */
DRFE_L0_HD uint32_t drfe_l0_blur_row(int y0, int t, int h, uint32_t rowStride) { return (uint32_t)drfe_l0_reflect(y0 + t - 3, h) * rowStride; }

/* ---- k_orient_desc: the raw 31 x 31 patch as 31 rows of 9 aligned dwords ---- */
DRFE_L0_HD uint32_t drfe_l0_patch_origin(int x, int y, uint32_t rowStride) { return (uint32_t)(y - 15) * rowStride + (uint32_t)(x - 15); }
DRFE_L0_HD void drfe_desc_raw_dword(int t, int* row, int* colBytes)
{
    *row = (int)(((uint32_t)t * 7282u) >> 16);
    *colBytes = (t - *row * 9) * 4;
}

#endif
