// Splat -> screen-tile rectangle: the pixel map, the conservative pixel range and its exact tightening.  Plain C++ that the
// host compiler takes as well (tests/test_tile_rect_cpu.py sweeps the straight-line form against the rolled loops on the CPU);
// under hipcc every function is __host__ __device__ and compiles for the device exactly as before.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DSS_HD __host__ __device__ __forceinline__
#else
#include <algorithm>
#define DSS_HD inline
#endif

#ifndef DSS_TILE
#define DSS_TILE 8           // screen tile side in pixels (one 256-thread workgroup per tile)
#endif

namespace dss {

#if !defined(__HIPCC__)
using std::max;
using std::min;
#endif

// Pixel index -> NDC centre.  Same expression, same fp32 rounding as PixToNdc
// (reference rasterization_utils.cuh:8-11): -1 + (2*i + 1.0f) / S.
DSS_HD float pix_to_ndc(int i, int S) { return -1 + (2 * i + 1.0f) / S; }

// Same value as pix_to_ndc for every S: when S is a power of two, multiplying by the exactly
// representable 1/S rounds identically to the division (one v_mul instead of a ~10-instruction
// IEEE divide in inner loops); otherwise fall back to the division.  `pow2` is wave-uniform.
struct NdcMap {
    int S;
    float invS;
    bool pow2;
    DSS_HD explicit NdcMap(int S_) : S(S_), invS(1.0f / (float)S_), pow2((S_ & (S_ - 1)) == 0) {}
    DSS_HD float operator()(int i) const
    {
        const float t = 2 * i + 1.0f;
        return pow2 ? -1 + t * invS : -1 + t / S;
    }
};

// Range [lo, hi] of NDC pixel indices i in [0,S) whose centre may satisfy |ndc(i) - x| <= r.
// Conservative (one pixel of slack each side); the exact fp32 test runs later per pixel.
// Non-finite inputs select the whole axis.  Returns false if the range is empty.
DSS_HD bool ndc_index_range(float x, float r, int S, int &lo, int &hi)
{
    const float flo = ((x - r + 1.0f) * S - 1.0f) * 0.5f;
    const float fhi = ((x + r + 1.0f) * S - 1.0f) * 0.5f;
    lo = 0;
    hi = S - 1;
    if (flo == flo && fhi == fhi) {  // not NaN
        if (fhi < -2.0f || flo > (float)S + 1.0f) return false;
        const float a = fmaxf(flo, -2.0f), b = fminf(fhi, (float)S + 1.0f);
        lo = max(0, (int)floorf(a) - 1);
        hi = min(S - 1, (int)ceilf(b) + 1);
    }
    return lo <= hi;
}

struct TileGrid {
    int S;        // image side
    int row0;     // first image row of the band
    int rows;     // rows in the band (band-local rows: the band tensors have this many rows)
    int tiles_x;  // tiles per band row
    int tiles_y;  // tile rows in the band
    int tshift;   // log2 of the image-row distance of two consecutive band tile rows: 3 for a contiguous band; 3 + log2(c)
                  // for a tile-row-CYCLIC band (multi-GPU: a rank owns every c-th 8-row tile row starting at row0, so that
                  // every rank gets the same mix of dense and empty screen regions).  Band-local row l <-> image row
                  // row0 + ((l >> 3) << tshift) + (l & 7).
};
// first image row of band tile row ty
DSS_HD int tile_row0(const TileGrid &g, int ty) { return g.row0 + (ty << g.tshift); }

// ---------------------------------------------------------------------------------------------
// Splat -> tile rectangle (band-local tile coordinates).  Image column c <-> NDC index S-1-c.
// The rectangle is exact: it is the set of tiles containing at least one pixel whose centre
// passes both axis tests |dx|<=rx and |dy|<=ry (the Q test can only remove pixels).
// ROLLED = true: the reference implementation (four rolled searches on every path); never instantiated in a kernel.
// ---------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
// (the empty asm keeps the optimiser from turning each search into an eightfold-unrolled batch evaluation)
#define DSS_KEEP_ROLLED(i) asm volatile("" : "+v"(i))
#else
#define DSS_KEEP_ROLLED(i) (void)0
#endif
// Tightens the index ranges [xlo, xhi], [ylo, yhi] of an S x S image from both ends with the exact per-pixel predicate
// |ndc(i) - centre| <= radius: each end moves inwards to the first index that passes, or past the other end (empty range).
// Exact for ANY starting range, however loose (splat_tile_rect hands over the one of ndc_index_range).
template <bool ROLLED = false>
DSS_HD void splat_tighten(float px, float py, float rx, float ry, int S, int &xlo, int &xhi, int &ylo, int &yhi)
{
    // tighten with the exact per-pixel predicate.  The searches take 1-3 steps (ndc_index_range leaves one pixel of slack per
    // side); as loops they must stay rolled and free of the IEEE divide of the non-power-of-two pixel map (unrolled eightfold
    // with the divide inlined they were 1100 instructions and 8.5k of the binning kernel's 30k cycles per wavefront).
    const NdcMap ndc(S);
#define DSS_TIGHTEN_LO(NDC_EXPR)                                                                \
    while (xlo <= xhi && fabsf(NDC_EXPR(xlo) - px) > rx) { ++xlo; DSS_KEEP_ROLLED(xlo); }       \
    while (ylo <= yhi && fabsf(NDC_EXPR(ylo) - py) > ry) { ++ylo; DSS_KEEP_ROLLED(ylo); }
#define DSS_TIGHTEN_HI(NDC_EXPR)                                                                \
    while (xhi >= xlo && fabsf(NDC_EXPR(xhi) - px) > rx) { --xhi; DSS_KEEP_ROLLED(xhi); }       \
    while (yhi >= ylo && fabsf(NDC_EXPR(yhi) - py) > ry) { --yhi; DSS_KEEP_ROLLED(yhi); }
    if (ndc.pow2) {  // uniform
        const float inv = ndc.invS;
#define DSS_NDC_POW2(i) (-1 + (2 * (i) + 1.0f) * inv)
        if (ROLLED) {
            DSS_TIGHTEN_LO(DSS_NDC_POW2)
            DSS_TIGHTEN_HI(DSS_NDC_POW2)
        } else {
            // The same searches in straight-line code: the first three steps of each are evaluated side by side (twelve
            // independent predicate evaluations instead of four dependent, divergent loops) and the step at which the loop
            // would have stopped -- index out of range, or predicate passed -- is selected; a search that needs a fourth step
            // continues in the loop itself.  (A candidate index may lie outside [0, S): it is only arithmetic, and the range
            // test in front of it in the selection discards it.)
#define DSS_FAILS(i, c, r) (fabsf(DSS_NDC_POW2(i) - (c)) > (r))
            const bool xl0 = DSS_FAILS(xlo, px, rx), xl1 = DSS_FAILS(xlo + 1, px, rx), xl2 = DSS_FAILS(xlo + 2, px, rx);
            const bool yl0 = DSS_FAILS(ylo, py, ry), yl1 = DSS_FAILS(ylo + 1, py, ry), yl2 = DSS_FAILS(ylo + 2, py, ry);
            const bool xh0 = DSS_FAILS(xhi, px, rx), xh1 = DSS_FAILS(xhi - 1, px, rx), xh2 = DSS_FAILS(xhi - 2, px, rx);
            const bool yh0 = DSS_FAILS(yhi, py, ry), yh1 = DSS_FAILS(yhi - 1, py, ry), yh2 = DSS_FAILS(yhi - 2, py, ry);
#undef DSS_FAILS
            const int kxl = (xlo > xhi || !xl0) ? 0 : (xlo + 1 > xhi || !xl1) ? 1 : (xlo + 2 > xhi || !xl2) ? 2 : 3;
            const int kyl = (ylo > yhi || !yl0) ? 0 : (ylo + 1 > yhi || !yl1) ? 1 : (ylo + 2 > yhi || !yl2) ? 2 : 3;
            xlo += kxl;
            ylo += kyl;
            if (kxl == 3 || kyl == 3) {   // (rare; a search that had stopped stops again at once)
                DSS_TIGHTEN_LO(DSS_NDC_POW2)
            }
            const int kxh = (xhi < xlo || !xh0) ? 0 : (xhi - 1 < xlo || !xh1) ? 1 : (xhi - 2 < xlo || !xh2) ? 2 : 3;
            const int kyh = (yhi < ylo || !yh0) ? 0 : (yhi - 1 < ylo || !yh1) ? 1 : (yhi - 2 < ylo || !yh2) ? 2 : 3;
            xhi -= kxh;
            yhi -= kyh;
            if (kxh == 3 || kyh == 3) {
                DSS_TIGHTEN_HI(DSS_NDC_POW2)
            }
        }
#undef DSS_NDC_POW2
    } else {
#define DSS_NDC_DIV(i) pix_to_ndc((i), S)
        DSS_TIGHTEN_LO(DSS_NDC_DIV)
        DSS_TIGHTEN_HI(DSS_NDC_DIV)
#undef DSS_NDC_DIV
    }
#undef DSS_TIGHTEN_LO
#undef DSS_TIGHTEN_HI
}

template <bool ROLLED = false>
DSS_HD bool splat_tile_rect(float px, float py, float pz, float rx, float ry, const TileGrid g, int &tx0, int &tx1, int &ty0,
                            int &ty1)
{
    if (pz < 0) return false;  // rasterize_points.cu:79-80
    int xlo, xhi, ylo, yhi;
    if (!ndc_index_range(px, rx, g.S, xlo, xhi)) return false;
    if (!ndc_index_range(py, ry, g.S, ylo, yhi)) return false;
    splat_tighten<ROLLED>(px, py, rx, ry, g.S, xlo, xhi, ylo, yhi);
    if (xlo > xhi || ylo > yhi) return false;
    const int c0 = g.S - 1 - xhi, c1 = g.S - 1 - xlo;
    int r0 = g.S - 1 - yhi, r1 = g.S - 1 - ylo;
    // band tile rows whose 8 image rows [R, R + 7], R = row0 + (ty << tshift), meet [r0, r1] (contiguous band, tshift = 3:
    // ty = (r - row0) / 8 as before; the last tile row of a band may be short: rows beyond g.rows are never stored)
    r0 = max(r0, g.row0);
    r1 = min(r1, tile_row0(g, g.tiles_y - 1) + (g.rows - 1 - (g.tiles_y - 1) * DSS_TILE));   // last image row of the band
    if (r0 > r1) return false;
    tx0 = c0 / DSS_TILE;
    tx1 = c1 / DSS_TILE;
    const int step = 1 << g.tshift;
    ty0 = (r0 - g.row0 - (DSS_TILE - 1) + step - 1) >> g.tshift;   // ceil((r0 - row0 - 7) / step), numerator + step - 1 >= 0
    ty0 = max(ty0, 0);
    ty1 = min((r1 - g.row0) >> g.tshift, g.tiles_y - 1);
    return ty0 <= ty1;
}

}  // namespace dss
