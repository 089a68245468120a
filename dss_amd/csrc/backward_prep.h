// List preparation of the render backward (raster_backward.hip), the rules its three generations share, stated once:
// the long-list sequence (visible_scan / median_hist / median_final / cell_hist), the two-launch sequence
// (backward_compact / median_visible / band_filter) and the fused form (fb_prep_segment / fb_median / the band filter inside
// render_backward_kernel).  The host still picks one of the three per call; what an entry is and what a kernel stores stay there.
//
// First part, plain C++ that the host compiler takes as well (tests/test_band_rows_cpu.py): the row maps of a band, the
// band's NDC edges and the reach test that drops a visible point from a rank's list.  That test is the one rule here whose
// drift loses gradient terms without a trace: too tight and a point the gather would have used is gone, too loose and only
// time is lost, which no value test sees.  Second part: the device bodies.
//
// WHO USES WHICH REACH (the callers choose the reach and handle n < 0; the test itself is `band_reached`):
//   band_filter_kernel   two-launch sequence, ONE filter in front of a gather that runs both halves of a task:
//                        max(rs[n], ry) -- the own box (blend half, |dy| <= ry) or the search window (occupancy half,
//                        d2 <= rs^2) may reach the band.  A point of no cloud (n < 0) is dropped.
//   cell_hist_kernel     long lists, the same single filter inside the cell sort: max(rs[n], ry).  n < 0 counts as cloud 0
//                        there (the kernel needs a cloud for the cell key and clamps before the filter); the code does not
//                        say why it keeps such a point where band_filter_kernel drops it.  The gather rejects it either way
//                        and visible_scan_kernel has stored its zeros (zero_all), so no output differs.
//   gather, BAND         one filter per half, each with the reach its half needs: ry alone before the blend half, rs[n]
//                        alone behind the wait for the medians.  n < 0 is dropped.
//   owner mode           (OwnArgs) the occupancy half of a point belongs to the rank that owns the image row of its CENTRE
//                        and sweeps the whole image there.  The two single filters switch to ry alone: the blend half
//                        needs the own box, and the owned centres are among the points whose box meets the band (the centre
//                        lies inside its box; a centre beyond the image, clamped to the first or last row, is no candidate of
//                        the surrogate).  The gather's second filter does not use the reach test at all then: it keeps
//                        band_owns_row(centre_image_row(py)), the rule the task itself applies.
//   cyclic               band_filter_kernel and cell_hist_kernel pass tshift > 3 at run time, the gather its template
//                        constant CYC (the host instantiates CYC exactly for tshift > 3).
#pragma once
#include "tile_rect.h"   // DSS_HD, min / max, pix_to_ndc, ndc_index_range

namespace dss {

// Band-local row <-> image row of a (possibly tile-row-cyclic) band, see TileGrid::tshift:
// image row of band row l = row0 + ((l >> 3) << tshift) + (l & 7); contiguous band: tshift = 3, i.e. row0 + l.
DSS_HD int band_image_row(int l, int row0, int tshift) { return row0 + ((l >> 3) << tshift) + (l & 7); }
// smallest band row whose image row is >= r (may equal `rows`: none)
DSS_HD int band_row_ceil(int r, int row0, int tshift)
{
    const int x = r - row0;
    if (x <= 0) return 0;
    const int q = x >> tshift, m = x & ((1 << tshift) - 1);
    return m < 8 ? 8 * q + m : 8 * (q + 1);
}
// largest band row whose image row is <= r (-1: none)
DSS_HD int band_row_floor(int r, int row0, int tshift)
{
    const int x = r - row0;
    if (x < 0) return -1;
    const int q = x >> tshift, m = x & ((1 << tshift) - 1);
    return 8 * q + min(m, 7);
}
// is image row r one of the band's rows?
DSS_HD bool band_owns_row(int r, int row0, int rows, int tshift)
{
    const int x = r - row0;
    if (x < 0) return false;
    const int m = x & ((1 << tshift) - 1);
    return m < 8 && 8 * (x >> tshift) + m < rows;
}
// image row of a point's centre (owner mode; any fixed partition of the axis does)
DSS_HD int centre_image_row(float py, int S)
{
    const float fy = (1.0f - py) * 0.5f * (float)S;
    return min(max((int)fy, 0), S - 1);
}

// NDC y extent of a band: image row r covers NDC index S - 1 - r.  For a tile-row-cyclic band the last band row's image row
// bounds the band from below and the rows between are checked by band_reached.
struct BandEdges {
    float lo;   // lower edge of the lowest pixel row
    float hi;   // upper edge of the highest one
};
DSS_HD BandEdges band_edges(int S, int row0, int rows, int tshift)
{
    const int last_row = band_image_row(rows - 1, row0, tshift);
    BandEdges e;
    e.lo = -1 + (2 * (S - 1 - last_row)) / (float)S;
    e.hi = -1 + (2 * (S - 1 - row0) + 2.0f) / (float)S;
    return e;
}
// Can a point at NDC y = py reach one of the band's rows within `reach`?  Conservative: never false when the centre of an
// owned pixel row lies within reach (the task evaluates the exact rows).  Cyclic band: some OWNED row must lie inside the
// conservative pixel range of ndc_index_range (one pixel of slack each side).
DSS_HD bool band_reached(float py, float reach, const BandEdges &e, bool cyclic, int S, int row0, int rows, int tshift)
{
    bool in_band = !(py + reach < e.lo || py - reach > e.hi);
    if (in_band && cyclic) {
        int ylo, yhi;
        in_band = ndc_index_range(py, reach, S, ylo, yhi) &&
                  band_row_ceil(S - 1 - yhi, row0, tshift) <= min(band_row_floor(S - 1 - ylo, row0, tshift), rows - 1);
    }
    return in_band;
}

// rank of the lower median among `total` sorted values (torch.median = lower median); 0 for none
DSS_HD uint32_t lower_median_rank(uint32_t total) { return total > 0 ? (total - 1) / 2 : 0; }

#if defined(__HIPCC__)
// ---- device bodies

// Lanes of the wavefront in front of this one whose predicate holds; `count`: all lanes whose predicate holds.
__device__ __forceinline__ uint32_t lane_rank(bool pred, uint32_t &count)
{
    const unsigned long long m = __ballot(pred);
    count = (uint32_t)__popcll(m);
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Zero gradient rows of point i: a point that is invisible, or dropped from a band's list, has a zero (partial) sum.
__device__ __forceinline__ void zero_pts_row(float *__restrict__ grad_pts, size_t i)
{
    grad_pts[3 * i] = 0.0f; grad_pts[3 * i + 1] = 0.0f; grad_pts[3 * i + 2] = 0.0f;
}
__device__ __forceinline__ void zero_feat_row(float *__restrict__ grad_feat, int C, size_t i)
{
    for (int ch = 0; ch < C; ++ch) grad_feat[i * C + ch] = 0.0f;
}
__device__ __forceinline__ void zero_grad_rows(float *__restrict__ grad_pts, float *__restrict__ grad_feat /* or NULL */, int C, size_t i)
{
    zero_pts_row(grad_pts, i);
    if (grad_feat) zero_feat_row(grad_feat, C, i);
}

// Ordered compaction of a segment by one workgroup of THREADS threads, PER entries per thread (entry u * THREADS + tid is
// bit u of `mask`): rank[u] = kept entries in front of (u, wave, lane) in that order, so the kept entries stay sorted by
// entry; returns their number.  s_w: PER * THREADS / 64 words.
template <int PER, int THREADS>
__device__ __forceinline__ uint32_t ordered_ranks(uint32_t mask, uint32_t (&rank)[PER], uint32_t *s_w)
{
    constexpr int WAVES = THREADS / 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        uint32_t cnt;
        rank[u] = lane_rank((mask >> u) & 1u, cnt);
        if (lane == 0) s_w[u * WAVES + wid] = cnt;
    }
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        uint32_t before = tot;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c = s_w[u * WAVES + w];
            if (w < wid) before += c;
            tot += c;
        }
        rank[u] += before;
    }
    return tot;
}

// Where the entries of the cloud that owns the points [lo, hi) sit inside a segment's compacted list (ids ascending, so they
// are one run): one step per entry of the thread -- s_rng[0] += kept entries in front of the run, s_rng[1] += entries of the
// run.  s_rng[0..1] are zeroed (and a barrier passed) before the first step; behind a barrier after the last they hold
// (first entry, count).  Returns whether the thread's entry belongs to the run.
__device__ __forceinline__ bool cloud_span_step(bool kept, int64_t i, int64_t lo, int64_t hi, uint32_t *s_rng)
{
    const bool mine = kept && i >= lo && i < hi;
    const unsigned long long mb = __ballot(kept && i < lo), mi = __ballot(mine);
    if ((threadIdx.x & 63) == 0) {
        if (mb) atomicAdd(&s_rng[0], (uint32_t)__popcll(mb));
        if (mi) atomicAdd(&s_rng[1], (uint32_t)__popcll(mi));
    }
    return mine;
}

// Wave-wide inclusive scan on the VALU (DPP row shifts + row broadcasts; `__shfl_up` would be six dependent
// ds_bpermute round trips).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u32_zero(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += dpp_u32_zero<0x111, 0xf>(v);  // row_shr:1
    v += dpp_u32_zero<0x112, 0xf>(v);  // row_shr:2
    v += dpp_u32_zero<0x114, 0xf>(v);  // row_shr:4
    v += dpp_u32_zero<0x118, 0xf>(v);  // row_shr:8  -> inclusive scan inside each row of 16
    v += dpp_u32_zero<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp_u32_zero<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}
// exclusive scan over the THREADS threads of a workgroup; total left in every thread.  s_w: THREADS / 64 words (any earlier
// use of them is over: the first barrier)
template <int THREADS>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_w, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t x = wave_incl_scan(v);
    __syncthreads();
    if (lane == 63) s_w[wid] = x;
    __syncthreads();
    uint32_t woff = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const uint32_t c = s_w[w];
        if (w < wid) woff += c;
        total += c;
    }
    return woff + x - v;
}

// Rank-k bin of a histogram held as NB consecutive bins per thread (counts h[], first bin of the thread `first_bin`) by a
// workgroup of THREADS threads; k_is_lower_median: k = the lower median's rank of all counts instead.  Uniform result.
// s: THREADS / 64 + 2 words, one more with COUNT (the kernels that do not ask for the count have no word for it).
struct RankBin {
    uint32_t bin, k;   // the bin that holds rank k, and the rank inside that bin
    uint32_t total;    // sum of all bins (bin and k mean nothing when it is 0)
    uint32_t count;    // COUNT: entries of the chosen bin
};
template <int THREADS, int NB, bool COUNT = false>
__device__ __forceinline__ RankBin rank_select(const uint32_t (&h)[NB], uint32_t first_bin, uint32_t k, bool k_is_lower_median,
                                               uint32_t *s)
{
    uint32_t *s_sel = s + THREADS / 64;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < NB; ++i) v += h[i];
    RankBin r;
    uint32_t excl = block_excl_scan<THREADS>(v, s, r.total);
    if (k_is_lower_median) k = lower_median_rank(r.total);
    if (r.total > 0 && k >= excl && k < excl + v) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (k >= excl && k < excl + h[i]) {
                s_sel[0] = first_bin + i;
                s_sel[1] = k - excl;
                if (COUNT) s_sel[2] = h[i];
            }
            excl += h[i];
        }
    }
    __syncthreads();
    r.bin = s_sel[0];
    r.k = s_sel[1];
    r.count = COUNT ? s_sel[2] : 0u;
    return r;
}
#endif  // __HIPCC__

}  // namespace dss
