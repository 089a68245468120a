// Counting sort by screen cell, stated once for the two places of the render that sort: the forward's cell-ordered binning
// (raster_forward.hip, above SORT_MIN_P splats) and the backward's ordering of the visible list (raster_backward.hip, above
// PREP_MAX_POINTS points).  The rule, without global atomics (they run at ~16 G/s on this part):
//   1. every workgroup of CELL_SORT_THREADS threads counts its entries' cells in LDS -> the row block_hist[block][cell];
//   2. an exclusive scan down every column -- over the blocks (backward), or over segments of blocks and then over the
//      segments (forward: 500+ blocks) -- leaves each block's first position within the cell, and the cell totals;
//   3. one workgroup scans the cell totals into cell_start and stores the sorted count;
//   4. every workgroup loads cell_start + its bases into LDS, ranks its entries again there and scatters them.
// The key only buys locality: no result depends on the order, so no GPU test fails when the rule is wrong -- the step just
// gets slower.  Hence the first part is plain C++ that the host compiler takes as well (tests/test_cell_sort_cpu.py pins the
// grid and the key against the two forms this header replaced); the second part holds the device bodies the kernels of both
// files wrap.  The per-entry loops (what an entry is, which entries get no cell, what the scatter stores) stay there.
#pragma once
#include "tile_rect.h"   // DSS_HD, min / max

#define CELL_SORT_MAX 16384           // cells of one grid at most: 64 KB of LDS counters
#define CELL_SORT_THREADS 1024        // workgroup of the histogram and scatter passes
#define CELL_SORT_NONE 0xffffffffu    // key of an entry that is left out of the sort

namespace dss {

struct CellGrid {
    int shift;     // cell side = 1 << shift pixels
    int cx, cy;    // cells per image row / column
    int total;     // N * cx * cy + extra_cells  (<= CELL_SORT_MAX: one LDS histogram)
};
// 32 x 32-pixel cells (16 measures the same, 64 is 4 % slower in the backward's gather), the side doubled until one LDS
// histogram holds the grid of all N cameras plus `extra_cells` cells behind them (forward: one, for the culled splats of a
// saved order; backward: none).  The extra cell moves the step: at exactly N * (S / 32)^2 = CELL_SORT_MAX -- one camera at
// 4096^2, 16 cameras at 1024^2 -- the backward keeps 32-pixel cells with 16384 counters, the forward goes to 64-pixel cells
// with 4097.  The two sorts never meet, so the grids need not agree; each side sizes its workspace with its own call.
DSS_HD CellGrid make_cell_grid(int N, int S, int extra_cells)
{
    CellGrid c;
    c.shift = 5;
    for (;;) {
        c.cx = ((S - 1) >> c.shift) + 1;
        c.cy = c.cx;
        c.total = N * c.cx * c.cy + extra_cells;
        if (c.total <= CELL_SORT_MAX || c.shift >= 14) break;
        ++c.shift;
    }
    return c;
}

// Key of the point (px, py) (NDC) of camera n: the cell of its pixel column / row.  Any monotone map of NDC does -- only
// neighbourhood matters --; this one falls with px and py and clamps to the image.  Always < N * cx * cy (the extra cells
// lie behind).  On the device a NaN coordinate converts to 0: cell column / row 0.
DSS_HD uint32_t screen_cell(float px, float py, int n, int S, const CellGrid &g)
{
    const float fx = (1.0f - px) * 0.5f * (float)S, fy = (1.0f - py) * 0.5f * (float)S;
    const int ix = min(max((int)fx, 0), S - 1) >> g.shift, iy = min(max((int)fy, 0), S - 1) >> g.shift;
    return (uint32_t)((n * g.cy + iy) * g.cx + ix);
}

#if defined(__HIPCC__)
// ---- device bodies (a workgroup of CELL_SORT_THREADS threads unless said otherwise; s_hist: `total` LDS counters)

// step 1, before the entries are counted
__device__ __forceinline__ void cell_hist_clear(uint32_t *s_hist, int total)
{
    for (int c = threadIdx.x; c < total; c += CELL_SORT_THREADS) s_hist[c] = 0u;
    __syncthreads();
}
// step 1, after: the workgroup's histogram -> its row of block_hist
__device__ __forceinline__ void cell_hist_store(const uint32_t *s_hist, int total, uint32_t *__restrict__ block_hist)
{
    __syncthreads();
    uint32_t *row = block_hist + (size_t)blockIdx.x * total;
    for (int c = threadIdx.x; c < total; c += CELL_SORT_THREADS) row[c] = s_hist[c];
}
// step 2, one thread per column c: rows[r][c] <- sum of rows[< r][c], eight independent loads in flight per trip (one at a
// time a walk over ~150 rows was 40 us of load latencies); returns the column's total
__device__ __forceinline__ uint32_t cell_column_scan(uint32_t *__restrict__ rows, uint32_t nrows, int total, int c)
{
    uint32_t run = 0, r = 0;
    for (; r + 8 <= nrows; r += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = rows[(size_t)(r + u) * total + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            rows[(size_t)(r + u) * total + c] = run;
            run += v[u];
        }
    }
    for (; r < nrows; ++r) {
        const uint32_t v = rows[(size_t)r * total + c];
        rows[(size_t)r * total + c] = run;
        run += v;
    }
    return run;
}
// step 3, ONE workgroup of 1024 threads: exclusive scan of the cell totals -> cell_start; the sorted count -> *sorted_count
__device__ __forceinline__ void cell_start_scan(const uint32_t *__restrict__ cell_total, uint32_t *__restrict__ cell_start,
                                                int total, uint32_t *__restrict__ sorted_count)
{
    __shared__ uint32_t s_part[1024];
    const int tid = threadIdx.x;
    const int per = (total + 1023) / 1024;
    const int b = tid * per, e = min(b + per, total);
    uint32_t sum = 0;
    for (int i = b; i < e; ++i) sum += cell_total[i];
    s_part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = tid >= o ? s_part[tid - o] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_part[tid] - sum;
    for (int i = b; i < e; ++i) {
        cell_start[i] = run;
        run += cell_total[i];
    }
    if (tid == 1023) *sorted_count = s_part[1023];
}
// step 4, before the entries are ranked: the workgroup's first position within every cell.  `block_row` is its row of
// block_hist after step 2; SEGMENTS: the scan had two levels and `seg_row` is the row of the workgroup's segment.
template <bool SEGMENTS>
__device__ __forceinline__ void cell_bases_load(uint32_t *s_hist, int total, const uint32_t *__restrict__ cell_start,
                                                const uint32_t *__restrict__ block_row,
                                                const uint32_t *__restrict__ seg_row = nullptr)
{
    for (int c = threadIdx.x; c < total; c += CELL_SORT_THREADS)
        s_hist[c] = SEGMENTS ? cell_start[c] + seg_row[c] + block_row[c] : cell_start[c] + block_row[c];
    __syncthreads();
}
#endif  // __HIPCC__

}  // namespace dss
