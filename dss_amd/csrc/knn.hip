// K-th nearest-neighbour squared distance on a uniform 3-D grid, gfx950.
//
// The source-space variance scale h of the EWA kernel is a kNN statistic
// (DSS/core/rasterizer.py:310-326 global, :366-388 per point):
//     sq_dist = knn(points, points, K=7)[:, :, 1:] ;  h_k = 0.5 * max(sq_dist)
// i.e. half the 7th-smallest squared distance from each point to the cloud INCLUDING itself.  The
// reference delegates the search to third-party CUDA (FRNN frnn_grid_points / pytorch3d knn_points);
// this is the "next" row of SURVEY 8f.  Exact search: counting-sort the points of every cloud into a
// res^3 grid, then one thread per point visits Chebyshev rings of cells until the K-th distance found
// is provably final (<= distance to the unvisited region).
//
// The kernels, and the chains of launches (host section below) that use them:
//   small build (build_grid: P <= KNN_SMALL_P, at most KNN_GRID_LDS clouds and KNN_SCAN1_BLOCKS scan blocks)
//       knn_bbox_partial (also zeroes the counts), knn_count_grid, knn_scan_single, knn_fill
//   eight-launch build (build_grid, otherwise)
//       memset of the counts, knn_init, knn_bbox, knn_grid, knn_count, knn_scan_local, knn_scan_add, knn_fill
//   skip structure of clustered clouds (build_skip_structure, P >= KNN_SKIP_MIN_P)
//       knn_dense_list, knn_subsort, knn_block_box
//   the two queries (query_plain, query_per_camera): K smallest squared distances in registers, IN CELL ORDER, so the
//   lanes of a wavefront walk the same few cells
//       knn_query        one thread per point
//       knn_query_coop   KNN_LPQ lanes per point
//   per-camera rows (dss_knn_kth_sqdist_view): knn_fill raises the "camera drops points" flags, the VIEW instantiations
//   of the two queries search among the kept points, knn_view_rows copies the row of a camera that drops nothing
//   statistics: cloud_mean (the global-h statistic), renderable_sum + renderable_mean (the same under depth culling)
//   another cloud's nearest point and the chamfer gradient (end of the file): nearest_query, chamfer_backward
// The rules that several of them share are device functions, each stated once: knn_box_reduce (box of a cloud),
// knn_make_grid (grid from a box), knn_cell_coords / knn_cell_of (cell of a position), wave_incl_scan / wave_xor_sum /
// block_excl_scan (scans and sums), KnnCamera (depth test of a camera), knn_insert (K-best list), knn_ring_bound /
// knn_search_done (when a ring search is final), knn_kth_of / knn_write_result (what a query reports).
#include "common.h"

namespace dss {

#define KNN_MAX_K 16
#define KNN_MAX_RES 128
#define KNN_SCAN_BLOCK 1024  // cells per workgroup of the two-level scan

struct KnnGrid {  // per cloud, device resident (8 floats)
    float minx, miny, minz, inv_cell, cell;
    int res;
    int pad0, pad1;
};

// Sum over the wavefront by xor butterfly, offsets 32 down to 1: every lane ends with the total.  (The float and double
// sums of the statistics are pinned to this order; common.h's wave_sum adds in another one.)
template <typename T>
__device__ __forceinline__ T wave_xor_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Inclusive scan over the wavefront: lane l ends with the sum of lanes 0..l.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// Box of the points f + i0, f + i0 + step, ... of a cloud (f, cnt), reduced over a 256-thread workgroup: registers ->
// wave (shuffles) -> workgroup (LDS).  Threads 0..5 return the workgroup's value d = threadIdx.x as an ordered int (0..2:
// min x y z, 3..5: max), +inf / -inf in that space when the workgroup saw no point; NaN positions are passed over.
__device__ __forceinline__ int knn_box_reduce(const float *__restrict__ pts, int64_t f, int64_t cnt, int64_t P, int64_t i0,
                                              int64_t step, int (&part)[4][6] /* LDS */)
{
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
    int hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    for (int64_t i = i0; i < cnt; i += step) {
        const int64_t p = f + i;
        if (p >= P) break;
        const float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
        if (!(x == x && y == y && z == z)) continue;
        const int ox = f2ord(x), oy = f2ord(y), oz = f2ord(z);
        lo[0] = min(lo[0], ox); lo[1] = min(lo[1], oy); lo[2] = min(lo[2], oz);
        hi[0] = max(hi[0], ox); hi[1] = max(hi[1], oy); hi[2] = max(hi[2], oz);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[d] = min(lo[d], __shfl_xor(lo[d], o));
            hi[d] = max(hi[d], __shfl_xor(hi[d], o));
        }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { part[wid][d] = lo[d]; part[wid][3 + d] = hi[d]; }
    }
    __syncthreads();
    int v = 0;
    if (threadIdx.x < 6) {
        const int d = threadIdx.x;
        v = part[0][d];
#pragma unroll
        for (int w = 1; w < 4; ++w) v = d < 3 ? min(v, part[w][d]) : max(v, part[w][d]);
    }
    return v;
}

// Bounding box per cloud.  Grid (G, N): workgroups of cloud n stride over its points and reduce them (knn_box_reduce) ->
// one atomic per bound and WORKGROUP.  (One atomic set per POINT, the first version, serialised P same-address atomics:
// 2.2 ms at 80k points.)
__global__ __launch_bounds__(256) void knn_bbox_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx,
                                                       const int64_t *__restrict__ num_pts, int N, int64_t P,
                                                       int *__restrict__ bbox /* (N,6) ordered ints */)
{
    __shared__ int part[4][6];
    const int n = blockIdx.y, d = threadIdx.x;
    const int v = knn_box_reduce(pts, first_idx[n], num_pts[n], P, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                                 (int64_t)gridDim.x * blockDim.x, part);
    if (d < 3 && v != 0x7fffffff) atomicMin(&bbox[6 * n + d], v);   // (an untouched value stays out of the atomics)
    if (d >= 3 && d < 6 && v != (int)0x80000000) atomicMax(&bbox[6 * n + d], v);
}

__global__ void knn_init_kernel(int N, int *__restrict__ bbox)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 6 * N) bbox[i] = (i % 6 < 3) ? 0x7fffffff : (int)0x80000000;  // +inf / -inf in ordered-int space
}

// Grid of a cloud from its box (six ordered ints: min x y z, max x y z) and its point count.
__device__ __forceinline__ KnnGrid knn_make_grid(const int (&box)[6], int64_t npts, int res_cap)
{
    KnnGrid g;
    const float x0 = ord2f(box[0]), y0 = ord2f(box[1]), z0 = ord2f(box[2]);
    const float x1 = ord2f(box[3]), y1 = ord2f(box[4]), z1 = ord2f(box[5]);
    const float ext = fmaxf(fmaxf(x1 - x0, y1 - y0), fmaxf(z1 - z0, 1e-12f));
    // surface-like clouds occupy ~3 res^2 cells: aim at ~8 points per occupied cell
    int res = (int)ceilf(sqrtf((float)npts / 24.0f));
    res = max(1, min(res_cap, res));  // res_cap: the resolution the workspace was sized for (knn_res_cap)
    g.minx = x0; g.miny = y0; g.minz = z0;
    g.cell = ext / (float)res * 1.0001f;
    g.inv_cell = 1.0f / g.cell;
    g.res = res;
    g.pad0 = g.pad1 = 0;
    return g;
}

__global__ void knn_grid_kernel(const int *__restrict__ bbox, const int64_t *__restrict__ num_pts, int N, int res_cap,
                                KnnGrid *__restrict__ grids)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int box[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) box[d] = bbox[6 * n + d];
    grids[n] = knn_make_grid(box, num_pts[n], res_cap);
}

__device__ __forceinline__ int cell_coord(float v, float mn, float inv_cell, int res)
{
    const int c = (int)floorf((v - mn) * inv_cell);
    return min(max(c, 0), res - 1);
}
// Cell of a position in a cloud's grid: its three coordinates, and its linear index (cells consecutive along x are
// consecutive in memory).
// (returned by value: coordinates handed back through references stay memory until the call is inlined, and the ring
// walk's tests on them compile to branches where they were mask arithmetic -- 1 to 3 % of a one-thread query call)
__device__ __forceinline__ int3 knn_cell_coords(const KnnGrid &g, float x, float y, float z)
{
    return make_int3(cell_coord(x, g.minx, g.inv_cell, g.res), cell_coord(y, g.miny, g.inv_cell, g.res),
                     cell_coord(z, g.minz, g.inv_cell, g.res));
}
__device__ __forceinline__ int knn_cell_index(const KnnGrid &g, int cx, int cy, int cz) { return (cz * g.res + cy) * g.res + cx; }
__device__ __forceinline__ int knn_cell_of(const KnnGrid &g, float x, float y, float z)
{
    const int3 c = knn_cell_coords(g, x, y, z);
    return knn_cell_index(g, c.x, c.y, c.z);
}

__global__ __launch_bounds__(256) void knn_count_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx,
                                                        const int64_t *__restrict__ num_pts, int N, int64_t P,
                                                        const KnnGrid *__restrict__ grids, size_t stride,
                                                        uint32_t *__restrict__ counts, int32_t *__restrict__ cell_of,
                                                        uint32_t *__restrict__ rank_of /* the point's arrival number in its cell */)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int n = find_cloud(p, first_idx, num_pts, N);
    if (n < 0) { cell_of[p] = -1; return; }
    const KnnGrid g = grids[n];
    const int c = knn_cell_of(g, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]);
    cell_of[p] = c;
    // the counting atomic's return value is the point's slot inside the cell: the fill pass needs no second atomic (on a
    // clustered cloud both passes are bound by the fullest cell: 3,900 same-address atomics, 86 us each way)
    rank_of[p] = atomicAdd(&counts[(size_t)n * stride + c], 1u);
}

// Two-level exclusive scan of the cell counts.  Grid (blocks, N); block b of cloud n owns cells [1024 b, 1024 b + 1024).
// Pass 1: local exclusive scan -> offsets, block total -> blk_tot.  Pass 2: every block sums the totals of the blocks
// before it (at most 2048 values) and adds that prefix; the block holding the last cell also writes the end sentinel.
// (The first version scanned all res^3 cells with ONE workgroup per cloud: 288 us at res = 64.)
// Exclusive scan over a workgroup of WAVES wavefronts (one barrier); `total` = the sum over the workgroup.
template <int WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *wave_tot /* LDS [WAVES] */, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63) wave_tot[wid] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t t = wave_tot[w];
        before += (w < wid) ? t : 0u;
        total += t;
    }
    return before + incl - v;
}

__global__ __launch_bounds__(256) void knn_scan_local_kernel(const uint32_t *__restrict__ counts,
                                                             const KnnGrid *__restrict__ grids, size_t stride, int nblk_max,
                                                             uint32_t *__restrict__ offsets, uint32_t *__restrict__ blk_tot)
{
    __shared__ uint32_t wave_tot[4];
    const int n = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const int res = grids[n].res;
    const int cells = res * res * res;
    if (b * KNN_SCAN_BLOCK >= cells) return;
    const size_t base = (size_t)n * stride;
    const int c0 = b * KNN_SCAN_BLOCK + 4 * tid;
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (c0 + i < cells) ? counts[base + c0 + i] : 0u;
    uint32_t total;
    uint32_t run = block_excl_scan<4>(v[0] + v[1] + v[2] + v[3], wave_tot, total);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (c0 + i < cells) offsets[base + c0 + i] = run;
        run += v[i];
    }
    if (tid == 0) blk_tot[(size_t)n * nblk_max + b] = total;
}

__global__ __launch_bounds__(256) void knn_scan_add_kernel(const KnnGrid *__restrict__ grids, size_t stride, int nblk_max,
                                                           const uint32_t *__restrict__ blk_tot, uint32_t *__restrict__ offsets,
                                                           uint32_t *__restrict__ cursor)
{
    __shared__ uint32_t wave_tot[4];
    const int n = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const int res = grids[n].res;
    const int cells = res * res * res;
    if (b * KNN_SCAN_BLOCK >= cells) return;
    const size_t base = (size_t)n * stride;
    uint32_t part = 0;
    for (int i = tid; i < b; i += 256) part += blk_tot[(size_t)n * nblk_max + i];
    uint32_t prefix;
    block_excl_scan<4>(part, wave_tot, prefix);  // only the total is needed: blocks before b
    const int c0 = b * KNN_SCAN_BLOCK + 4 * tid;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (c0 + i < cells) {
            const uint32_t o = offsets[base + c0 + i] + prefix;
            offsets[base + c0 + i] = o;
            cursor[base + c0 + i] = o;
        }
    if (tid == 0 && (b + 1) * KNN_SCAN_BLOCK >= cells) offsets[base + cells] = prefix + blk_tot[(size_t)n * nblk_max + b];
}

// Per-camera depth culling inside the search (dss_knn_kth_sqdist_view): the reference runs its neighbour search AFTER
// filter_renderable has dropped, per camera, the points outside [znear, zfar] (rasterizer.py:599, 183-217, 310-326) -- a point's
// neighbours are then the ones the SAME camera keeps.  mode 1: one cloud shared by the cameras, blockIdx.y = camera, results at
// kth_sqdist[camera * P + p]; mode 2: cloud n belongs to camera n.  A query point its camera drops gets 0 (never read).
struct KnnView {
    const float *V;        // (cameras, 4, 4) world -> view, row-vector convention
    const float *znear, *zfar;
    int mode;              // 0: off
    uint32_t *culls;       // (cameras) != 0: the camera drops at least one point of its cloud (written by knn_fill_kernel)
    int n_cams;
};
// What the depth test needs of a camera: the depth column of its view matrix and its two planes.  kept() is the test of
// setup_point_compute, same expression.
struct KnnCamera {
    float v2, v6, v10, v14, zn, zf;
    __device__ __forceinline__ static KnnCamera load(const float *V, const float *znear, const float *zfar, int cam)
    {
        const float *vm = V + 16 * cam;
        return {vm[2], vm[6], vm[10], vm[14], znear[cam], zfar[cam]};
    }
    __device__ __forceinline__ float depth(float x, float y, float z) const { return x * v2 + y * v6 + z * v10 + 1.0f * v14; }
    __device__ __forceinline__ bool kept(float x, float y, float z) const
    {
        const float zview = depth(x, y, z);
        return (zview >= zn) && (zview <= zf);
    }
};
// The unmasked search of the whole cloud runs FIRST (one launch: statistic and K-th distance of every point); a camera's
// masked search is only needed for a query that has a dropped point among the neighbours that count, and a dropped point
// lies on the far side of one of the camera's two depth planes: the distance from a KEPT query to it is at least the
// query's distance to that plane.  So whenever both planes are farther from the query than rho -- the K-th distance of the
// unmasked search, or the search radius r if that is smaller (neighbours beyond r do not count) -- the camera's result is
// the unmasked one and is copied.  Likewise for a camera that drops nothing at all.  (With the near plane where the
// reference's data sets put it, znear = 0.1, no camera drops anything: one search, N copies.  With znear = 1.0 cutting
// through the cloud, only the queries within their neighbourhood's reach of the cut search again: 8 cameras x 99,790
// points of the trained cloud of tools/clustered_timing.py took 1.26 ms as eight masked searches.)
// Exactness: every dropped point is farther than rho; with rho = the K-th distance the K nearest are all kept, so the
// masked list is the unmasked list; with rho = r < the K-th distance, the entries within r are the same in both lists and
// the others do not count.  The margin allows for the rounding of the view depth (1e-5 (1 + |z|)) and for a view matrix
// whose depth axis is not a unit vector.  plain_dk = inf (fewer than K points in the cloud) never takes the shortcut.
__device__ __forceinline__ bool knn_view_shortcut(uint32_t camera_drops, float x, float y, float z, const KnnCamera &c,
                                                  float plain_dk, float r2)
{
    if (camera_drops == 0u) return true;
    const float zview = c.depth(x, y, z);
    const float margin = fminf(zview - c.zn, c.zf - zview) - 1e-5f * (1.0f + fabsf(zview));
    const float rho2 = r2 > 0.0f ? fminf(plain_dk, r2) : plain_dk;
    return margin > 0.0f && margin * margin > rho2 * (c.v2 * c.v2 + c.v6 * c.v6 + c.v10 * c.v10) * 1.0002f;
}
// mode 1 of dss_knn_kth_sqdist_view (one cloud, several cameras): the row of a camera that drops nothing is the unmasked search
// itself -- a coalesced copy; the query launches skip such cameras
__global__ __launch_bounds__(256) void knn_view_rows_kernel(float *__restrict__ kth, const float *__restrict__ plain, int64_t P,
                                                            const uint32_t *__restrict__ culls)
{
    const int cam = blockIdx.y;
    if (culls[cam] != 0u) return;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    float *row = kth + (size_t)cam * (size_t)P;
    if (i + 3 < P && ((((uintptr_t)row) | ((uintptr_t)plain)) & 15u) == 0) {
        reinterpret_cast<float4 *>(row)[i >> 2] = reinterpret_cast<const float4 *>(plain)[i >> 2];
    } else {
        for (int64_t j = i; j < min(i + 4, P); ++j) row[j] = plain[j];
    }
}

__global__ __launch_bounds__(256) void knn_fill_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx,
                                                       const int64_t *__restrict__ num_pts, int N, int64_t P,
                                                       const int32_t *__restrict__ cell_of, size_t stride,
                                                       uint32_t *__restrict__ cursor,
                                                       float4 *__restrict__ sorted /* (P) xyz + id, grouped by cell */,
                                                       const KnnView view = KnnView(),
                                                       const uint32_t *__restrict__ rank_of = nullptr /* given: `cursor` = the cell offsets, read only */)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int c = cell_of[p];
    if (c < 0) return;
    const int n = find_cloud(p, first_idx, num_pts, N);
    const float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
    const uint32_t pos = rank_of ? cursor[(size_t)n * stride + c] + rank_of[p] : atomicAdd(&cursor[(size_t)n * stride + c], 1u);
    sorted[first_idx[n] + pos] = make_float4(x, y, z, __int_as_float((int)p));
    if (view.mode != 0) {
        // which cameras drop a point of their cloud (dss_knn_kth_sqdist_view): one atomic per wavefront and camera that does
        const int c0 = view.mode == 1 ? 0 : n, c1 = view.mode == 1 ? view.n_cams : n + 1;
        for (int cam = c0; cam < c1; ++cam) {
            const bool drop = !KnnCamera::load(view.V, view.znear, view.zfar, cam).kept(x, y, z);
            unsigned long long m = __ballot(drop);
            // (one atomic per wavefront and camera, and none once the flag is seen up: 12,000 atomics on eight words took 100 us
            // at 8 x 100k.)  mode 2: a wavefront that straddles a cloud boundary holds lanes of different cameras -- one leader
            // per distinct camera among the dropping lanes, or the later cloud's flag is lost when all its dropped points sit in
            // such a wavefront.  mode 1: every lane has the same camera, one trip.
            while (m != 0ull) {   // (wave-uniform)
                const int leader = __builtin_ctzll(m);
                const int lcam = __shfl(cam, leader);
                if ((threadIdx.x & 63) == leader &&
                    __hip_atomic_load(&view.culls[lcam], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
                    atomicOr(&view.culls[lcam], 1u);
                m &= ~__ballot(drop && cam == lcam);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Clustered clouds.  The grid is uniform, sized for ~8 points per occupied cell of an evenly sampled surface.  The model of
// the reference's training loop does not stay that way: after ~900 iterations at BASELINE configs[2] a few outliers have
// stretched the bounding box to +-2 while nine tenths of the points sit within 0.55 of the origin -- a typical point shares
// its cell with 650 others (3,900 in the fullest cell), every query scans ~4,000 candidates instead of ~200, and the two
// searches of an iteration go from 0.13 / 0.16 ms to 1.7 / 2.3 ms (profiles/r6_b_train_mvr_ref_kernel_stats.csv, before this).  No
// single cell size serves a cloud whose neighbour distances span two orders of magnitude.  So, from KNN_SKIP_MIN_P points
// on, the cell-sorted array gets a skip structure:
//   * knn_dense_list_kernel lists the DENSE cells (more than KNN_DENSE_CELL points) and counts the points they hold;
//     knn_subsort_kernel orders the points of each along a Morton curve of their position inside the cell, so that
//     consecutive slots are close in space, and raises `dense_flag` when those cells hold a real share of the cloud;
//   * knn_block_box_kernel records the bounding box of every KNN_BLOCK consecutive slots;
//   * a query (both kernels) first looks at its own sorted neighbourhood (own cell dense: the KNN_SEED slots around the
//     query's slot) -- which gives a K-th distance close to the final one at once -- and then walks long candidate runs
//     block by block, skipping every block whose box lies farther than the current K-th distance.  The cooperative kernel
//     tests 32 boxes per trip (two per lane) and reads up to four surviving blocks together; clouds with `dense_flag` up go
//     to it at every size (a second launch next to the one-thread kernel's where that one is the choice for even clouds:
//     each leaves at once when the cloud is not its kind).
// Same candidates rule, same (distance, id) order: results are identical; only points that cannot enter the list are skipped.
// On the trained cloud: 3,999 -> 200 candidates + 250 box tests per query.  A cloud without dense cells pays four launches
// that find nothing to do (~13 us at 100k-200k points; `dense_flag` stays 0, the boxes are neither built nor read and the
// queries run as before).
// ---------------------------------------------------------------------------------------------------------------
#define KNN_SKIP_MIN_P 65536     // per call: below, the grid build is a chain of launch latencies and clouds are small
#define KNN_DENSE 64             // slots in a candidate run (and points in the query's own cell, for the seed) from which the blocks are walked
#define KNN_DENSE_CELL 64        // points in a cell from which it is listed and sub-sorted
#define KNN_DENSE_SHARE 8        // `dense_flag` goes up when at least 1 / KNN_DENSE_SHARE of the points live in such cells (a 1M-point
                                 // evenly sampled cloud at the resolution cap has a few of them: the cooperative walk it would
                                 // select is 2.5x slower there than the one-thread kernel, 2.21 against 0.88 ms for K = 12 lists)
#define KNN_BLOCK 16             // slots per box
#define KNN_SEED 16              // slots on either side of the query's own slot looked at first
#define KNN_SUBSORT_MAX 4096     // largest cell that is sub-sorted (larger ones stay in arrival order: correct, loose boxes)
#define KNN_SUBSORT_WGS 1024     // workgroups of the (persistent) sub-sort launch
#define KNN_SUBSORT_THREADS 1024  // (the launch lasts as long as its largest cell: ~80 bitonic stages of 4096 keys)

__device__ __forceinline__ uint32_t knn_spread5(uint32_t v)   // bit i of v (i < 5) -> bit 3 i
{
    return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6) | ((v & 16u) << 8);
}

// Dense cells of all clouds -> list[] (cloud, cell), *n_list, and the number of points they hold.
// One thread per cell, one atomic per wavefront that found any.
__global__ __launch_bounds__(256) void knn_dense_list_kernel(const KnnGrid *__restrict__ grids, size_t stride,
                                                             const uint32_t *__restrict__ offsets, uint2 *__restrict__ list,
                                                             uint32_t *__restrict__ n_list, uint32_t *__restrict__ n_dense_pts)
{
    const int n = blockIdx.y;
    const int res = grids[n].res, cells = res * res * res;
    const int c = blockIdx.x * 256 + threadIdx.x;
    const uint32_t *off = offsets + (size_t)n * stride;
    const uint32_t cnt = c < cells ? off[c + 1] - off[c] : 0u;
    const bool dense = cnt > (uint32_t)KNN_DENSE_CELL;
    const unsigned long long m = __ballot(dense);
    if (m == 0ull) return;
    const int lane = threadIdx.x & 63, leader = __builtin_ctzll(m);
    const uint32_t pts_here = wave_xor_sum(dense ? cnt : 0u);
    uint32_t base = 0;
    if (lane == leader) {
        base = atomicAdd(n_list, (uint32_t)__popcll(m));
        atomicAdd(n_dense_pts, pts_here);
    }
    base = (uint32_t)__shfl((int)base, leader);
    if (dense) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = make_uint2((uint32_t)n, (uint32_t)c);
}

// Persistent grid over the list: one workgroup sorts one dense cell at a time in LDS -- keys = (15-bit Morton code of the
// position inside the cell) << 12 | local slot, bitonic network over the next power of two; the points travel through
// registers (read in sorted order, barrier, written back in place).
__global__ __launch_bounds__(KNN_SUBSORT_THREADS) void knn_subsort_kernel(const KnnGrid *__restrict__ grids, size_t stride,
                                                          const uint32_t *__restrict__ offsets,
                                                          const int64_t *__restrict__ first_idx, float4 *__restrict__ sorted,
                                                          const uint2 *__restrict__ list, const uint32_t *__restrict__ n_list,
                                                          const uint32_t *__restrict__ n_dense_pts, int64_t P,
                                                          uint32_t *__restrict__ dense_flag)
{
    __shared__ uint32_t s_key[KNN_SUBSORT_MAX];
    const int tid = threadIdx.x;
    const uint32_t total = *n_list;
    // the later launches walk the blocks only if the dense cells hold a real share of the points (KNN_DENSE_SHARE)
    if (blockIdx.x == 0 && tid == 0) *dense_flag = (unsigned long long)*n_dense_pts * KNN_DENSE_SHARE >= (unsigned long long)P ? 1u : 0u;
    for (uint32_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint2 e = list[it];
        const int n = (int)e.x, cell = (int)e.y;
        const KnnGrid g = grids[n];
        const uint32_t *off = offsets + (size_t)n * stride;
        const int64_t f0 = first_idx[n];
        const uint32_t s = off[cell], cnt = off[cell + 1] - s;
        if (cnt > (uint32_t)KNN_SUBSORT_MAX) continue;   // (workgroup-uniform)
        uint32_t m = 128;
        while (m < cnt) m <<= 1;
        const int cx = cell % g.res, cy = (cell / g.res) % g.res, cz = cell / (g.res * g.res);
        const float bx = g.minx + (float)cx * g.cell, by = g.miny + (float)cy * g.cell, bz = g.minz + (float)cz * g.cell;
        for (uint32_t i = tid; i < m; i += KNN_SUBSORT_THREADS) {
            uint32_t key = 0xffffffffu;
            if (i < cnt) {
                const float4 q = sorted[f0 + s + i];
                const uint32_t ux = (uint32_t)min(31, max(0, (int)((q.x - bx) * g.inv_cell * 32.0f)));
                const uint32_t uy = (uint32_t)min(31, max(0, (int)((q.y - by) * g.inv_cell * 32.0f)));
                const uint32_t uz = (uint32_t)min(31, max(0, (int)((q.z - bz) * g.inv_cell * 32.0f)));
                key = ((knn_spread5(ux) | (knn_spread5(uy) << 1) | (knn_spread5(uz) << 2)) << 12) | i;
            }
            s_key[i] = key;
        }
        __syncthreads();
        for (uint32_t k = 2; k <= m; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < (m >> 1); t += KNN_SUBSORT_THREADS) {
                    const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;   // the pair (lo, lo ^ j)
                    const uint32_t a = s_key[lo], b = s_key[hi];
                    const bool up = (lo & k) == 0;
                    if ((a > b) == up) { s_key[lo] = b; s_key[hi] = a; }
                }
                __syncthreads();
            }
        float4 hold[KNN_SUBSORT_MAX / KNN_SUBSORT_THREADS];
#pragma unroll
        for (int u = 0; u < KNN_SUBSORT_MAX / KNN_SUBSORT_THREADS; ++u) {
            const uint32_t i = (uint32_t)u * KNN_SUBSORT_THREADS + tid;
            if (i < cnt) hold[u] = sorted[f0 + s + (s_key[i] & 0xfffu)];
        }
        __builtin_amdgcn_s_waitcnt(0);   // every read of the cell's slots has returned ...
        __syncthreads();                 // ... in every wavefront, before the first slot is overwritten
#pragma unroll
        for (int u = 0; u < KNN_SUBSORT_MAX / KNN_SUBSORT_THREADS; ++u) {
            const uint32_t i = (uint32_t)u * KNN_SUBSORT_THREADS + tid;
            if (i < cnt) sorted[f0 + s + i] = hold[u];
        }
        __syncthreads();   // (s_key is rewritten by the next cell)
    }
}

// boxes[2 b], boxes[2 b + 1] = min / max corner of the packed slots [16 b, 16 b + 16) of the cell-sorted array.  Slots that
// belong to no cloud hold stale bytes: a box can only grow by them (NaN is ignored by fminf / fmaxf), never lose a point.
__global__ __launch_bounds__(256) void knn_block_box_kernel(const float4 *__restrict__ sorted, int64_t P,
                                                            const uint32_t *__restrict__ dense_flag, float4 *__restrict__ boxes)
{
    if (*dense_flag == 0u) return;
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b * KNN_BLOCK >= P) return;
    float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
#pragma unroll
    for (int i = 0; i < KNN_BLOCK; ++i) {
        const int64_t j = b * KNN_BLOCK + i;
        if (j < P) {
            const float4 q = sorted[j];
            lo[0] = fminf(lo[0], q.x); lo[1] = fminf(lo[1], q.y); lo[2] = fminf(lo[2], q.z);
            hi[0] = fmaxf(hi[0], q.x); hi[1] = fmaxf(hi[1], q.y); hi[2] = fmaxf(hi[2], q.z);
        }
    }
    boxes[2 * b] = make_float4(lo[0], lo[1], lo[2], 0.f);
    boxes[2 * b + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

// ---------------------------------------------------------------------------------------------------------------
// Small inputs (P <= KNN_SMALL_P): the grid build is a chain of launch latencies (ten launches, ~45 us at 32k points for
// a few us of work).  Three of them disappear here: [bbox partials + zeroed counts] -> [grid + count] -> [scan, one
// launch] -> [fill] instead of memset, init, bbox, grid, count, scan x 2, fill.  (A whole-build-in-one-workgroup kernel was
// tried first: 180 us -- 32 points per thread through dependent load -> returning atomic -> store chains on ONE CU.)
// ---------------------------------------------------------------------------------------------------------------
#define KNN_SMALL_P 131072
#define KNN_BB_WGS 32           // bounding-box workgroups per cloud
// grid (KNN_BB_WGS + zero workgroups, N): the first KNN_BB_WGS workgroups of cloud n reduce their share of its points to
// one partial box each (plain stores: no init, no atomics); the others zero the cell counts of cloud n
__global__ __launch_bounds__(256) void knn_bbox_partial_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx,
                                                               const int64_t *__restrict__ num_pts, int64_t P,
                                                               int *__restrict__ partial /* (N, KNN_BB_WGS, 6) */,
                                                               uint32_t *__restrict__ counts, size_t stride)
{
    const int n = blockIdx.y;
    if (blockIdx.x >= KNN_BB_WGS) {
        const size_t zw = gridDim.x - KNN_BB_WGS;
        uint32_t *c = counts + (size_t)n * stride;
        for (size_t i = (size_t)(blockIdx.x - KNN_BB_WGS) * 256 + threadIdx.x; i < stride; i += zw * 256) c[i] = 0u;
        return;
    }
    __shared__ int part[4][6];
    const int v = knn_box_reduce(pts, first_idx[n], num_pts[n], P, (int64_t)blockIdx.x * 256 + threadIdx.x,
                                 (int64_t)KNN_BB_WGS * 256, part);
    if (threadIdx.x < 6) partial[((size_t)n * KNN_BB_WGS + blockIdx.x) * 6 + threadIdx.x] = v;
}

// grid parameters of cloud n from the partial boxes, reduced over the lanes of a wavefront
__device__ __forceinline__ KnnGrid knn_grid_from_partials(const int *__restrict__ partial, int n, int64_t npts, int res_cap, int lane)
{
    int v[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        v[d] = lane < KNN_BB_WGS ? partial[((size_t)n * KNN_BB_WGS + lane) * 6 + d] : (d < 3 ? 0x7fffffff : (int)0x80000000);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int t = __shfl_xor(v[d], o);
            v[d] = d < 3 ? min(v[d], t) : max(v[d], t);
        }
    }
    return knn_make_grid(v, npts, res_cap);
}

// count with the grid derived in place: one workgroup handles 256 consecutive packed points, its first wavefront reduces
// the partial boxes of the (at most KNN_GRID_LDS) clouds it touches into LDS; workgroup 0 also publishes grids[] for the
// later launches.  Clouds beyond KNN_GRID_LDS fall back to the separate grid kernel (host side).
#define KNN_GRID_LDS 16
__global__ __launch_bounds__(256) void knn_count_grid_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx,
                                                             const int64_t *__restrict__ num_pts, int N, int64_t P,
                                                             const int *__restrict__ partial, int res_cap,
                                                             KnnGrid *__restrict__ grids, size_t stride,
                                                             uint32_t *__restrict__ counts, int32_t *__restrict__ cell_of)
{
    __shared__ KnnGrid s_g[KNN_GRID_LDS];
    if (threadIdx.x < 64) {
        for (int n = 0; n < N; ++n) {
            const KnnGrid g = knn_grid_from_partials(partial, n, num_pts[n], res_cap, threadIdx.x);
            if (threadIdx.x == 0) {
                s_g[n] = g;
                if (blockIdx.x == 0) grids[n] = g;
            }
        }
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int n = find_cloud(p, first_idx, num_pts, N);
    if (n < 0) { cell_of[p] = -1; return; }
    const KnnGrid g = s_g[n];
    const int c = knn_cell_of(g, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]);
    cell_of[p] = c;
    atomicAdd(&counts[(size_t)n * stride + c], 1u);
}

// exclusive scan of the cell counts in ONE launch (at most KNN_SCAN1_BLOCKS blocks of 1024 cells per cloud): block b first
// sums the counts of all the cells in front of it (coalesced, eight independent loads in flight per thread: with 256
// threads and one load at a time the last block of 50 took 28 us), then scans its own 1024 cells, one per thread
#define KNN_SCAN1_BLOCKS 160
__global__ __launch_bounds__(1024) void knn_scan_single_kernel(const uint32_t *__restrict__ counts,
                                                               const KnnGrid *__restrict__ grids, size_t stride,
                                                               uint32_t *__restrict__ offsets, uint32_t *__restrict__ cursor)
{
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t wave_pre[16];
    const int n = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int res = grids[n].res;
    const int cells = res * res * res;
    if (b * KNN_SCAN_BLOCK >= cells) return;
    const uint32_t *c = counts + (size_t)n * stride;
    const int lim = b * KNN_SCAN_BLOCK;
    uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0, p4 = 0, p5 = 0, p6 = 0, p7 = 0;
    int i = tid;
    for (; i + 7 * 1024 < lim; i += 8 * 1024) {
        p0 += c[i]; p1 += c[i + 1024]; p2 += c[i + 2048]; p3 += c[i + 3072];
        p4 += c[i + 4096]; p5 += c[i + 5120]; p6 += c[i + 6144]; p7 += c[i + 7168];
    }
    for (; i < lim; i += 1024) p0 += c[i];
    const uint32_t part = wave_xor_sum(((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)));
    const int c0 = lim + tid;
    const uint32_t v = c0 < cells ? c[c0] : 0u;
    if (lane == 0) wave_pre[wid] = part;   // (published by the barrier of the scan)
    uint32_t total, prefix = 0;
    const uint32_t own = block_excl_scan<16>(v, wave_tot, total);
#pragma unroll
    for (int w = 0; w < 16; ++w) prefix += wave_pre[w];
    const uint32_t run = prefix + own;
    if (c0 < cells) {
        offsets[(size_t)n * stride + c0] = run;
        cursor[(size_t)n * stride + c0] = run;
    }
    if (tid == 0 && (b + 1) * KNN_SCAN_BLOCK >= cells) offsets[(size_t)n * stride + cells] = prefix + total;
}

// ---------------------------------------------------------------------------------------------------------------
// What the two query kernels share.  `best` is a query's ascending list of K squared distances, `bid` the ids that go
// with them (FULL only), padded with (inf, 0x7fffffff); kk = min(K asked for, points in the cloud) entries count.
// The lists stay in registers only while every entry that feeds a select is a VALUE, which the empty
// `asm volatile("" : "+v"(x))` below makes it: left alone, the compiler rewrites select(c, a[i], a[j]) as a LOAD from
// select(c, &a[i], &a[j]), which pins the array in scratch memory (or LDS) and puts loads and stores into the loops.
// ---------------------------------------------------------------------------------------------------------------
// (distance, id) total order; ids are unique within a cloud, the padding entries (inf, 0x7fffffff) compare equal
// (bitwise | and &: the short-circuit forms compile to two nested exec-mask branches per comparison)
__device__ __forceinline__ bool knn_less(float da, int ia, float db, int ib) { return (da < db) | ((da == db) & (ia < ib)); }

// One candidate: keep the K best in (distance, id) order (FULL: deterministic lists whatever the cell order) or by
// distance (K-th only; `id` is not read).
template <int K, bool FULL>
__device__ __forceinline__ void knn_insert(float (&best)[K], int (&bid)[FULL ? K : 1], float d2, int id)
{
    if (FULL) {
        if (knn_less(d2, id, best[K - 1], bid[FULL ? K - 1 : 0])) {
            bool lt[K];
#pragma unroll
            for (int k = 0; k < K; ++k) lt[k] = knn_less(d2, id, best[k], bid[FULL ? k : 0]);
#pragma unroll
            for (int k = K - 1; k >= 1; --k) {
                float pb = best[k - 1];
                int pi = bid[FULL ? k - 1 : 0];
                asm volatile("" : "+v"(pb), "+v"(pi));   // (values, see above)
                best[k] = lt[k - 1] ? pb : (lt[k] ? d2 : best[k]);
                bid[FULL ? k : 0] = lt[k - 1] ? pi : (lt[k] ? id : bid[FULL ? k : 0]);
            }
            best[0] = lt[0] ? d2 : best[0];
            bid[0] = lt[0] ? id : bid[0];
        }
    } else if (d2 < best[K - 1]) {
#pragma unroll
        for (int k = K - 1; k >= 1; --k) {
            const bool sh = d2 < best[k - 1];
            best[k] = sh ? best[k - 1] : (d2 < best[k] ? d2 : best[k]);
        }
        best[0] = d2 < best[0] ? d2 : best[0];
    }
}

// Distance from the query (qx, qy, qz) in cell (cx, cy, cz) to the boundary of the block of cells within `ring` of its own: an exact
// lower bound for every point not yet visited, less a slack for the fp32 cell-boundary arithmetic.  Faces that coincide
// with the grid boundary have nothing behind them: +inf when no face is open.
__device__ __forceinline__ float knn_ring_bound(const KnnGrid &g, int cx, int cy, int cz, int ring, float qx, float qy, float qz)
{
    float bound = __builtin_huge_valf();
    if (cx - ring > 0) bound = fminf(bound, qx - (g.minx + (float)(cx - ring) * g.cell));
    if (cx + ring < g.res - 1) bound = fminf(bound, (g.minx + (float)(cx + ring + 1) * g.cell) - qx);
    if (cy - ring > 0) bound = fminf(bound, qy - (g.miny + (float)(cy - ring) * g.cell));
    if (cy + ring < g.res - 1) bound = fminf(bound, (g.miny + (float)(cy + ring + 1) * g.cell) - qy);
    if (cz - ring > 0) bound = fminf(bound, qz - (g.minz + (float)(cz - ring) * g.cell));
    if (cz + ring < g.res - 1) bound = fminf(bound, (g.minz + (float)(cz + ring + 1) * g.cell) - qz);
    return bound - 1e-6f * fmaxf(fabsf(bound), g.cell);
}

// Is the search finished after a ring?  Yes when every cell has been visited, or when the K-th distance found is
// provably final (<= the distance to the unvisited region).  Fixed-radius statistic (r2 > 0, K-th only): nothing beyond
// r counts, and everything not yet visited is farther than `bound`.  (knn_query_kernel's K-th distance instances carry these
// two tests written out, for speed: a change here is a change there.)
template <bool FULL>
__device__ __forceinline__ bool knn_search_done(float bound, float kth, float r2)
{
    if (bound == __builtin_huge_valf() || (bound > 0.0f && kth <= bound * bound)) return true;
    return !FULL && r2 > 0.0f && bound > 0.0f && bound * bound > r2;
}

// The K-th distance among the kk entries that count (fewer points than K: the farthest available).
template <int K>
__device__ __forceinline__ float knn_kth_of(const float (&best)[K], int kk)
{
    float kth = best[0];
#pragma unroll
    for (int k = 1; k < K; ++k) {
        float b = best[k];
        asm volatile("" : "+v"(b));   // (a value, see above)
        kth = (k < kk) ? b : kth;
    }
    return kth;
}

// What a packed slot outside every cloud gets: a zero list, or a zero in the K-th distance row `kth_row`.
template <bool FULL>
__device__ __forceinline__ void knn_write_no_cloud(int64_t slot, int Krt, float *__restrict__ kth_row, float *__restrict__ dists,
                                                   int64_t *__restrict__ idx)
{
    if (FULL) {
        for (int k = 0; k < Krt; ++k) { dists[slot * Krt + k] = 0.0f; idx[slot * Krt + k] = 0; }
    } else {
        kth_row[slot] = 0.0f;
    }
}

// What query point p (first packed slot of its cloud: f0) reports.  FULL: its list, zero-padded behind kk entries.
// Otherwise the statistic, and (!VIEW, dk_out given) the K-th distance itself, inf when the cloud has fewer than K points.
template <int K, bool FULL, bool VIEW>
__device__ __forceinline__ void knn_write_result(const float (&best)[K], const int (&bid)[FULL ? K : 1], int kk, int Krt, int64_t p,
                                                 int64_t f0, float r2, float *__restrict__ kth_sqdist, float *__restrict__ dists,
                                                 int64_t *__restrict__ idx, float *__restrict__ dk_out)
{
    if (FULL) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k < Krt) {
                dists[p * Krt + k] = k < kk ? best[k] : 0.0f;
                idx[p * Krt + k] = k < kk ? (int64_t)bid[FULL ? k : 0] - f0 : 0;
            }
        return;
    }
    float kth = knn_kth_of<K>(best, kk);
    if (!VIEW && dk_out != nullptr) dk_out[p] = kk < Krt ? __builtin_huge_valf() : kth;
    if (r2 > 0.0f) {
        // fixed-radius semantics of the reference's default neighbour search (frnn_grid_points(K, r), rasterizer.py:317-326):
        // neighbours beyond r come back as -1 and the statistic is the MAX over the K - 1 returned distances -- the farthest
        // neighbour found within r, or -1 for a point without any
        kth = -1.0f;
#pragma unroll
        for (int k = 1; k < K; ++k) kth = (k < kk && best[k] <= r2) ? best[k] : kth;
    }
    kth_sqdist[p] = kth;
}

// FULL = false: K-th squared distance only (kth_sqdist (P,)).  FULL = true: the whole neighbour list, ascending in
// (distance, id): dists (P,Krt) squared distances and idx (P,Krt) cloud-local ids, zero-padded when the cloud has
// fewer than Krt points (the layout pytorch3d.ops.knn_points returns for a self query, losses.py:157-180).
template <int K, bool FULL, bool VIEW = false>
__global__ __launch_bounds__(256) void knn_query_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx,
                                                        const int64_t *__restrict__ num_pts, int N, int64_t P,
                                                        const KnnGrid *__restrict__ grids, size_t stride,
                                                        const uint32_t *__restrict__ offsets,
                                                        const float4 *__restrict__ sorted, int Krt,
                                                        float *__restrict__ kth_sqdist, float *__restrict__ dists,
                                                        int64_t *__restrict__ idx, float r2 /* > 0: FRNN semantics, see dss_knn_kth_sqdist_radius */,
    const KnnView view = KnnView(), const float4 *__restrict__ boxes = nullptr /* skip structure, see knn_subsort_kernel */,
    const uint32_t *__restrict__ dense_flag = nullptr, const int role = 0 /* 1: only clouds without dense cells, 2: only clouds with */,
    float *__restrict__ dk_out = nullptr /* !VIEW: the K-th distance itself (inf: fewer than K points), see knn_view_shortcut */,
    const float *__restrict__ plain_stat = nullptr, const float *__restrict__ plain_dk = nullptr /* VIEW: the unmasked search */)
{
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= P) return;
    const bool skip = boxes != nullptr && *dense_flag != 0u;
    if ((role == 1 && skip) || (role == 2 && !skip)) return;   // (the launch next to this one takes the cloud)
    const int n = find_cloud(slot, first_idx, num_pts, N);
    if (n < 0) {  // packed slot outside every cloud
        // (one cloud, several cameras: the slot of THIS camera's row -- every row of the result is defined everywhere)
        knn_write_no_cloud<FULL>(slot, Krt, kth_sqdist + (VIEW && view.mode == 1 ? (size_t)blockIdx.y * (size_t)P : (size_t)0), dists, idx);
        return;
    }
    const KnnGrid g = grids[n];
    const int64_t f0 = first_idx[n];
    const int64_t cnt_n = num_pts[n];
    const uint32_t *off = offsets + (size_t)n * stride;
    // the query of this thread is the slot-th point of the cell-sorted order (every slot of a cloud's range holds
    // exactly one of its points): neighbouring lanes query neighbouring points
    const float4 self = sorted[slot];
    const int64_t p = (int64_t)__float_as_int(self.w);
    const float qx = self.x, qy = self.y, qz = self.z;
    KnnCamera camera = {};
    if (VIEW) {
        const int cam = view.mode == 1 ? (int)blockIdx.y : n;
        if (view.mode == 1 && view.culls[cam] == 0u) return;   // (the row is a copy: knn_view_rows_kernel)
        camera = KnnCamera::load(view.V, view.znear, view.zfar, cam);
        if (view.mode == 1) kth_sqdist += (size_t)cam * (size_t)P;
        if (!camera.kept(qx, qy, qz)) { kth_sqdist[p] = 0.0f; return; }
        if (knn_view_shortcut(view.culls[cam], qx, qy, qz, camera, plain_dk[p], r2)) { kth_sqdist[p] = plain_stat[p]; return; }
    }
    const int3 cell = knn_cell_coords(g, qx, qy, qz);
    const int cx = cell.x, cy = cell.y, cz = cell.z;
    float best[K];
    int bid[FULL ? K : 1];
#pragma unroll
    for (int k = 0; k < K; ++k) best[k] = __builtin_huge_valf();
#pragma unroll
    for (int k = 0; k < (FULL ? K : 1); ++k) bid[k] = 0x7fffffff;
    const int kk = (int)min((int64_t)Krt, cnt_n);  // fewer points than K: k-th = farthest available
    if (kk <= 0) {
        if (!FULL) kth_sqdist[p] = 0.0f;
        return;
    }
    auto consider = [&](const float4 q) __attribute__((always_inline)) {
        const float dx = q.x - qx, dy = q.y - qy, dz = q.z - qz;
        float d2 = dx * dx + dy * dy + dz * dz;
        if (VIEW && !camera.kept(q.x, q.y, q.z)) d2 = __builtin_huge_valf();   // the camera drops it
        knn_insert<K, FULL>(best, bid, d2, __float_as_int(q.w));
    };
    // Candidates [s, e) of the cell-sorted array: cells that are consecutive along x are consecutive in memory, so a
    // whole (z, y) row of the search block is ONE contiguous range.  Four candidates are requested per memory round
    // trip (clamped, unconditional loads): the walk is latency-bound -- ~100 dependent 16-byte loads per query at
    // 2 wavefronts per CU took 210 us for 32k points when issued one at a time.
    // skip structure (clustered clouds, see knn_subsort_kernel): the slots [seed_lo, seed_hi) around the query's own slot
    // have been looked at before the rings start and are passed over afterwards; runs longer than KNN_DENSE slots are
    // walked block by block, a block whose box is farther than the current K-th distance is not read.  The box distance
    // uses the expression of `consider` on the clamped offsets, which are never larger in magnitude than those of a point
    // inside the box: rounding is monotone, so box distance <= point distance in fp32 as well -- and the comparison is
    // strict, so a candidate that ties with the K-th entry (and may win on its id) is still read.
    uint32_t seed_lo = 0, seed_hi = 0;
    auto visit = [&](uint32_t s, uint32_t e) __attribute__((always_inline)) {
        if (skip && e - s > (uint32_t)KNN_DENSE) {
            const uint64_t a0 = (uint64_t)f0 + s, a1 = (uint64_t)f0 + e;   // packed slots
            for (uint64_t b = a0 / KNN_BLOCK; b * KNN_BLOCK < a1; ++b) {
                const float4 mn = boxes[2 * b], mx = boxes[2 * b + 1];
                const float dx = fmaxf(fmaxf(mn.x - qx, qx - mx.x), 0.0f), dy = fmaxf(fmaxf(mn.y - qy, qy - mx.y), 0.0f),
                            dz = fmaxf(fmaxf(mn.z - qz, qz - mx.z), 0.0f);
                if (dx * dx + dy * dy + dz * dz > best[K - 1]) continue;
                const uint32_t j0 = (uint32_t)(max(b * KNN_BLOCK, a0) - (uint64_t)f0);
                const uint32_t j1 = (uint32_t)(min(b * KNN_BLOCK + KNN_BLOCK, a1) - (uint64_t)f0);
                for (uint32_t j = j0; j < j1; j += 4) {
                    const float4 q0 = sorted[f0 + j], q1 = sorted[f0 + min(j + 1, j1 - 1)], q2 = sorted[f0 + min(j + 2, j1 - 1)],
                                 q3 = sorted[f0 + min(j + 3, j1 - 1)];
                    const int cnt = (int)min(j1 - j, 4u);
#pragma nounroll
                    for (int i = 0; i < cnt; ++i)
                        if (j + i < seed_lo || j + i >= seed_hi) consider(i == 0 ? q0 : (i == 1 ? q1 : (i == 2 ? q2 : q3)));
                }
            }
            return;
        }
        for (uint32_t j = s; j < e; j += 4) {
            const float4 q0 = sorted[f0 + j], q1 = sorted[f0 + min(j + 1, e - 1)], q2 = sorted[f0 + min(j + 2, e - 1)],
                         q3 = sorted[f0 + min(j + 3, e - 1)];
            const int cnt = (int)min(e - j, 4u);
#pragma nounroll
            for (int i = 0; i < cnt; ++i) consider(i == 0 ? q0 : (i == 1 ? q1 : (i == 2 ? q2 : q3)));  // ONE copy of the insert
        }
    };
    if (skip) {
        // own cell dense (its points lie along a Morton curve): the neighbours of the query's slot are neighbours in space
        const int c_own = knn_cell_index(g, cx, cy, cz);
        const uint32_t cs = off[c_own], ce = off[c_own + 1];
        if (ce - cs > (uint32_t)KNN_DENSE) {
            const uint32_t me = (uint32_t)(slot - f0);
            seed_lo = me > cs + KNN_SEED ? me - KNN_SEED : cs;
            seed_hi = min(ce, me + KNN_SEED);
            for (uint32_t j = seed_lo; j < seed_hi; ++j) consider(sorted[f0 + j]);
        }
    }
    // The search starts with the 3x3x3 block (the own cell alone almost never proves K >= 7 neighbours final): the
    // offsets of its nine rows are requested together and parked in LDS (a register array indexed by a rolled loop
    // would go to scratch, nine unrolled copies of the walk cost 246 VGPRs).  Further rings, rarely needed, add their
    // shell: full rows on the y/z faces, the two end cells of the other rows.
    __shared__ uint32_t row_lo[9][256], row_hi[9][256];
    {
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.res - 1);
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int z = cz + r / 3 - 1, y = cy + r % 3 - 1;
            const bool in = z >= 0 && z < g.res && y >= 0 && y < g.res;
            const int c = in ? (z * g.res + y) * g.res : 0;
            const uint32_t s = off[c + x0], e = off[c + x1 + 1];
            row_lo[r][threadIdx.x] = in ? s : 0u;
            row_hi[r][threadIdx.x] = in ? e : 0u;
        }
    }
    for (int ring = 1; ring <= g.res; ++ring) {
        const int x0 = max(cx - ring, 0), x1 = min(cx + ring, g.res - 1);
        const int y0 = max(cy - ring, 0), y1 = min(cy + ring, g.res - 1);
        const int z0 = max(cz - ring, 0), z1 = min(cz + ring, g.res - 1);
        const int ny = y1 - y0 + 1;
        const int walks = ring == 1 ? 9 : 2 * ny * (z1 - z0 + 1);  // rows of the block, or (row, end) pairs of the shell
#pragma nounroll
        for (int t = 0; t < walks; ++t) {
            uint32_t s, e;
            if (ring == 1) {
                s = row_lo[t][threadIdx.x];
                e = row_hi[t][threadIdx.x];
            } else {
                const int row = t >> 1, z = z0 + row / ny, y = y0 + row % ny;
                const int c = (z * g.res + y) * g.res;
                const bool full = z == cz - ring || z == cz + ring || y == cy - ring || y == cy + ring;
                const int xa = full ? x0 : ((t & 1) ? cx + ring : cx - ring);
                const int xb = full ? x1 : xa;
                if ((full && (t & 1)) || xa < 0 || xb >= g.res) continue;  // a full row is one walk
                s = off[c + xa];
                e = off[c + xb + 1];
            }
            visit(s, e);
        }
        const float bound = knn_ring_bound(g, cx, cy, cz, ring, qx, qy, qz), kth = knn_kth_of<K>(best, kk);
        if constexpr (FULL) {
            if (knn_search_done<true>(bound, kth, r2)) break;
        } else {
            // knn_search_done, the statement of record, written out: called here it costs the K-th distance instances
            // 1.3 % of a whole call at 131k points; written out for the lists it costs those 0.5 to 1 %
            // (profiles/knn_device_refactor.txt)
            if (bound == __builtin_huge_valf() || (bound > 0.0f && kth <= bound * bound)) break;
            if (r2 > 0.0f && bound > 0.0f && bound * bound > r2) break;
        }
    }
    knn_write_result<K, FULL, VIEW>(best, bid, kk, Krt, p, f0, r2, kth_sqdist, dists, idx, dk_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Cooperative query: KNN_LPQ = 16 lanes (one DPP row) per query point.  The one-thread-per-point kernel above is a chain
// of ~100 dependent 16-byte loads per query with two wavefronts per CU at DSS sizes (32k points = 512 wavefronts): 58 us,
// the slowest kernel of a training iteration.  Here the 16 lanes of a group take every 16th
// candidate of each row range -- one coalesced 256-byte request per trip, ~18 dependent trips per query, 16 x the
// wavefronts to hide them behind --, keep their own sorted K-lists and merge them with four DPP rounds (quad_perm x 2,
// row_half_mirror, row_mirror: plain VALU moves inside the row, no LDS round trip), after which every lane holds the
// group's K best.  Same candidates, same (distance, id) order, same ring termination rule: identical results.
// Further rings (rare) start from the merged list in lane 0 and empty lists elsewhere, so nothing is counted twice.
// ---------------------------------------------------------------------------------------------------------------
#define KNN_LPQ 16
template <int CTRL>
__device__ __forceinline__ float knn_dpp_f(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int knn_dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }

// this lane's ascending K-list merged with the list of the lane CTRL maps to: min(A[i], B[K-1-i]) picks the K smallest of
// the union as a bitonic sequence, an odd-even transposition network sorts it (see merge_round in raster_forward.hip)
template <int K, bool FULL, int CTRL>
__device__ __forceinline__ void knn_merge_round(float (&best)[K], int (&bid)[FULL ? K : 1])
{
    float ob[K];
    int oi[FULL ? K : 1];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        ob[k] = knn_dpp_f<CTRL>(best[k]);
        if (FULL) oi[FULL ? k : 0] = knn_dpp_i<CTRL>(bid[FULL ? k : 0]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool lt = FULL ? knn_less(ob[K - 1 - k], oi[FULL ? K - 1 - k : 0], best[k], bid[FULL ? k : 0]) : ob[K - 1 - k] < best[k];
        best[k] = lt ? ob[K - 1 - k] : best[k];
        if (FULL) bid[FULL ? k : 0] = lt ? oi[FULL ? K - 1 - k : 0] : bid[FULL ? k : 0];
    }
#pragma unroll
    for (int round = 0; round < K; ++round) {
#pragma unroll
        for (int k = round & 1; k + 1 < K; k += 2) {
            const bool sw = FULL ? knn_less(best[k + 1], bid[FULL ? k + 1 : 0], best[k], bid[FULL ? k : 0]) : best[k + 1] < best[k];
            const float a = best[k], b = best[k + 1];
            best[k] = sw ? b : a;
            best[k + 1] = sw ? a : b;
            if (FULL) {
                const int x = bid[FULL ? k : 0], y = bid[FULL ? k + 1 : 0];
                bid[FULL ? k : 0] = sw ? y : x;
                bid[FULL ? k + 1 : 0] = sw ? x : y;
            }
        }
    }
}

template <int K, bool FULL, bool VIEW = false, bool SKIP = false /* compiled with the skip structure (P >= KNN_SKIP_MIN_P): +20 VGPRs */>
__global__ __launch_bounds__(256) void knn_query_coop_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx,
                                                             const int64_t *__restrict__ num_pts, int N, int64_t P,
                                                             const KnnGrid *__restrict__ grids, size_t stride,
                                                             const uint32_t *__restrict__ offsets,
                                                             const float4 *__restrict__ sorted, int Krt,
                                                             float *__restrict__ kth_sqdist, float *__restrict__ dists,
                                                             int64_t *__restrict__ idx, float r2 /* > 0: FRNN semantics, see dss_knn_kth_sqdist_radius */,
    const KnnView view = KnnView(), const uint32_t chunks = 0 /* VIEW: query chunks per camera (the grid is persistent) */,
    const float4 *__restrict__ boxes = nullptr /* skip structure, see knn_subsort_kernel */,
    const uint32_t *__restrict__ dense_flag = nullptr, const int role = 0 /* 1: only clouds without dense cells, 2: only clouds with */,
    float *__restrict__ dk_out = nullptr /* !VIEW: the K-th distance itself (inf: fewer than K points), see knn_view_shortcut */,
    const float *__restrict__ plain_stat = nullptr, const float *__restrict__ plain_dk = nullptr /* VIEW: the unmasked search */)
{
    const bool skip = SKIP && boxes != nullptr && *dense_flag != 0u;
    if ((role == 1 && skip) || (role == 2 && !skip)) return;
    constexpr int GPB = 256 / KNN_LPQ;   // query groups per workgroup
    const int grp = threadIdx.x / KNN_LPQ, sub = threadIdx.x % KNN_LPQ;
    __shared__ uint32_t row_lo[KNN_LPQ][GPB], row_hi[KNN_LPQ][GPB];
    float *const kth_base = kth_sqdist;
    // VIEW, one cloud seen by several cameras: a grid row covers the query chunks of ONE camera (at most 16,384 workgroups, the
    // rest by stride), there are two rows, and every workgroup takes its chunks for each camera of its row's share that drops
    // points, one camera after the other (two rows: half the serial depth when every camera drops points) -- a
    // camera that drops nothing costs a scalar load (its row is a copy, knn_view_rows_kernel), where a grid row per camera cost
    // a workgroup dispatch per chunk.  Otherwise: one pass, chunk = this workgroup.
    const bool walk = VIEW && view.mode == 1;
    for (int cam_y = walk ? (int)blockIdx.y : 0; cam_y < (walk ? view.n_cams : 1); cam_y += walk ? (int)gridDim.y : 1) {
    if (walk && view.culls[cam_y] == 0u) continue;
    for (uint32_t bx = blockIdx.x; bx < (walk ? chunks : blockIdx.x + 1u); bx += gridDim.x) {
    kth_sqdist = kth_base;
    const int64_t slot = (int64_t)bx * GPB + grp;
    if (slot >= P) continue;   // (whole DPP rows leave together)
    const int n = find_cloud(slot, first_idx, num_pts, N);
    if (n < 0) {  // packed slot outside every cloud
        // (one cloud, several cameras: the slot of THIS camera's row -- every row of the result is defined everywhere)
        if (sub == 0) knn_write_no_cloud<FULL>(slot, Krt, kth_base + (walk ? (size_t)cam_y * (size_t)P : (size_t)0), dists, idx);
        continue;
    }
    const KnnGrid g = grids[n];
    const int64_t f0 = first_idx[n];
    const int64_t cnt_n = num_pts[n];
    const uint32_t *off = offsets + (size_t)n * stride;
    const float4 self = sorted[slot];   // the slot-th point of the cell-sorted order
    const int64_t p = (int64_t)__float_as_int(self.w);
    const float qx = self.x, qy = self.y, qz = self.z;
    KnnCamera camera = {};
    if (VIEW) {
        const int cam = view.mode == 1 ? cam_y : n;
        camera = KnnCamera::load(view.V, view.znear, view.zfar, cam);
        if (view.mode == 1) kth_sqdist = kth_base + (size_t)cam * (size_t)P;
        if (!camera.kept(qx, qy, qz)) {   // (the whole 16-lane group shares the query: leaves together)
            if (sub == 0) kth_sqdist[p] = 0.0f;
            continue;
        }
        if (knn_view_shortcut(view.culls[cam], qx, qy, qz, camera, plain_dk[p], r2)) {
            if (sub == 0) kth_sqdist[p] = plain_stat[p];
            continue;
        }
    }
    const int3 cell = knn_cell_coords(g, qx, qy, qz);
    const int cx = cell.x, cy = cell.y, cz = cell.z;
    float best[K];
    int bid[FULL ? K : 1];
#pragma unroll
    for (int k = 0; k < K; ++k) best[k] = __builtin_huge_valf();
#pragma unroll
    for (int k = 0; k < (FULL ? K : 1); ++k) bid[k] = 0x7fffffff;
    const int kk = (int)min((int64_t)Krt, cnt_n);
    if (kk <= 0) {
        if (!FULL && sub == 0) kth_sqdist[p] = 0.0f;
        continue;
    }
    auto consider = [&](const float4 q, bool on) __attribute__((always_inline)) {
        const float dx = q.x - qx, dy = q.y - qy, dz = q.z - qz;
        if (VIEW) on = on && camera.kept(q.x, q.y, q.z);   // the camera drops it
        // a lane without a candidate (`on` down) offers the padding entry, which enters no list
        const float d2 = on ? dx * dx + dy * dy + dz * dz : __builtin_huge_valf();
        const int id = on ? __float_as_int(q.w) : 0x7fffffff;
        knn_insert<K, FULL>(best, bid, d2, id);
    };
    // candidates [s, e) of the cell-sorted array, every KNN_LPQ-th one for this lane: the group's 16 loads of a trip are
    // one contiguous 256-byte run; two trips are requested together
    // skip structure (clustered clouds, see knn_subsort_kernel; the reasoning about exactness is in knn_query_kernel): `kb` is
    // a K-th distance the GROUP has established (after the seed, after every ring, and after a long run walked without one);
    // a lane prunes with the smaller of it and its own list's K-th entry.  Lane i tests the box of block i of sixteen; the
    // group then reads the surviving blocks one after the other, a slot per lane.
    float kb = __builtin_huge_valf();
    uint32_t seed_lo = 0, seed_hi = 0;
    const int gsh = (int)(threadIdx.x & 48u);   // bit position of the group's lanes in the wavefront's ballot
    auto merge_all = [&]() __attribute__((always_inline)) {
        knn_merge_round<K, FULL, 0xB1>(best, bid);    // quad_perm [1,0,3,2]
        knn_merge_round<K, FULL, 0x4E>(best, bid);    // quad_perm [2,3,0,1]
        knn_merge_round<K, FULL, 0x141>(best, bid);   // row_half_mirror
        knn_merge_round<K, FULL, 0x140>(best, bid);   // row_mirror
    };
    auto keep_lane0 = [&]() __attribute__((always_inline)) {   // lane 0 carries the merged list, the others start empty (nothing is counted twice)
        const bool drop = sub != 0;   // (selects on values: a branch around stores to bid[] sends the array to scratch memory)
#pragma unroll
        for (int k = 0; k < K; ++k) best[k] = drop ? __builtin_huge_valf() : best[k];
#pragma unroll
        for (int k = 0; k < (FULL ? K : 1); ++k) bid[k] = drop ? 0x7fffffff : bid[k];
    };
    auto visit = [&](uint32_t s, uint32_t e) __attribute__((always_inline)) {
        if (skip && e - s > (uint32_t)KNN_DENSE) {
            const uint64_t a0 = (uint64_t)f0 + s, a1 = (uint64_t)f0 + e;   // packed slots
            const uint64_t b_last = (a1 - 1) / KNN_BLOCK;
            for (uint64_t bb = a0 / KNN_BLOCK; bb <= b_last; bb += 2 * KNN_LPQ) {   // (group-uniform) 32 blocks per trip
                // two boxes per lane, their four loads in flight together: the walk is a chain of dependent round trips (boxes,
                // then the survivors' slots) at ~6 wavefronts per SIMD -- the fewer trips, the faster
                const uint64_t bA = bb + (uint64_t)sub, bB = bA + KNN_LPQ;
                const bool inA = bA <= b_last, inB = bB <= b_last;
                const float4 mnA = boxes[2 * (inA ? bA : b_last)], mxA = boxes[2 * (inA ? bA : b_last) + 1];
                const float4 mnB = boxes[2 * (inB ? bB : b_last)], mxB = boxes[2 * (inB ? bB : b_last) + 1];
                const float lim = fminf(kb, best[K - 1]);
                const float ax = fmaxf(fmaxf(mnA.x - qx, qx - mxA.x), 0.0f), ay = fmaxf(fmaxf(mnA.y - qy, qy - mxA.y), 0.0f),
                            az = fmaxf(fmaxf(mnA.z - qz, qz - mxA.z), 0.0f);
                const float cx2 = fmaxf(fmaxf(mnB.x - qx, qx - mxB.x), 0.0f), cy2 = fmaxf(fmaxf(mnB.y - qy, qy - mxB.y), 0.0f),
                            cz2 = fmaxf(fmaxf(mnB.z - qz, qz - mxB.z), 0.0f);
                const bool passA = inA && !(ax * ax + ay * ay + az * az > lim);
                const bool passB = inB && !(cx2 * cx2 + cy2 * cy2 + cz2 * cz2 > lim);
                unsigned gm = ((unsigned)(__ballot(passA) >> gsh) & 0xffffu) | (((unsigned)(__ballot(passB) >> gsh) & 0xffffu) << 16);
                while (gm != 0u) {
                    // up to four surviving blocks per trip, their loads in flight together
                    uint64_t j[4];
                    bool on[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool have = gm != 0u;
                        j[u] = (bb + (uint64_t)(have ? __builtin_ctz(gm) : 0)) * KNN_BLOCK + (uint64_t)sub;
                        gm &= gm - (have ? 1u : 0u);
                        const uint32_t jl = (uint32_t)(j[u] - (uint64_t)f0);
                        on[u] = have && j[u] >= a0 && j[u] < a1 && (jl < seed_lo || jl >= seed_hi);
                    }
                    const float4 q0 = sorted[on[0] ? j[0] : a0], q1 = sorted[on[1] ? j[1] : a0], q2 = sorted[on[2] ? j[2] : a0],
                                 q3 = sorted[on[3] ? j[3] : a0];
                    consider(q0, on[0]);
                    consider(q1, on[1]);
                    consider(q2, on[2]);
                    consider(q3, on[3]);
                }
            }
            if (kb == __builtin_huge_valf()) {   // a long run without a group bound: establish one now
                merge_all();
                kb = best[K - 1];
                keep_lane0();
            }
            return;
        }
        for (uint32_t base = s; base < e; base += 2 * KNN_LPQ) {   // (group-uniform trip count)
            const uint32_t j0 = base + (uint32_t)sub, j1 = j0 + KNN_LPQ;
            const bool on0 = j0 < e, on1 = j1 < e;
            const float4 q0 = sorted[f0 + (on0 ? j0 : s)], q1 = sorted[f0 + (on1 ? j1 : s)];   // clamped, unconditional
            consider(q0, on0);
            consider(q1, on1);
        }
    };
    if (skip) {
        // own cell dense (its points lie along a Morton curve): the neighbours of the query's slot are neighbours in space
        const int c_own = knn_cell_index(g, cx, cy, cz);
        const uint32_t cs = off[c_own], ce = off[c_own + 1];
        if (ce - cs > (uint32_t)KNN_DENSE) {
            const uint32_t me = (uint32_t)(slot - f0);
            seed_lo = me > cs + KNN_SEED ? me - KNN_SEED : cs;
            seed_hi = min(ce, me + KNN_SEED);
            for (uint32_t j = seed_lo + (uint32_t)sub; j < seed_lo + 2 * KNN_SEED; j += KNN_LPQ) {   // (two trips, group-uniform)
                const bool on = j < seed_hi;
                consider(sorted[f0 + (on ? j : seed_lo)], on);
            }
            merge_all();
            kb = best[K - 1];
            keep_lane0();
        }
    }
    uint32_t s1 = 0, e1 = 0;
    if (sub < 9) {   // lane r of the group fetches the offsets of row r of the 3 x 3 x 3 block
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.res - 1);
        const int z = cz + sub / 3 - 1, y = cy + sub % 3 - 1;
        const bool in = z >= 0 && z < g.res && y >= 0 && y < g.res;
        const int c = in ? (z * g.res + y) * g.res : 0;
        const uint32_t s = off[c + x0], e = off[c + x1 + 1];
        s1 = in ? s : 0u;
        e1 = in ? e : 0u;
        if (!SKIP) {
            row_lo[sub][grp] = s1;
            row_hi[sub][grp] = e1;
        }
    }
    if (!SKIP) __builtin_amdgcn_wave_barrier();   // same wavefront wrote and reads the row table (LDS operations of a wave complete in order)
    for (int ring = 1; ring <= g.res; ++ring) {
        const int x0 = max(cx - ring, 0), x1 = min(cx + ring, g.res - 1);
        const int y0 = max(cy - ring, 0), y1 = min(cy + ring, g.res - 1);
        const int z0 = max(cz - ring, 0), z1 = min(cz + ring, g.res - 1);
        const int ny = y1 - y0 + 1;
        const int walks = ring == 1 ? 9 : 2 * ny * (z1 - z0 + 1);
        if constexpr (!SKIP) {
            // (small clouds, P < KNN_SKIP_MIN_P: one walk after the other -- the batched form below costs this instantiation ten
            // VGPRs, i.e. the eighth wavefront per SIMD that the latency-bound launch at 32k points lives on)
#pragma nounroll
            for (int t = 0; t < walks; ++t) {
                uint32_t s, e;
                if (ring == 1) {
                    s = row_lo[t][grp];
                    e = row_hi[t][grp];
                } else {
                    const int row = t >> 1, z = z0 + row / ny, y = y0 + row % ny;
                    const int c = (z * g.res + y) * g.res;
                    const bool full = z == cz - ring || z == cz + ring || y == cy - ring || y == cy + ring;
                    const int xa = full ? x0 : ((t & 1) ? cx + ring : cx - ring);
                    const int xb = full ? x1 : xa;
                    if ((full && (t & 1)) || xa < 0 || xb >= g.res) continue;
                    s = off[c + xa];
                    e = off[c + xb + 1];
                }
                visit(s, e);
            }
        } else {
        // The sixteen lanes fetch the candidate ranges of sixteen walks together and the group visits the non-empty ones (ring 1:
        // the nine rows requested above).  One walk after the other is a dependent round trip per walk, most of them for an
        // EMPTY range: a stray point needs four or five rings -- ~600 walks --, and the launch lasts as long as its slowest
        // query (0.55 ms for the trained cloud of tools/clustered_timing.py whatever the rest of the kernel did).
#pragma nounroll
        for (int t0 = 0; t0 < walks; t0 += KNN_LPQ) {
            uint32_t s = s1, e = e1;
            if (ring > 1) {
                const int t = t0 + sub;
                s = e = 0u;
                if (t < walks) {
                    const int row = t >> 1, z = z0 + row / ny, y = y0 + row % ny;
                    const int c = (z * g.res + y) * g.res;
                    const bool full = z == cz - ring || z == cz + ring || y == cy - ring || y == cy + ring;
                    const int xa = full ? x0 : ((t & 1) ? cx + ring : cx - ring);
                    const int xb = full ? x1 : xa;
                    if (!((full && (t & 1)) || xa < 0 || xb >= g.res)) {   // (a full row is one walk)
                        s = off[c + xa];
                        e = off[c + xb + 1];
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            row_lo[sub][grp] = s;
            row_hi[sub][grp] = e;
            __builtin_amdgcn_wave_barrier();   // (same wavefront writes and reads: LDS operations of a wave complete in order)
            unsigned ne = (unsigned)(__ballot(e > s) >> gsh) & 0xffffu;
            while (ne != 0u) {
                const int i = __builtin_ctz(ne);
                ne &= ne - 1u;
                visit(row_lo[i][grp], row_hi[i][grp]);
            }
        }
        }   // (SKIP)
        // the group's K best: four merge rounds inside the DPP row, every lane ends with the same list
        merge_all();
        kb = best[K - 1];
        if (knn_search_done<FULL>(knn_ring_bound(g, cx, cy, cz, ring, qx, qy, qz), knn_kth_of<K>(best, kk), r2)) break;
        if (sub != 0) {   // next ring: lane 0 carries the merged list, the others start empty (nothing is counted twice)
#pragma unroll
            for (int k = 0; k < K; ++k) best[k] = __builtin_huge_valf();
#pragma unroll
            for (int k = 0; k < (FULL ? K : 1); ++k) bid[k] = 0x7fffffff;
        }
    }
    if (sub == 0) knn_write_result<K, FULL, VIEW>(best, bid, kk, Krt, p, f0, r2, kth_sqdist, dists, idx, dk_out);
    }   // (chunks)
    }   // (cameras)
}

// deterministic per-cloud mean of values*scale clamped to [lo,hi]: one workgroup per cloud, fixed order (four independent
// partial sums per thread, wave reduction on shuffles, 16 wave totals: the 10-step LDS tree of round 1 took 19 us)
__global__ __launch_bounds__(1024) void cloud_mean_kernel(const float *__restrict__ vals, const int64_t *__restrict__ first_idx,
                                                          const int64_t *__restrict__ num_pts, float scale, float lo,
                                                          float hi, float fallback, int min_points,
                                                          float *__restrict__ out)
{
    __shared__ double part[16];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int64_t f0 = first_idx[n], cnt = num_pts[n];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t i = tid;
    for (; i + 3 * 1024 < cnt; i += 4 * 1024) {
        const float v0 = vals[f0 + i], v1 = vals[f0 + i + 1024], v2 = vals[f0 + i + 2048], v3 = vals[f0 + i + 3072];
        a0 += (double)(v0 * scale); a1 += (double)(v1 * scale); a2 += (double)(v2 * scale); a3 += (double)(v3 * scale);
    }
    for (; i < cnt; i += 1024) a0 += (double)(vals[f0 + i] * scale);
    double acc = (a0 + a1) + (a2 + a3);
    // wave_xor_sum, the statement of record, written out: called here the load loop above is scheduled differently, 0.5 us
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += part[w];
        float m = (cnt >= min_points && cnt > 0) ? (float)(t / (double)cnt) : fallback;
        out[n] = fminf(fmaxf(m, lo), hi);
    }
}

// The reference's Vrk_invariant statistic under culling (rasterizer.py:236-240, 183-217, 320-326): the cloud is extended
// to the N cameras, every camera DROPS the points outside its depth range, and h_n = clamp(mean over the PADDED cloud n of
// 0.5 max kNN-7 d^2) -- `h_k.mean(dim=1)` runs over the padded length P_max = the largest kept count of the batch, the padding
// contributing zeros.  Here the points are masked, not dropped: phase 1 sums values * scale over the points camera n keeps
// (the depth test of setup_point_compute, same expression) and counts them; phase 2 divides by the largest count.
// (values = K-th neighbour distances within the WHOLE cloud: a kept point whose 7 nearest include a dropped point sees a
// slightly smaller distance than the reference's search among the kept points -- second order, documented.)
#define RENDERABLE_BLOCKS 32   // workgroups per camera (one per camera left seven eighths of a 22 us launch to 8 CUs)
__global__ __launch_bounds__(1024) void renderable_sum_kernel(const float *__restrict__ vals, const float *__restrict__ world,
                                                              const float *__restrict__ V, const float *__restrict__ znear,
                                                              const float *__restrict__ zfar, const int64_t *__restrict__ first_idx,
                                                              const int64_t *__restrict__ num_pts, int shared, float scale,
                                                              double *__restrict__ part /* (N, RENDERABLE_BLOCKS, 2): sum, count */,
                                                              int64_t vals_cam_stride /* 0: one value per world point */)
{
    __shared__ double psum[16], pcnt[16];
    const int n = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const int64_t f0 = shared ? 0 : first_idx[n], cnt = num_pts[n];
    const KnnCamera camera = KnnCamera::load(V, znear, zfar, n);
    double a = 0.0;
    float c = 0.f;
    // block b of a camera takes the points b * 1024 + tid + k * (RENDERABLE_BLOCKS * 1024): a fixed assignment, so the sums
    // are reproducible; four points per trip with their loads in flight together
    const int64_t stride = (int64_t)RENDERABLE_BLOCKS * 1024;
    for (int64_t i0 = (int64_t)b * 1024 + tid; i0 < cnt; i0 += 4 * stride) {
        float x[4], y[4], z[4], q[4];
        bool in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * stride;
            in[u] = i < cnt;
            const int64_t wi = f0 + (in[u] ? i : i0);
            x[u] = world[3 * wi]; y[u] = world[3 * wi + 1]; z[u] = world[3 * wi + 2];
            q[u] = vals[(size_t)n * (size_t)vals_cam_stride + wi];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = in[u] && camera.kept(x[u], y[u], z[u]);
            a += ok ? (double)(q[u] * scale) : 0.0;
            c += ok ? 1.f : 0.f;
        }
    }
    a = wave_xor_sum(a);
    const double cc = wave_xor_sum((double)c);
    if ((tid & 63) == 0) { psum[tid >> 6] = a; pcnt[tid >> 6] = cc; }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0, tc = 0.0;
        for (int w = 0; w < 16; ++w) { t += psum[w]; tc += pcnt[w]; }
        part[((size_t)n * RENDERABLE_BLOCKS + b) * 2] = t;
        part[((size_t)n * RENDERABLE_BLOCKS + b) * 2 + 1] = tc;
    }
}
__global__ __launch_bounds__(64) void renderable_mean_kernel(double *__restrict__ part, int N, float lo, float hi,
                                                             float fallback, int min_points, float *__restrict__ out)
{
    // ONE wavefront.  Pass 1: lane l adds up the block partials of cameras l, l + 64, ... in block order (fixed) and parks
    // the totals in the camera's first slot; the largest kept count of the batch is a wave maximum.  Pass 2: the means.
    double cmax = 0.0;
    for (int n = threadIdx.x; n < N; n += 64) {
        double s = 0.0, c = 0.0;
#pragma unroll 8
        for (int b = 0; b < RENDERABLE_BLOCKS; ++b) {
            s += part[((size_t)n * RENDERABLE_BLOCKS + b) * 2];
            c += part[((size_t)n * RENDERABLE_BLOCKS + b) * 2 + 1];
        }
        part[(size_t)n * RENDERABLE_BLOCKS * 2] = s;
        part[(size_t)n * RENDERABLE_BLOCKS * 2 + 1] = c;
        cmax = fmax(cmax, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cmax = fmax(cmax, __shfl_xor(cmax, o));
    for (int n = threadIdx.x; n < N; n += 64) {
        const double s = part[(size_t)n * RENDERABLE_BLOCKS * 2], cnt = part[(size_t)n * RENDERABLE_BLOCKS * 2 + 1];
        // `sq_dist[num_points_per_cloud < 7] = 1e-3` fills the whole padded row of a small cloud (rasterizer.py:322)
        const float m = (cnt >= (double)min_points && cmax > 0.0) ? (float)(s / cmax) : fallback;
        out[n] = fminf(fmaxf(m, lo), hi);
    }
}

}  // namespace dss

using namespace dss;

// Largest grid resolution a cloud of at most P points can ask for (knn_grid_kernel: ~8 points per occupied cell of a
// surface-like cloud), and the per-cloud stride of the cell arrays it implies (cells + end sentinel).
static int knn_res_cap(int64_t P)
{
    int res = (int)ceil(sqrt((double)(P > 0 ? P : 1) / 24.0));
    return res < 1 ? 1 : (res > KNN_MAX_RES ? KNN_MAX_RES : res);
}
static size_t knn_stride(int64_t P)
{
    const size_t r = (size_t)knn_res_cap(P);
    return r * r * r + 1;
}
static size_t knn_cells(int N, int64_t P) { return (size_t)(N > 0 ? N : 1) * knn_stride(P); }
static int knn_blocks(int64_t P) { return (int)((knn_stride(P) - 1 + KNN_SCAN_BLOCK - 1) / KNN_SCAN_BLOCK); }

#define KNN_MAX_VIEW_CAMS 1024
#define KNN_FULL_MAX_K 40
#define KNN_COOP_KTH_MAX_P 120000   // K-th distance: crossover of the two query kernels between 65k (cooperative +24 %) and 131k points (tie), profiles/r4_d_knn_sweep.json

// The regions of the workspace.  A function of (N, P) alone, so that the size query and the call agree.
struct KnnWorkspace {
    int *bbox;                           // (N, 6) box per cloud as ordered ints, or the small form's partial boxes (N, KNN_BB_WGS, 6)
    KnnGrid *grids;                      // (N)
    uint32_t *counts, *offsets, *cursor; // (cells + 1) each, `cbytes` bytes: points per cell, its scan, the fill's write heads
    uint32_t *blk_tot;                   // (N, nblk) block totals of the two-level scan
    int32_t *cell_of;                    // (P) cell of every point (-1: not in a cloud, or NaN)
    float4 *sorted;                      // (P) xyz + id, grouped by cell
    uint32_t *cam_flags;                 // dss_knn_kth_sqdist_view: one "drops points" flag per camera (knn_fill_kernel)
    uint32_t *dense_flag, *n_dense, *n_dense_pts;   // the "dense cells" flag and the two counters of the dense-cell list: KNN_DENSE_WORDS
                                                    // words at the head of one 256-byte block, cleared together (knn_dense_list_kernel, knn_subsort_kernel)
    float4 *boxes;                       // the block boxes of the skip structure (knn_subsort_kernel, knn_block_box_kernel)
    uint2 *dense_list;                   // and its list of dense cells
    uint32_t *rank_of;                   // (P) arrival numbers (knn_count_kernel)
    float *plain_stat, *plain_dk;        // (P) each, dss_knn_kth_sqdist_view: the unmasked search's two rows
    size_t stride;                       // per-cloud stride of the cell arrays
    int nblk;                            // scan workgroups per cloud
    size_t cbytes;                       // bytes of one cell array
    size_t bytes;
};
#define KNN_DENSE_WORDS 3

// ws == nullptr: size query (bytes)
static KnnWorkspace carve_knn(void *ws, int N, int64_t P)
{
    KnnWorkspace w = {};
    const size_t n = N > 0 ? N : 1, p = P > 0 ? P : 1;
    w.stride = knn_stride(P);
    w.nblk = knn_blocks(P);
    Bump b = {reinterpret_cast<char *>(ws), 0};
    w.bbox = b.take<int>(n * 6 * KNN_BB_WGS);
    w.grids = b.take<KnnGrid>(n);
    const size_t cells_at = b.used;
    w.counts = b.take<uint32_t>(knn_cells(N, P) + 1);
    w.cbytes = b.used - cells_at;
    w.offsets = b.take<uint32_t>(knn_cells(N, P) + 1);
    w.cursor = b.take<uint32_t>(knn_cells(N, P) + 1);
    w.blk_tot = b.take<uint32_t>(n * (size_t)w.nblk);
    w.cell_of = b.take<int32_t>(p);
    w.sorted = b.take<float4>(p);
    w.cam_flags = b.take<uint32_t>(KNN_MAX_VIEW_CAMS);
    w.dense_flag = b.take<uint32_t>(64);
    w.n_dense = ws ? w.dense_flag + 1 : nullptr;
    w.n_dense_pts = ws ? w.dense_flag + 2 : nullptr;
    w.boxes = b.take<float4>((p / KNN_BLOCK + 1) * 2);
    w.dense_list = b.take<uint2>(p / KNN_DENSE_CELL + 1);
    w.rank_of = b.take<uint32_t>(p);
    w.plain_stat = b.take<float>(p);
    w.plain_dk = b.take<float>(p);
    w.bytes = b.used;
    return w;
}

extern "C" size_t dss_knn_workspace(int N, int64_t P) { return carve_knn(nullptr, N, P).bytes; }

// Per-cloud bounding boxes as ordered ints (decode with ord2f), for callers outside this file (regularizers.hip).
int dss::launch_cloud_bbox(const float *points, const int64_t *first_idx, const int64_t *num_pts, int N, int64_t P,
                           int *bbox, hipStream_t st)
{
    hipLaunchKernelGGL(knn_init_kernel, dim3((6 * N + 63) / 64), dim3(64), 0, st, N, bbox);
    const unsigned bb = (unsigned)((P / N + 2047) / 2048 > 64 ? 64 : (P / N + 2047) / 2048);
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(bb ? bb : 1, N), dim3(256), 0, st, points, first_idx, num_pts, N, P, bbox);
    return check_launch("cloud bbox");
}

// How a call is searched, decided once from (P, K, lists or K-th distance) and DSS_OPT_KNN_QUERY
struct QueryPlan {
    bool skip;      // the skip structure is built and read (see knn_subsort_kernel)
    bool coop;      // the cooperative kernel; else one thread per query
    int k;          // K of the template instance
    unsigned one_block, one_grid;   // the one-thread kernel's workgroup size and workgroups
    unsigned chunks;                // the cooperative kernel's workgroups (256 / KNN_LPQ queries each)
};
static QueryPlan plan_query(int64_t P, int K, bool full)
{
    const int opt = option(DSS_OPT_KNN_QUERY);   // 0: by size, 1: cooperative, 2: one thread per query, 3: by size, no skip structure
    QueryPlan q;
    q.skip = P >= KNN_SKIP_MIN_P && opt != 3;   // (3: the uniform-grid walk whatever the cloud, for A/B)
    // full lists: the cooperative kernel wins while the launch is latency-bound (32k points, K = 12: 58 us against
    // ~100); at 100k points of an evenly sampled cloud the merges of (distance, id) lists cost more than the shorter
    // chains save (182 vs 155 us) -- but the one-thread kernel falls off a cliff as soon as cells fill up (30-60 points
    // per cell, the training loop on its way to the clustered state: 1.0 ms), the cooperative one does not
    // K-th distance only: cooperative up to KNN_COOP_KTH_MAX_P points (tools/knn_sweep.py, profiles/r4_d_knn_sweep.json)
    q.coop = opt == 1 || ((opt == 0 || opt == 3) && P <= KNN_COOP_KTH_MAX_P);
    // cooperative kernel: 16 lanes per query (K <= 16); the one-thread-per-query kernel keeps the deep lists
    if (full) q.k = K <= 8 ? 8 : (K <= 12 ? 12 /* the regularisers' knn_k (trainer.py:134-137) */ : (K <= 16 ? 16 : KNN_FULL_MAX_K));
    else q.k = K <= 8 ? 8 : KNN_MAX_K;
    if (q.k > KNN_MAX_K) q.coop = false;
    // small inputs: one wavefront per workgroup, so that the few hundred wavefronts spread over all 256 CUs
    q.one_block = P <= 131072 ? 64u : 256u;
    q.one_grid = (unsigned)((P + q.one_block - 1) / q.one_block);
    q.chunks = (unsigned)((P + (256 / KNN_LPQ) - 1) / (256 / KNN_LPQ));
    return q;
}

// Everything about a call that its launches share
struct KnnCall {
    const char *who;
    const float *points;
    const int64_t *first_idx, *num_pts;
    int N;
    int64_t P;
    int K;
    float *dists;      // full lists (dss_knn_points), else nullptr
    int64_t *idx;
    float r2;
    hipStream_t st;
    KnnWorkspace w;
    QueryPlan plan;
};

// One instantiation of knn_query_kernel<K, FULL, VIEW> / knn_query_coop_kernel<K, FULL, VIEW, SKIP> as data (the one-thread
// kernel has no SKIP parameter: it reads the skip structure whenever it is handed one)
struct QueryVariant {
    int k;
    bool full, view, skip;
};
using OneThreadKernel = decltype(&knn_query_kernel<8, false>);
using CoopKernel = decltype(&knn_query_coop_kernel<8, false>);

// The instantiations that exist, and no others (nullptr for any other combination):
//   K-th distance <8|16, false>, lists <8|12|16|40, true>, per camera <8, false, true>
static OneThreadKernel one_thread_kernel(const QueryVariant &v)
{
    if (v.view) return (v.k == 8 && !v.full) ? knn_query_kernel<8, false, true> : nullptr;
    if (v.full)
        return v.k == 8 ? knn_query_kernel<8, true>
                        : (v.k == 12 ? knn_query_kernel<12, true>
                                     : (v.k == 16 ? knn_query_kernel<16, true>
                                                  : (v.k == KNN_FULL_MAX_K ? knn_query_kernel<KNN_FULL_MAX_K, true> : nullptr)));
    return v.k == 8 ? knn_query_kernel<8, false> : (v.k == KNN_MAX_K ? knn_query_kernel<KNN_MAX_K, false> : nullptr);
}

template <int K, bool FULL, bool VIEW>
static CoopKernel coop_by_skip(bool skip)
{
    return skip ? knn_query_coop_kernel<K, FULL, VIEW, true> : knn_query_coop_kernel<K, FULL, VIEW, false>;
}
//   K-th distance <8|16, false>, lists <8|12|16, true>, per camera <8, false, true>, each with and without SKIP
static CoopKernel coop_kernel(const QueryVariant &v)
{
    if (v.view) return (v.k == 8 && !v.full) ? coop_by_skip<8, false, true>(v.skip) : nullptr;
    if (v.full)
        return v.k == 8 ? coop_by_skip<8, true, false>(v.skip)
                        : (v.k == 12 ? coop_by_skip<12, true, false>(v.skip) : (v.k == 16 ? coop_by_skip<16, true, false>(v.skip) : nullptr));
    return v.k == 8 ? coop_by_skip<8, false, false>(v.skip) : (v.k == KNN_MAX_K ? coop_by_skip<KNN_MAX_K, false, false>(v.skip) : nullptr);
}

static int no_query_kernel(const KnnCall &c, const QueryVariant &v)
{
    set_error("%s: internal error, no query kernel <%d, %d, %d, %d>", c.who, v.k, (int)v.full, (int)v.view, (int)v.skip);
    return DSS_ERR_UNSUPPORTED;
}

// The two query launch sites.  `out`: the K-th distance row(s) (nullptr with full lists).  role 0: the launch takes every
// cloud (and uses the skip structure where `dense_flag` is up); 1: only clouds without dense cells; 2: only clouds with.
// dk_out: the K-th distance itself (the unmasked search of the per-camera statistic); plain_stat / plain_dk: that search's
// two rows, read by the per-camera launch (`view`).
static int launch_one_thread(const KnnCall &c, const QueryVariant &v, dim3 grid, float *out, const KnnView &view, int role,
                             float *dk_out, const float *plain_stat, const float *plain_dk)
{
    const OneThreadKernel fn = one_thread_kernel(v);
    if (!fn) return no_query_kernel(c, v);
    hipLaunchKernelGGL(fn, grid, dim3(c.plan.one_block), 0, c.st, c.points, c.first_idx, c.num_pts, c.N, c.P, c.w.grids, c.w.stride,
                       c.w.offsets, c.w.sorted, c.K, out, c.dists, c.idx, c.r2, view, c.plan.skip ? c.w.boxes : nullptr,
                       c.plan.skip ? c.w.dense_flag : nullptr, role, dk_out, plain_stat, plain_dk);
    return DSS_OK;
}
// chunks: per-camera launch only, the query chunks per camera (its grid is persistent)
static int launch_coop(const KnnCall &c, const QueryVariant &v, dim3 grid, float *out, const KnnView &view, unsigned chunks,
                       int role, float *dk_out, const float *plain_stat, const float *plain_dk)
{
    const CoopKernel fn = coop_kernel(v);
    if (!fn) return no_query_kernel(c, v);
    hipLaunchKernelGGL(fn, grid, dim3(256), 0, c.st, c.points, c.first_idx, c.num_pts, c.N, c.P, c.w.grids, c.w.stride, c.w.offsets,
                       c.w.sorted, c.K, out, c.dists, c.idx, c.r2, view, chunks, c.plan.skip ? c.w.boxes : nullptr,
                       c.plan.skip ? c.w.dense_flag : nullptr, role, dk_out, plain_stat, plain_dk);
    return DSS_OK;
}

// Cell grid of every cloud and the points grouped by cell (w.grids, w.offsets, w.sorted); with `view`, the cameras' flags
static int build_grid(const KnnCall &c, const KnnView &view)
{
    const KnnWorkspace &w = c.w;
    const unsigned pb = (unsigned)((c.P + 255) / 256);
    if (c.P <= KNN_SMALL_P && c.N <= KNN_GRID_LDS && w.nblk <= KNN_SCAN1_BLOCKS) {
        // small inputs: four launches instead of eight (see knn_bbox_partial_kernel)
        int *partial = w.bbox;   // (N, KNN_BB_WGS, 6)
        const unsigned zero_wgs = (unsigned)((w.stride + 4095) / 4096);
        hipLaunchKernelGGL(knn_bbox_partial_kernel, dim3(KNN_BB_WGS + (zero_wgs ? zero_wgs : 1), c.N), dim3(256), 0, c.st, c.points,
                           c.first_idx, c.num_pts, c.P, partial, w.counts, w.stride);
        hipLaunchKernelGGL(knn_count_grid_kernel, dim3(pb), dim3(256), 0, c.st, c.points, c.first_idx, c.num_pts, c.N, c.P, partial,
                           knn_res_cap(c.P), w.grids, w.stride, w.counts, w.cell_of);
        hipLaunchKernelGGL(knn_scan_single_kernel, dim3(w.nblk, c.N), dim3(1024), 0, c.st, w.counts, w.grids, w.stride, w.offsets,
                           w.cursor);
        hipLaunchKernelGGL(knn_fill_kernel, dim3(pb), dim3(256), 0, c.st, c.points, c.first_idx, c.num_pts, c.N, c.P, w.cell_of,
                           w.stride, w.cursor, w.sorted, view);
        return DSS_OK;
    }
    if (hipMemsetAsync(w.counts, 0, w.cbytes, c.st) != hipSuccess) return check_launch("knn memset");
    if (int rc = launch_cloud_bbox(c.points, c.first_idx, c.num_pts, c.N, c.P, w.bbox, c.st)) return rc;
    hipLaunchKernelGGL(knn_grid_kernel, dim3((c.N + 63) / 64), dim3(64), 0, c.st, w.bbox, c.num_pts, c.N, knn_res_cap(c.P), w.grids);
    hipLaunchKernelGGL(knn_count_kernel, dim3(pb), dim3(256), 0, c.st, c.points, c.first_idx, c.num_pts, c.N, c.P, w.grids, w.stride,
                       w.counts, w.cell_of, w.rank_of);
    hipLaunchKernelGGL(knn_scan_local_kernel, dim3(w.nblk, c.N), dim3(256), 0, c.st, w.counts, w.grids, w.stride, w.nblk, w.offsets,
                       w.blk_tot);
    hipLaunchKernelGGL(knn_scan_add_kernel, dim3(w.nblk, c.N), dim3(256), 0, c.st, w.grids, w.stride, w.nblk, w.blk_tot, w.offsets,
                       w.cursor);
    hipLaunchKernelGGL(knn_fill_kernel, dim3(pb), dim3(256), 0, c.st, c.points, c.first_idx, c.num_pts, c.N, c.P, w.cell_of, w.stride,
                       w.offsets, w.sorted, view, w.rank_of);
    return DSS_OK;
}

// The list of dense cells, their sub-sort and the block boxes (see knn_subsort_kernel)
static void build_skip_structure(const KnnCall &c)
{
    const KnnWorkspace &w = c.w;
    hipLaunchKernelGGL(knn_dense_list_kernel, dim3((unsigned)((w.stride + 254) / 256), c.N), dim3(256), 0, c.st, w.grids, w.stride,
                       w.offsets, w.dense_list, w.n_dense, w.n_dense_pts);
    hipLaunchKernelGGL(knn_subsort_kernel, dim3(KNN_SUBSORT_WGS), dim3(KNN_SUBSORT_THREADS), 0, c.st, w.grids, w.stride, w.offsets,
                       c.first_idx, w.sorted, w.dense_list, w.n_dense, w.n_dense_pts, c.P, w.dense_flag);
    hipLaunchKernelGGL(knn_block_box_kernel, dim3((unsigned)((c.P / KNN_BLOCK + 256) / 256)), dim3(256), 0, c.st, w.sorted, c.P,
                       w.dense_flag, w.boxes);
}

// Every point among all the points of its cloud: `out` = the K-th distance row, or the lists of the call
static int query_plain(const KnnCall &c, float *out, float *dk_out)
{
    const QueryPlan &q = c.plan;
    const QueryVariant v = {q.k, c.dists != nullptr, false, q.skip};
    if (q.coop) return launch_coop(c, v, dim3(q.chunks), out, KnnView(), 0u, 0, dk_out, nullptr, nullptr);
    if (!q.skip || q.k > KNN_MAX_K) return launch_one_thread(c, v, dim3(q.one_grid), out, KnnView(), 0, dk_out, nullptr, nullptr);
    // a size at which the one-thread kernel is the choice for an evenly sampled cloud, K <= 16: clouds with dense cells go to
    // the cooperative kernel all the same (sixteen boxes tested per trip), as a second launch; each launch leaves at once
    // when the cloud is not its kind
    if (int rc = launch_one_thread(c, v, dim3(q.one_grid), out, KnnView(), 1, dk_out, nullptr, nullptr)) return rc;
    return launch_coop(c, v, dim3(q.chunks), out, KnnView(), 0u, 2, dk_out, nullptr, nullptr);
}

// K-th distance under per-camera culling (K <= 8: the variance-scale statistic): one grid row per camera
static int query_per_camera(const KnnCall &c, const KnnView &view, float *kth_sqdist)
{
    const QueryPlan &q = c.plan;
    const KnnWorkspace &w = c.w;
    // (1) the unmasked search of every point: statistic + K-th distance (see knn_view_shortcut)
    if (int rc = query_plain(c, w.plain_stat, w.plain_dk)) return rc;
    // (2) per camera: copy, or search again among the points the camera keeps
    const QueryVariant masked = {q.k, false, true, q.skip};
    if (q.coop) {
        // one cloud, several cameras: the grid covers one camera's chunks (see knn_query_coop_kernel)
        const dim3 grid = view.mode == 1 ? dim3(q.chunks < 16384u ? q.chunks : 16384u, view.n_cams > 1 ? 2u : 1u) : dim3(q.chunks);
        if (int rc = launch_coop(c, masked, grid, kth_sqdist, view, q.chunks, 0, nullptr, w.plain_stat, w.plain_dk)) return rc;
    } else {
        const dim3 grid(q.one_grid, view.mode == 1 ? (unsigned)view.n_cams : 1u);
        if (int rc = launch_one_thread(c, masked, grid, kth_sqdist, view, 0, nullptr, w.plain_stat, w.plain_dk)) return rc;
    }
    if (view.mode == 1)   // the rows of the cameras that drop nothing = the unmasked search
        hipLaunchKernelGGL(knn_view_rows_kernel, dim3((unsigned)((c.P + 1023) / 1024), (unsigned)view.n_cams), dim3(256), 0, c.st,
                           kth_sqdist, w.plain_stat, c.P, view.culls);
    return DSS_OK;
}

// grid build + query; exactly one of (kth_sqdist) / (dists, idx) is written.  radius > 0: the fixed-radius semantics of
// dss_knn_kth_sqdist_radius.  view.mode != 0: the per-camera search of view.n_cams cameras (view.culls is set here).
// Stages: validate -> carve the workspace, choose the plan -> clear the flags -> grid -> skip structure -> query.
static int knn_run(const char *who, const float *points, const int64_t *first_idx, const int64_t *num_pts, int N, int64_t P,
                   int K, float *kth_sqdist, float *dists, int64_t *idx, void *workspace, size_t workspace_bytes,
                   void *stream, float radius, KnnView view = KnnView())
{
    // ---- validate
    const bool full = dists != nullptr;
    if (N <= 0 || P < 0 || K < 1 || K > (full ? KNN_FULL_MAX_K : KNN_MAX_K)) {
        set_error("%s: bad sizes N=%d P=%lld K=%d (K <= %d)", who, N, (long long)P, K, full ? KNN_FULL_MAX_K : KNN_MAX_K);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return DSS_OK;
    if (!points || !first_idx || !num_pts || (!full && !kth_sqdist) || (full && !idx)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || workspace_bytes < dss_knn_workspace(N, P)) {
        set_error("%s: workspace too small", who);
        return DSS_ERR_WORKSPACE;
    }
    if (view.mode != 0) {
        if (view.n_cams > KNN_MAX_VIEW_CAMS) { set_error("%s: at most %d cameras", who, KNN_MAX_VIEW_CAMS); return DSS_ERR_UNSUPPORTED; }
        if (full || K > 8) { set_error("%s: the per-camera search is built for the K-th distance with K <= 8", who); return DSS_ERR_UNSUPPORTED; }
    }
    // ---- carve, plan
    const KnnCall c = {who, points, first_idx, num_pts, N, P, K, dists, idx, radius > 0.0f ? radius * radius : -1.0f,
                       as_stream(stream), carve_knn(workspace, N, P), plan_query(P, K, full)};
    // ---- clear the flags
    if (view.mode != 0) {
        view.culls = c.w.cam_flags;
        if (hipMemsetAsync(view.culls, 0, (size_t)view.n_cams * 4, c.st) != hipSuccess) return check_launch("knn view memset");
    }
    if (c.plan.skip && hipMemsetAsync(c.w.dense_flag, 0, KNN_DENSE_WORDS * 4, c.st) != hipSuccess) return check_launch("knn flag memset");
    // ---- build
    if (int rc = build_grid(c, view)) return rc;
    if (c.plan.skip) build_skip_structure(c);
    // ---- query
    if (int rc = view.mode != 0 ? query_per_camera(c, view, kth_sqdist) : query_plain(c, kth_sqdist, nullptr)) return rc;
    return check_launch(who);
}

extern "C" int dss_knn_kth_sqdist(const float *points, const int64_t *first_idx, const int64_t *num_pts, int N,
                                  int64_t P, int K, float *kth_sqdist, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    return knn_run("dss_knn_kth_sqdist", points, first_idx, num_pts, N, P, K, kth_sqdist, nullptr, nullptr, workspace,
                   workspace_bytes, stream, 0.0f);
}

extern "C" int dss_knn_points(const float *points, const int64_t *first_idx, const int64_t *num_pts, int N, int64_t P,
                              int K, float *dists, int64_t *idx, void *workspace, size_t workspace_bytes, void *stream)
{
    if (P == 0 && N > 0 && K >= 1 && K <= KNN_FULL_MAX_K) return DSS_OK;  // empty input: nothing to write
    if (!dists) {
        set_error("dss_knn_points: NULL tensor pointer");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    return knn_run("dss_knn_points", points, first_idx, num_pts, N, P, K, nullptr, dists, idx, workspace, workspace_bytes,
                   stream, 0.0f);
}

extern "C" int dss_cloud_mean_clamp(const float *values, const int64_t *first_idx, const int64_t *num_pts, int N,
                                    float scale, float lo, float hi, float fallback, int min_points, float *out,
                                    void *stream)
{
    if (N <= 0 || !values || !first_idx || !num_pts || !out) {
        set_error("dss_cloud_mean_clamp: bad arguments");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(cloud_mean_kernel, dim3(N), dim3(1024), 0, as_stream(stream), values, first_idx, num_pts, scale,
                       lo, hi, fallback, min_points, out);
    return check_launch("dss_cloud_mean_clamp");
}

// dss_cloud_mean_clamp under the reference's depth culling, for clouds whose culled points are masked instead of dropped
// (see renderable_sum_kernel).  values (Pw,) per WORLD point; shared_cloud = 1: one cloud of num_pts[0] points seen by N
// cameras; workspace: 512 N bytes (RENDERABLE_BLOCKS partial (sum, count) pairs of doubles per camera).
extern "C" int dss_renderable_mean_clamp(const float *values, const float *world, const float *V, const float *znear,
                                         const float *zfar, const int64_t *first_idx, const int64_t *num_pts, int N,
                                         int shared_cloud, float scale, float lo, float hi, float fallback, int min_points,
                                         int64_t values_cam_stride, float *out, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    if (N <= 0 || !values || !world || !V || !znear || !zfar || !first_idx || !num_pts || !out || !workspace ||
        workspace_bytes < (size_t)N * 16 * RENDERABLE_BLOCKS) {
        set_error("dss_renderable_mean_clamp: bad arguments (workspace of 512 N bytes)");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    double *sums = reinterpret_cast<double *>(workspace);
    hipLaunchKernelGGL(renderable_sum_kernel, dim3(RENDERABLE_BLOCKS, N), dim3(1024), 0, as_stream(stream), values, world, V, znear, zfar,
                       first_idx, num_pts, shared_cloud, scale, sums, values_cam_stride);
    hipLaunchKernelGGL(renderable_mean_kernel, dim3(1), dim3(64), 0, as_stream(stream), sums, N, lo, hi, fallback, min_points, out);
    return check_launch("dss_renderable_mean_clamp");
}

// dss_knn_kth_sqdist with the fixed-radius semantics of the reference's DEFAULT neighbour search: SurfaceSplatting is built
// with frnn_radius = 0.2 (rasterizer.py:110) and then calls frnn.frnn_grid_points(K = 7, r = frnn_radius) (:317, :373), which
// reports neighbours beyond r as -1 [third party, lxxue/FRNN, not vendored: behaviour as restated by tests/ref_loop/launcher.py];
// the statistic 0.5 * max over the K - 1 returned distances is then the farthest neighbour FOUND within r -- or -0.5 for an
// isolated point, which pulls the cloud's mean h down once points have drifted away from the surface.  radius <= 0: the plain
// K-th distance (the reference's knn_points branch, frnn_radius <= 0).
extern "C" int dss_knn_kth_sqdist_radius(const float *points, const int64_t *first_idx, const int64_t *num_pts, int N,
                                         int64_t P, int K, float radius, float *kth_sqdist, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    return knn_run("dss_knn_kth_sqdist_radius", points, first_idx, num_pts, N, P, K, kth_sqdist, nullptr, nullptr, workspace,
                   workspace_bytes, stream, radius);
}

// dss_knn_kth_sqdist[_radius] in the reference's ORDER under depth culling: filter_renderable extends the cloud to the
// cameras and drops, per camera, the points outside [znear, zfar] BEFORE the neighbour search (rasterizer.py:599, 236-240,
// 183-217, 310-326), so a point's neighbours are the ones the same camera keeps.  shared_cloud = 1: ONE cloud (N must be 1)
// seen by n_cams cameras; kth_sqdist (n_cams, P): row c = the statistic among the points camera c keeps (0 for the points it
// drops).  shared_cloud = 0: cloud n is seen by camera n (n_cams == N); kth_sqdist (P,).  K <= 8.  One grid build, one query
// launch with a grid row per camera.
extern "C" int dss_knn_kth_sqdist_view(const float *points, const int64_t *first_idx, const int64_t *num_pts, int N,
                                       int64_t P, int K, float radius, const float *V, const float *znear, const float *zfar,
                                       int n_cams, int shared_cloud, float *kth_sqdist, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    if (!V || !znear || !zfar || n_cams <= 0 || (shared_cloud ? N != 1 : n_cams != N)) {
        set_error("dss_knn_kth_sqdist_view: cameras missing, or the cloud / camera counts do not fit (shared: one cloud; else one camera per cloud)");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    KnnView view = {V, znear, zfar, shared_cloud ? 1 : 2, nullptr, n_cams};
    return knn_run("dss_knn_kth_sqdist_view", points, first_idx, num_pts, N, P, K, kth_sqdist, nullptr, nullptr, workspace,
                   workspace_bytes, stream, radius, view);
}

// ---------------------------------------------------------------------------------------------------------------
// Nearest point of ANOTHER cloud (dss_nearest_points) and the chamfer point term's gradient (dss_chamfer_backward): the
// 3-D metric of the reference's loop, Trainer.evaluate_3d (DSS/training/trainer.py:144-171) =
// pytorch3d.loss.chamfer_distance(target, model).  Every search above is a self query; here cloud n of x is searched
// in cloud n of y.  The grid of the TARGET y is built by build_grid, unchanged (same KnnGrid, same counting sort); only
// the query is new: one thread per query point of x, in input order, K = 1.
//
// Exactness.  The query's start cell is its position's cell CLAMPED into the target's grid (a query may lie outside the
// target's bounding box).  Ring 1 visits the 3x3x3 block around it, ring r the shell that grows the block to
// [c - r, c + r]^3, cut at the grid's sides.  Every point not yet visited lies in a cell beyond one of the block's faces
// that has cells behind it -- on the low x side: cell index < cx - r, hence x < F = minx + (cx - r) cell -- AND inside
// the grid's box [min, min + res cell] on the two other axes (the box holds every point: min is the clouds' own
// minimum, res cell >= 1.0001 extent).  Its distance to the query at its REAL position q is therefore at least
//     sqrt((qx - F)^2 + oy^2 + oz^2),     o = distance of q to the grid's box along that axis (0 when inside),
// and the smallest of these over the (at most six) open faces bounds everything unvisited.  Inside the box this is the
// self query's rule; outside, the `o` terms keep the bound close to the true distance, so a query 50 cells away stops
// after the rings that cover its nearest face region instead of walking the whole grid.  Nothing guarantees a hit in
// the first block: the best distance starts at +inf, empty rings go on until the bound passes it, and when no face is
// open (at the latest ring = res) every cell has been visited.  Rounding: each term is reduced by
// tol = 1e-6 (res cell + |q| + |min|) before it is squared, which exceeds the fp32 error of the cell assignment
// ((v - min) inv_cell, ~5 ulp of res cell), of F and of the subtraction (1 ulp of |F| + |q|) several times over, so an
// unvisited point's fp32 distance is strictly larger than the bound: the search stops at best <= bound^2 and an
// unvisited point can neither beat the result nor tie with it.  Among the visited candidates the order is
// (distance, id), the order of dss_knn_points: ties go to the smaller id whatever the cell order.  Distances are the
// difference form of knn_query_kernel's `consider` ("dx = q.x - qx ... d2 = dx * dx + dy * dy + dz * dz", built with
// -ffp-contract=off) on the world coordinates: (dx dx + dy dy) + dz dz, dx = x - y.
// A query that compares with nothing (NaN position) reports (0, -1) like a query whose target cloud is empty.
// ---------------------------------------------------------------------------------------------------------------
namespace dss {

__device__ __forceinline__ int nearest_start_cell(float v, float mn, float inv_cell, int res)
{
    // clamped as a float: the quotient of a far query (or of a degenerate grid, cell ~ 1e-12) does not fit an int
    return (int)fminf(fmaxf(floorf((v - mn) * inv_cell), 0.0f), (float)(res - 1));
}

// What the cross walks share, stated once for point_face_query and face_point_query.  nearest_query_kernel below keeps its
// own written-out copy of the same rules: routed through these functions it compiles to 78 instead of 70 VGPRs (six
// instead of seven wavefronts per SIMD), and no existing kernel is to change with this section.
// The searcher is a box [lo, hi] per axis (a query point: lo == hi).  tol: the rounding allowance of one axis; o2: the
// squared distance of the searcher to the grid's box along each axis, rounded down (see the exactness note above).
struct CrossGap { float tolx, toly, tolz, ox2, oy2, oz2; };
__device__ __forceinline__ CrossGap cross_gap(const KnnGrid &g, float span, float lox, float hix, float loy, float hiy, float loz, float hiz)
{
    CrossGap t;
    t.tolx = 1e-6f * (span + fmaxf(fabsf(lox), fabsf(hix)) + fabsf(g.minx));
    t.toly = 1e-6f * (span + fmaxf(fabsf(loy), fabsf(hiy)) + fabsf(g.miny));
    t.tolz = 1e-6f * (span + fmaxf(fabsf(loz), fabsf(hiz)) + fabsf(g.minz));
    const float ox = fmaxf(fmaxf(g.minx - hix, lox - (g.minx + span)) - t.tolx, 0.0f);
    const float oy = fmaxf(fmaxf(g.miny - hiy, loy - (g.miny + span)) - t.toly, 0.0f);
    const float oz = fmaxf(fmaxf(g.minz - hiz, loz - (g.minz + span)) - t.tolz, 0.0f);
    t.ox2 = ox * ox; t.oy2 = oy * oy; t.oz2 = oz * oz;
    return t;
}
// Squared distance from the searcher to everything outside the visited block of cells [x0, x1] x [y0, y1] x [z0, z1]
// (already cut at the grid's sides): the smallest over the block's open faces; +inf when no face is open.
__device__ __forceinline__ float cross_unvisited_b2(const KnnGrid &g, int res, const CrossGap &t, int x0, int x1, int y0, int y1, int z0,
                                                    int z1, float lox, float hix, float loy, float hiy, float loz, float hiz)
{
    float b2 = __builtin_huge_valf();
    if (x0 > 0) { const float d = fmaxf(lox - (g.minx + (float)x0 * g.cell) - t.tolx, 0.0f); b2 = fminf(b2, d * d + t.oy2 + t.oz2); }
    if (x1 < res - 1) { const float d = fmaxf((g.minx + (float)(x1 + 1) * g.cell) - hix - t.tolx, 0.0f); b2 = fminf(b2, d * d + t.oy2 + t.oz2); }
    if (y0 > 0) { const float d = fmaxf(loy - (g.miny + (float)y0 * g.cell) - t.toly, 0.0f); b2 = fminf(b2, d * d + t.ox2 + t.oz2); }
    if (y1 < res - 1) { const float d = fmaxf((g.miny + (float)(y1 + 1) * g.cell) - hiy - t.toly, 0.0f); b2 = fminf(b2, d * d + t.ox2 + t.oz2); }
    if (z0 > 0) { const float d = fmaxf(loz - (g.minz + (float)z0 * g.cell) - t.tolz, 0.0f); b2 = fminf(b2, d * d + t.ox2 + t.oy2); }
    if (z1 < res - 1) { const float d = fmaxf((g.minz + (float)(z1 + 1) * g.cell) - hiz - t.tolz, 0.0f); b2 = fminf(b2, d * d + t.ox2 + t.oy2); }
    return b2;
}
// The cells that grow the visited block from `old` to `now` (both cut at the grid's sides; old empty: x1 < x0), as ranges
// of the cell-sorted array: cells consecutive along x are consecutive in memory, so a row outside the old block is ONE
// range, and a row that crosses it contributes the cells in front of and behind it.
struct CellBlock { int x0, x1, y0, y1, z0, z1; };
template <typename Visit>
__device__ __forceinline__ void cross_visit_shell(const uint32_t *__restrict__ off, int res, const CellBlock &old, const CellBlock &now,
                                                  Visit visit)
{
    for (int z = now.z0; z <= now.z1; ++z)
        for (int y = now.y0; y <= now.y1; ++y) {
            const int c = (z * res + y) * res;
            if (z < old.z0 || z > old.z1 || y < old.y0 || y > old.y1) {
                visit(off[c + now.x0], off[c + now.x1 + 1]);
            } else {
                if (now.x0 < old.x0) visit(off[c + now.x0], off[c + old.x0]);
                if (now.x1 > old.x1) visit(off[c + old.x1 + 1], off[c + now.x1 + 1]);
            }
        }
}

__global__ __launch_bounds__(256) void nearest_query_kernel(const float *__restrict__ x, const int64_t *__restrict__ x_first,
                                                            const int64_t *__restrict__ x_num, int64_t Px,
                                                            const int64_t *__restrict__ y_first, const int64_t *__restrict__ y_num,
                                                            int N, const KnnGrid *__restrict__ grids, size_t stride,
                                                            const uint32_t *__restrict__ offsets, const float4 *__restrict__ sorted,
                                                            float *__restrict__ d2_out, int64_t *__restrict__ idx_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Px) return;
    const int n = find_cloud(i, x_first, x_num, N);
    if (n < 0 || y_num[n] <= 0) {   // slot of no cloud (its position is not read), or nothing to search
        d2_out[i] = 0.0f;
        idx_out[i] = -1;
        return;
    }
    const KnnGrid g = grids[n];
    const int64_t f0 = y_first[n];
    const uint32_t *off = offsets + (size_t)n * stride;
    const float qx = x[3 * i], qy = x[3 * i + 1], qz = x[3 * i + 2];
    const int res = g.res;
    const int cx = nearest_start_cell(qx, g.minx, g.inv_cell, res);
    const int cy = nearest_start_cell(qy, g.miny, g.inv_cell, res);
    const int cz = nearest_start_cell(qz, g.minz, g.inv_cell, res);
    const float span = (float)res * g.cell;
    const float tolx = 1e-6f * (span + fabsf(qx) + fabsf(g.minx)), toly = 1e-6f * (span + fabsf(qy) + fabsf(g.miny)),
                tolz = 1e-6f * (span + fabsf(qz) + fabsf(g.minz));
    // distance of the query to the grid's box along each axis, rounded down
    const float ox = fmaxf(fmaxf(g.minx - qx, qx - (g.minx + span)) - tolx, 0.0f);
    const float oy = fmaxf(fmaxf(g.miny - qy, qy - (g.miny + span)) - toly, 0.0f);
    const float oz = fmaxf(fmaxf(g.minz - qz, qz - (g.minz + span)) - tolz, 0.0f);
    const float ox2 = ox * ox, oy2 = oy * oy, oz2 = oz * oz;
    float best = __builtin_huge_valf();
    int bid = 0x7fffffff;
    auto consider = [&](const float4 q) __attribute__((always_inline)) {
        const float dx = qx - q.x, dy = qy - q.y, dz = qz - q.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int id = __float_as_int(q.w);
        const bool lt = (d2 < best) | ((d2 == best) & (id < bid));
        best = lt ? d2 : best;
        bid = lt ? id : bid;
    };
    // candidates [s, e) of the cell-sorted array, four per memory round trip (clamped loads: a repeated candidate
    // changes nothing when K = 1)
    auto visit = [&](uint32_t s, uint32_t e) __attribute__((always_inline)) {
        for (uint32_t j = s; j < e; j += 4) {
            const float4 q0 = sorted[f0 + j], q1 = sorted[f0 + min(j + 1, e - 1)], q2 = sorted[f0 + min(j + 2, e - 1)],
                         q3 = sorted[f0 + min(j + 3, e - 1)];
            consider(q0); consider(q1); consider(q2); consider(q3);
        }
    };
    for (int ring = 1; ring <= res; ++ring) {
        const int x0 = max(cx - ring, 0), x1 = min(cx + ring, res - 1);
        const int y0 = max(cy - ring, 0), y1 = min(cy + ring, res - 1);
        const int z0 = max(cz - ring, 0), z1 = min(cz + ring, res - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int c = (z * res + y) * res;
                // cells consecutive along x are consecutive in memory: a row of the first block, or of a y / z face of
                // the shell, is ONE range; the other rows of a shell contribute their two end cells
                if (ring == 1 || z == cz - ring || z == cz + ring || y == cy - ring || y == cy + ring) {
                    visit(off[c + x0], off[c + x1 + 1]);
                } else {
                    if (cx - ring >= 0) visit(off[c + cx - ring], off[c + cx - ring + 1]);
                    if (cx + ring < res) visit(off[c + cx + ring], off[c + cx + ring + 1]);
                }
            }
        // squared distance from the query's real position to everything not visited (see the exactness note above)
        float b2 = __builtin_huge_valf();
        if (cx - ring > 0) { const float d = fmaxf(qx - (g.minx + (float)(cx - ring) * g.cell) - tolx, 0.0f); b2 = fminf(b2, d * d + oy2 + oz2); }
        if (cx + ring < res - 1) { const float d = fmaxf((g.minx + (float)(cx + ring + 1) * g.cell) - qx - tolx, 0.0f); b2 = fminf(b2, d * d + oy2 + oz2); }
        if (cy - ring > 0) { const float d = fmaxf(qy - (g.miny + (float)(cy - ring) * g.cell) - toly, 0.0f); b2 = fminf(b2, d * d + ox2 + oz2); }
        if (cy + ring < res - 1) { const float d = fmaxf((g.miny + (float)(cy + ring + 1) * g.cell) - qy - toly, 0.0f); b2 = fminf(b2, d * d + ox2 + oz2); }
        if (cz - ring > 0) { const float d = fmaxf(qz - (g.minz + (float)(cz - ring) * g.cell) - tolz, 0.0f); b2 = fminf(b2, d * d + ox2 + oy2); }
        if (cz + ring < res - 1) { const float d = fmaxf((g.minz + (float)(cz + ring + 1) * g.cell) - qz - tolz, 0.0f); b2 = fminf(b2, d * d + ox2 + oy2); }
        if (b2 == __builtin_huge_valf() || best <= b2) break;
    }
    const bool found = bid != 0x7fffffff;
    d2_out[i] = found ? best : 0.0f;
    idx_out[i] = found ? (int64_t)bid - f0 : -1;
}

// Gradient of the chamfer point term for ONE point i of cloud set a (x or y) against set b, the index lists constant:
//     grad_a[i] = 2 ga[i] (a_i - b_nn(i))  +  sum over the points j of b whose nearest point is i of  2 gb[j] (a_i - b_j).
// The sum is many-to-one.  No atomics: order_ba lists b's packed ids sorted by (packed id of their nearest point in a, own
// id), so the contributors of i are one contiguous segment; the thread finds its start by binary search and adds the
// segment front to back, in double, rounding once -- the same bits on every run.  Pairs with idx < 0, and slots of no
// cloud, sort behind every real target and contribute nothing.
__device__ __forceinline__ int64_t chamfer_target(int64_t j, const int64_t *__restrict__ b_first, const int64_t *__restrict__ b_num,
                                                  const int64_t *__restrict__ a_first, int N, int64_t Pb,
                                                  const int64_t *__restrict__ idx_ba)
{
    if ((uint64_t)j >= (uint64_t)Pb) return 0x7fffffffffffffffll;
    const int m = find_cloud(j, b_first, b_num, N);
    const int64_t t = idx_ba[j];
    return (m < 0 || t < 0) ? 0x7fffffffffffffffll : a_first[m] + t;
}

__device__ __forceinline__ void chamfer_grad_point(int64_t i, const float *__restrict__ a, const float *__restrict__ b,
                                                   const int64_t *__restrict__ a_first, const int64_t *__restrict__ a_num,
                                                   const int64_t *__restrict__ b_first, const int64_t *__restrict__ b_num, int N,
                                                   int64_t Pb, const int64_t *__restrict__ idx_ab, const int64_t *__restrict__ idx_ba,
                                                   const int64_t *__restrict__ order_ba, const float *__restrict__ ga,
                                                   const float *__restrict__ gb, float *__restrict__ grad_a)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int n = find_cloud(i, a_first, a_num, N);
    if (n >= 0) {
        const double ax = (double)a[3 * i], ay = (double)a[3 * i + 1], az = (double)a[3 * i + 2];
        const int64_t t = idx_ab[i];
        const int64_t jn = b_first[n] + t;
        if (t >= 0 && jn < Pb) {
            const double w = 2.0 * (double)ga[i];
            s0 = w * (ax - (double)b[3 * jn]); s1 = w * (ay - (double)b[3 * jn + 1]); s2 = w * (az - (double)b[3 * jn + 2]);
        }
        int64_t lo = 0, hi = Pb;   // first k with target(order_ba[k]) >= i
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (chamfer_target(order_ba[mid], b_first, b_num, a_first, N, Pb, idx_ba) < i) lo = mid + 1;
            else hi = mid;
        }
        for (int64_t k = lo; k < Pb; ++k) {
            const int64_t j = order_ba[k];
            if (chamfer_target(j, b_first, b_num, a_first, N, Pb, idx_ba) != i) break;
            const double w = 2.0 * (double)gb[j];
            s0 += w * (ax - (double)b[3 * j]); s1 += w * (ay - (double)b[3 * j + 1]); s2 += w * (az - (double)b[3 * j + 2]);
        }
    }
    grad_a[3 * i] = (float)s0; grad_a[3 * i + 1] = (float)s1; grad_a[3 * i + 2] = (float)s2;
}

// one thread per point: threads [0, Px) write grad_x (when given), threads [Px, Px + Py) grad_y
__global__ __launch_bounds__(256) void chamfer_backward_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                               const int64_t *__restrict__ x_first, const int64_t *__restrict__ x_num, int64_t Px,
                                                               const int64_t *__restrict__ y_first, const int64_t *__restrict__ y_num, int64_t Py,
                                                               int N, const int64_t *__restrict__ idx_xy, const int64_t *__restrict__ idx_yx,
                                                               const int64_t *__restrict__ order_xy, const int64_t *__restrict__ order_yx,
                                                               const float *__restrict__ gx, const float *__restrict__ gy,
                                                               float *__restrict__ grad_x, float *__restrict__ grad_y)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < Px) {
        if (grad_x) chamfer_grad_point(t, x, y, x_first, x_num, y_first, y_num, N, Py, idx_xy, idx_yx, order_yx, gx, gy, grad_x);
    } else if (t < Px + Py) {
        if (grad_y) chamfer_grad_point(t - Px, y, x, y_first, y_num, x_first, x_num, N, Px, idx_yx, idx_xy, order_xy, gy, gx, grad_y);
    }
}

}  // namespace dss

extern "C" size_t dss_nearest_workspace(int N, int64_t Py) { return dss_knn_workspace(N, Py); }

extern "C" int dss_nearest_points(const float *x, const int64_t *x_first, const int64_t *x_num, int64_t Px, const float *y,
                                  const int64_t *y_first, const int64_t *y_num, int64_t Py, int N, float *d2, int64_t *idx,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "dss_nearest_points";
    if (N <= 0 || Px < 0 || Py < 0) {
        set_error("%s: bad sizes N=%d Px=%lld Py=%lld", who, N, (long long)Px, (long long)Py);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (Px == 0) return DSS_OK;
    if (!x || !x_first || !x_num || !y_first || !y_num || !d2 || !idx || (Py > 0 && !y)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || workspace_bytes < dss_nearest_workspace(N, Py)) {
        set_error("%s: workspace too small", who);
        return DSS_ERR_WORKSPACE;
    }
    // the target's grid, by the self query's build (the plan only matters to the queries above: none is launched)
    const KnnCall c = {who, y, y_first, y_num, N, Py, 1, nullptr, nullptr, -1.0f, as_stream(stream), carve_knn(workspace, N, Py),
                       plan_query(Py, 1, false)};
    if (Py > 0)
        if (int rc = build_grid(c, KnnView())) return rc;
    // small inputs: one wavefront per workgroup, so that the wavefronts spread over all CUs (as plan_query does)
    const unsigned block = Px <= 131072 ? 64u : 256u;
    hipLaunchKernelGGL(nearest_query_kernel, dim3((unsigned)((Px + block - 1) / block)), dim3(block), 0, c.st, x, x_first, x_num, Px,
                       y_first, y_num, N, c.w.grids, c.w.stride, c.w.offsets, c.w.sorted, d2, idx);
    return check_launch(who);
}

extern "C" int dss_chamfer_backward(const float *x, const float *y, const int64_t *x_first, const int64_t *x_num, int64_t Px,
                                    const int64_t *y_first, const int64_t *y_num, int64_t Py, int N, const int64_t *idx_xy,
                                    const int64_t *idx_yx, const int64_t *order_xy, const int64_t *order_yx, const float *gx,
                                    const float *gy, float *grad_x, float *grad_y, void *stream)
{
    const char *who = "dss_chamfer_backward";
    if (N <= 0 || Px < 0 || Py < 0) {
        set_error("%s: bad sizes N=%d Px=%lld Py=%lld", who, N, (long long)Px, (long long)Py);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (Px + Py == 0 || (!grad_x && !grad_y)) return DSS_OK;
    if (!x_first || !x_num || !y_first || !y_num || (Px > 0 && (!x || !idx_xy || !gx)) || (Py > 0 && (!y || !idx_yx || !gy)) ||
        (grad_x && Py > 0 && !order_yx) || (grad_y && Px > 0 && !order_xy)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const int64_t blocks = (Px + Py + 255) / 256;
    if (blocks > 0x7fffffffll) { set_error("%s: too many points", who); return DSS_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(chamfer_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, y, x_first, x_num, Px,
                       y_first, y_num, Py, N, idx_xy, idx_yx, order_xy, order_yx, gx, gy, grad_x, grad_y);
    return check_launch(who);
}

// ---------------------------------------------------------------------------------------------------------------
// Point-to-mesh distance (dss_point_face_distance, dss_face_point_distance, dss_mesh_distance_backward): the p2f columns
// of the reference's evaluation row (scripts/evaluatePointClouds.py:52,103-132) and the surface term
// pytorch3d.loss.point_mesh_face_distance.  Cloud n is measured against mesh n.  The code lives in this file because
// both searches use build_grid as it stands (file-static): over the triangles' centroids one way, over the points the
// other.
//
// The distance (mesh_d2), fp32, no contraction, correctly rounded division, dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z:
//   seg(q, P, R): p0 = the lexicographically smaller endpoint (x, then y, then z, by value), e = p1 - p0, w = q - p0,
//       ee = dot(e, e), we = dot(w, e);  we <= 0 or ee == 0: r = w;  we >= ee: r = q - p1;  else t = we / ee, r = w - t e;
//       result dot(r, r)
//   interior: e0 = B - A, e1 = C - A, n = e0 x e1, nn = dot(n, n); for A->B, B->C, C->A: s = dot((R - P) x (q - P), n);
//       inside = nn > 0 and all three s > 0;  plane = (h h) / nn, h = dot(q - A, n)
//   d2 = the first minimum under `<` of seg(A,B), seg(B,C), seg(C,A), inside ? plane : +inf, starting from +inf: a NaN
//       never wins.  An edge shared by two faces gives both the same bits (its endpoints are ordered by position, not by
//       the face's winding), so "ties go to the smaller face id" is meaningful; a degenerate triangle is the union of its
//       edges without any threshold.
//
// No face id outside [0, F) and no vertex id outside [0, V) reaches a load: mesh_load_face is the ONLY function that reads
// `verts` through `faces`; it is called with 0 <= f < F (every caller checks, stated at the call), reads the three ids of
// row f, and returns false BEFORE any vertex load when one of them is outside [0, V); it also returns false for a face
// with a non-finite vertex.  A face it refuses is ABSENT: its centroid is written as NaN (knn_box_reduce passes NaN over,
// so the grid's box does not see it; knn_cell_of clamps whatever cell a NaN converts to into the grid), its radius as -1,
// its record in cell order carries radius -1 and no vertex, and the large list never receives it.
//
// The error of mesh_d2 against the exact distance D.  The segment terms lose c eps (D^2 + L D + eps L^2), L = D + longest
// edge, eps = 2^-23 (the middle term is the cancellation in w - t e).  The PLANE term is worse conditioned: n = e0 x e1 is
// a difference of products of size |e0| |e1|, so its direction is off by eps kappa, kappa = (longest edge)^2 / |n| (1 for
// an equilateral-ish triangle, ~aspect for a sliver); h = dot(q - A, n) and the three side tests inherit that, and a
// query a wrongly signed side test lets into the plane branch is within eps kappa |q - A| of the edge.  Together
//     |d2 - D^2| <= E(D) = c eps kappa (D^2 + L D + eps kappa L^2)
// with c <= 1 measured on every scene of tests/test_mesh_distance_cpu.py, slivers of aspect 1 to 1e6 sampled ABOVE THEIR
// INTERIORS included (without kappa the same samples give c = 12 at aspect 100 and 1e4 at aspect 1e4); c = 8 is taken
// below.  mesh_kappa computes kappa in fp32 with the operations of mesh_d2's own nn: nn == 0 means the plane branch is
// never taken (kappa = 1); an nn too small to carry its digits counts as unbounded.
//
// Point -> face.  mesh_prep writes, per face, the centroid c = ((A + B) + C) / 3, the radius R_f >= max |vertex - c|
// (rounded up) and kappa_f; build_grid sorts the centroids; mesh_classify sends the faces with R_f > mult * cell, and the
// faces with kappa_f > MESH_KAPPA_MAX, to their mesh's LARGE LIST (length counted on the device, never read by the host)
// and takes R_grid = max R_f and K_grid = max kappa_f of the others; mesh_gather writes the nine floats of every face in
// CELL ORDER (48 bytes per face: three float4 with radius and id) so that the walk reads records, not indices.  A face of
// the large list keeps its centroid in the grid (classification needs the cell size, so it comes after the build): its
// record carries radius -2 and the walk passes it over; one huge triangle therefore stretches the centroids' box only by
// its centroid, not by its vertices.  The query is nearest_query_kernel's ring walk (clamped start cell, `o` terms, tol),
// over centroids.  Exactness: after a ring, every unvisited centroid is at least b away from q (the argument above
// nearest_query_kernel, b2 = b^2 computed there); its triangle lies within R_grid of the centroid, so its true distance is
// D >= lim = b - R_grid, and its computed d2 >= D^2 - E(D) with kappa <= K_grid and longest edge <= 2 R_grid.
// D^2 - E(D) grows with D once D > c eps kappa R_grid, so with
//     floor = lim^2 - 2e-6 K (lim + 2 R_grid)^2,   lim = 0.999999 sqrt(b2) - R_grid  (R_grid carries its own 1e-6 inflation)
// every unvisited triangle computes d2 >= floor: 2e-6 K s^2 = 16.8 eps K s^2 >= 8 eps K (2 lim^2 + 2 R lim + eps K s^2) as
// long as 8 eps K <= 0.8, and beyond that 2e-6 K >= 1 makes the floor negative.  For lim below c eps K R_grid the floor is
// negative too and nothing stops.  The walk stops at best < floor, strictly: an unvisited triangle neither beats the result
// nor ties with it.  The same floor, from a candidate's own centroid distance, rejects it before its record is loaded.
// Faces of the large list are tested by every query of the mesh, by brute force, whatever their kappa.  Among everything
// tested the order is (d2, face id).
//
// Face -> point.  The cloud's ordinary point grid; one WAVEFRONT per triangle (candidate counts differ by orders of
// magnitude: two triangles under 100,000 points is legal input), lanes stride the candidates of a row of cells, one
// cross-lane (d2, id) minimum at the end.  Ring 0 is the block of cells the triangle's bounding box covers (clamped),
// ring r grows it by r cells on every side.  An unvisited point lies in a cell beyond an open side of the block -- low
// x: x < F = minx + X0 cell -- and inside the grid's box on the other axes; the triangle lies inside its bounding box;
// so their distance is at least sqrt(gap^2 + oy^2 + oz^2), gap = box.lo.x - F, o = distance between the triangle's box
// and the grid's box along that axis, each reduced by tol first as in nearest_query_kernel.  floor as above with
// lim = 0.999999 sqrt(b2), the longest edge bounded by the box diagonal and K = the wavefront's own triangle's kappa: a
// sliver of kappa above 5e5 never stops early and compares with every point of its cloud.
// ---------------------------------------------------------------------------------------------------------------
namespace dss {

struct MeshTri { float ax, ay, az, bx, by, bz, cx, cy, cz; };

__device__ __forceinline__ bool mesh_finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

// The one reader of vertices through face ids.  REQUIRES 0 <= f < F.
__device__ __forceinline__ bool mesh_load_face(int64_t f, const int64_t *__restrict__ faces, const float *__restrict__ verts,
                                               int64_t V, MeshTri &t)
{
    const int64_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if ((uint64_t)ia >= (uint64_t)V || (uint64_t)ib >= (uint64_t)V || (uint64_t)ic >= (uint64_t)V) return false;
    t.ax = verts[3 * ia]; t.ay = verts[3 * ia + 1]; t.az = verts[3 * ia + 2];
    t.bx = verts[3 * ib]; t.by = verts[3 * ib + 1]; t.bz = verts[3 * ib + 2];
    t.cx = verts[3 * ic]; t.cy = verts[3 * ic + 1]; t.cz = verts[3 * ic + 2];
    return mesh_finite(t.ax) && mesh_finite(t.ay) && mesh_finite(t.az) && mesh_finite(t.bx) && mesh_finite(t.by) && mesh_finite(t.bz) &&
           mesh_finite(t.cx) && mesh_finite(t.cy) && mesh_finite(t.cz);
}

// The arithmetic of the distance, once, for float (the searches) and double (the backward's closest point)
template <typename T>
__device__ __forceinline__ T mesh_dot(T ax, T ay, T az, T bx, T by, T bz) { return (ax * bx + ay * by) + az * bz; }

// seg(q, P, R) -> squared distance; t_out = parameter along p0 -> p1, swapped = (p0 is R)
template <typename T>
__device__ __forceinline__ T mesh_seg(T qx, T qy, T qz, T px, T py, T pz, T rx, T ry, T rz, T &t_out, bool &swapped)
{
    const bool sw = (rx < px) | ((rx == px) & ((ry < py) | ((ry == py) & (rz < pz))));
    const T p0x = sw ? rx : px, p0y = sw ? ry : py, p0z = sw ? rz : pz;
    const T p1x = sw ? px : rx, p1y = sw ? py : ry, p1z = sw ? pz : rz;
    const T ex = p1x - p0x, ey = p1y - p0y, ez = p1z - p0z;
    const T wx = qx - p0x, wy = qy - p0y, wz = qz - p0z;
    const T ee = mesh_dot(ex, ey, ez, ex, ey, ez), we = mesh_dot(wx, wy, wz, ex, ey, ez);
    T rx_, ry_, rz_, t;
    if ((we <= (T)0) | (ee == (T)0)) { rx_ = wx; ry_ = wy; rz_ = wz; t = (T)0; }
    else if (we >= ee) { rx_ = qx - p1x; ry_ = qy - p1y; rz_ = qz - p1z; t = (T)1; }
    else { t = we / ee; rx_ = wx - t * ex; ry_ = wy - t * ey; rz_ = wz - t * ez; }
    t_out = t;
    swapped = sw;
    return mesh_dot(rx_, ry_, rz_, rx_, ry_, rz_);
}

// s = dot((R - P) x (q - P), n)
template <typename T>
__device__ __forceinline__ T mesh_side(T qx, T qy, T qz, T px, T py, T pz, T rx, T ry, T rz, T nx, T ny, T nz)
{
    const T ux = rx - px, uy = ry - py, uz = rz - pz, vx = qx - px, vy = qy - py, vz = qz - pz;
    return mesh_dot(uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx, nx, ny, nz);
}

// d2 of the definition; WEIGHTS: also the barycentric weights (wa, wb, wc) of the closest point, of the first minimum
// in the order AB, BC, CA, plane
template <typename T, bool WEIGHTS>
__device__ __forceinline__ T mesh_d2(T qx, T qy, T qz, T ax, T ay, T az, T bx, T by, T bz, T cx, T cy, T cz, T &wa, T &wb, T &wc)
{
    const T inf = (T)__builtin_huge_valf();
    T best = inf;
    T t0, t1, t2;
    bool s0, s1, s2;
    const T dab = mesh_seg(qx, qy, qz, ax, ay, az, bx, by, bz, t0, s0);
    const T dbc = mesh_seg(qx, qy, qz, bx, by, bz, cx, cy, cz, t1, s1);
    const T dca = mesh_seg(qx, qy, qz, cx, cy, cz, ax, ay, az, t2, s2);
    const T e0x = bx - ax, e0y = by - ay, e0z = bz - az, e1x = cx - ax, e1y = cy - ay, e1z = cz - az;
    const T nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
    const T nn = mesh_dot(nx, ny, nz, nx, ny, nz);
    const T sab = mesh_side(qx, qy, qz, ax, ay, az, bx, by, bz, nx, ny, nz);
    const T sbc = mesh_side(qx, qy, qz, bx, by, bz, cx, cy, cz, nx, ny, nz);
    const T sca = mesh_side(qx, qy, qz, cx, cy, cz, ax, ay, az, nx, ny, nz);
    const bool inside = (nn > (T)0) & (sab > (T)0) & (sbc > (T)0) & (sca > (T)0);
    const T h = mesh_dot(qx - ax, qy - ay, qz - az, nx, ny, nz);
    const T plane = inside ? (h * h) / nn : inf;
    int win = -1;
    if (dab < best) { best = dab; win = 0; }
    if (dbc < best) { best = dbc; win = 1; }
    if (dca < best) { best = dca; win = 2; }
    if (plane < best) { best = plane; win = 3; }
    if (WEIGHTS) {
        wa = (T)1; wb = (T)0; wc = (T)0;   // (nothing won: a NaN pair, which no index list names)
        if (win == 0) { const T u = s0 ? (T)1 - t0 : t0; wa = (T)1 - u; wb = u; wc = (T)0; }          // u = weight of the edge's second vertex
        if (win == 1) { const T u = s1 ? (T)1 - t1 : t1; wb = (T)1 - u; wc = u; wa = (T)0; }
        if (win == 2) { const T u = s2 ? (T)1 - t2 : t2; wc = (T)1 - u; wa = u; wb = (T)0; }
        if (win == 3) { wa = sbc / nn; wb = sca / nn; wc = sab / nn; }   // s of the edge opposite a vertex = its weight * nn
    }
    return best;
}

__device__ __forceinline__ float mesh_d2f(float qx, float qy, float qz, const MeshTri &t)
{
    float wa, wb, wc;
    return mesh_d2<float, false>(qx, qy, qz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, wa, wb, wc);
}

// Every triangle of kappa <= `kappa` and longest edge <= edge_max whose reference point (its centroid, at most `reach` from
// its vertices; or the triangle itself, reach = 0) is at least sqrt(b2) away computes d2 >= the returned value (see the
// exactness note above).  Point -> face: reach = R_grid, edge_max = 2 R_grid, kappa = K_grid; face -> point: 0, the box
// diagonal, the triangle's own kappa.
__device__ __forceinline__ float mesh_floor(float b2, float reach, float edge_max, float kappa)
{
    const float lim = sqrtf(b2) * 0.999999f - reach;
    const float s = lim + edge_max;
    return lim > 0.0f ? lim * lim - (2e-6f * kappa) * (s * s) : -1.0f;
}

// kappa = (longest edge)^2 / |n| >= 1, rounded up: the conditioning of the plane term (see the error note above).  nn is
// mesh_d2's own expression, so nn == 0 here means the plane branch is never taken there: kappa = 1.  An nn below 1e-30
// (triangles a few 1e-8 across) loses digits to underflow: +inf, no bound is claimed.
__device__ __forceinline__ float mesh_kappa(const MeshTri &t)
{
    const float e0x = t.bx - t.ax, e0y = t.by - t.ay, e0z = t.bz - t.az, e1x = t.cx - t.ax, e1y = t.cy - t.ay, e1z = t.cz - t.az;
    const float e2x = t.cx - t.bx, e2y = t.cy - t.by, e2z = t.cz - t.bz;
    const float nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
    const float nn = mesh_dot(nx, ny, nz, nx, ny, nz);
    const float l2 = fmaxf(fmaxf(mesh_dot(e0x, e0y, e0z, e0x, e0y, e0z), mesh_dot(e1x, e1y, e1z, e1x, e1y, e1z)),
                           mesh_dot(e2x, e2y, e2z, e2x, e2y, e2z));
    if (nn == 0.0f) return 1.0f;
    if (!(nn >= 1e-30f)) return __builtin_huge_valf();
    const float k = l2 / sqrtf(nn) * 1.01f;
    return k >= 1.0f ? k : (k == k ? 1.0f : __builtin_huge_valf());
}

// Faces with R_f above MESH_LARGE_QUARTERS / 4 cells go to the large list (DSS_OPT_MESH_LARGE overrides, for A/B runs:
// tools/mesh_distance_timing.py).  Any value is exact; it trades the walk's reach R_grid against the list's length.
#define MESH_LARGE_QUARTERS 8
// and so do faces whose kappa exceeds this: the walk's floor loses 2e-6 K_grid of (lim + 2 R_grid)^2, and a single sliver
// must not take that from every query of its mesh
#define MESH_KAPPA_MAX 256.0f
#define MESH_ABSENT (-1.0f)   // radius of a face that is not searched through the grid: absent (-1) or on the large list (-2)

// per packed face slot: centroid (NaN when absent / not a grid face) and radius
__global__ __launch_bounds__(256) void mesh_prep_kernel(const float *__restrict__ verts, int64_t V, const int64_t *__restrict__ faces,
                                                        const int64_t *__restrict__ f_first, const int64_t *__restrict__ f_num, int N,
                                                        int64_t F, float *__restrict__ cent, float *__restrict__ rf, float *__restrict__ kap)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float nan = __builtin_nanf("");
    float cx = nan, cy = nan, cz = nan, r = MESH_ABSENT, k = 1.0f;
    MeshTri t;
    if (find_cloud(f, f_first, f_num, N) >= 0 && mesh_load_face(f, faces, verts, V, t)) {   // (0 <= f < F)
        k = mesh_kappa(t);
        cx = ((t.ax + t.bx) + t.cx) / 3.0f; cy = ((t.ay + t.by) + t.cy) / 3.0f; cz = ((t.az + t.bz) + t.cz) / 3.0f;
        const float da = mesh_dot(t.ax - cx, t.ay - cy, t.az - cz, t.ax - cx, t.ay - cy, t.az - cz);
        const float db = mesh_dot(t.bx - cx, t.by - cy, t.bz - cz, t.bx - cx, t.by - cy, t.bz - cz);
        const float dc = mesh_dot(t.cx - cx, t.cy - cy, t.cz - cz, t.cx - cx, t.cy - cy, t.cz - cz);
        r = sqrtf(fmaxf(fmaxf(da, db), dc)) * 1.000001f + 1e-30f;   // rounded up, and > 0 (R_grid == 0 means "no grid face")
        if (!(mesh_finite(cx) && mesh_finite(cy) && mesh_finite(cz) && mesh_finite(r))) {
            cx = cy = cz = nan;                 // sums that overflow: off the grid, onto the large list
            r = __builtin_huge_valf();
        }
    }
    cent[3 * f] = cx; cent[3 * f + 1] = cy; cent[3 * f + 2] = cz;
    rf[f] = r;
    kap[f] = k;
}

// after build_grid: large and ill-conditioned faces to their mesh's list, R_grid and K_grid of the others.  per_mesh: (N, 3)
// ints = {bits of R_grid, length of the large list, bits of K_grid}, zeroed before.  quarter_cells: the multiple, in
// quarters of a cell.
__global__ __launch_bounds__(256) void mesh_classify_kernel(const int64_t *__restrict__ f_first, const int64_t *__restrict__ f_num, int N,
                                                            int64_t F, const KnnGrid *__restrict__ grids, float quarter_cells,
                                                            float *__restrict__ rf, const float *__restrict__ kap, int *__restrict__ per_mesh,
                                                            int *__restrict__ large)
{
    // (no early return: every lane takes part in the wavefront's reductions below)
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int m = f < F ? find_cloud(f, f_first, f_num, N) : -1;
    const float r = m >= 0 ? rf[f] : MESH_ABSENT;
    const float k = m >= 0 ? kap[f] : 1.0f;
    const bool usable = r >= 0.0f;
    const bool in_grid = usable && r <= 0.25f * quarter_cells * grids[m].cell && k <= MESH_KAPPA_MAX;
    // R_grid and K_grid: one pair of atomics per wavefront and mesh among its lanes, not per face (one atomic per face is
    // F same-address atomics in a row: 1.1 ms each at 100,000 faces, as knn_bbox_kernel found for the box)
    unsigned long long todo = __ballot(in_grid);
    while (todo != 0ull) {   // (wave-uniform)
        const int leader = __builtin_ctzll(todo);
        const int lm = __shfl(m, leader);
        const bool mine = in_grid && m == lm;
        int vr = mine ? __float_as_int(r) : 0, vk = mine ? __float_as_int(k) : 0;   // (r > 0, k >= 1: positive floats order like their bits)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            vr = max(vr, __shfl_xor(vr, o));
            vk = max(vk, __shfl_xor(vk, o));
        }
        if (lane == leader) {
            atomicMax(&per_mesh[3 * lm], vr);
            atomicMax(&per_mesh[3 * lm + 2], vk);
        }
        todo &= ~__ballot(mine);
    }
    if (usable && !in_grid) {
        // f_first[m] + pos < F: the faces counted here are slots of mesh m below F, and pos counts fewer than all of them
        // (checked all the same: a negative f_first is merely wrong input, the query kernel refuses such a mesh)
        const int pos = atomicAdd(&per_mesh[3 * m + 1], 1);
        const int64_t at = f_first[m] + pos;
        if ((uint64_t)at < (uint64_t)F) large[at] = (int)f;
        rf[f] = -2.0f;
    }
}

// the faces' vertices in cell order: rec[3 j .. 3 j + 2] = (A, B.x) (B.yz, C.xy) (C.z, radius or -1, packed face id, 0)
__global__ __launch_bounds__(256) void mesh_gather_kernel(const float *__restrict__ verts, int64_t V, const int64_t *__restrict__ faces,
                                                          const int64_t *__restrict__ f_first, const int64_t *__restrict__ f_num, int N,
                                                          int64_t F, const float4 *__restrict__ sorted, const float *__restrict__ rf,
                                                          float4 *__restrict__ rec)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= F) return;
    if (find_cloud(j, f_first, f_num, N) < 0) return;   // (a slot of no mesh: `sorted` holds nothing there)
    const int id = __float_as_int(sorted[j].w);
    MeshTri t = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float r = MESH_ABSENT;
    if ((uint32_t)id < (uint64_t)F) {                  // (0 <= id < F before rf and mesh_load_face see it)
        r = rf[id];
        if (!(r >= 0.0f && mesh_load_face(id, faces, verts, V, t))) r = MESH_ABSENT;
    }
    rec[3 * j] = make_float4(t.ax, t.ay, t.az, t.bx);
    rec[3 * j + 1] = make_float4(t.by, t.bz, t.cx, t.cy);
    rec[3 * j + 2] = make_float4(t.cz, r, __int_as_float(id), 0.0f);
}

__global__ __launch_bounds__(256) void point_face_query_kernel(const float *__restrict__ x, const int64_t *__restrict__ p_first,
                                                               const int64_t *__restrict__ p_num, int64_t P,
                                                               const float *__restrict__ verts, int64_t V, const int64_t *__restrict__ faces,
                                                               const int64_t *__restrict__ f_first, const int64_t *__restrict__ f_num,
                                                               int64_t F, int N, const KnnGrid *__restrict__ grids, size_t stride,
                                                               const uint32_t *__restrict__ offsets, const float4 *__restrict__ sorted,
                                                               const float4 *__restrict__ rec, const int *__restrict__ per_mesh,
                                                               const int *__restrict__ large, float *__restrict__ d2_out,
                                                               int64_t *__restrict__ idx_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int n = find_cloud(i, p_first, p_num, N);
    int64_t f0 = 0, fn = 0;
    if (n >= 0) { f0 = f_first[n]; fn = f_num[n]; }
    if (n < 0 || fn <= 0 || f0 < 0 || f0 + fn > F) {   // slot of no cloud (its position is not read), or nothing to search
        d2_out[i] = 0.0f;
        idx_out[i] = -1;
        return;
    }
    const float qx = x[3 * i], qy = x[3 * i + 1], qz = x[3 * i + 2];
    float best = __builtin_huge_valf();
    int bid = 0x7fffffff;
    auto consider = [&](const MeshTri &t, int id) __attribute__((always_inline)) {
        const float d2 = mesh_d2f(qx, qy, qz, t);
        const bool lt = (d2 < best) | ((d2 == best) & (id < bid));
        best = lt ? d2 : best;
        bid = lt ? id : bid;
    };
    // the large list first: it seeds `best` for the walk's rejects
    const int n_large = min(max(per_mesh[3 * n + 1], 0), (int)min(fn, (int64_t)0x7fffffff));
    for (int k = 0; k < n_large; ++k) {
        const int f = large[f0 + k];
        MeshTri t;
        if ((uint32_t)f < (uint64_t)F && mesh_load_face(f, faces, verts, V, t)) consider(t, f);   // (0 <= f < F)
    }
    const float rgrid = __int_as_float(per_mesh[3 * n]), kgrid = __int_as_float(per_mesh[3 * n + 2]);
    if (rgrid > 0.0f) {   // (0: no face of this mesh is searched through the grid)
        const KnnGrid g = grids[n];
        const uint32_t *off = offsets + (size_t)n * stride;
        const int res = g.res;
        const int cx = nearest_start_cell(qx, g.minx, g.inv_cell, res);
        const int cy = nearest_start_cell(qy, g.miny, g.inv_cell, res);
        const int cz = nearest_start_cell(qz, g.minz, g.inv_cell, res);
        const CrossGap gap = cross_gap(g, (float)res * g.cell, qx, qx, qy, qy, qz, qz);
        const float edge_max = 2.0f * rgrid;
        auto visit = [&](uint32_t s, uint32_t e) __attribute__((always_inline)) {
            for (uint32_t j = s; j < e; ++j) {
                const float4 c = sorted[f0 + j];
                const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                // (a NaN centroid -- an absent face, or one whose sums overflowed -- fails this test and is passed over; a face
                // of the large list has a finite centroid and is passed over by its record's radius below)
                if (!(mesh_floor((dx * dx + dy * dy) + dz * dz, rgrid, edge_max, kgrid) <= best)) continue;
                const float4 r0 = rec[3 * (f0 + j)], r1 = rec[3 * (f0 + j) + 1], r2 = rec[3 * (f0 + j) + 2];
                if (!(r2.y >= 0.0f)) continue;
                const MeshTri t = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
                consider(t, __float_as_int(r2.z));
            }
        };
        CellBlock old = {0, -1, 0, -1, 0, -1};
        for (int ring = 1; ring <= res; ++ring) {
            const CellBlock now = {max(cx - ring, 0), min(cx + ring, res - 1), max(cy - ring, 0), min(cy + ring, res - 1),
                                   max(cz - ring, 0), min(cz + ring, res - 1)};
            cross_visit_shell(off, res, old, now, visit);
            old = now;
            // squared distance from the query to every unvisited CENTROID (nearest_query_kernel's bound)
            const float b2 = cross_unvisited_b2(g, res, gap, now.x0, now.x1, now.y0, now.y1, now.z0, now.z1, qx, qx, qy, qy, qz, qz);
            if (b2 == __builtin_huge_valf() || best < mesh_floor(b2, rgrid, edge_max, kgrid)) break;
            if (!(qx == qx && qy == qy && qz == qz)) break;   // a NaN query compares with nothing: no ring changes that
        }
    }
    // (a d2 that is not below +inf is no answer: a NaN query's minimum stays at the +inf it started from)
    const bool found = bid != 0x7fffffff && best < __builtin_huge_valf();
    d2_out[i] = found ? best : 0.0f;
    idx_out[i] = found ? (int64_t)bid - f0 : -1;
}

// one wavefront per face; 256-thread workgroups hold four faces
__global__ __launch_bounds__(256) void face_point_query_kernel(const float *__restrict__ verts, int64_t V, const int64_t *__restrict__ faces,
                                                               const int64_t *__restrict__ f_first, const int64_t *__restrict__ f_num,
                                                               int64_t F, const int64_t *__restrict__ p_first,
                                                               const int64_t *__restrict__ p_num, int64_t P, int N,
                                                               const KnnGrid *__restrict__ grids, size_t stride,
                                                               const uint32_t *__restrict__ offsets, const float4 *__restrict__ sorted,
                                                               float *__restrict__ d2_out, int64_t *__restrict__ idx_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (f >= F) return;
    const int m = find_cloud(f, f_first, f_num, N);
    MeshTri t;
    int64_t p0 = 0, pn = 0;
    if (m >= 0) { p0 = p_first[m]; pn = p_num[m]; }
    // (wave-uniform) a slot of no mesh, an empty or misplaced cloud, an absent face
    if (m < 0 || pn <= 0 || p0 < 0 || p0 + pn > P || !mesh_load_face(f, faces, verts, V, t)) {   // (0 <= f < F)
        if (lane == 0) { d2_out[f] = 0.0f; idx_out[f] = -1; }
        return;
    }
    const KnnGrid g = grids[m];
    const uint32_t *off = offsets + (size_t)m * stride;
    const int res = g.res;
    const float lox = fminf(fminf(t.ax, t.bx), t.cx), hix = fmaxf(fmaxf(t.ax, t.bx), t.cx);
    const float loy = fminf(fminf(t.ay, t.by), t.cy), hiy = fmaxf(fmaxf(t.ay, t.by), t.cy);
    const float loz = fminf(fminf(t.az, t.bz), t.cz), hiz = fmaxf(fmaxf(t.az, t.bz), t.cz);
    const int cx0 = nearest_start_cell(lox, g.minx, g.inv_cell, res), cx1 = nearest_start_cell(hix, g.minx, g.inv_cell, res);
    const int cy0 = nearest_start_cell(loy, g.miny, g.inv_cell, res), cy1 = nearest_start_cell(hiy, g.miny, g.inv_cell, res);
    const int cz0 = nearest_start_cell(loz, g.minz, g.inv_cell, res), cz1 = nearest_start_cell(hiz, g.minz, g.inv_cell, res);
    const CrossGap gap = cross_gap(g, (float)res * g.cell, lox, hix, loy, hiy, loz, hiz);
    const float ddx = hix - lox, ddy = hiy - loy, ddz = hiz - loz;
    const float edge_max = sqrtf((ddx * ddx + ddy * ddy) + ddz * ddz) * 1.000001f;
    const float kappa = mesh_kappa(t);
    float best = __builtin_huge_valf();
    int bid = 0x7fffffff;
    auto visit = [&](uint32_t s, uint32_t e) __attribute__((always_inline)) {
        for (uint32_t j = s + (uint32_t)lane; j < e; j += 64u) {
            const float4 q = sorted[p0 + j];
            const float d2 = mesh_d2f(q.x, q.y, q.z, t);
            const int id = __float_as_int(q.w);
            const bool lt = (d2 < best) | ((d2 == best) & (id < bid));
            best = lt ? d2 : best;
            bid = lt ? id : bid;
        }
    };
    CellBlock old = {0, -1, 0, -1, 0, -1};   // the block already visited (empty before ring 0)
    for (int ring = 0; ring <= res; ++ring) {
        const CellBlock now = {max(cx0 - ring, 0), min(cx1 + ring, res - 1), max(cy0 - ring, 0), min(cy1 + ring, res - 1),
                               max(cz0 - ring, 0), min(cz1 + ring, res - 1)};
        cross_visit_shell(off, res, old, now, visit);
        old = now;
        const float b2 = cross_unvisited_b2(g, res, gap, now.x0, now.x1, now.y0, now.y1, now.z0, now.z1, lox, hix, loy, hiy, loz, hiz);
        if (b2 == __builtin_huge_valf()) break;   // (wave-uniform: every operand is)
        float wbest = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wbest = fminf(wbest, __shfl_xor(wbest, o));
        if (wbest < mesh_floor(b2, 0.0f, edge_max, kappa)) break;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bid, o);
        const bool lt = (ob < best) | ((ob == best) & (oi < bid));
        best = lt ? ob : best;
        bid = lt ? oi : bid;
    }
    if (lane == 0) {
        const bool found = bid != 0x7fffffff && best < __builtin_huge_valf();   // (as in point_face_query_kernel)
        d2_out[f] = found ? best : 0.0f;
        idx_out[f] = found ? (int64_t)bid - p0 : -1;
    }
}

// ---- backward: d2 = |q - c*|^2 with c* = wa A + wb B + wc C held to its face; r = q - c* in double from the fp32 inputs
struct MeshPair { double rx, ry, rz, wa, wb, wc; };
// REQUIRES 0 <= i < P and 0 <= f < F.  false: the face is absent (contributes nothing)
__device__ __forceinline__ bool mesh_pair(int64_t i, int64_t f, const float *__restrict__ pts, const float *__restrict__ verts, int64_t V,
                                          const int64_t *__restrict__ faces, MeshPair &o)
{
    MeshTri t;
    if (!mesh_load_face(f, faces, verts, V, t)) return false;
    const double qx = pts[3 * i], qy = pts[3 * i + 1], qz = pts[3 * i + 2];
    mesh_d2<double, true>(qx, qy, qz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, o.wa, o.wb, o.wc);
    o.rx = qx - ((o.wa * t.ax + o.wb * t.bx) + o.wc * t.cx);
    o.ry = qy - ((o.wa * t.ay + o.wb * t.by) + o.wc * t.cy);
    o.rz = qz - ((o.wa * t.az + o.wb * t.bz) + o.wc * t.cz);
    return true;
}

struct MeshLists {
    const int64_t *p_first, *p_num, *f_first, *f_num;
    int N;
    int64_t P, F, V;
    const int64_t *idx_pf, *idx_fp;   // (P,) mesh-local face of every point, (F,) cloud-local point of every face
};
#define MESH_NO_KEY 0x7fffffffffffffffll
// the pair a point names: its packed face, or -1
__device__ __forceinline__ int64_t mesh_face_of_point(const MeshLists &l, int64_t i)
{
    if ((uint64_t)i >= (uint64_t)l.P) return -1;
    const int n = find_cloud(i, l.p_first, l.p_num, l.N);
    const int64_t t = l.idx_pf[i];
    if (n < 0 || t < 0) return -1;
    const int64_t f = l.f_first[n] + t;
    return (uint64_t)f < (uint64_t)l.F ? f : -1;
}
// the pair a face names: its packed point, or -1
__device__ __forceinline__ int64_t mesh_point_of_face(const MeshLists &l, int64_t f)
{
    if ((uint64_t)f >= (uint64_t)l.F) return -1;
    const int m = find_cloud(f, l.f_first, l.f_num, l.N);
    const int64_t t = l.idx_fp[f];
    if (m < 0 || t < 0) return -1;
    const int64_t i = l.p_first[m] + t;
    return (uint64_t)i < (uint64_t)l.P ? i : -1;
}
// entry e = 3 pair + corner of the vertices' contributor list; pairs [0, P) are the points' (i, face of i), pairs
// [P, P + F) the faces' (point of f, f).  -> the packed vertex the entry adds to (MESH_NO_KEY: none), its pair (i, f)
__device__ __forceinline__ int64_t mesh_vertex_entry(const MeshLists &l, const int64_t *__restrict__ faces, int64_t e, int64_t &i, int64_t &f)
{
    if ((uint64_t)e >= (uint64_t)(3 * (l.P + l.F))) return MESH_NO_KEY;
    const int64_t pair = e / 3;
    const int k = (int)(e - 3 * pair);
    if (pair < l.P) { i = pair; f = mesh_face_of_point(l, pair); }
    else { f = pair - l.P; i = mesh_point_of_face(l, f); }
    if (i < 0 || f < 0) return MESH_NO_KEY;
    const int64_t v = faces[3 * f + k];   // (0 <= f < F: both helpers return -1 otherwise)
    return (uint64_t)v < (uint64_t)l.V ? v : MESH_NO_KEY;
}

// one thread per output row: threads [0, P) write grad_points, threads [P, P + V) grad_verts (each when given).  Its
// contributors are one segment of a list sorted in the Python layer (stable sort of int64 keys): found by binary search,
// added front to back in double, rounded once.
__global__ __launch_bounds__(256) void mesh_backward_kernel(const float *__restrict__ pts, const float *__restrict__ verts,
                                                            const int64_t *__restrict__ faces, const MeshLists l,
                                                            const int64_t *__restrict__ order_f /* (F,) */,
                                                            const int64_t *__restrict__ order_v /* (3 (P + F),) */,
                                                            const float *__restrict__ g_p, const float *__restrict__ g_f,
                                                            float *__restrict__ grad_points, float *__restrict__ grad_verts)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    MeshPair pr;
    if (t < l.P) {
        if (!grad_points) return;
        const int64_t i = t;
        const int64_t fown = mesh_face_of_point(l, i);
        if (fown >= 0 && mesh_pair(i, fown, pts, verts, l.V, faces, pr)) {
            const double w = 2.0 * (double)g_p[i];
            s0 = w * pr.rx; s1 = w * pr.ry; s2 = w * pr.rz;
        }
        int64_t lo = 0, hi = l.F;   // first k whose face names a point >= i (no point: behind every real one)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const int64_t tgt = mesh_point_of_face(l, order_f[mid]);
            if ((tgt < 0 ? MESH_NO_KEY : tgt) < i) lo = mid + 1;
            else hi = mid;
        }
        for (int64_t k = lo; k < l.F; ++k) {
            const int64_t f = order_f[k];
            if (mesh_point_of_face(l, f) != i) break;
            if (!mesh_pair(i, f, pts, verts, l.V, faces, pr)) continue;
            const double w = 2.0 * (double)g_f[f];
            s0 += w * pr.rx; s1 += w * pr.ry; s2 += w * pr.rz;
        }
        grad_points[3 * i] = (float)s0; grad_points[3 * i + 1] = (float)s1; grad_points[3 * i + 2] = (float)s2;
    } else if (t < l.P + l.V) {
        if (!grad_verts) return;
        const int64_t v = t - l.P, E = 3 * (l.P + l.F);
        int64_t i = -1, f = -1;
        int64_t lo = 0, hi = E;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (mesh_vertex_entry(l, faces, order_v[mid], i, f) < v) lo = mid + 1;
            else hi = mid;
        }
        for (int64_t k = lo; k < E; ++k) {
            const int64_t e = order_v[k];
            if (mesh_vertex_entry(l, faces, e, i, f) != v) break;
            if (!mesh_pair(i, f, pts, verts, l.V, faces, pr)) continue;
            const int corner = (int)(e % 3);
            const double wk = corner == 0 ? pr.wa : (corner == 1 ? pr.wb : pr.wc);
            const double w = -2.0 * (double)(e / 3 < l.P ? g_p[i] : g_f[f]) * wk;
            s0 += w * pr.rx; s1 += w * pr.ry; s2 += w * pr.rz;
        }
        grad_verts[3 * v] = (float)s0; grad_verts[3 * v + 1] = (float)s1; grad_verts[3 * v + 2] = (float)s2;
    }
}

}  // namespace dss

// The regions behind the grid's own workspace (the grid is built over F centroids)
struct MeshWorkspace {
    float *cent;      // (F,3) centroids
    float *rf;        // (F) radii
    float4 *rec;      // (3 F) the faces in cell order
    int *large;       // (F) large lists, mesh n's at f_first[n]
    int *per_mesh;    // (N,3) bits of R_grid, length of the large list, bits of K_grid
    float *kap;       // (F) kappa of every face
    size_t bytes;
};
static MeshWorkspace carve_mesh(void *ws, int N, int64_t F)
{
    MeshWorkspace m = {};
    const size_t n = N > 0 ? N : 1, f = F > 0 ? F : 1;
    Bump b = {reinterpret_cast<char *>(ws), align_up(carve_knn(nullptr, N, F).bytes, 256)};
    m.cent = b.take<float>(3 * f);
    m.rf = b.take<float>(f);
    m.rec = b.take<float4>(3 * f);
    m.large = b.take<int>(f);
    m.per_mesh = b.take<int>(3 * n);
    m.kap = b.take<float>(f);
    m.bytes = b.used;
    return m;
}

extern "C" size_t dss_point_face_workspace(int N, int64_t F) { return carve_mesh(nullptr, N, F).bytes; }

static int mesh_check_sizes(const char *who, int N, int64_t P, int64_t V, int64_t F)
{
    if (N <= 0 || P < 0 || V < 0 || F < 0 || P > 0x7fffffffll || F > 0x7fffffffll) {
        set_error("%s: bad sizes N=%d P=%lld V=%lld F=%lld (P, F below 2^31)", who, N, (long long)P, (long long)V, (long long)F);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    return DSS_OK;
}

extern "C" int dss_point_face_distance(const float *points, const int64_t *p_first, const int64_t *p_num, int64_t P,
                                       const float *verts, int64_t V, const int64_t *faces, const int64_t *f_first,
                                       const int64_t *f_num, int64_t F, int N, float *d2, int64_t *idx, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *who = "dss_point_face_distance";
    if (int rc = mesh_check_sizes(who, N, P, V, F)) return rc;
    if (P == 0) return DSS_OK;
    if (!points || !p_first || !p_num || !f_first || !f_num || !d2 || !idx || (F > 0 && !faces) || (V > 0 && !verts)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || workspace_bytes < dss_point_face_workspace(N, F)) {
        set_error("%s: workspace too small", who);
        return DSS_ERR_WORKSPACE;
    }
    const MeshWorkspace m = carve_mesh(workspace, N, F);
    // the grid of the centroids, by the self query's build (the plan only matters to the queries above: none is launched)
    const KnnCall c = {who, m.cent, f_first, f_num, N, F, 1, nullptr, nullptr, -1.0f, as_stream(stream), carve_knn(workspace, N, F),
                       plan_query(F, 1, false)};
    if (hipMemsetAsync(m.per_mesh, 0, (size_t)N * 12, c.st) != hipSuccess) return check_launch("mesh memset");
    if (F > 0) {
        const unsigned fb = (unsigned)((F + 255) / 256);
        const int q = option(DSS_OPT_MESH_LARGE);
        hipLaunchKernelGGL(mesh_prep_kernel, dim3(fb), dim3(256), 0, c.st, verts, V, faces, f_first, f_num, N, F, m.cent, m.rf, m.kap);
        if (int rc = build_grid(c, KnnView())) return rc;
        hipLaunchKernelGGL(mesh_classify_kernel, dim3(fb), dim3(256), 0, c.st, f_first, f_num, N, F, c.w.grids, (float)(q > 0 ? q : MESH_LARGE_QUARTERS),
                           m.rf, m.kap, m.per_mesh, m.large);
        hipLaunchKernelGGL(mesh_gather_kernel, dim3(fb), dim3(256), 0, c.st, verts, V, faces, f_first, f_num, N, F, c.w.sorted, m.rf, m.rec);
    }
    const unsigned block = P <= 131072 ? 64u : 256u;
    hipLaunchKernelGGL(point_face_query_kernel, dim3((unsigned)((P + block - 1) / block)), dim3(block), 0, c.st, points, p_first, p_num, P,
                       verts, V, faces, f_first, f_num, F, N, c.w.grids, c.w.stride, c.w.offsets, c.w.sorted, m.rec, m.per_mesh, m.large,
                       d2, idx);
    return check_launch(who);
}

extern "C" int dss_face_point_distance(const float *points, const int64_t *p_first, const int64_t *p_num, int64_t P,
                                       const float *verts, int64_t V, const int64_t *faces, const int64_t *f_first,
                                       const int64_t *f_num, int64_t F, int N, float *d2, int64_t *idx, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *who = "dss_face_point_distance";
    if (int rc = mesh_check_sizes(who, N, P, V, F)) return rc;
    if (F == 0) return DSS_OK;
    if (!p_first || !p_num || !f_first || !f_num || !faces || !d2 || !idx || (P > 0 && !points) || (V > 0 && !verts)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || workspace_bytes < dss_nearest_workspace(N, P)) {
        set_error("%s: workspace too small", who);
        return DSS_ERR_WORKSPACE;
    }
    const KnnCall c = {who, points, p_first, p_num, N, P, 1, nullptr, nullptr, -1.0f, as_stream(stream), carve_knn(workspace, N, P),
                       plan_query(P, 1, false)};
    if (P > 0)
        if (int rc = build_grid(c, KnnView())) return rc;
    hipLaunchKernelGGL(face_point_query_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, c.st, verts, V, faces, f_first, f_num, F,
                       p_first, p_num, P, N, c.w.grids, c.w.stride, c.w.offsets, c.w.sorted, d2, idx);
    return check_launch(who);
}

extern "C" int dss_mesh_distance_backward(const float *points, const int64_t *p_first, const int64_t *p_num, int64_t P,
                                          const float *verts, int64_t V, const int64_t *faces, const int64_t *f_first,
                                          const int64_t *f_num, int64_t F, int N, const int64_t *idx_pf, const int64_t *idx_fp,
                                          const int64_t *order_f, const int64_t *order_v, const float *g_p, const float *g_f,
                                          float *grad_points, float *grad_verts, void *stream)
{
    const char *who = "dss_mesh_distance_backward";
    if (int rc = mesh_check_sizes(who, N, P, V, F)) return rc;
    if ((!grad_points || P == 0) && (!grad_verts || V == 0)) return DSS_OK;
    if (!p_first || !p_num || !f_first || !f_num || (P > 0 && (!points || !idx_pf || !g_p)) || (F > 0 && (!faces || !idx_fp || !g_f)) ||
        (V > 0 && !verts) || (grad_points && F > 0 && !order_f) || (grad_verts && P + F > 0 && !order_v)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const int64_t blocks = (P + V + 255) / 256;
    if (blocks > 0x7fffffffll) { set_error("%s: too many rows", who); return DSS_ERR_UNSUPPORTED; }
    const MeshLists l = {p_first, p_num, f_first, f_num, N, P, F, V, idx_pf, idx_fp};
    hipLaunchKernelGGL(mesh_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), points, verts, faces, l, order_f,
                       order_v, g_p, g_f, grad_points, grad_verts);
    return check_launch(who);
}
