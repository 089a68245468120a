// Farthest point sampling of every cloud of a packed batch (dss_farthest_points).  DESIGN 4.16 states the contract;
// include/dss_hip.h repeats it.
//
// Cloud n, P_n points, k_n = min(n_samples[n], P_n) samples, start id s_n:
//   d[i] = +inf, c_0 = s_n, r_0 = +inf;  step t emits (c_t, r_t), then for every i
//   dist = (dx dx + dy dy) + dz dz  (fp32, every operation rounded on its own: -ffp-contract=off),
//   d[i] = dist < d[i] ? dist : d[i]  (a NaN distance never changes d),  d[c_t] = -1 after the update,
//   c_{t+1} = the i with the largest d[i], ties to the SMALLEST id, r_{t+1} = that d.
//
// The chain of dependent steps is the whole cost, so ONE workgroup owns a cloud for all of its steps: grid = N, no
// atomics, no workgroup waits for another, the trip count k_n is read once and is uniform over the workgroup.
//
// Register path, fps_register_kernel<T, R>: thread t of T owns ids t, t + T, ..., t + (R - 1) T and keeps x, y, z, d of them
// in registers (static indexing only: nothing goes to scratch).  A step: update the R distances, take the thread's best
// (d, id), reduce over the 64 lanes by DPP (fps_best below); the winning lane of each wavefront writes (d, id, x, y, z) into
// its wavefront's LDS slot; after ONE barrier the lanes 0 .. T/64 - 1 of every wavefront read one slot each, reduce again by
// DPP and broadcast the next centre's coordinates by v_readlane.  The slots are double buffered: a wavefront writes the slots
// of step t + 2 only behind the barrier of step t + 1, which every wavefront reaches after it has used what it read in
// step t.  T = 64 needs neither LDS nor a barrier.
// The order `d_a > d_b || (d_a == d_b && id_a < id_b)` is total on pairs with distinct ids, and every level of the reduction
// applies it in two passes: the largest d first, then the smallest id among the lanes that hold it.
//
// Streaming path, fps_stream_kernel: clouds above the largest register capacity keep d in the caller's workspace (one float
// per packed row) and the 1024 threads stride over the cloud's points in every step; same comparison, same reduction.
// Correct for any size and slow by design: one workgroup re-reads 12 B and rewrites 4 B per point per step.
//
// The cloud sizes are device arrays, so every instantiation is launched over all N clouds and a workgroup leaves at once
// when its cloud's size belongs to another instantiation (those that no cloud of at most P points can reach are not
// launched).  The workgroup that owns the cloud writes the whole row of both outputs, padding included.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "common.h"

namespace dss {

// (T, R) of the register instantiations, capacity T * R ascending; sampling_ops.REGISTER_CAPACITIES repeats the capacities
// 1024 threads wherever a cloud has the points for them: a wavefront's step is a chain of dependent instructions, and four
// wavefronts per SIMD hide one another's latencies (measured, DESIGN 4.16: 8,192 points as 256 x 32 take 1.7 us per step,
// as 1024 x 8 1.2 - 1.3 us; 24,576 as 512 x 48 3.1 us, as 1024 x 24 2.4 - 2.5 us)
#define FPS_INSTANCES(X) X(64, 4) X(512, 4) X(1024, 8) X(1024, 16) X(1024, 24)
#define FPS_MAX_REGISTER_POINTS (1024 * 24)
#define FPS_STREAM_THREADS 1024
#define FPS_STREAM_UNROLL 4

// The reductions work on KEYS: the bits of d as a signed integer.  d is never NaN, and a non-negative float orders like its
// bits, so among candidates with d >= 0 -- every point that can still be selected -- the largest key is the largest d.  The
// marks below 0 (-1 selected, -2 a slot beyond the cloud, -3 a thread without a candidate) have negative keys: they lose to
// every d >= 0, and which of them wins among themselves never matters, because a reduction is only made while an unselected
// point exists.  Integer max / min are single DPP instructions; a (d, id) pair compare is eight.

__device__ __forceinline__ float fps_readlane(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int CTRL>
__device__ __forceinline__ int fps_dpp(int v)   // every lane reads a lane of its own row: the four row permutations
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}

// The reduction of `v` by OP (`unit`: its neutral element) over the first 16 lanes (ROWS == 1) or over all 64 (ROWS == 4),
// uniform.  Row stages: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror leave the result of a row in
// each of its lanes.  Then row_bcast:15 hands lane 15 of a row to the next row (rows 1 and 3 take it: row_mask 0xa) and
// row_bcast:31 lane 31 to rows 2 and 3 (row_mask 0xc); a lane outside the row mask gets `unit`.  Lane 63 then holds all four
// rows.  (old = 0 with bound_ctrl, old = unit: the forms that the compiler folds into the max / min instruction itself)
template <int ROWS, typename Op>
__device__ __forceinline__ int fps_reduce(int v, int unit, Op op)
{
    v = op(v, fps_dpp<0xB1>(v));
    v = op(v, fps_dpp<0x4E>(v));
    v = op(v, fps_dpp<0x141>(v));
    v = op(v, fps_dpp<0x140>(v));
    if (ROWS == 1) return __builtin_amdgcn_readlane(v, 0);
    v = op(v, __builtin_amdgcn_update_dpp(unit, v, 0x142, 0xa, 0xf, false));
    v = op(v, __builtin_amdgcn_update_dpp(unit, v, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(v, 63);
}

// (key, id) of every lane -> the largest key and, among the lanes that hold it, the smallest id; both uniform.  Ties are
// rare: one lane holds the largest key as a rule, and its id is read directly; the second reduction runs only otherwise
// (the branch is uniform).  `on`: the lanes that take part.
template <int ROWS>
__device__ __forceinline__ void fps_best(int &key, int &id, bool on)
{
    const int top = fps_reduce<ROWS>(on ? key : INT_MIN, INT_MIN, [](int a, int b) { return max(a, b); });
    const bool tie = on && key == top;
    const unsigned long long mask = __ballot(tie);
    int first;
    if (__popcll(mask) == 1)
        first = __builtin_amdgcn_readlane(id, __ffsll((long long)mask) - 1);
    else
        first = fps_reduce<ROWS>(tie ? id : INT_MAX, INT_MAX, [](int a, int b) { return min(a, b); });
    key = top;
    id = first;
}

// One wavefront's candidate for the next centre.
struct FpsSlots {
    float4 head[2][16];   // key, id (as bits), x, y
    float z[2][16];
};

// From every thread's best (d, id) to the workgroup's, uniform over the workgroup, with the winner's coordinates.
// `coords(x, y, z)` gives the coordinates of the calling thread's best point; only a wavefront's winning lane calls it.
// Thread t owns the ids congruent to t modulo T (T a power of two), so lane and wavefront of the winner follow from its id.
template <int T, typename Coords>
__device__ __forceinline__ void fps_block_best(float &d, int &id, float &x, float &y, float &z, FpsSlots &slots, int buf,
                                               Coords coords)
{
    constexpr int NW = T / DSS_WAVE;
    const int own = id;
    int key = __float_as_int(d);
    fps_best<4>(key, id, true);
    float bx = 0.f, by = 0.f, bz = 0.f;
    if (own == id) coords(bx, by, bz);
    if constexpr (NW == 1) {
        const int lane = id & (DSS_WAVE - 1);
        d = __int_as_float(key);
        x = fps_readlane(bx, lane); y = fps_readlane(by, lane); z = fps_readlane(bz, lane);
        return;
    }
    const int lane = threadIdx.x & (DSS_WAVE - 1), wave = threadIdx.x / DSS_WAVE;
    if (own == id) {
        slots.head[buf][wave] = make_float4(__int_as_float(key), __int_as_float(id), bx, by);
        slots.z[buf][wave] = bz;
    }
    // the barrier of the step.  Only LDS is handed over: `__syncthreads()` would also wait for the global stores of this
    // step's outputs (vmcnt(0))
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    float hz = 0.f;
    if (lane < NW) {
        h = slots.head[buf][lane];
        hz = slots.z[buf][lane];
    }
    key = __float_as_int(h.x);
    id = __float_as_int(h.y);
    fps_best<1>(key, id, lane < NW);   // NW <= 16: the first row holds every slot
    d = __int_as_float(key);
    const int from = (id & (T - 1)) / DSS_WAVE;
    x = fps_readlane(h.z, from); y = fps_readlane(h.w, from); z = fps_readlane(hz, from);
}

// What a workgroup needs of its cloud: rows f0 .. f0 + np - 1 of the packed array (clamped into it), k samples, start s.
struct FpsCloud {
    int64_t f0;
    int np, k, s;
};

__device__ __forceinline__ FpsCloud fps_cloud(const int64_t *__restrict__ first_idx, const int64_t *__restrict__ num_pts,
                                              const int64_t *__restrict__ n_samples, const int64_t *__restrict__ start, int n,
                                              int64_t P, int64_t K_max)
{
    FpsCloud c;
    c.f0 = min(max(first_idx[n], (int64_t)0), P);
    c.np = (int)min(max(num_pts[n], (int64_t)0), P - c.f0);
    c.k = (int)min(min(max(n_samples[n], (int64_t)0), K_max), (int64_t)c.np);
    c.s = start ? (int)min(max(start[n], (int64_t)0), (int64_t)max(c.np - 1, 0)) : 0;
    return c;
}

// entries t >= k of row n: idx = -1, sel_sqdist = 0
__device__ __forceinline__ void fps_pad_row(int64_t *__restrict__ idx, float *__restrict__ sqd, int n, int k, int64_t K_max,
                                            int T)
{
    for (int64_t t = k + (int64_t)threadIdx.x; t < K_max; t += T) {
        idx[n * K_max + t] = -1;
        if (sqd) sqd[n * K_max + t] = 0.f;
    }
}

// Clouds of lo < P_n <= T * R points.
template <int T, int R>
__global__ void __launch_bounds__(T)
fps_register_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx, const int64_t *__restrict__ num_pts,
                    const int64_t *__restrict__ n_samples, const int64_t *__restrict__ start, int64_t P, int64_t K_max,
                    int lo, int64_t *__restrict__ idx, float *__restrict__ sqd)
{
    __shared__ FpsSlots slots;
    const int n = blockIdx.x;
    const FpsCloud c = fps_cloud(first_idx, num_pts, n_samples, start, n, P, K_max);
    if (c.np <= lo || c.np > T * R) return;   // another instantiation's cloud
    fps_pad_row(idx, sqd, n, c.k, K_max, T);
    if (c.k == 0) return;
    const int tid = threadIdx.x;
    float x[R], y[R], z[R], d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + r * T;
        const bool real = i < c.np;
        const float *q = pts + 3 * (c.f0 + (real ? i : 0));
        x[r] = real ? q[0] : 0.f; y[r] = real ? q[1] : 0.f; z[r] = real ? q[2] : 0.f;
        d[r] = real ? INFINITY : -2.0f;   // a slot beyond the cloud: below every real point, and no distance lowers it
    }
    int cur = c.s;
    float rad = INFINITY;
    const float *q = pts + 3 * (c.f0 + cur);
    float cx = q[0], cy = q[1], cz = q[2];
    for (int t = 0;; ++t) {
        if (tid == 0) {
            idx[n * K_max + t] = cur;
            if (sqd) sqd[n * K_max + t] = rad;
        }
        if (t + 1 >= c.k) break;
        // d[c_t] = -1.  Set BEFORE the update, which leaves it alone (no distance, NaN included, is below -1), so the
        // update itself carries no test for the centre: one select per slot here against two per point there
        const bool mine = (cur & (T - 1)) == tid;
        const int slot = cur / T;
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] = mine && r == slot ? -1.0f : d[r];
        float bd = -3.0f;
        int br = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float dx = x[r] - cx, dy = y[r] - cy, dz = z[r] - cz;
            const float dist = (dx * dx + dy * dy) + dz * dz;
            const float v = dist < d[r] ? dist : d[r];
            d[r] = v;
            const bool take = v > bd;   // ids ascend with r: strict keeps the smallest id
            bd = take ? v : bd;
            br = take ? r : br;
        }
        int bi = tid + br * T;
        fps_block_best<T>(bd, bi, cx, cy, cz, slots, t & 1, [&](float &ox, float &oy, float &oz) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (br == r) { ox = x[r]; oy = y[r]; oz = z[r]; }
        });
        cur = bi;
        rad = bd;
    }
}

// Clouds of more than FPS_MAX_REGISTER_POINTS points; dws (P,) holds d of every packed row of such a cloud.
__global__ void __launch_bounds__(FPS_STREAM_THREADS)
fps_stream_kernel(const float *__restrict__ pts, const int64_t *__restrict__ first_idx, const int64_t *__restrict__ num_pts,
                  const int64_t *__restrict__ n_samples, const int64_t *__restrict__ start, int64_t P, int64_t K_max,
                  int64_t *__restrict__ idx, float *__restrict__ sqd, float *__restrict__ dws)
{
    constexpr int T = FPS_STREAM_THREADS;
    __shared__ FpsSlots slots;
    const int n = blockIdx.x;
    const FpsCloud c = fps_cloud(first_idx, num_pts, n_samples, start, n, P, K_max);
    if (c.np <= FPS_MAX_REGISTER_POINTS) return;
    fps_pad_row(idx, sqd, n, c.k, K_max, T);
    if (c.k == 0) return;
    const int tid = threadIdx.x;
    const float *base = pts + 3 * c.f0;
    float *dn = dws + c.f0;
    int cur = c.s;
    float rad = INFINITY;
    float cx = base[3 * (int64_t)cur], cy = base[3 * (int64_t)cur + 1], cz = base[3 * (int64_t)cur + 2];
    for (int t = 0;; ++t) {
        if (tid == 0) {
            idx[n * K_max + t] = cur;
            if (sqd) sqd[n * K_max + t] = rad;
        }
        if (t + 1 >= c.k) break;
        float bd = -3.0f, bx = 0.f, by = 0.f, bz = 0.f;
        int bi = tid;   // a thread without points: distinct ids keep the comparison a total order
        // a thread meets the same rows in every step, in ascending order: no other thread reads its d.  FPS_STREAM_UNROLL
        // rows at a time, all their loads issued before the first use: the loop is bound by the latency of a load
        for (int64_t i0 = tid; i0 < c.np; i0 += FPS_STREAM_UNROLL * T) {
            float px[FPS_STREAM_UNROLL], py[FPS_STREAM_UNROLL], pz[FPS_STREAM_UNROLL], old[FPS_STREAM_UNROLL];
#pragma unroll
            for (int u = 0; u < FPS_STREAM_UNROLL; ++u) {
                const int64_t i = i0 + u * T;
                const bool real = i < c.np;
                const int64_t row = real ? i : i0;
                px[u] = base[3 * row]; py[u] = base[3 * row + 1]; pz[u] = base[3 * row + 2];
                old[u] = t == 0 ? INFINITY : dn[row];
                if (!real) old[u] = -4.0f;   // a slot beyond the cloud: below every start value, never the best, never stored
            }
#pragma unroll
            for (int u = 0; u < FPS_STREAM_UNROLL; ++u) {
                const int64_t i = i0 + u * T;
                const float dx = px[u] - cx, dy = py[u] - cy, dz = pz[u] - cz;
                const float dist = (dx * dx + dy * dy) + dz * dz;
                float v = dist < old[u] ? dist : old[u];
                v = i == cur ? -1.0f : v;
                if (i < c.np) dn[i] = v;
                if (v > bd) { bd = v; bi = (int)i; bx = px[u]; by = py[u]; bz = pz[u]; }
            }
        }
        fps_block_best<T>(bd, bi, cx, cy, cz, slots, t & 1, [&](float &ox, float &oy, float &oz) { ox = bx; oy = by; oz = bz; });
        cur = bi;
        rad = bd;
    }
}

}  // namespace dss

using namespace dss;

extern "C" size_t dss_farthest_points_workspace(int N, int64_t P)
{
    (void)N;
    return P > FPS_MAX_REGISTER_POINTS ? align_up((size_t)P * sizeof(float), 256) : 0;
}

extern "C" int dss_farthest_points(const float *points, const int64_t *first_idx, const int64_t *num_pts,
                                   const int64_t *n_samples, const int64_t *start, int N, int64_t P, int64_t K_max,
                                   int64_t *idx, float *sel_sqdist, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "dss_farthest_points";
    if (N < 1 || P < 0 || K_max < 0 || P > INT_MAX) {
        set_error("%s: bad sizes N=%d P=%lld K_max=%lld (1 <= N, 0 <= P < 2^31, 0 <= K_max)", who, N, (long long)P,
                  (long long)K_max);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0 || K_max == 0) return DSS_OK;
    if (!points || !first_idx || !num_pts || !n_samples || !idx) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const size_t need = dss_farthest_points_workspace(N, P);
    if (need && (!workspace || workspace_bytes < need)) {
        set_error("%s: workspace of %zu bytes, dss_farthest_points_workspace asks for %zu", who, workspace ? workspace_bytes : 0,
                  need);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const dim3 grid((unsigned)N);
    int lo = -1;   // the capacity of the instantiation before: its clouds are not this one's
#define FPS_LAUNCH(T, R)                                                                                               \
    if (lo < P) {                                                                                                      \
        hipLaunchKernelGGL((fps_register_kernel<T, R>), grid, dim3(T), 0, as_stream(stream), points, first_idx,       \
                           num_pts, n_samples, start, P, K_max, lo, idx, sel_sqdist);                                  \
        lo = T * R;                                                                                                    \
    }
    FPS_INSTANCES(FPS_LAUNCH)
#undef FPS_LAUNCH
    if (need)
        hipLaunchKernelGGL(fps_stream_kernel, grid, dim3(FPS_STREAM_THREADS), 0, as_stream(stream), points, first_idx,
                           num_pts, n_samples, start, P, K_max, idx, sel_sqdist, static_cast<float *>(workspace));
    return check_launch(who);
}
