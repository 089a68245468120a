// The sign of estimated normals (dss_disambiguate_normals, dss_orient_normals).  DESIGN 4.17 states the contracts;
// include/dss_hip.h repeats them.
//
// dss_disambiguate_normals: one thread per packed slot, no workspace.  Mode 0 is the majority vote of the neighbourhood
// (pytorch3d's and the reference's `_disambiguate_vector_directions`), mode 1 turns every normal towards its cloud's viewpoint.
//
// dss_orient_normals: the sign is propagated from seeds over the neighbour lists, most parallel neighbours first.  Cloud n,
// alone: level = 0, it = 0, every point unoriented.  While an unoriented point exists, it += 1 and
//   candidates: an unoriented i with a neighbour j oriented in an EARLIER iteration and |d_ij| >= tau[level],
//               d_ij = (n_i.x o_j.x + n_i.y o_j.y) + n_i.z o_j.z  (fp32, every operation rounded on its own: -ffp-contract=off);
//   round:      if one exists, every candidate takes the j of its largest passing |d_ij| (ties: smallest id) as parent,
//               o_i = d_ij < 0 ? -n_i : n_i, stamp[i] = it, and level = 0;
//   level drop: else if level < 3, level += 1;
//   seed:       else the unoriented point of the largest z (ties: smallest id, NaN below every number) is oriented by the
//               sign of the first of (n.z, n.y, n.x) that is positive or negative, stamp = it, parent = -1, level = 0.
//
// The chain of dependent iterations is the whole cost, so ONE workgroup of 1024 threads owns a cloud for all of them:
// grid = N, no atomics, no workgroup waits for another.  Thread t owns the points t, t + 1024, ...: only the owner ever
// writes a point's normal, stamp and parent.  An iteration is ONE pass over the thread's unoriented points and ONE barrier:
//   - a point reads the stamps of its neighbours and takes those with 0 < stamp < it.  A stamp written in this very pass is
//     `it`, one not yet written is 0: both fail the test, so the pass needs no second buffer and no order among the threads,
//     and the normals it reads (o_j of an earlier iteration) are behind a barrier;
//   - the pass counts the points it oriented; at level 3 it also keeps the thread's best seed among the points it left
//     unoriented.  Count and seed are reduced over the wavefront by shuffles, over the workgroup through one LDS slot per
//     wavefront (double buffered: a wavefront writes the slots of iteration it + 2 only behind the barrier of it + 1, which
//     every wavefront reaches after it has read the slots of it).  Every thread computes the same sums from the same
//     slots, so `level`, the seed and the end of the loop are uniform and every barrier stands in uniform control flow;
//   - a seed is written by its owner behind that barrier, and a second barrier (seed iterations only) publishes it.
// The loop carries its bound as a trip limit: every iteration orients a point, drops a level or seeds, at most three drops
// stand between two orientations, so 5 P_n iterations are never reached; points left over would keep their input normal,
// stamp 0 and parent -1, which every point gets before the loop.
//
// Stamps: int32, in LDS while the cloud has at most NORMALS_LDS_POINTS points (normals_ops.LDS_CAPACITY repeats the number;
// 160,000 of the CU's 163,840 bytes), else in the caller's workspace (one int per packed row): the same code, slower loads.
//
// Lists: a pass reads the lists of every unoriented point, and a wavefront's 64 rows of the caller's (P,K) int64 array lie
// K * 8 bytes apart -- 64 cache lines per entry.  Lists of at most NORMALS_FAST_LIST entries (the usual 8, self included)
// are therefore copied once, before the loop, into the workspace as int32, entry-major within the cloud (entry k of point
// i at k P_n + i), with -1 where there is nothing to follow (behind KP_n, outside the cloud, the point itself): 256
// contiguous bytes per wavefront and entry.  Longer lists are read from the caller's array, entry by entry.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace dss {

#define NORMALS_THREADS 1024
#define NORMALS_LDS_POINTS 40000
#define NORMALS_FAST_LIST 8   // lists of at most this many entries (self included) are read without a branch
#define NORMALS_MAX_POINTS (INT_MAX / 5)   // 5 P_n, the trip limit and the largest stamp, is an int

// What a workgroup needs of its cloud: rows f0 .. f0 + np - 1 of the packed array (clamped into it).
struct NormalsCloud {
    int64_t f0;
    int np;
};

__device__ __forceinline__ NormalsCloud normals_cloud(const int64_t *__restrict__ first_idx,
                                                      const int64_t *__restrict__ num_pts, int n, int64_t P)
{
    NormalsCloud c;
    c.f0 = min(max(first_idx[n], (int64_t)0), P);
    c.np = (int)min(max(num_pts[n], (int64_t)0), P - c.f0);
    return c;
}

// One wavefront's share of an iteration: the points it oriented and its best seed.
struct NormalsSlots {
    int count[2][NORMALS_THREADS / DSS_WAVE];
    long long seed[2][NORMALS_THREADS / DSS_WAVE];
};

// The seed order as one integer, larger = better: the ordered bits of z above INT_MAX - id.  -0 counts as +0 (z + 0), a
// NaN takes the smallest key of all (below -inf), and among equal z the smaller id gives the larger low word.
__device__ __forceinline__ long long normals_seed_key(float z, int id)
{
    const int hi = z == z ? f2ord(z + 0.0f) : INT_MIN;
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)(INT_MAX - id));
}
#define NORMALS_NO_SEED LLONG_MIN   // below every key: the low word of a key is INT_MAX - id > 0

template <bool IN_LDS>
__global__ void __launch_bounds__(NORMALS_THREADS)
orient_normals_kernel(const float *__restrict__ nin, const float *__restrict__ pts, const int64_t *__restrict__ knn,
                      const int64_t *__restrict__ first_idx, const int64_t *__restrict__ num_pts, int64_t P, int K, int KP,
                      float *nout, int *stamp_out, int64_t *parent_out, int *stamp_ws, int *__restrict__ nbr_ws)
{
    constexpr int T = NORMALS_THREADS, NW = T / DSS_WAVE;
    __shared__ NormalsSlots slots;
    __shared__ int st_lds[IN_LDS ? NORMALS_LDS_POINTS : 1];
    const int n = blockIdx.x;
    const NormalsCloud c = normals_cloud(first_idx, num_pts, n, P);
    if (c.np == 0 || (c.np <= NORMALS_LDS_POINTS) != IN_LDS) return;   // the other instantiation's cloud
    const int tid = threadIdx.x, lane = tid & (DSS_WAVE - 1), wave = tid / DSS_WAVE;
    int *st = IN_LDS ? st_lds : stamp_ws + c.f0;
    const float *ni = nin + 3 * c.f0;
    const float *px = pts + 3 * c.f0;
    const int64_t *rows = knn + c.f0 * K;
    float *no = nout + 3 * c.f0;
    int *so = stamp_out ? stamp_out + c.f0 : nullptr;
    int64_t *po = parent_out ? parent_out + c.f0 : nullptr;
    const int kp = min(min(KP, K), c.np);
    // the cloud's region of the transposed lists: entry k of point i at nb[k np + i], -1 where there is nothing to follow
    int *nb = nbr_ws + (NORMALS_FAST_LIST - 1) * c.f0;
    const bool fast = kp <= NORMALS_FAST_LIST;

    for (int i = tid; i < c.np; i += T) {
        if (fast) {
            const int64_t *row = rows + (int64_t)i * K;
#pragma unroll
            for (int k = 0; k < NORMALS_FAST_LIST - 1; ++k) {
                const int64_t j = row[min(k + 1, kp - 1)];
                nb[(int64_t)k * c.np + i] = k + 1 < kp && j >= 0 && j < c.np && j != i ? (int)j : -1;
            }
        }
        st[i] = 0;
        no[3 * (int64_t)i] = ni[3 * (int64_t)i];
        no[3 * (int64_t)i + 1] = ni[3 * (int64_t)i + 1];
        no[3 * (int64_t)i + 2] = ni[3 * (int64_t)i + 2];
        if (so) so[i] = 0;
        if (po) po[i] = -1;
    }
    __syncthreads();

    const int limit = 5 * c.np;
    int level = 0, oriented = 0;
    for (int it = 1; it <= limit && oriented < c.np; ++it) {
        const float tau = level == 0 ? 0.95f : level == 1 ? 0.8f : level == 2 ? 0.5f : 0.0f;
        int count = 0;
        long long seed = NORMALS_NO_SEED;
        // the state of the point that a thread is deciding: n_i, and the best neighbour so far
        float nx = 0.f, ny = 0.f, nz = 0.f, best_a = 0.f, best_d = 0.f;
        int best_j = -1;
        // one neighbour: o_j of an earlier iteration against n_i; the largest passing |d|, ties to the smallest id
        auto visit = [&](int j) {
            const float ox = no[3 * (int64_t)j], oy = no[3 * (int64_t)j + 1], oz = no[3 * (int64_t)j + 2];
            const float d = (nx * ox + ny * oy) + nz * oz;
            const float a = fabsf(d);
            if (a >= tau && (best_j < 0 || a > best_a || (a == best_a && j < best_j))) {   // a NaN never passes
                best_a = a; best_d = d; best_j = j;
            }
        };
        auto load = [&](int i) {
            nx = ni[3 * (int64_t)i]; ny = ni[3 * (int64_t)i + 1]; nz = ni[3 * (int64_t)i + 2];
            best_j = -1;
        };
        // the unoriented point i after its neighbours: oriented by the best of them, or a candidate for the seed
        auto settle = [&](int i) {
            if (best_j >= 0) {
                const bool flip = best_d < 0.0f;
                no[3 * (int64_t)i] = flip ? -nx : nx;
                no[3 * (int64_t)i + 1] = flip ? -ny : ny;
                no[3 * (int64_t)i + 2] = flip ? -nz : nz;
                st[i] = it;
                if (so) so[i] = it;
                if (po) po[i] = best_j;
                ++count;
            } else if (level == 3) {
                seed = max(seed, normals_seed_key(px[3 * (int64_t)i + 2], i));
            }
            best_j = -1;
        };
        if (fast) {
            // the usual list, from the transposed copy: the entries and the stamps behind them are read without a branch
            // between them (an entry of -1 reads the point's own stamp, which is 0).  Most points of a pass have no oriented
            // neighbour: these loads are the pass
            constexpr int L = NORMALS_FAST_LIST - 1;
            for (int i = tid; i < c.np; i += T) {
                if (st[i] != 0) continue;
                int jr[L];
#pragma unroll
                for (int k = 0; k < L; ++k) jr[k] = nb[(int64_t)k * c.np + i];
                unsigned hit = 0;
#pragma unroll
                for (int k = 0; k < L; ++k) {
                    const int sj = st[jr[k] >= 0 ? jr[k] : i];
                    hit |= (sj != 0 && sj < it ? 1u : 0u) << k;
                }
                if (hit) {
                    load(i);
#pragma unroll
                    for (int k = 0; k < L; ++k)
                        if ((hit >> k) & 1u) visit(jr[k]);
                }
                settle(i);
            }
        } else {
            for (int i = tid; i < c.np; i += T) {
                if (st[i] != 0) continue;
                const int64_t *row = rows + (int64_t)i * K;
                bool loaded = false;
                for (int k = 1; k < kp; ++k) {
                    const int64_t j64 = row[k];
                    if (j64 < 0 || j64 >= c.np || j64 == i) continue;
                    const int sj = st[(int)j64];
                    if (sj == 0 || sj >= it) continue;          // unoriented, or oriented in this very pass
                    if (!loaded) {
                        load(i);
                        loaded = true;
                    }
                    visit((int)j64);
                }
                settle(i);
            }
        }
        // over the wavefront, then over the workgroup
#pragma unroll
        for (int m = DSS_WAVE / 2; m > 0; m >>= 1) count += __shfl_xor(count, m);
        if (level == 3) {
#pragma unroll
            for (int m = DSS_WAVE / 2; m > 0; m >>= 1) seed = max(seed, (long long)__shfl_xor(seed, m));
        }
        const int buf = it & 1;
        if (lane == 0) {
            slots.count[buf][wave] = count;
            slots.seed[buf][wave] = seed;
        }
        __syncthreads();   // the barrier of the iteration: the slots, and every normal and stamp written in the pass
        count = 0;
        seed = NORMALS_NO_SEED;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            count += slots.count[buf][w];
            seed = max(seed, slots.seed[buf][w]);
        }
        if (count > 0) {
            oriented += count;
            level = 0;
        } else if (level < 3) {
            ++level;
        } else {
            // nothing was oriented in the pass, so the best of the points it left is the best unoriented point; one exists
            const int s = INT_MAX - (int)(unsigned)(seed & 0xffffffffLL);
            if ((s & (T - 1)) == tid && s >= 0 && s < c.np) {
                const float nx = ni[3 * (int64_t)s], ny = ni[3 * (int64_t)s + 1], nz = ni[3 * (int64_t)s + 2];
                const bool flip = nz > 0.f ? false : nz < 0.f ? true : ny > 0.f ? false : ny < 0.f ? true : nx < 0.f;
                no[3 * (int64_t)s] = flip ? -nx : nx;
                no[3 * (int64_t)s + 1] = flip ? -ny : ny;
                no[3 * (int64_t)s + 2] = flip ? -nz : nz;
                st[s] = it;
                if (so) so[s] = it;
            }
            oriented += 1;
            level = 0;
            __syncthreads();   // publishes the seed: the next pass reads its stamp and its normal
        }
    }
}

// Packed slots that no cloud owns: (0,0,1), stamp 0, parent -1 (stamp / parent may be NULL).  Nothing is read of them.
__global__ void __launch_bounds__(256)
normals_unowned_kernel(const int64_t *__restrict__ first_idx, const int64_t *__restrict__ num_pts, int N, int64_t P,
                       float *__restrict__ nout, int *__restrict__ stamp, int64_t *__restrict__ parent)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || find_cloud(p, first_idx, num_pts, N) >= 0) return;
    nout[3 * p] = 0.f; nout[3 * p + 1] = 0.f; nout[3 * p + 2] = 1.f;
    if (stamp) stamp[p] = 0;
    if (parent) parent[p] = -1;
}

__global__ void __launch_bounds__(256)
disambiguate_normals_kernel(const float *__restrict__ pts, const float *__restrict__ nin, const int64_t *__restrict__ knn,
                            const int64_t *__restrict__ first_idx, const int64_t *__restrict__ num_pts, int N, int64_t P, int K,
                            int mode, const float *__restrict__ viewpoint, float *__restrict__ nout)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int n = find_cloud(p, first_idx, num_pts, N);
    float nx = 0.f, ny = 0.f, nz = 1.f;
    if (n >= 0) {
        nx = nin[3 * p]; ny = nin[3 * p + 1]; nz = nin[3 * p + 2];
        const float qx = pts[3 * p], qy = pts[3 * p + 1], qz = pts[3 * p + 2];
        bool flip;
        if (mode == 0) {
            const int64_t f0 = first_idx[n], np = num_pts[n];
            const int kn = (int)min((int64_t)K, np);
            int pos = 0;
            for (int k = 0; k < kn; ++k) {
                const int64_t j = knn[p * K + k];
                if (j < 0 || j >= np || f0 + j >= P) continue;   // an entry outside the cloud is not followed: not positive
                const int64_t r = f0 + j;
                const float dx = pts[3 * r] - qx, dy = pts[3 * r + 1] - qy, dz = pts[3 * r + 2] - qz;
                const float proj = (nx * dx + ny * dy) + nz * dz;
                pos += proj > 0.0f ? 1 : 0;
            }
            flip = 2 * pos < kn;
        } else {
            const float vx = viewpoint[3 * n] - qx, vy = viewpoint[3 * n + 1] - qy, vz = viewpoint[3 * n + 2] - qz;
            flip = (nx * vx + ny * vy) + nz * vz < 0.0f;
        }
        if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    }
    nout[3 * p] = nx; nout[3 * p + 1] = ny; nout[3 * p + 2] = nz;
}

}  // namespace dss

using namespace dss;

extern "C" int dss_disambiguate_normals(const float *points, const float *normals_in, const int64_t *knn_idx,
                                        const int64_t *first_idx, const int64_t *num_pts, int N, int64_t P, int K, int mode,
                                        const float *viewpoint, float *normals_out, void *stream)
{
    const char *who = "dss_disambiguate_normals";
    if (N < 1 || P < 0 || P > INT_MAX || K < 1 || mode < 0 || mode > 1) {
        set_error("%s: bad sizes N=%d P=%lld K=%d mode=%d (1 <= N, 0 <= P < 2^31, 1 <= K, mode 0 or 1)", who, N, (long long)P,
                  K, mode);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if ((mode == 1) != (viewpoint != nullptr)) {
        set_error("%s: mode 1 needs a viewpoint and mode 0 takes none", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return DSS_OK;
    if (!points || !normals_in || (mode == 0 && !knn_idx) || !first_idx || !num_pts || !normals_out) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(disambiguate_normals_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, as_stream(stream), points,
                       normals_in, knn_idx, first_idx, num_pts, N, P, K, mode, viewpoint, normals_out);
    return check_launch(who);
}

// The two regions of the workspace: the stamps of the clouds that do not fit LDS (none when no cloud can be that large), and
// the transposed lists of every cloud whose lists are short enough for them.
struct NormalsWorkspace {
    int *stamps, *lists;
};

static NormalsWorkspace normals_workspace(Bump &ws, int64_t P)
{
    NormalsWorkspace w;
    w.stamps = ws.take<int>(P > NORMALS_LDS_POINTS ? (size_t)P : 0);
    w.lists = ws.take<int>((size_t)P * (NORMALS_FAST_LIST - 1));
    return w;
}

extern "C" size_t dss_orient_normals_workspace(int N, int64_t P)
{
    (void)N;
    Bump ws{nullptr, 0};
    normals_workspace(ws, P);
    return ws.used;
}

extern "C" int dss_orient_normals(const float *normals_in, const float *points, const int64_t *knn_idx,
                                  const int64_t *first_idx, const int64_t *num_pts, int N, int64_t P, int K, int KP,
                                  float *normals_out, int *stamp, int64_t *parent, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    const char *who = "dss_orient_normals";
    if (N < 1 || P < 0 || P > NORMALS_MAX_POINTS || K < 1 || KP < 1) {
        set_error("%s: bad sizes N=%d P=%lld K=%d KP=%d (1 <= N, 0 <= P <= %d, 1 <= K, 1 <= KP)", who, N, (long long)P, K, KP,
                  NORMALS_MAX_POINTS);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return DSS_OK;
    if (!normals_in || !points || !knn_idx || !first_idx || !num_pts || !normals_out) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (normals_out == normals_in) {
        set_error("%s: normals_out must not be normals_in", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const size_t need = dss_orient_normals_workspace(N, P);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, dss_orient_normals_workspace asks for %zu", who, workspace ? workspace_bytes : 0,
                  need);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    Bump ws{static_cast<char *>(workspace), 0};
    const NormalsWorkspace w = normals_workspace(ws, P);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(normals_unowned_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, first_idx, num_pts, N, P,
                       normals_out, stamp, parent);
    const dim3 grid((unsigned)N);
    hipLaunchKernelGGL(orient_normals_kernel<true>, grid, dim3(NORMALS_THREADS), 0, st, normals_in, points, knn_idx, first_idx,
                       num_pts, P, K, KP, normals_out, stamp, parent, w.stamps, w.lists);
    if (P > NORMALS_LDS_POINTS)
        hipLaunchKernelGGL(orient_normals_kernel<false>, grid, dim3(NORMALS_THREADS), 0, st, normals_in, points, knn_idx,
                           first_idx, num_pts, P, K, KP, normals_out, stamp, parent, w.stamps, w.lists);
    return check_launch(who);
}
