// Cleaning a cloud in place: the bilateral filter of the normals (DSS/core/cloud.py:515-552 `denoise_normals`,
// dss_denoise_normals) and one outer iteration of the robust implicit MLS projection (:442-513
// `project_to_latent_surface`, dss_rimls_step).  DESIGN 4.15 states both contracts; include/dss_hip.h repeats them.
//
// Neighbourhood of point p of cloud n, for both: entries 1 .. K of its dss_knn_points(K + 1) list (self dropped).  Entry j
// is LIVE iff j < num_pts[n] - 1 (a real point, not the zero padding of a short list) and its list distance d_j < r_n^2 in
// fp32.  A dead entry contributes NOTHING -- the reference gathers zeros for it (frnn_gather), which makes its result
// depend on where the origin lies.
//
// Lane layout: 8 lanes per point, neighbour j in slot j / 8 of lane j % 8 (S = ceil(K / 8) <= 5 slots, template parameter,
// so every slot array stays in registers).  A sum over the neighbourhood is the lane's slots in ascending order, then three
// DPP stages (quad_perm, quad_perm, row_half_mirror); fp addition is commutative, so after every stage both partners hold
// the same bits and the sum is uniform over the group without a broadcast -- and independent of the launch.  No LDS, no
// atomics.  Every operation is a separately rounded fp32 operation (-ffp-contract=off), exp is the accurate expf.
#include <float.h>
#include "common.h"

namespace dss {

#define SM_LANES 8

// Sum over the 8 lanes of a group, in every lane of the group.
__device__ __forceinline__ float group8_sum(float v)
{
    v = quad_sum(v);
    v += dpp_f32<0x141>(v);   // row_half_mirror: lane i <-> lane 7 - i of each 8
    return v;
}

__device__ __forceinline__ void normalize3(float &x, float &y, float &z)   // F.normalize: v / max(|v|, 1e-12)
{
    const float len = fmaxf(sqrtf((x * x + y * y) + z * z), 1e-12f);
    x /= len; y /= len; z /= len;
}

// What a lane holds of its point's neighbourhood after the gather of a launch.
template <int S>
struct Slots {
    float dx[S], dy[S], dz[S];   // p - q_j   (0 for a dead slot)
    float nx[S], ny[S], nz[S];   // normalised normal of q_j (0 for a dead slot)
    bool on[S];
};

// The point of this lane's group and its cloud; rows beyond P and slots of no cloud have n = -1 and read nothing.
struct Owner {
    int64_t p, f0, np_;
    int n, kk, l;
    float r2;
};

__device__ __forceinline__ Owner find_owner(const int64_t *__restrict__ first_idx, const int64_t *__restrict__ num_pts,
                                            const float *__restrict__ radius, int N, int64_t P, int K)
{
    Owner o;
    o.p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / SM_LANES;
    o.l = threadIdx.x % SM_LANES;
    o.n = o.p < P ? find_cloud(o.p, first_idx, num_pts, N) : -1;
    o.f0 = 0; o.np_ = 0; o.kk = 0; o.r2 = 0.f;
    if (o.n >= 0) {
        o.f0 = first_idx[o.n];
        o.np_ = num_pts[o.n];
        o.kk = (int)min((int64_t)K, o.np_ - 1);
        const float r = radius[o.n];
        o.r2 = r * r;
    }
    return o;
}

// Gathers the lane's slots: positions from `pts` (the state of this launch), normals from `nrm`.  All loads of a lane are
// issued before any arithmetic on them.  (ids outside the cloud or the packed array are not followed)
template <int S>
__device__ __forceinline__ void gather_slots(Slots<S> &s, const Owner &o, const float *__restrict__ pts,
                                             const float *__restrict__ nrm, const float *__restrict__ knn_d,
                                             const int64_t *__restrict__ knn_idx, int64_t P, int K, float px, float py, float pz)
{
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const int j = i * SM_LANES + o.l;
        bool on = o.n >= 0 && j < o.kk;
        int64_t q = 0;
        if (on) {
            const int64_t e = o.p * (K + 1) + 1 + j;
            on = knn_d[e] < o.r2;   // NaN: dead
            q = max(min(o.f0 + min(max(knn_idx[e], (int64_t)0), o.np_ - 1), P - 1), (int64_t)0);
        }
        float qx = 0.f, qy = 0.f, qz = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
        if (on) {
            qx = pts[3 * q]; qy = pts[3 * q + 1]; qz = pts[3 * q + 2];
            ax = nrm[3 * q]; ay = nrm[3 * q + 1]; az = nrm[3 * q + 2];
            normalize3(ax, ay, az);
        }
        s.on[i] = on;
        s.dx[i] = on ? px - qx : 0.f; s.dy[i] = on ? py - qy : 0.f; s.dz[i] = on ? pz - qz : 0.f;
        s.nx[i] = ax; s.ny[i] = ay; s.nz[i] = az;
    }
}

// out[p] = normalize(sum_j wn_j wp_j n_j) over the live neighbours,
//   wn_j = exp(-((1 - n_j . n) / sigma)^2)         wp_j = exp(-dp_j inv) if dp_j <= 16 / inv else 0
//   inv = P_n / 2                                  dp_j = |q_j - p|^2 = (dx dx + dy dy) + dz dz
// A point whose weights sum to 0 keeps its normalised input normal (the reference returns the zero vector).
template <int S>
__global__ void __launch_bounds__(256)
denoise_normals_kernel(const float *__restrict__ pts, const float *__restrict__ nrm, const float *__restrict__ knn_d,
                       const int64_t *__restrict__ knn_idx, const int64_t *__restrict__ first_idx,
                       const int64_t *__restrict__ num_pts, const float *__restrict__ radius, int N, int64_t P, int K,
                       float sigma, float *__restrict__ out)
{
    const Owner o = find_owner(first_idx, num_pts, radius, N, P, K);
    float px = 0.f, py = 0.f, pz = 0.f, mx = 0.f, my = 0.f, mz = 0.f;
    if (o.n >= 0) {
        px = pts[3 * o.p]; py = pts[3 * o.p + 1]; pz = pts[3 * o.p + 2];
        mx = nrm[3 * o.p]; my = nrm[3 * o.p + 1]; mz = nrm[3 * o.p + 2];
    }
    Slots<S> s;
    gather_slots<S>(s, o, pts, nrm, knn_d, knn_idx, P, K, px, py, pz);
    normalize3(mx, my, mz);
    const float inv = (float)o.np_ / 2.0f;
    const float cut = 16.0f / inv;
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const float dp = (s.dx[i] * s.dx[i] + s.dy[i] * s.dy[i]) + s.dz[i] * s.dz[i];
        const float c = (1.0f - ((s.nx[i] * mx + s.ny[i] * my) + s.nz[i] * mz)) / sigma;
        const float wn = expf(-(c * c));
        const float wp = dp <= cut ? expf(-dp * inv) : 0.f;
        const float w = s.on[i] ? wn * wp : 0.f;
        sw += w;
        sx += w * s.nx[i]; sy += w * s.ny[i]; sz += w * s.nz[i];
    }
    sw = group8_sum(sw); sx = group8_sum(sx); sy = group8_sum(sy); sz = group8_sum(sz);
    if (sw > 0.f) {
        normalize3(sx, sy, sz);
        mx = sx; my = sy; mz = sz;
    }
    if (o.l == 0 && o.p < P) {
        const bool real = o.n >= 0;   // a slot that no cloud owns: zeros
        out[3 * o.p] = real ? mx : 0.f; out[3 * o.p + 1] = real ? my : 0.f; out[3 * o.p + 2] = real ? mz : 0.f;
    }
}

// One outer iteration of the projection for every live point: `max_est` reweighting passes on the neighbourhood gathered
// ONCE from pts_in (the state of step t - 1), then p <- p - f g into pts_out.  A point that is not live is copied and still
// read by its neighbours.  inv = 1 / (16 d_0), d_0 = the list distance of the nearest live neighbour = entry 1 of the
// ascending list (no live entry, or d_0 = 0: the point is never live).
template <int S>
__global__ void __launch_bounds__(256)
rimls_step_kernel(const float *__restrict__ pts_in, const float *__restrict__ nrm, const float *__restrict__ knn_d,
                  const int64_t *__restrict__ knn_idx, const int64_t *__restrict__ first_idx,
                  const int64_t *__restrict__ num_pts, const float *__restrict__ radius,
                  const unsigned char *__restrict__ live_in, int N, int64_t P, int K, int max_est,
                  float *__restrict__ pts_out, unsigned char *__restrict__ live_out)
{
    const Owner o = find_owner(first_idx, num_pts, radius, N, P, K);
    float px = 0.f, py = 0.f, pz = 0.f, d0 = 0.f;
    bool live = false;
    if (o.p < P) { px = pts_in[3 * o.p]; py = pts_in[3 * o.p + 1]; pz = pts_in[3 * o.p + 2]; }
    if (o.n >= 0 && o.kk > 0) {
        d0 = knn_d[o.p * (K + 1) + 1];
        live = (live_in ? live_in[o.p] != 0 : true) && d0 < o.r2 && d0 > 0.f;
    }
    // a group of converged points skips the gather; the cross-lane sums below stay inside a group, and a wave's groups
    // take this branch independently only around code without cross-lane operations
    Slots<S> s;
    if (live) {
        gather_slots<S>(s, o, pts_in, nrm, knn_d, knn_idx, P, K, px, py, pz);
    } else {
#pragma unroll
        for (int i = 0; i < S; ++i) {
            s.on[i] = false;
            s.dx[i] = s.dy[i] = s.dz[i] = s.nx[i] = s.ny[i] = s.nz[i] = 0.f;
        }
    }
    const float inv = live ? 1.0f / (16.0f * d0) : 0.f;
    float fx[S], phi[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        fx[i] = (s.dx[i] * s.nx[i] + s.dy[i] * s.ny[i]) + s.dz[i] * s.nz[i];
        const float dp = (s.dx[i] * s.dx[i] + s.dy[i] * s.dy[i]) + s.dz[i] * s.dz[i];
        phi[i] = s.on[i] ? expf(-dp * inv) : 0.f;
    }
    float f = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    for (int it = 0; it < max_est; ++it) {   // max_est is uniform over the grid: every lane of a wave reaches every DPP
        float sw = 0.f, sf = 0.f, wx = 0.f, wy = 0.f, wz = 0.f, hx = 0.f, hy = 0.f, hz = 0.f, mx = 0.f, my = 0.f, mz = 0.f;
#pragma unroll
        for (int i = 0; i < S; ++i) {
            float alpha = 1.0f;
            if (it > 0) {
                const float ex = s.nx[i] - gx, ey = s.ny[i] - gy, ez = s.nz[i] - gz;
                const float a = sqrtf((ex * ex + ey * ey) + ez * ez) / 0.5f;
                const float b = fx[i] - f;
                alpha = expf(-(a * a)) * expf(-(b * b * inv / 4.0f));
            }
            const float w = phi[i] * alpha;           // 0 for a dead slot (phi = 0, alpha finite)
            const float c = inv * phi[i] * w;         // phi enters twice (cloud.py:487-492)
            const float ux = 2.0f * s.dx[i] * c, uy = 2.0f * s.dy[i] * c, uz = 2.0f * s.dz[i] * c;
            sw += w;
            sf += w * fx[i];
            wx += ux; wy += uy; wz += uz;
            hx += ux * fx[i]; hy += uy * fx[i]; hz += uz * fx[i];
            mx += w * s.nx[i]; my += w * s.ny[i]; mz += w * s.nz[i];
        }
        sw = group8_sum(sw); sf = group8_sum(sf);
        wx = group8_sum(wx); wy = group8_sum(wy); wz = group8_sum(wz);
        hx = group8_sum(hx); hy = group8_sum(hy); hz = group8_sum(hz);
        mx = group8_sum(mx); my = group8_sum(my); mz = group8_sum(mz);
        const float den = eps_denom_py(sw);
        f = sf / den;
        gx = ((hx - f * wx) + mx) / den;
        gy = ((hy - f * wy) + my) / den;
        gz = ((hz - f * wz) + mz) / den;
    }
    if (o.l == 0 && o.p < P) {
        bool still = false;
        if (live) {
            const float vx = f * gx, vy = f * gy, vz = f * gz;
            px -= vx; py -= vy; pz -= vz;
            still = sqrtf((vx * vx + vy * vy) + vz * vz) > 5e-4f;
        }
        pts_out[3 * o.p] = px; pts_out[3 * o.p + 1] = py; pts_out[3 * o.p + 2] = pz;
        live_out[o.p] = still ? 1 : 0;
    }
}

static int smoothing_grid(const char *who, int N, int64_t P, int K, const void *const *ptrs, int n_ptrs, dim3 &grid)
{
    if (N <= 0 || P < 0 || K < 1 || K + 1 > 40) {
        set_error("%s: bad sizes N=%d P=%lld K=%d (1 <= K, K + 1 <= 40)", who, N, (long long)P, K);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return 1;
    for (int i = 0; i < n_ptrs; ++i)
        if (!ptrs[i]) {
            set_error("%s: NULL tensor pointer", who);
            return DSS_ERR_INVALID_ARGUMENT;
        }
    const int64_t blocks = (P * SM_LANES + 255) / 256;
    if (blocks > 0x7fffffff) {
        set_error("%s: P=%lld too large", who, (long long)P);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    grid = dim3((unsigned)blocks);
    return DSS_OK;
}

}  // namespace dss

using namespace dss;

#define SM_DISPATCH(KERNEL, ...)                                                                              \
    switch ((K + SM_LANES - 1) / SM_LANES) {                                                                  \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, as_stream(stream), __VA_ARGS__); break;         \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, as_stream(stream), __VA_ARGS__); break;         \
    case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(256), 0, as_stream(stream), __VA_ARGS__); break;         \
    case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, as_stream(stream), __VA_ARGS__); break;         \
    default: hipLaunchKernelGGL(KERNEL<5>, grid, dim3(256), 0, as_stream(stream), __VA_ARGS__); break;        \
    }

extern "C" int dss_denoise_normals(const float *points, const float *normals, const float *knn_dists, const int64_t *knn_idx,
                                   const int64_t *first_idx, const int64_t *num_pts, const float *radius, int N, int64_t P,
                                   int K, float sharpness_sigma, float *out_normals, void *stream)
{
    const char *who = "dss_denoise_normals";
    if (!(sharpness_sigma > 0.f)) {
        set_error("%s: sharpness_sigma must be positive, got %g", who, (double)sharpness_sigma);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const void *ptrs[] = {points, normals, knn_dists, knn_idx, first_idx, num_pts, radius, out_normals};
    dim3 grid;
    const int rc = smoothing_grid(who, N, P, K, ptrs, 8, grid);
    if (rc) return rc < 0 ? rc : DSS_OK;
    SM_DISPATCH(denoise_normals_kernel, points, normals, knn_dists, knn_idx, first_idx, num_pts, radius, N, P, K,
                sharpness_sigma, out_normals)
    return check_launch(who);
}

extern "C" int dss_rimls_step(const float *points_in, const float *normals, const float *knn_dists, const int64_t *knn_idx,
                              const int64_t *first_idx, const int64_t *num_pts, const float *radius,
                              const uint8_t *live_in, int N, int64_t P, int K, int max_est_iter, float *points_out,
                              uint8_t *live_out, void *stream)
{
    const char *who = "dss_rimls_step";
    if (max_est_iter < 1) {
        set_error("%s: max_est_iter must be at least 1, got %d", who, max_est_iter);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if ((points_in && points_in == points_out) || (live_in && live_in == live_out)) {
        set_error("%s: points_out / live_out must not be points_in / live_in (a step reads the state of the step before)", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const void *ptrs[] = {points_in, normals, knn_dists, knn_idx, first_idx, num_pts, radius, points_out, live_out};
    dim3 grid;
    const int rc = smoothing_grid(who, N, P, K, ptrs, 9, grid);
    if (rc) return rc < 0 ? rc : DSS_OK;
    SM_DISPATCH(rimls_step_kernel, points_in, normals, knn_dists, knn_idx, first_idx, num_pts, radius, live_in, N, P, K,
                max_est_iter, points_out, live_out)
    return check_launch(who);
}
