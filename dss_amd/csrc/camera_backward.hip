// Camera gradients for gfx950: the render differentiated w.r.t. the camera matrices and the camera centre.
//
// In the reference the cameras are ordinary tensors of the autograd graph: SurfaceSplatting.forward projects with
// pytorch3d's transform (DSS/core/rasterizer.py:614), EllipticalRasterizer.backward hands pts_grad back to it (:975-977)
// and the clip hook (:667-673) sits on that same tensor; LightingTexture passes cameras.get_camera_center() to the
// specular term (DSS/core/texture.py:65-125, lighting.py:80-172).  Two reductions over the (camera, point) pairs:
//
//   dss_camera_backward        row-vector convention, x = (x, y, z, 1), clip = x @ M[n], ndc = clip.xy / clip.w,
//                              view_z = (x @ V[n]).z, g = the pair's (clipped) screen gradient, 0 where valid == 0:
//                                  grad_M[n][:, 0] = sum_p x gx / w          grad_M[n][:, 1] = sum_p x gy / w
//                                  grad_M[n][:, 3] = sum_p x (-(gx ndc_x + gy ndc_y) / w)       grad_M[n][:, 2] = 0
//                                  grad_V[n][:, 2] = sum_p x gz              (the other columns of grad_V are 0)
//   dss_phong_backward_camera  grad_cam[n] = + sum_p gw(n, p), gw = the gradient of w = camera - x that phong_kernel<true>
//                              (shading.hip) subtracts from the point's gradient; the pair's arithmetic is phong.h's for
//                              that kernel and the two Phong kernels here alike.
//   dss_phong_backward_lights  the same shading differentiated w.r.t. the LIGHTS, which the reference keeps on the tape
//                              (DSS/core/texture.py:25-63, :118-122; DSS/core/lighting.py:10-77, :80-172, :175-302):
//                                  grad_ambient[n]     = sum_p g c            grad_diffuse[n][l]   = sum_p g c D_l
//                                  grad_specular[n][l] = sum_p g S_l          grad_light_vec[n][l] = sum_p normalize_backward(u_l, gdv_l)
//                              in the notation of phong_kernel<true> (g = grad_out, c = rgb of the pair).
//
// All are bitwise reproducible (no atomics) and do not depend on the device they run on: a fixed assignment of
// (camera, point range) to workgroups that is a function of the sizes only (`reduce_plan`), per-thread fp32 sums over a
// bounded run of points, a fixed wave tree (DPP) and workgroup tree (LDS), ONE partial per workgroup stored to the
// workspace, and a second small launch that adds the partials of every row (a camera, or a (camera, light)) in index order
// in fp64 and writes fp32.  The launch boundary is the hand-off between the two stages: no flags, no fences, no counters
// to re-initialise.
#include "phong.h"

namespace dss {

constexpr int RB_BLOCK = 256;              // threads of a workgroup of either stage
constexpr int RB_WAVES = RB_BLOCK / DSS_WAVE;
constexpr int RB_CAP = 512;                // most partials per camera

// `units` of work per camera (groups of four points, or pairs) at RB_BLOCK units per workgroup and sweep: `sweeps` per
// thread so that a camera has at most RB_CAP workgroups (= partials).  A function of the sizes only.
struct ReducePlan {
    int sweeps, blocks;
};
static ReducePlan reduce_plan(int64_t units)
{
    ReducePlan pl;
    const int64_t per = (units + RB_BLOCK - 1) / RB_BLOCK;                 // workgroups at one sweep
    pl.sweeps = (int)((per + RB_CAP - 1) / RB_CAP);
    if (pl.sweeps < 1) pl.sweeps = 1;
    pl.blocks = (int)((per + pl.sweeps - 1) / pl.sweeps);
    return pl;
}
// 16-byte groups of four packed points that can overlap a camera's range of at most `pc` points (first_idx is not
// aligned to four: one group more than pc / 4 rounded up)
static int64_t point_groups(int64_t pc) { return (pc + 3) / 4 + 1; }

// Sum of W values per thread over the workgroup in a fixed order -> dst[0..W) (the workgroup's partial)
template <int W>
__device__ __forceinline__ void block_sum_store(const float (&acc)[W], float *__restrict__ dst)
{
    __shared__ float part[RB_WAVES][W];
    const int lane = threadIdx.x & (DSS_WAVE - 1), wave = threadIdx.x / DSS_WAVE;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        const float s = wave_sum(acc[e]);
        if (lane == 0) part[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int e = threadIdx.x;
        dst[e] = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
    }
}
static_assert(RB_WAVES == 4, "block_sum_store adds four waves");

// One valid pair of dss_camera_backward.  The projection and the clip are the arithmetic of project_backward_kernel
// (setup.hip), so that the cameras see the clipped gradient the points see.
__device__ __forceinline__ void camera_pair(float (&acc)[16], const float x, const float y, const float z,
                                            const float *__restrict__ m, float gx, float gy, float gz, const float clip)
{
    const float cx = x * m[0] + y * m[4] + z * m[8] + m[12];
    const float cy = x * m[1] + y * m[5] + z * m[9] + m[13];
    const float w = x * m[3] + y * m[7] + z * m[11] + m[15];
    const float iw = 1.0f / w;
    const float nx = cx * iw, ny = cy * iw;
    if (clip > 0.0f) {  // the per-point norm clip hook (rasterizer.py:667-673), same arithmetic as clip_grad_kernel
        const float nrm = sqrtf(gx * gx + gy * gy + gz * gz);
        const float sc = fminf(nrm, clip), den = fmaxf(nrm, 1e-12f);
        gx = gx / den * sc;
        gy = gy / den * sc;
        gz = gz / den * sc;
    }
    const float a0 = gx * iw, a1 = gy * iw, a3 = -(gx * nx + gy * ny) * iw;
    acc[0] += x * a0;  acc[1] += y * a0;  acc[2] += z * a0;  acc[3] += a0;     // grad_M[:, 0]
    acc[4] += x * a1;  acc[5] += y * a1;  acc[6] += z * a1;  acc[7] += a1;     // grad_M[:, 1]
    acc[8] += x * a3;  acc[9] += y * a3;  acc[10] += z * a3; acc[11] += a3;    // grad_M[:, 3]
    acc[12] += x * gz; acc[13] += y * gz; acc[14] += z * gz; acc[15] += gz;    // grad_V[:, 2]
}

// Stage 1 of dss_camera_backward: workgroup (b, n) sums the pairs of camera n in its share of the camera's packed range.
// A thread takes groups of FOUR consecutive packed points aligned to four in the packed order: their screen gradients are
// three 16-byte loads and their flags one 4-byte load whatever first_idx[n] is (a group that straddles two cameras is
// read by both, each keeping its own points).  `vec` = 0 (pointers not aligned) takes the scalar loads for every group.
__global__ __launch_bounds__(RB_BLOCK) void camera_partial_kernel(
    const float *__restrict__ world, const float *__restrict__ M, const int64_t *__restrict__ first_idx,
    const int64_t *__restrict__ num_pts, int64_t Pw, int64_t P, int shared, const float *__restrict__ grad_screen,
    const uint8_t *__restrict__ valid, float clip, int sweeps, int vec, float *__restrict__ partials)
{
    const int n = blockIdx.y;
    const float *m = M + 16 * n;
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int64_t f = first_idx[n];
    const int64_t lo = max(f, (int64_t)0), hi = min(f + num_pts[n], P);     // the camera's packed range [lo, hi)
    if (lo < hi) {
        const int64_t g_first = lo >> 2, g_last = (hi - 1) >> 2;
        for (int s = 0; s < sweeps; ++s) {
            const int64_t g = g_first + ((int64_t)blockIdx.x * sweeps + s) * RB_BLOCK + threadIdx.x;
            if (g > g_last) break;
            const int64_t p0 = g << 2;
            float gs[4][3];
            uint8_t vl[4];
            if (vec && p0 + 4 <= P) {
                const float4 q0 = *reinterpret_cast<const float4 *>(grad_screen + 3 * p0);
                const float4 q1 = *reinterpret_cast<const float4 *>(grad_screen + 3 * p0 + 4);
                const float4 q2 = *reinterpret_cast<const float4 *>(grad_screen + 3 * p0 + 8);
                const uint32_t v4 = *reinterpret_cast<const uint32_t *>(valid + p0);
                gs[0][0] = q0.x; gs[0][1] = q0.y; gs[0][2] = q0.z;
                gs[1][0] = q0.w; gs[1][1] = q1.x; gs[1][2] = q1.y;
                gs[2][0] = q1.z; gs[2][1] = q1.w; gs[2][2] = q2.x;
                gs[3][0] = q2.y; gs[3][1] = q2.z; gs[3][2] = q2.w;
#pragma unroll
                for (int k = 0; k < 4; ++k) vl[k] = (uint8_t)((v4 >> (8 * k)) & 0xffu);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t p = min(p0 + k, P - 1);                   // (a valid address: masked below)
                    vl[k] = valid[p];
                    gs[k][0] = grad_screen[3 * p]; gs[k][1] = grad_screen[3 * p + 1]; gs[k][2] = grad_screen[3 * p + 2];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t p = p0 + k;
                if (p < lo || p >= hi || !vl[k]) continue;
                const int64_t wi = shared ? p - f : p;
                if (wi >= Pw) continue;
                camera_pair(acc, world[3 * wi], world[3 * wi + 1], world[3 * wi + 2], m, gs[k][0], gs[k][1], gs[k][2], clip);
            }
        }
    }
    block_sum_store<16>(acc, partials + ((size_t)n * gridDim.x + blockIdx.x) * 16);
}

// Stage 1 of dss_phong_backward_camera: one (camera, point) pair per lane and sweep.  The pair's gv (d loss / d v^) and
// gw = normalize_backward(w, gv) are those of phong_kernel<true> (shading.hip) through phong.h, keeping only the terms
// gv depends on (the specular chain; the diffuse colour and the point's rgb do not reach it).
__global__ __launch_bounds__(RB_BLOCK) void phong_camera_partial_kernel(const PhongArgs A, const float *__restrict__ grad_out,
                                                                        int sweeps, float *__restrict__ partials)
{
    const int n = blockIdx.y;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int64_t f = A.first_idx[n];
    const int64_t lo = max(f, (int64_t)0), hi = min(f + A.num_pts[n], A.P);
    for (int s = 0; s < sweeps; ++s) {
        const int64_t p = lo + ((int64_t)blockIdx.x * sweeps + s) * RB_BLOCK + threadIdx.x;
        if (p >= hi) break;
        const int64_t wi = A.shared ? p - f : p;
        if (wi >= A.Pw) continue;
        const float x[3] = {A.world[3 * wi], A.world[3 * wi + 1], A.world[3 * wi + 2]};
        const float m[3] = {A.normals[3 * wi], A.normals[3 * wi + 1], A.normals[3 * wi + 2]};
        const float g[3] = {grad_out[3 * p], grad_out[3 * p + 1], grad_out[3 * p + 2]};
        const float w[3] = {A.cam[3 * n] - x[0], A.cam[3 * n + 1] - x[1], A.cam[3 * n + 2] - x[2]};
        float nh[3], v[3];
        unit(m, nh);
        unit(w, v);
        float gv[3] = {0.f, 0.f, 0.f};
        for (int l = 0; l < A.L; ++l) {
            const float *ks = A.ks + ((size_t)n * A.L + l) * 3;
            const PhongLight t = phong_light(A, n, l, x, nh, v);
            const float gs = g[0] * ks[0] + g[1] * ks[1] + g[2] * ks[2];                        // d loss / d S
            const float ga0 = phong_ga0(t, gs, A.shininess);
#pragma unroll
            for (int i = 0; i < 3; ++i) gv[i] += ga0 * t.r[i];
        }
        float gw[3];
        normalize_backward(w, gv, gw);                          // w = camera - x
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[i] += gw[i];
    }
    block_sum_store<4>(acc, partials + ((size_t)n * gridDim.x + blockIdx.x) * 4);
}

// The 16-float slot of one (camera, light) of dss_phong_backward_lights: [g_kd(3), g_ks(3), g_vec(3), g_amb(3), pad(4)];
// g_amb is carried by light 0 only (zeros in the other slots).  L == 0: one slot per camera with the ambient term alone.
constexpr int LS_W = 16, LS_KD = 0, LS_KS = 3, LS_VEC = 6, LS_AMB = 9;

// Stage 1 of dss_phong_backward_lights: workgroup (b, n, l) sums ONE light's terms over its share of camera n's pairs, one
// pair per lane and sweep; gridDim.z = max(L, 1) and its partial lands in slot n * gridDim.z + l, so that stage 2 sees the
// slots as rows.  L is a launch dimension, not a template argument, so the cost per thread does not depend on it: 12 live
// fp32 accumulators (the pad of the slot is a constant zero) next to the ~40 values of one pair and one light -- 72 VGPRs
// as compiled for gfx950, no scratch -- and 64 floats of LDS per WORKGROUP (block_sum_store<16>), a quarter of a float per
// thread.  The price is that every light re-reads the pair (48 bytes) and re-normalises n^ and v^; accumulating all lights
// in one pass would need 9 L + 3 accumulators per thread, i.e. either a kernel per L or 16 L floats of LDS per thread.
// The pair's D, S and gdv (d loss / d d^) are those of phong_kernel<true> (shading.hip) through phong.h, for the one light
// of this workgroup: the sums over lights of that kernel (dif, spec, gn, gv) do not reach these outputs.
__global__ __launch_bounds__(RB_BLOCK) void phong_light_partial_kernel(const PhongArgs A, const float *__restrict__ grad_out,
                                                                       int sweeps, float *__restrict__ partials)
{
    const int n = blockIdx.y, l = blockIdx.z;
    float acc[LS_W];
#pragma unroll
    for (int e = 0; e < LS_W; ++e) acc[e] = 0.f;
    const int64_t f = A.first_idx[n];
    const int64_t lo = max(f, (int64_t)0), hi = min(f + A.num_pts[n], A.P);
    for (int s = 0; s < sweeps; ++s) {
        const int64_t p = lo + ((int64_t)blockIdx.x * sweeps + s) * RB_BLOCK + threadIdx.x;
        if (p >= hi) break;
        const int64_t wi = A.shared ? p - f : p;
        if (wi >= A.Pw) continue;
        const float c[3] = {A.rgb[3 * p], A.rgb[3 * p + 1], A.rgb[3 * p + 2]};
        const float g[3] = {grad_out[3 * p], grad_out[3 * p + 1], grad_out[3 * p + 2]};
        if (l == 0) {                                           // out = c * (ambient + ...) + ...
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[LS_AMB + ch] += g[ch] * c[ch];
        }
        if (A.L == 0) continue;
        const float x[3] = {A.world[3 * wi], A.world[3 * wi + 1], A.world[3 * wi + 2]};
        const float m[3] = {A.normals[3 * wi], A.normals[3 * wi + 1], A.normals[3 * wi + 2]};
        const float w[3] = {A.cam[3 * n] - x[0], A.cam[3 * n + 1] - x[1], A.cam[3 * n + 2] - x[2]};
        float nh[3], v[3];
        unit(m, nh);
        unit(w, v);
        const float *kd = A.kd + ((size_t)n * A.L + l) * 3;
        const float *ks = A.ks + ((size_t)n * A.L + l) * 3;
        const PhongLight t = phong_light(A, n, l, x, nh, v);
        const float D = fmaxf(t.ca, 0.0f);
        const float S = powf(t.alpha, A.shininess);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            acc[LS_KD + ch] += g[ch] * c[ch] * D;               // dif += kd * D, out = c * (... + dif)
            acc[LS_KS + ch] += g[ch] * S;                       // spec += ks * S
        }
        const float gd = g[0] * c[0] * kd[0] + g[1] * c[1] * kd[1] + g[2] * c[2] * kd[2];   // d loss / d D
        const float gs = g[0] * ks[0] + g[1] * ks[1] + g[2] * ks[2];                        // d loss / d S
        float gdv[3], gu[3];  // d loss / d d^, d u
        phong_gdv(t, nh, v, gd, phong_ga0(t, gs, A.shininess), gdv);
        normalize_backward(t.u, gdv, gu);                       // u = location - x, or the direction itself
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[LS_VEC + i] += gu[i];
    }
    block_sum_store<LS_W>(acc, partials + (((size_t)n * gridDim.z + l) * gridDim.x + blockIdx.x) * LS_W);
}

// Stage 2 of all three: a workgroup adds the `blocks` partials (W floats each) of row `row` in fp64 -- RB_BLOCK / W contiguous
// runs of the index range in parallel, each in index order, then the runs in order -- and rounds to fp32 once.
// -> total[0..W) in LDS, visible to every thread of the workgroup.
template <int W>
__device__ __forceinline__ const float *row_total(const float *__restrict__ partials, int blocks, int row)
{
    constexpr int RUNS = RB_BLOCK / W;
    __shared__ double run_sum[RUNS][W];
    __shared__ float total[W];
    const int e = threadIdx.x % W, j = threadIdx.x / W;
    const int i0 = (int)((int64_t)blocks * j / RUNS), i1 = (int)((int64_t)blocks * (j + 1) / RUNS);
    const float *src = partials + (size_t)row * blocks * W;
    double s = 0.0;
    for (int i = i0; i < i1; ++i) s += (double)src[(size_t)i * W + e];
    run_sum[j][e] = s;
    __syncthreads();
    if (threadIdx.x < W) {
        double t = 0.0;
        for (int r = 0; r < RUNS; ++r) t += run_sum[r][threadIdx.x];
        total[threadIdx.x] = (float)t;
    }
    __syncthreads();
    return total;
}

// Stage 2 of the two camera entries: workgroup n = camera n.
//   CAMERA: W = 16 -> grad_M[n], grad_V[n] (4,4) fully written, zeros included;  otherwise W = 4 -> grad_cam[n] (3).
template <int W, bool CAMERA>
__global__ __launch_bounds__(RB_BLOCK) void sum_partials_kernel(const float *__restrict__ partials, int blocks,
                                                                float *__restrict__ out0, float *__restrict__ out1)
{
    const int n = blockIdx.x;
    const float *total = row_total<W>(partials, blocks, n);
    if (CAMERA) {
        if (threadIdx.x < 16) {
            const int r = threadIdx.x >> 2, c = threadIdx.x & 3;                 // entry [r][c] of both matrices
            out0[16 * n + threadIdx.x] = c == 0 ? total[r] : c == 1 ? total[4 + r] : c == 3 ? total[8 + r] : 0.0f;
            out1[16 * n + threadIdx.x] = c == 2 ? total[12 + r] : 0.0f;
        }
    } else if (threadIdx.x < 3) {
        out0[3 * n + threadIdx.x] = total[threadIdx.x];
    }
}

// Stage 2 of dss_phong_backward_lights: workgroup n * slots + l = slot (camera n, light l), slots = max(L, 1).  Every
// non-NULL output entry is written by exactly one thread of one workgroup (blocks == 0: exact zeros).
__global__ __launch_bounds__(RB_BLOCK) void sum_light_partials_kernel(const float *__restrict__ partials, int blocks, int L,
                                                                      float *__restrict__ grad_ambient,
                                                                      float *__restrict__ grad_diffuse,
                                                                      float *__restrict__ grad_specular,
                                                                      float *__restrict__ grad_light_vec)
{
    const int row = blockIdx.x, slots = max(L, 1);
    const int n = row / slots, l = row - n * slots;
    const float *total = row_total<LS_W>(partials, blocks, row);
    const int e = threadIdx.x;
    if (e >= 12) return;
    const int i = e % 3;
    if (e >= LS_AMB) {
        if (l == 0 && grad_ambient) grad_ambient[3 * n + i] = total[e];
    } else if (L > 0) {
        float *out = e < LS_KS ? grad_diffuse : e < LS_VEC ? grad_specular : grad_light_vec;
        if (out) out[3 * (size_t)row + i] = total[e];
    }
}

}  // namespace dss

using namespace dss;

// Partials of the largest launch either entry makes for (N, P): a camera of a cloud that is not shared can own all P points.
// (dss_phong_backward_camera stores 4 floats per partial and has at most four times the workgroups: it fits as well.)
extern "C" size_t dss_camera_backward_workspace(int N, int64_t P)
{
    if (N <= 0 || P < 0) return 0;
    int64_t per = (point_groups(P) + RB_BLOCK - 1) / RB_BLOCK;                 // >= reduce_plan(...).blocks, monotonic in P
    if (per > RB_CAP) per = RB_CAP;
    return align_up((size_t)N * (size_t)per * 16 * sizeof(float), 256);
}

extern "C" int dss_camera_backward(const float *world, const float *M, const float *V, const int64_t *first_idx,
                                   const int64_t *num_pts, int N, int64_t Pw, int shared_cloud, const float *grad_screen,
                                   const uint8_t *valid, float clip, float *grad_M, float *grad_V, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    if (N <= 0 || N > 65535 || Pw < 0) {
        set_error("dss_camera_backward: bad sizes N=%d Pw=%lld", N, (long long)Pw);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (!M || !V || !first_idx || !num_pts || !grad_M || !grad_V || (Pw > 0 && (!world || !grad_screen || !valid))) {
        set_error("dss_camera_backward: NULL tensor pointer");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const int64_t P = shared_cloud ? (int64_t)N * Pw : Pw;
    const ReducePlan pl = reduce_plan(point_groups(Pw));   // (a camera holds at most Pw of the points either way)
    const int blocks = Pw > 0 ? pl.blocks : 0;
    const size_t need = dss_camera_backward_workspace(N, P);   // >= N * blocks * 16 floats
    if (!workspace || workspace_bytes < need) {
        set_error("dss_camera_backward: workspace %zu bytes < required %zu", workspace_bytes, need);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    float *partials = static_cast<float *>(workspace);
    if (blocks > 0) {
        const int vec = (reinterpret_cast<uintptr_t>(grad_screen) & 15) == 0 && (reinterpret_cast<uintptr_t>(valid) & 3) == 0;
        hipLaunchKernelGGL(camera_partial_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(RB_BLOCK), 0, as_stream(stream), world,
                           M, first_idx, num_pts, Pw, P, shared_cloud, grad_screen, valid, clip, pl.sweeps, vec, partials);
        const int rc = check_launch("dss_camera_backward");
        if (rc) return rc;
    }
    hipLaunchKernelGGL((sum_partials_kernel<16, true>), dim3((unsigned)N), dim3(RB_BLOCK), 0, as_stream(stream), partials, blocks,
                       grad_M, grad_V);
    return check_launch("dss_camera_backward");
}

extern "C" int dss_phong_backward_camera(const float *grad_out, const float *world, const float *normals, const float *rgb,
                                         const int64_t *first_idx, const int64_t *num_pts, int N, int64_t Pw, int shared_cloud,
                                         const float *ambient, const float *diffuse_color, const float *specular_color,
                                         const float *light_vec, int L, int point_lights, const float *cam_center,
                                         float shininess, float *grad_cam, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N > 65535) {                                            // cameras are gridDim.y
        set_error("dss_phong_backward_camera: bad sizes N=%d Pw=%lld L=%d", N, (long long)Pw, L);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    PhongArgs A;
    int rc = phong_args("dss_phong_backward_camera", A, world, normals, rgb, first_idx, num_pts, N, Pw, shared_cloud, ambient,
                        diffuse_color, specular_color, light_vec, L, point_lights, cam_center, shininess);
    if (rc) return rc;
    if (!first_idx || !num_pts || !cam_center || !grad_cam || (Pw > 0 && !grad_out)) {   // needed without points as well
        set_error("dss_phong_backward_camera: NULL tensor pointer");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const ReducePlan pl = reduce_plan(Pw);
    const int blocks = Pw > 0 ? pl.blocks : 0;
    const size_t need = dss_camera_backward_workspace(N, A.P);   // >= N * blocks * 4 floats
    if (!workspace || workspace_bytes < need) {
        set_error("dss_phong_backward_camera: workspace %zu bytes < required %zu", workspace_bytes, need);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    float *partials = static_cast<float *>(workspace);
    if (blocks > 0) {
        hipLaunchKernelGGL(phong_camera_partial_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(RB_BLOCK), 0, as_stream(stream),
                           A, grad_out, pl.sweeps, partials);
        rc = check_launch("dss_phong_backward_camera");
        if (rc) return rc;
    }
    hipLaunchKernelGGL((sum_partials_kernel<4, false>), dim3((unsigned)N), dim3(RB_BLOCK), 0, as_stream(stream), partials, blocks,
                       grad_cam, nullptr);
    return check_launch("dss_phong_backward_camera");
}

// One 16-float slot per (camera, light) and workgroup (L == 0: per camera), at most RB_CAP workgroups per camera.
extern "C" size_t dss_phong_backward_lights_workspace(int N, int64_t P, int L)
{
    if (N <= 0 || P < 0 || L < 0) return 0;
    int64_t per = (P + RB_BLOCK - 1) / RB_BLOCK;                               // >= reduce_plan(Pw).blocks for Pw <= P
    if (per > RB_CAP) per = RB_CAP;
    return align_up((size_t)N * (size_t)(L > 0 ? L : 1) * (size_t)per * LS_W * sizeof(float), 256);
}

extern "C" int dss_phong_backward_lights(const float *grad_out, const float *world, const float *normals, const float *rgb,
                                         const int64_t *first_idx, const int64_t *num_pts, int N, int64_t Pw, int shared_cloud,
                                         const float *ambient, const float *diffuse_color, const float *specular_color,
                                         const float *light_vec, int L, int point_lights, const float *cam_center,
                                         float shininess, float *grad_ambient, float *grad_diffuse, float *grad_specular,
                                         float *grad_light_vec, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N > 65535 || L > 65535) {                               // cameras are gridDim.y, lights gridDim.z
        set_error("dss_phong_backward_lights: bad sizes N=%d Pw=%lld L=%d", N, (long long)Pw, L);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    PhongArgs A;
    int rc = phong_args("dss_phong_backward_lights", A, world, normals, rgb, first_idx, num_pts, N, Pw, shared_cloud, ambient,
                        diffuse_color, specular_color, light_vec, L, point_lights, cam_center, shininess);
    if (rc) return rc;
    if (!first_idx || !num_pts || !cam_center || (Pw > 0 && !grad_out)) {                 // needed without points as well
        set_error("dss_phong_backward_lights: NULL tensor pointer");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const ReducePlan pl = reduce_plan(Pw);
    const int blocks = Pw > 0 ? pl.blocks : 0;
    const int slots = L > 0 ? L : 1;
    const size_t need = dss_phong_backward_lights_workspace(N, A.P, L);   // >= N * slots * blocks * 16 floats
    if (!workspace || workspace_bytes < need) {
        set_error("dss_phong_backward_lights: workspace %zu bytes < required %zu", workspace_bytes, need);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    float *partials = static_cast<float *>(workspace);
    if (blocks > 0) {
        hipLaunchKernelGGL(phong_light_partial_kernel, dim3((unsigned)blocks, (unsigned)N, (unsigned)slots), dim3(RB_BLOCK), 0,
                           as_stream(stream), A, grad_out, pl.sweeps, partials);
        rc = check_launch("dss_phong_backward_lights");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(sum_light_partials_kernel, dim3((unsigned)N * (unsigned)slots), dim3(RB_BLOCK), 0, as_stream(stream),
                       partials, blocks, L, grad_ambient, grad_diffuse, grad_specular, grad_light_vec);
    return check_launch("dss_phong_backward_lights");
}
