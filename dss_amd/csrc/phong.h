// The arithmetic of one shaded (camera, point, light) triple, stated once for the four kernels that need it:
// phong_kernel<false/true> (shading.hip), phong_camera_partial_kernel and phong_light_partial_kernel
// (camera_backward.hip).  The library builds with -ffp-contract=off -fno-fast-math, so every caller gets the same bits
// from the same inputs: the camera centre and the lights see the pair's values that the points see.  Notation: shading.hip.
#pragma once
#include "common.h"

namespace dss {

// What the four Phong entries are given, for all four kernels (a kernel ignores the fields it does not read)
struct PhongArgs {
    const float *world, *normals, *rgb;       // (Pw,3), (Pw,3), (P,3)
    const int64_t *first_idx, *num_pts;
    int N, shared, L, point_lights;
    int64_t Pw, P;                            // P = N * Pw packed rows for a shared cloud, otherwise Pw
    const float *ambient, *kd, *ks, *lvec;    // (N,3), (N,L,3), (N,L,3), (N,L,3) location or direction
    const float *cam;                         // (N,3) camera centres
    float shininess;
};

// shading.hip: what the four entries refuse alike -- bad sizes, then, only when there are points, a NULL input tensor --
// under the entry's name `who`; fills A.  The grid limits, the outputs and the workspaces are the entries' own.
int phong_args(const char *who, PhongArgs &A, const float *world, const float *normals, const float *rgb,
               const int64_t *first_idx, const int64_t *num_pts, int N, int64_t Pw, int shared_cloud, const float *ambient,
               const float *diffuse_color, const float *specular_color, const float *light_vec, int L, int point_lights,
               const float *cam_center, float shininess);

__device__ __forceinline__ float safe_norm(float x, float y, float z) { return fmaxf(sqrtf(x * x + y * y + z * z), 1e-6f); }

// h = a / max(|a|, eps): n^ of a normal, v^ of w = camera - x, d^ of u
__device__ __forceinline__ void unit(const float a[3], float h[3])
{
    const float an = safe_norm(a[0], a[1], a[2]);
    h[0] = a[0] / an; h[1] = a[1] / an; h[2] = a[2] / an;
}

// d/du of u / max(|u|, eps) applied to an upstream gradient g
__device__ __forceinline__ void normalize_backward(const float u[3], const float g[3], float out[3])
{
    const float raw = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);  // the clamp decision is safe_norm's, in fp32
    if (raw > 1e-6f) {
        // g - h (h . g) cancels in a component wherever g is nearly parallel to u there.  In fp32 the roundings of 1 / |u|, h
        // and h . g are amplified by that cancellation (an entry that cancels 1768-fold: 1.1e-4 of its absolute terms);
        // evaluated in fp64 from the fp32 inputs and rounded once, only the error of the inputs is (1.8e-5).
        const double ud[3] = {(double)u[0], (double)u[1], (double)u[2]};
        const double inv = 1.0 / sqrt(ud[0] * ud[0] + ud[1] * ud[1] + ud[2] * ud[2]);
        const double h[3] = {ud[0] * inv, ud[1] * inv, ud[2] * inv};
        const double dot = h[0] * (double)g[0] + h[1] * (double)g[1] + h[2] * (double)g[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = (float)(((double)g[i] - h[i] * dot) * inv);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = g[i] * 1e6f;  // clamped denominator: a constant scale
    }
}

// One light of one pair
struct PhongLight {
    float u[3], d[3], r[3];   // u = location - x or the direction, d^ = normalize(u), r = -d^ + 2 (n^ . d^) n^
    float ca, a0, alpha;      // n^ . d^, v^ . r, relu(a0) [ca > 0]
    bool lit;                 // ca > 0
};

__device__ __forceinline__ PhongLight phong_light(const PhongArgs &A, int n, int l, const float x[3], const float nh[3],
                                                  const float v[3])
{
    const float *lv = A.lvec + ((size_t)n * A.L + l) * 3;
    PhongLight t;
    t.u[0] = lv[0]; t.u[1] = lv[1]; t.u[2] = lv[2];
    if (A.point_lights) { t.u[0] -= x[0]; t.u[1] -= x[1]; t.u[2] -= x[2]; }
    unit(t.u, t.d);
    t.ca = nh[0] * t.d[0] + nh[1] * t.d[1] + nh[2] * t.d[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) t.r[i] = -t.d[i] + 2.0f * (t.ca * nh[i]);
    t.a0 = v[0] * t.r[0] + v[1] * t.r[1] + v[2] * t.r[2];
    t.lit = t.ca > 0.0f;
    t.alpha = t.lit ? fmaxf(t.a0, 0.0f) : 0.0f;
    return t;
}

// d loss / d a0 from gs = d loss / d S, S = alpha ^ shininess
__device__ __forceinline__ float phong_ga0(const PhongLight &t, float gs, float shininess)
{
    return (t.lit && t.a0 > 0.0f) ? gs * shininess * powf(t.alpha, shininess - 1.0f) : 0.0f;
}

// -> gdv = d loss / d d^ from gd = d loss / d D, D = relu(ca), and ga0; returns gca = d loss / d ca (the normal needs it)
__device__ __forceinline__ float phong_gdv(const PhongLight &t, const float nh[3], const float v[3], float gd, float ga0,
                                           float gdv[3])
{
    float gca = t.lit ? gd : 0.0f;
    const float gr_n = ga0 * (v[0] * nh[0] + v[1] * nh[1] + v[2] * nh[2]);
    gca += 2.0f * gr_n;                                           // r = ... + 2 ca n^
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gdv[i] = -ga0 * v[i];                                     // r = -d^ + ...
        gdv[i] += gca * nh[i];
    }
    return gca;
}

}  // namespace dss
