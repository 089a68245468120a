// Phong shading of the points: the reference's LightingTexture
// (DSS/core/texture.py:65-125) = apply_lighting (:26-63) with the diffuse / specular terms of
// DSS/core/lighting.py:10-77 and :80-172 for PointLights (:239-302, direction = location - point) or
// DirectionalLights (:175-236), L lights per cloud:
//     n^ = normalize(normal), d^ = normalize(direction)           (F.normalize, eps 1e-6)
//     diffuse  = sum_l kd_l * relu(n^ . d^)
//     specular = sum_l ks_l * (relu(v^ . (-d^ + 2 (n^ . d^) n^)) * [n^ . d^ > 0]) ^ shininess,  v^ = normalize(camera - x)
//     out      = rgb * (ambient + diffuse) + specular
// This is where the RGB loss reaches the NORMALS (and, through point lights and the view direction, the
// positions): the EWA terms are constants for autograd (rasterizer.py:562-565).  One thread per world point; a
// cloud shared by N cameras is looped in camera order (deterministic sums, no atomics).
// The arithmetic of a (camera, point, light) triple is phong.h's, shared with the camera and light reductions.
#include "phong.h"

namespace dss {

template <bool BACKWARD>
__global__ __launch_bounds__(256) void phong_kernel(const PhongArgs A, const float *__restrict__ grad_out,
                                                    float *__restrict__ out, float *__restrict__ grad_world,
                                                    float *__restrict__ grad_normals, float *__restrict__ grad_rgb)
{
    const int64_t wi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= A.Pw) return;
    const float x[3] = {A.world[3 * wi], A.world[3 * wi + 1], A.world[3 * wi + 2]};
    const float m[3] = {A.normals[3 * wi], A.normals[3 * wi + 1], A.normals[3 * wi + 2]};
    float nh[3];
    unit(m, nh);
    float gx[3] = {0.f, 0.f, 0.f}, gm[3] = {0.f, 0.f, 0.f};
    const int n_lo = A.shared ? 0 : find_cloud(wi, A.first_idx, A.num_pts, A.N);
    const int n_hi = A.shared ? A.N : n_lo + 1;
    if (n_lo < 0) {  // per-camera clouds, a packed point that no cloud owns: its row (index wi) is zeros in every output
        float *row = BACKWARD ? grad_rgb : out;
        if (row) { row[3 * wi] = 0.f; row[3 * wi + 1] = 0.f; row[3 * wi + 2] = 0.f; }
    }
    for (int n = max(n_lo, 0); n < n_hi && n_lo >= 0; ++n) {
        int64_t p = wi;
        if (A.shared) {
            if (wi >= A.num_pts[n]) continue;
            p = A.first_idx[n] + wi;
        }
        const float c[3] = {A.rgb[3 * p], A.rgb[3 * p + 1], A.rgb[3 * p + 2]};
        float g[3] = {0.f, 0.f, 0.f};
        if (BACKWARD) { g[0] = grad_out[3 * p]; g[1] = grad_out[3 * p + 1]; g[2] = grad_out[3 * p + 2]; }
        const float w[3] = {A.cam[3 * n] - x[0], A.cam[3 * n + 1] - x[1], A.cam[3 * n + 2] - x[2]};
        float v[3];
        unit(w, v);
        float dif[3] = {0.f, 0.f, 0.f}, spec[3] = {0.f, 0.f, 0.f};
        float gn[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f};  // d loss / d n^, d v^ (this camera)
        for (int l = 0; l < A.L; ++l) {
            const float *kd = A.kd + ((size_t)n * A.L + l) * 3;
            const float *ks = A.ks + ((size_t)n * A.L + l) * 3;
            const PhongLight t = phong_light(A, n, l, x, nh, v);
            const float D = fmaxf(t.ca, 0.0f);
            const float S = powf(t.alpha, A.shininess);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                dif[ch] += kd[ch] * D;
                spec[ch] += ks[ch] * S;
            }
            if (BACKWARD) {
                const float gd = g[0] * c[0] * kd[0] + g[1] * c[1] * kd[1] + g[2] * c[2] * kd[2];   // d loss / d D
                const float gs = g[0] * ks[0] + g[1] * ks[1] + g[2] * ks[2];                        // d loss / d S
                const float ga0 = phong_ga0(t, gs, A.shininess);
                float gdv[3];  // d loss / d d^
                const float gca = phong_gdv(t, nh, v, gd, ga0, gdv);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    gv[i] += ga0 * t.r[i];
                    gn[i] += 2.0f * t.ca * ga0 * v[i] + gca * t.d[i];
                }
                if (A.point_lights) {                           // u = location - x
                    float gu[3];
                    normalize_backward(t.u, gdv, gu);
#pragma unroll
                    for (int i = 0; i < 3; ++i) gx[i] -= gu[i];
                }
            }
        }
        const float *amb = A.ambient + 3 * n;
        if (!BACKWARD) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[3 * p + ch] = c[ch] * (amb[ch] + dif[ch]) + spec[ch];
        } else {
            if (grad_rgb) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) grad_rgb[3 * p + ch] = g[ch] * (amb[ch] + dif[ch]);
            }
            float gw[3], gmi[3];
            normalize_backward(w, gv, gw);                      // w = camera - x
            normalize_backward(m, gn, gmi);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                gx[i] -= gw[i];
                gm[i] += gmi[i];
            }
        }
    }
    if (BACKWARD) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (grad_world) grad_world[3 * wi + i] = gx[i];
            if (grad_normals) grad_normals[3 * wi + i] = gm[i];
        }
    }
}

int phong_args(const char *who, PhongArgs &A, const float *world, const float *normals, const float *rgb,
               const int64_t *first_idx, const int64_t *num_pts, int N, int64_t Pw, int shared_cloud, const float *ambient,
               const float *diffuse_color, const float *specular_color, const float *light_vec, int L, int point_lights,
               const float *cam_center, float shininess)
{
    if (N <= 0 || Pw < 0 || L < 0) {
        set_error("%s: bad sizes N=%d Pw=%lld L=%d", who, N, (long long)Pw, L);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (Pw > 0 && (!world || !normals || !rgb || !first_idx || !num_pts || !ambient || !cam_center ||
                   (L > 0 && (!diffuse_color || !specular_color || !light_vec)))) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    A.world = world; A.normals = normals; A.rgb = rgb; A.first_idx = first_idx; A.num_pts = num_pts; A.N = N;
    A.shared = shared_cloud; A.L = L; A.point_lights = point_lights; A.Pw = Pw; A.P = shared_cloud ? (int64_t)N * Pw : Pw;
    A.ambient = ambient; A.kd = diffuse_color; A.ks = specular_color; A.lvec = light_vec; A.cam = cam_center;
    A.shininess = shininess;
    return DSS_OK;
}

}  // namespace dss

using namespace dss;

extern "C" int dss_phong_forward(const float *world, const float *normals, const float *rgb, const int64_t *first_idx,
                                 const int64_t *num_pts, int N, int64_t Pw, int shared_cloud, const float *ambient,
                                 const float *diffuse_color, const float *specular_color, const float *light_vec, int L,
                                 int point_lights, const float *cam_center, float shininess, float *out, void *stream)
{
    PhongArgs A;
    int rc = phong_args("dss_phong_forward", A, world, normals, rgb, first_idx, num_pts, N, Pw, shared_cloud, ambient,
                        diffuse_color, specular_color, light_vec, L, point_lights, cam_center, shininess);
    if (rc) return rc;
    if (Pw == 0) return DSS_OK;
    if (!out) { set_error("dss_phong_forward: NULL output"); return DSS_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(phong_kernel<false>, dim3((unsigned)((Pw + 255) / 256)), dim3(256), 0, as_stream(stream), A, nullptr,
                       out, nullptr, nullptr, nullptr);
    return check_launch("dss_phong_forward");
}

extern "C" int dss_phong_backward(const float *grad_out, const float *world, const float *normals, const float *rgb,
                                  const int64_t *first_idx, const int64_t *num_pts, int N, int64_t Pw, int shared_cloud,
                                  const float *ambient, const float *diffuse_color, const float *specular_color,
                                  const float *light_vec, int L, int point_lights, const float *cam_center,
                                  float shininess, float *grad_world, float *grad_normals, float *grad_rgb, void *stream)
{
    PhongArgs A;
    int rc = phong_args("dss_phong_backward", A, world, normals, rgb, first_idx, num_pts, N, Pw, shared_cloud, ambient,
                        diffuse_color, specular_color, light_vec, L, point_lights, cam_center, shininess);
    if (rc) return rc;
    if (Pw == 0) return DSS_OK;
    if (!grad_out) { set_error("dss_phong_backward: NULL grad_out"); return DSS_ERR_INVALID_ARGUMENT; }
    hipLaunchKernelGGL(phong_kernel<true>, dim3((unsigned)((Pw + 255) / 256)), dim3(256), 0, as_stream(stream), A, grad_out,
                       nullptr, grad_world, grad_normals, grad_rgb);
    return check_launch("dss_phong_backward");
}
