// Points and normals on a triangle mesh's surface: the area-weighted sampler behind the reference's ground-truth cloud
// (scripts/create_mvr_data_from_mesh.py:174-181, pytorch3d's sample_points_from_meshes) and its gradient w.r.t. the
// vertices.  The rule is stated in include/dss_hip.h ("Surface samples of a triangle mesh"); every kernel below follows it
// operation for operation (the library builds with -ffp-contract=off -fno-fast-math).
//   mesh_sample_len_kernel    one thread per packed face: absent test, len = |(B - A) x (C - A)|, and the maximum of every
//                             mesh that holds the face (integer atomicMax on the bits: len >= 0, so exact and order-free)
//   mesh_sample_scan_kernel   one workgroup per mesh: integer keys by the mesh's power of two, inclusive uint64 scan in
//                             chunks of MESH_SAMPLE_CHUNK faces with a carried total
//   mesh_sample_draw_kernel   one thread per (mesh, sample): Philox, upper bound in cum, the four outputs
//   mesh_sample_backward_kernel  one thread per vertex: its segment of the sorted entry list, added front to back in fp32
// No float atomics, nothing read back to the host; the workspace is a function of (N, F).
#include "common.h"
#include "philox.h"

#define MESH_SAMPLE_THREADS 1024
#define MESH_SAMPLE_ITEMS 4
#define MESH_SAMPLE_CHUNK (MESH_SAMPLE_THREADS * MESH_SAMPLE_ITEMS)   // faces per step of the scan

namespace dss {

struct SampleArgs {
    const float *verts;                       // (V,3)
    const int64_t *faces, *f_first, *f_num;   // (F,3) packed vertex ids; (N,)
    int64_t V, F, S;
    int N;
    uint64_t seed;
    // workspace
    float *len;                               // (F,)
    uint64_t *cum;                            // (F,) inclusive sums of the keys within every mesh
    uint64_t *total;                          // (N,)
    uint32_t *len_max;                        // (N,) bits of the largest len; zero before the face pass
};

// mesh n's faces as a range of the packed array, empty unless it lies within [0, F)
__device__ __forceinline__ int64_t sample_mesh_range(const SampleArgs &A, int n, int64_t &first)
{
    first = A.f_first[n];
    const int64_t num = A.f_num[n];
    return first >= 0 && num > 0 && first <= A.F - num ? num : 0;
}

// (B - A) x (C - A) and its length, in the operations and order of mesh_flat_shade_kernel (mesh_raster.hip)
__device__ __forceinline__ float sample_face_normal(const float *a, const float *b, const float *c, float nrm[3])
{
    float u[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u[k] = b[k] - a[k];
        w[k] = c[k] - a[k];
    }
    nrm[0] = u[1] * w[2] - u[2] * w[1];
    nrm[1] = u[2] * w[0] - u[0] * w[2];
    nrm[2] = u[0] * w[1] - u[1] * w[0];
    return sqrtf((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
}

__device__ __forceinline__ bool sample_finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

__global__ __launch_bounds__(256) void mesh_sample_len_kernel(const SampleArgs A)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= A.F) return;
    const int64_t id[3] = {A.faces[3 * f], A.faces[3 * f + 1], A.faces[3 * f + 2]};
    float len = 0.0f;
    if ((uint64_t)id[0] < (uint64_t)A.V && (uint64_t)id[1] < (uint64_t)A.V && (uint64_t)id[2] < (uint64_t)A.V) {
        const float *a = A.verts + 3 * id[0], *b = A.verts + 3 * id[1], *c = A.verts + 3 * id[2];
        if (sample_finite3(a) && sample_finite3(b) && sample_finite3(c)) {
            float nrm[3];
            const float l = sample_face_normal(a, b, c, nrm);
            if (isfinite(l)) len = l;
        }
    }
    A.len[f] = len;
    if (len > 0.0f) {
        const uint32_t bits = __float_as_uint(len);
        for (int n = 0; n < A.N; ++n) {
            int64_t first;
            const int64_t num = sample_mesh_range(A, n, first);
            // the plain read only spares atomics: the maximum never falls, so a stale value costs one atomic more
            if (f >= first && f - first < num &&
                bits > __hip_atomic_load(A.len_max + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(A.len_max + n, bits);
        }
    }
}

__global__ __launch_bounds__(MESH_SAMPLE_THREADS) void mesh_sample_scan_kernel(const SampleArgs A)
{
    __shared__ uint64_t s_wave[MESH_SAMPLE_THREADS / DSS_WAVE];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & (DSS_WAVE - 1), wave = tid / DSS_WAVE;
    int64_t first;
    const int64_t num = sample_mesh_range(A, n, first);
    const float len_max = __uint_as_float(A.len_max[n]);
    if (num == 0 || !(len_max > 0.0f)) {   // (uniform over the workgroup)
        if (tid == 0) A.total[n] = 0;
        return;
    }
    int e;
    frexp((double)len_max, &e);
    uint64_t carry = 0;
    for (int64_t base = 0; base < num; base += MESH_SAMPLE_CHUNK) {
        const int64_t f0 = base + (int64_t)tid * MESH_SAMPLE_ITEMS;
        uint64_t k[MESH_SAMPLE_ITEMS];
        uint64_t run = 0;
#pragma unroll
        for (int j = 0; j < MESH_SAMPLE_ITEMS; ++j) {
            const float len = f0 + j < num ? A.len[first + f0 + j] : 0.0f;
            run += (uint64_t)floor(ldexp((double)len, 32 - e));
            k[j] = run;
        }
        uint64_t x = run;   // -> inclusive over the wavefront
#pragma unroll
        for (int o = 1; o < DSS_WAVE; o <<= 1) {
            const uint64_t v = __shfl_up((unsigned long long)x, (unsigned)o, DSS_WAVE);
            if (lane >= o) x += v;
        }
        if (lane == DSS_WAVE - 1) s_wave[wave] = x;
        __syncthreads();
        uint64_t before = carry, chunk = 0;
#pragma unroll
        for (int w = 0; w < MESH_SAMPLE_THREADS / DSS_WAVE; ++w) {
            const uint64_t t = s_wave[w];
            if (w < wave) before += t;
            chunk += t;
        }
        before += x - run;
#pragma unroll
        for (int j = 0; j < MESH_SAMPLE_ITEMS; ++j)
            if (f0 + j < num) A.cum[first + f0 + j] = before + k[j];
        carry += chunk;
        __syncthreads();   // s_wave is written again in the next step
    }
    if (tid == 0) A.total[n] = carry;
}

__global__ __launch_bounds__(256) void mesh_sample_draw_kernel(const SampleArgs A, float *__restrict__ points,
                                                               float *__restrict__ normals, int64_t *__restrict__ face_idx,
                                                               float *__restrict__ bary)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)A.N * A.S) return;
    const int n = (int)(i / A.S);
    const uint64_t s = (uint64_t)(i - (int64_t)n * A.S);
    int64_t first;
    const int64_t num = sample_mesh_range(A, n, first);
    const uint64_t total = num > 0 ? A.total[n] : 0;
    float p[3] = {0.f, 0.f, 0.f}, nh[3] = {0.f, 0.f, 0.f}, w[3] = {0.f, 0.f, 0.f};
    int64_t fl = -1;
    if (total > 0) {
        const Philox4 r = philox4x32_10((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)n, 0u, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
        const uint64_t target = __umul64hi(((uint64_t)r.r[0] << 32) | r.r[1], total);   // in [0, total)
        const uint64_t *cum = A.cum + first;
        int64_t lo = 0, hi = num - 1;          // cum[num - 1] = total > target: the answer is at most num - 1
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (cum[mid] > target) hi = mid;
            else lo = mid + 1;
        }
        fl = lo;
        // a face with a positive key is present: its ids are inside [0, V) and its vertices finite
        const int64_t f = first + fl;
        const float *a = A.verts + 3 * A.faces[3 * f], *b = A.verts + 3 * A.faces[3 * f + 1], *c = A.verts + 3 * A.faces[3 * f + 2];
        const float u1 = (float)(r.r[2] >> 8) * 0x1p-24f, u2 = (float)(r.r[3] >> 8) * 0x1p-24f;
        const float su = sqrtf(u1);
        w[0] = 1.0f - su;
        w[1] = su * (1.0f - u2);
        w[2] = su * u2;
        float nrm[3];
        const float len = sample_face_normal(a, b, c, nrm);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = (w[0] * a[k] + w[1] * b[k]) + w[2] * c[k];
            nh[k] = nrm[k] / len;
        }
    }
    face_idx[i] = fl;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        points[3 * i + k] = p[k];
        if (normals) normals[3 * i + k] = nh[k];
        if (bary) bary[3 * i + k] = w[k];
    }
}

struct SampleLists {
    const int64_t *faces, *f_first, *f_num, *face_idx;
    int64_t F, V, S, E;   // E = 3 N S entries
    int N;
};
#define SAMPLE_NO_KEY INT64_MAX

// packed id of the vertex that entry e = 3 (n S + s) + corner names; SAMPLE_NO_KEY for an entry of no face
__device__ __forceinline__ int64_t sample_vertex_entry(const SampleLists &l, int64_t e)
{
    if (e < 0 || e >= l.E) return SAMPLE_NO_KEY;
    const int64_t pair = e / 3;
    const int n = (int)(pair / l.S);
    const int64_t fl = l.face_idx[pair], first = l.f_first[n];
    if (fl < 0 || fl >= l.f_num[n] || first < 0 || first >= l.F - fl) return SAMPLE_NO_KEY;
    const int64_t v = l.faces[3 * (first + fl) + (e - 3 * pair)];
    return (uint64_t)v < (uint64_t)l.V ? v : SAMPLE_NO_KEY;
}

// as mesh_backward_kernel (knn.hip) walks a vertex's segment of order_v
__global__ __launch_bounds__(256) void mesh_sample_backward_kernel(const SampleLists l, const int64_t *__restrict__ order,
                                                                   const float *__restrict__ bary, const float *__restrict__ g_points,
                                                                   float *__restrict__ grad_verts)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= l.V) return;
    int64_t lo = 0, hi = l.E;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sample_vertex_entry(l, order[mid]) < v) lo = mid + 1;
        else hi = mid;
    }
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int64_t k = lo; k < l.E; ++k) {
        const int64_t e = order[k];
        if (sample_vertex_entry(l, e) != v) break;
        const float w = bary[e];
        const float *g = g_points + 3 * (e / 3);
        s0 += w * g[0]; s1 += w * g[1]; s2 += w * g[2];
    }
    grad_verts[3 * v] = s0; grad_verts[3 * v + 1] = s1; grad_verts[3 * v + 2] = s2;
}

// The regions of the workspace; base == nullptr: the size query
static size_t sample_carve(SampleArgs &A, void *base, int N, int64_t F)
{
    Bump ws{static_cast<char *>(base), 0};
    const size_t n = N > 0 ? (size_t)N : 1, f = F > 0 ? (size_t)F : 1;
    A.cum = ws.take<uint64_t>(f);
    A.total = ws.take<uint64_t>(n);
    A.len = ws.take<float>(f);
    A.len_max = ws.take<uint32_t>(n);
    return ws.used;
}

// What the entries refuse alike.  F, V < 2^31 as every mesh entry; N S <= 2^38 keeps the grid of the draw kernel and the
// entry ids 3 (n S + s) + c far inside their types.
static int sample_sizes(const char *who, int N, int64_t F, int64_t V, int64_t S)
{
    if (N <= 0 || N > 65535 || F < 0 || V < 0 || S < 0 || F >= ((int64_t)1 << 31) || V >= ((int64_t)1 << 31) ||
        S > ((int64_t)1 << 38) || (int64_t)N * S > ((int64_t)1 << 38)) {
        set_error("%s: bad sizes N=%d F=%lld V=%lld S=%lld (N in [1, 65535], F, V < 2^31, N S <= 2^38)", who, N, (long long)F,
                  (long long)V, (long long)S);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    return DSS_OK;
}

}  // namespace dss

using namespace dss;

extern "C" size_t dss_mesh_sample_workspace(int N, int64_t F)
{
    if (sample_sizes("dss_mesh_sample_workspace", N, F, 0, 0)) return 0;
    SampleArgs A;
    return sample_carve(A, nullptr, N, F);
}

extern "C" int dss_sample_mesh_surface(const float *verts, int64_t V, const int64_t *faces, const int64_t *f_first,
                                       const int64_t *f_num, int64_t F, int N, int64_t S, uint64_t seed, float *points,
                                       float *normals, int64_t *face_idx, float *bary, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *who = "dss_sample_mesh_surface";
    if (int rc = sample_sizes(who, N, F, V, S)) return rc;
    if (S == 0) return DSS_OK;
    if (!f_first || !f_num || !points || !face_idx || (V > 0 && !verts) || (F > 0 && !faces)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    SampleArgs A;
    const size_t need = sample_carve(A, nullptr, N, F);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, need %zu", who, workspace ? workspace_bytes : (size_t)0, need);
        return DSS_ERR_WORKSPACE;
    }
    sample_carve(A, workspace, N, F);
    A.verts = verts; A.faces = faces; A.f_first = f_first; A.f_num = f_num; A.V = V; A.F = F; A.S = S; A.N = N; A.seed = seed;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(A.len_max, 0, (size_t)N * sizeof(uint32_t), st) != hipSuccess) return check_launch(who);
    if (F > 0) hipLaunchKernelGGL(mesh_sample_len_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(mesh_sample_scan_kernel, dim3((unsigned)N), dim3(MESH_SAMPLE_THREADS), 0, st, A);
    const int64_t NS = (int64_t)N * S;
    hipLaunchKernelGGL(mesh_sample_draw_kernel, dim3((unsigned)((NS + 255) / 256)), dim3(256), 0, st, A, points, normals, face_idx, bary);
    return check_launch(who);
}

extern "C" int dss_mesh_sample_backward(const int64_t *faces, const int64_t *f_first, const int64_t *f_num, int64_t F, int N,
                                        int64_t S, int64_t V, const int64_t *face_idx, const float *bary, const int64_t *order,
                                        const float *g_points, float *grad_verts, void *stream)
{
    const char *who = "dss_mesh_sample_backward";
    if (int rc = sample_sizes(who, N, F, V, S)) return rc;
    if (V == 0) return DSS_OK;
    const int64_t E = 3 * (int64_t)N * S;
    if (!grad_verts || !f_first || !f_num || (E > 0 && (!face_idx || !bary || !order || !g_points)) || (F > 0 && !faces)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const SampleLists l = {faces, f_first, f_num, face_idx, F, V, S, E, N};
    hipLaunchKernelGGL(mesh_sample_backward_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, as_stream(stream), l, order, bary,
                       g_points, grad_verts);
    return check_launch(who);
}
