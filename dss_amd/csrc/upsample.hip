// One round of sparsity upsampling (DSS/core/cloud.py:555-632 `upsample`): the per-point K x K sparsity search
// (dss_upsample_candidates) and the assembly of the grown cloud (dss_upsample_insert).  The selection between the two is one
// integer sort of the keys written here, done by the caller (dss_amd/cloud_ops.py).
//
// The contract of a round, for point p with the neighbours q_0 .. q_{K-1} = entries 1 .. K of its
// dss_knn_points(K + 1) list (self dropped, (distance, id) order):
//   mid_j = (q_j + 2 p) / 3          m_j = min_l |mid_j - q_l|^2, l = 0 .. K-1, in the form (dx dx + dy dy) + dz dz
//   s(p) = max_j m_j                 j*(p) = the SMALLEST j that attains it
// Every operation is a separately rounded fp32 operation (the Makefile's -ffp-contract=off), so the numpy restatement in
// tests/upsample_reference.py can be compared value by value.
#include <float.h>
#include "common.h"

namespace dss {

// Value of lane J of every 16-lane row in all lanes of that row: one DPP move (row_newbcast, gfx90a and later), plain VALU.
template <int J>
__device__ __forceinline__ float row_bcast16(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + J, 0xf, 0xf, true));
}

// Value of lane j of every G-lane group in all lanes of that group, G = 32 or 64: j is wave-uniform, so the lane select of
// v_readlane is a scalar; no LDS round trip.
template <int G>
__device__ __forceinline__ float group_bcast(float v, int j, bool upper)
{
    const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
    if (G == 64) return a;
    const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32 + j));
    return upper ? b : a;
}

// Minimum over the G lanes of a group, in every lane of the group.  Four DPP stages reduce a 16-lane row (the pattern of
// wave_sum in common.h); wider groups combine their rows through v_readlane.
template <int G>
__device__ __forceinline__ float group_min(float v, bool upper)
{
    v = fminf(v, dpp_f32<0xB1>(v));   // quad_perm [1,0,3,2]
    v = fminf(v, dpp_f32<0x4E>(v));   // quad_perm [2,3,0,1]
    v = fminf(v, dpp_f32<0x141>(v));  // row_half_mirror
    v = fminf(v, dpp_f32<0x140>(v));  // row_mirror
    if (G == 16) return v;
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    if (G == 64) return fminf(fminf(r0, r1), fminf(r2, r3));
    return upper ? fminf(r2, r3) : fminf(r0, r1);
}

struct Father {
    float best;   // running max_j m_j (-1 before the first candidate: every m_j >= 0)
    int j;        // smallest j that attains it
};

// Candidate j of the group's point: all lanes hold (bx, by, bz) = q_j; lane l holds its own q_l (on == l < kk).
template <int G>
__device__ __forceinline__ void consider_mid(Father &f, int j, float bx, float by, float bz, float px, float py, float pz,
                                             float qx, float qy, float qz, bool on, bool upper)
{
    const float mx = (bx + 2.0f * px) / 3.0f, my = (by + 2.0f * py) / 3.0f, mz = (bz + 2.0f * pz) / 3.0f;
    const float dx = mx - qx, dy = my - qy, dz = mz - qz;
    const float d2 = on ? (dx * dx + dy * dy) + dz * dz : __builtin_huge_valf();
    const float m = group_min<G>(d2, upper);
    if (m > f.best) { f.best = m; f.j = j; }   // strict: a tie keeps the smaller j
}

template <int J>
__device__ __forceinline__ void consider_mid16(Father &f, int kk, float px, float py, float pz, float qx, float qy, float qz,
                                               bool on)
{
    if (J < kk)   // kk is uniform over the row (one point per row)
        consider_mid<16>(f, J, row_bcast16<J>(qx), row_bcast16<J>(qy), row_bcast16<J>(qz), px, py, pz, qx, qy, qz, on, false);
}

// G lanes per point (16 at K <= 16, 32 at K <= 32, else 64), lane l of a group holds q_l.  The K + 1 positions of a point are
// the only gathers and are issued before any arithmetic; no LDS, no scratch.  Rows beyond P do the arithmetic on zeros (the
// cross-lane operations need every lane of the wave) and store nothing.
template <int G>
__global__ void __launch_bounds__(256)
upsample_candidates_kernel(const float *__restrict__ pts, const int64_t *__restrict__ knn_idx,
                           const int64_t *__restrict__ first_idx, const int64_t *__restrict__ num_pts, int N, int64_t P, int K,
                           float *__restrict__ sparsity_sq, int *__restrict__ father, unsigned long long *__restrict__ key)
{
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int l = threadIdx.x % G;
    const bool upper = (threadIdx.x & 32) != 0;
    const int n = p < P ? find_cloud(p, first_idx, num_pts, N) : -1;
    int64_t f0 = 0, np_ = 0;
    int kk = 0;
    if (n >= 0) {
        f0 = first_idx[n];
        np_ = num_pts[n];
        kk = (int)min((int64_t)K, np_ - 1);   // a cloud of fewer than K + 1 points: its list is zero-padded behind them
    }
    const bool on = l < kk;
    float px = 0.f, py = 0.f, pz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
    if (n >= 0) {
        int64_t q = p;
        // (ids outside the cloud or the packed array are not followed)
        if (on) q = min(f0 + min(max(knn_idx[p * (K + 1) + 1 + l], (int64_t)0), np_ - 1), P - 1);
        qx = pts[3 * q]; qy = pts[3 * q + 1]; qz = pts[3 * q + 2];
        px = pts[3 * p]; py = pts[3 * p + 1]; pz = pts[3 * p + 2];
    }
    Father f = {-1.0f, 0};
    if (G == 16) {
        consider_mid16<0>(f, kk, px, py, pz, qx, qy, qz, on);   consider_mid16<1>(f, kk, px, py, pz, qx, qy, qz, on);
        consider_mid16<2>(f, kk, px, py, pz, qx, qy, qz, on);   consider_mid16<3>(f, kk, px, py, pz, qx, qy, qz, on);
        consider_mid16<4>(f, kk, px, py, pz, qx, qy, qz, on);   consider_mid16<5>(f, kk, px, py, pz, qx, qy, qz, on);
        consider_mid16<6>(f, kk, px, py, pz, qx, qy, qz, on);   consider_mid16<7>(f, kk, px, py, pz, qx, qy, qz, on);
        consider_mid16<8>(f, kk, px, py, pz, qx, qy, qz, on);   consider_mid16<9>(f, kk, px, py, pz, qx, qy, qz, on);
        consider_mid16<10>(f, kk, px, py, pz, qx, qy, qz, on);  consider_mid16<11>(f, kk, px, py, pz, qx, qy, qz, on);
        consider_mid16<12>(f, kk, px, py, pz, qx, qy, qz, on);  consider_mid16<13>(f, kk, px, py, pz, qx, qy, qz, on);
        consider_mid16<14>(f, kk, px, py, pz, qx, qy, qz, on);  consider_mid16<15>(f, kk, px, py, pz, qx, qy, qz, on);
    } else {
        // v_readlane needs a wave-uniform j, and the groups of a wave may belong to clouds of different kk: walk to K and
        // let each group ignore the candidates beyond its own kk
        for (int j = 0; j < K; ++j) {
            const float bx = group_bcast<G>(qx, j, upper), by = group_bcast<G>(qy, j, upper), bz = group_bcast<G>(qz, j, upper);
            Father g = f;
            consider_mid<G>(g, j, bx, by, bz, px, py, pz, qx, qy, qz, on, upper);
            if (j < kk) f = g;
        }
    }
    if (l == 0 && p < P) {
        const float s = fmaxf(f.best, 0.0f);   // no neighbour (kk == 0), a slot of no cloud: 0; NaN positions: 0
        const unsigned local = n >= 0 ? (unsigned)(p - f0) : 0xffffffffu;
        sparsity_sq[p] = s;
        father[p] = f.j;
        key[p] = n >= 0 ? ((unsigned long long)__float_as_uint(s) << 32 | (0xffffffffu - local)) : 0ull;
    }
}

// One thread per row of the grown cloud.  Rows [0, n_new[n]) of cloud n are the selected candidates in emission order,
// recomputed from the old cloud with the arithmetic above; the rest are the old rows in their order.
__global__ void __launch_bounds__(256)
upsample_insert_kernel(const float *__restrict__ pts, const float *__restrict__ attrs, int C, const int64_t *__restrict__ knn_idx,
                       const int *__restrict__ father, const int64_t *__restrict__ sel, const int64_t *__restrict__ old_first,
                       const int64_t *__restrict__ old_num, const int64_t *__restrict__ new_first,
                       const int64_t *__restrict__ new_num, const int64_t *__restrict__ n_new, int N, int K, int64_t P,
                       int64_t P_out, int64_t n_sel, float *__restrict__ out_pts, float *__restrict__ out_attrs)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= P_out) return;
    int n = -1;
    int64_t sel0 = 0;   // where cloud n's ids start in `sel`: the n_new of the clouds before it
    for (int c = 0; c < N; ++c) {
        const int64_t f = new_first[c];
        if (r >= f && r < f + new_num[c]) { n = c; break; }
        sel0 += n_new[c];
    }
    float o[3] = {0.f, 0.f, 0.f};
    int64_t src = -1, pa = -1, qa = -1;   // a copied row, or the parents p and q_{j*} of a new one
    if (n >= 0 && old_first[n] >= 0 && old_num[n] >= 0 && old_first[n] + old_num[n] <= P) {   // else: a range that leaves the old cloud
        const int64_t local = r - new_first[n], nn = n_new[n], f0 = old_first[n], np_ = old_num[n];
        if (local < nn) {
            if (np_ > 0 && sel0 + local < n_sel) {
                pa = min(max(sel[sel0 + local], f0), f0 + np_ - 1);
                const int j = min(max(father[pa], 0), K - 1);
                qa = f0 + min(max(knn_idx[pa * (K + 1) + 1 + j], (int64_t)0), np_ - 1);
#pragma unroll
                for (int a = 0; a < 3; ++a) o[a] = (pts[3 * qa + a] + 2.0f * pts[3 * pa + a]) / 3.0f;
            }
        } else if (local - nn < np_) {
            src = f0 + (local - nn);
#pragma unroll
            for (int a = 0; a < 3; ++a) o[a] = pts[3 * src + a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) out_pts[3 * r + a] = o[a];
    if (out_attrs) {
        for (int c = 0; c < C; ++c) {
            float v = 0.f;
            if (src >= 0) v = attrs[src * C + c];
            else if (pa >= 0) v = (attrs[qa * C + c] + 2.0f * attrs[pa * C + c]) / 3.0f;
            out_attrs[r * C + c] = v;
        }
    }
}

}  // namespace dss

using namespace dss;

extern "C" int dss_upsample_candidates(const float *points, const int64_t *knn_idx, const int64_t *first_idx,
                                       const int64_t *num_pts, int N, int64_t P, int K, float *sparsity_sq, int32_t *father,
                                       uint64_t *key, void *stream)
{
    if (N <= 0 || P < 0 || K < 1 || K + 1 > 40) {
        set_error("dss_upsample_candidates: bad sizes N=%d P=%lld K=%d (1 <= K, K + 1 <= 40)", N, (long long)P, K);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return DSS_OK;
    if (!points || !knn_idx || !first_idx || !num_pts || !sparsity_sq || !father || !key) {
        set_error("dss_upsample_candidates: NULL tensor pointer");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const int G = K <= 16 ? 16 : (K <= 32 ? 32 : 64);
    const int64_t blocks = (P * G + 255) / 256;
    if (blocks > 0x7fffffff) {
        set_error("dss_upsample_candidates: P=%lld too large", (long long)P);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const dim3 grid((unsigned)blocks), block(256);
    unsigned long long *k64 = reinterpret_cast<unsigned long long *>(key);
    if (G == 16)
        hipLaunchKernelGGL(upsample_candidates_kernel<16>, grid, block, 0, as_stream(stream), points, knn_idx, first_idx, num_pts,
                           N, P, K, sparsity_sq, father, k64);
    else if (G == 32)
        hipLaunchKernelGGL(upsample_candidates_kernel<32>, grid, block, 0, as_stream(stream), points, knn_idx, first_idx, num_pts,
                           N, P, K, sparsity_sq, father, k64);
    else
        hipLaunchKernelGGL(upsample_candidates_kernel<64>, grid, block, 0, as_stream(stream), points, knn_idx, first_idx, num_pts,
                           N, P, K, sparsity_sq, father, k64);
    return check_launch("dss_upsample_candidates");
}

extern "C" int dss_upsample_insert(const float *points, const float *attrs, int C, const int64_t *knn_idx, const int32_t *father,
                                   const int64_t *sel, const int64_t *old_first, const int64_t *old_num,
                                   const int64_t *new_first, const int64_t *new_num, const int64_t *n_new, int N, int K,
                                   int64_t P, int64_t P_out, int64_t n_sel, float *out_points, float *out_attrs, void *stream)
{
    const char *who = "dss_upsample_insert";
    if (N <= 0 || P < 0 || K < 1 || K + 1 > 40 || n_sel < 0) {
        set_error("%s: bad sizes N=%d P=%lld K=%d n_sel=%lld (1 <= K, K + 1 <= 40)", who, N, (long long)P, K, (long long)n_sel);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (P_out != P + n_sel) {   // a round only grows a cloud: a target below the current size has no grown cloud
        set_error("%s: the grown cloud has P_out=%lld rows, expected P + n_sel = %lld + %lld", who, (long long)P_out, (long long)P,
                  (long long)n_sel);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if ((attrs != nullptr) != (out_attrs != nullptr) || (attrs && (C < 1 || C > 16))) {
        set_error("%s: attrs and out_attrs come together, with 1 <= C <= 16 (C=%d)", who, C);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (P_out == 0) return DSS_OK;
    if (!points || !knn_idx || !father || (!sel && n_sel > 0) || !old_first || !old_num || !new_first || !new_num || !n_new ||
        !out_points) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    const int64_t blocks = (P_out + 255) / 256;
    if (blocks > 0x7fffffff) {
        set_error("%s: P_out=%lld too large", who, (long long)P_out);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(upsample_insert_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), points, attrs, C, knn_idx,
                       father, sel, old_first, old_num, new_first, new_num, n_new, N, K, P, P_out, n_sel, out_points, out_attrs);
    return check_launch(who);
}
