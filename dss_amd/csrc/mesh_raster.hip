// Triangle meshes -> target images: the hard rasteriser and the flat shader behind the reference's data script
// (scripts/create_mvr_data_from_mesh.py:148-219: pytorch3d's MeshRasterizer with blur_radius 0, slot 0 of its fragments,
// and HardFlatShader).  Forward only.  The coverage and depth rule is stated in include/dss_hip.h; every kernel below
// follows it operation for operation (the library builds with -ffp-contract=off -fno-fast-math).
//   mesh_vertex_kernel      one thread per (camera, vertex): screen_verts, by the per-point setup's own projection
//   mesh_face_kernel        one thread per (camera, face): absent test, A, pixel rectangle -> a 48-byte record; a face whose
//                           rectangle meets at most MESH_BIN_TILES 8x8 tiles counts itself into them, a larger one goes on
//                           its camera's large list, which every tile tests against the record's rectangle
//   mesh_scan_kernel        exclusive scan of the tile counts (cell_sort.h, step 3)
//   mesh_fill_kernel        one thread per record: the binned faces take their slots in the tiles' lists
//   mesh_fine_kernel        one wavefront per tile, one lane per pixel: every face of the two lists is read uniformly and
//                           tested by all 64 lanes; (zbuf, face id) reduced under the rule's order, so the order of a list
//                           (integer atomics hand out the slots) never shows in the result
//   mesh_flat_shade_kernel  one thread per pixel: phong.h's light on the face normal
// No float atomics, nothing read back to the host; the workspace is a function of (N, F, V, S).
#include <limits.h>
#include "setup_body.h"
#include "cell_sort.h"
#include "phong.h"

#define MESH_BIN_TILES 16     // a face whose rectangle meets more tiles than this goes on the large list
#define MESH_ABSENT 0
#define MESH_BINNED 1
#define MESH_LARGE 2

namespace dss {

struct MeshArgs {
    const float *verts;                       // (V,3)
    const int64_t *faces, *f_first, *f_num;   // (F,3) packed vertex ids; (1,) shared, else (N,)
    int64_t V, F;
    const float *M, *Vm, *znear, *zfar, *cam; // (N,4,4) x 2, (N,) x 2, (N,3)
    int N, shared, cull, S, tiles;            // tiles = tile columns = tile rows
    float *screen_verts;                      // (N,V,3)
    // workspace
    float4 *frec;                             // 3 per record: {x0 y0 z0 x1} {y1 z1 x2 y2} {z2, c0 | c1 << 16, r0 | r1 << 16, route}
    uint32_t *tile_count, *large_count;       // (N tiles^2), (N,): zero before the face pass
    uint32_t *tile_start;                     // (N tiles^2 + 1,)
    uint32_t *large, *list;                   // record ids: (N, F) and the tiles' lists back to back
};

__device__ __forceinline__ int64_t mesh_records(const MeshArgs &A) { return A.shared ? (int64_t)A.N * A.F : A.F; }

// Edge function of the edge (a, b) at p: the endpoint with the lexicographically smaller screen (x, y) first, so that the
// two faces of a shared edge get the same bits with opposite sign.
__device__ __forceinline__ float mesh_edge(float ax, float ay, float bx, float by, float px, float py)
{
    const bool swap = bx < ax || (bx == ax && by < ay);
    const float ux = swap ? bx : ax, uy = swap ? by : ay, vx = swap ? ax : bx, vy = swap ? ay : by;
    const float e = (vx - ux) * (py - uy) - (vy - uy) * (px - ux);
    return swap ? -e : e;
}

__global__ __launch_bounds__(256) void mesh_vertex_kernel(const MeshArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)A.N * A.V) return;
    const int n = (int)(i / A.V);
    const int64_t v = i - (int64_t)n * A.V;
    const float ph0 = A.verts[3 * v], ph1 = A.verts[3 * v + 1], ph2 = A.verts[3 * v + 2], ph3 = 1.0f;
    const CamLane cam(A.M, A.Vm, A.znear, A.zfar, nullptr, n);
    const float zview = project_view_z(cam, ph0, ph1, ph2, ph3);
    const float w = project_clip(cam, 3, ph0, ph1, ph2, ph3);
    const float sx = project_ndc(project_clip(cam, 0, ph0, ph1, ph2, ph3), w);
    const float sy = project_ndc(project_clip(cam, 1, ph0, ph1, ph2, ph3), w);
    A.screen_verts[3 * i] = sx; A.screen_verts[3 * i + 1] = sy; A.screen_verts[3 * i + 2] = zview;
}

__device__ __forceinline__ bool mesh_finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

__global__ __launch_bounds__(256) void mesh_face_kernel(const MeshArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mesh_records(A)) return;
    int n;
    int64_t f;
    if (A.shared) {
        n = (int)(i / A.F);
        f = i - (int64_t)n * A.F;
        if (f < A.f_first[0] || f >= A.f_first[0] + A.f_num[0]) n = -1;
    } else {
        f = i;
        n = find_cloud(f, A.f_first, A.f_num, A.N);
    }
    int route = MESH_ABSENT;
    int c0 = 1, c1 = 0, r0 = 1, r1 = 0;
    float s[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    const int64_t id[3] = {A.faces[3 * f], A.faces[3 * f + 1], A.faces[3 * f + 2]};
    bool ok = n >= 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && id[k] >= 0 && id[k] < A.V;
    if (ok) {
        const float zn = A.znear[n], zf = A.zfar[n];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float *p = A.screen_verts + 3 * ((int64_t)n * A.V + id[k]);
            s[k][0] = p[0]; s[k][1] = p[1]; s[k][2] = p[2];
            ok = ok && mesh_finite3(s[k]) && s[k][2] >= zn && s[k][2] <= zf;   // no clipping: the whole face or nothing
        }
    }
    if (ok) ok = mesh_edge(s[0][0], s[0][1], s[1][0], s[1][1], s[2][0], s[2][1]) != 0.0f;
    if (ok && A.cull) {
        const float *a = A.verts + 3 * id[0], *b = A.verts + 3 * id[1], *c = A.verts + 3 * id[2], *e = A.cam + 3 * n;
        const float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const float g[3] = {e[0] - a[0], e[1] - a[1], e[2] - a[2]};
        const float nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
        ok = (nx * g[0] + ny * g[1]) + nz * g[2] > 0.0f;
    }
    if (ok) {
        const float xmin = fminf(fminf(s[0][0], s[1][0]), s[2][0]), xmax = fmaxf(fmaxf(s[0][0], s[1][0]), s[2][0]);
        const float ymin = fminf(fminf(s[0][1], s[1][1]), s[2][1]), ymax = fmaxf(fmaxf(s[0][1], s[1][1]), s[2][1]);
        int xlo, xhi, ylo, yhi;
        ok = ndc_index_range((xmin + xmax) * 0.5f, (xmax - xmin) * 0.5f, A.S, xlo, xhi) &&
             ndc_index_range((ymin + ymax) * 0.5f, (ymax - ymin) * 0.5f, A.S, ylo, yhi);
        if (ok) {   // image column c <-> NDC index S - 1 - c, likewise the rows
            c0 = A.S - 1 - xhi; c1 = A.S - 1 - xlo; r0 = A.S - 1 - yhi; r1 = A.S - 1 - ylo;
            const int tx0 = c0 / DSS_TILE, tx1 = c1 / DSS_TILE, ty0 = r0 / DSS_TILE, ty1 = r1 / DSS_TILE;
            if ((int64_t)(tx1 - tx0 + 1) * (ty1 - ty0 + 1) <= MESH_BIN_TILES) {
                route = MESH_BINNED;
                uint32_t *cnt = A.tile_count + (size_t)n * A.tiles * A.tiles;
                for (int ty = ty0; ty <= ty1; ++ty)
                    for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(cnt + (size_t)ty * A.tiles + tx, 1u);
            } else {
                route = MESH_LARGE;
                const uint32_t pos = atomicAdd(A.large_count + n, 1u);
                A.large[(size_t)n * A.F + pos] = (uint32_t)i;
            }
        }
    }
    float4 *R = A.frec + 3 * (size_t)i;
    R[0] = make_float4(s[0][0], s[0][1], s[0][2], s[1][0]);
    R[1] = make_float4(s[1][1], s[1][2], s[2][0], s[2][1]);
    R[2] = make_float4(s[2][2], __int_as_float(c0 | (c1 << 16)), __int_as_float(r0 | (r1 << 16)), __int_as_float(route));
}

__global__ __launch_bounds__(1024) void mesh_scan_kernel(const MeshArgs A)
{
    const int total = A.N * A.tiles * A.tiles;
    cell_start_scan(A.tile_count, A.tile_start, total, A.tile_start + total);
}

// (counts a tile's counter back down to zero while it hands out the slots: the lists' lengths are the differences of
// tile_start)
__global__ __launch_bounds__(256) void mesh_fill_kernel(const MeshArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mesh_records(A)) return;
    const float4 r = A.frec[3 * (size_t)i + 2];
    if (__float_as_int(r.w) != MESH_BINNED) return;
    const int n = A.shared ? (int)(i / A.F) : find_cloud(i, A.f_first, A.f_num, A.N);
    const int cx = __float_as_int(r.y), cy = __float_as_int(r.z);
    const int tx0 = (cx & 0xffff) / DSS_TILE, tx1 = (cx >> 16) / DSS_TILE, ty0 = (cy & 0xffff) / DSS_TILE, ty1 = (cy >> 16) / DSS_TILE;
    const size_t t0 = (size_t)n * A.tiles * A.tiles;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const size_t t = t0 + (size_t)ty * A.tiles + tx;
            const uint32_t pos = atomicSub(A.tile_count + t, 1u) - 1u;
            A.list[(size_t)A.tile_start[t] + pos] = (uint32_t)i;
        }
}

// The winner of one pixel so far
struct MeshBest {
    float z, b0, b1, b2;
    int f;   // packed face id; INT_MAX: none
};

// Record ri (wave-uniform) against the lane's pixel (col, row) with centre (px, py): the face's rectangle (the rule tests a
// face at the pixels of its rectangle only), coverage, perspective-correct depth, winner.
__device__ __forceinline__ void mesh_test(const float4 *__restrict__ frec, uint32_t ri, int f, int col, int row, float px,
                                          float py, MeshBest &best)
{
    const float *r = reinterpret_cast<const float *>(frec + 3 * (size_t)ri);
    const float x0 = uniform_load(r), y0 = uniform_load(r + 1), z0 = uniform_load(r + 2), x1 = uniform_load(r + 3),
                y1 = uniform_load(r + 4), z1 = uniform_load(r + 5), x2 = uniform_load(r + 6), y2 = uniform_load(r + 7),
                z2 = uniform_load(r + 8);
    const int cx = __float_as_int(uniform_load(r + 9)), cy = __float_as_int(uniform_load(r + 10));
    const bool in_rect = col >= (cx & 0xffff) && col <= (cx >> 16) && row >= (cy & 0xffff) && row <= (cy >> 16);
    const float area = mesh_edge(x0, y0, x1, y1, x2, y2);
    const float s = area > 0.0f ? 1.0f : -1.0f;
    const float w0 = s * mesh_edge(x1, y1, x2, y2, px, py);
    const float w1 = s * mesh_edge(x2, y2, x0, y0, px, py);
    const float w2 = s * mesh_edge(x0, y0, x1, y1, px, py);
    const float bs = (w0 + w1) + w2;
    if (in_rect && w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f && bs > 0.0f) {
        const float q0 = (w0 / bs) / z0, q1 = (w1 / bs) / z1, q2 = (w2 / bs) / z2;
        const float t = (q0 + q1) + q2;
        const float zb = 1.0f / t;
        if (zb < best.z || (zb == best.z && f < best.f)) {
            best.z = zb; best.f = f;
            best.b0 = q0 * zb; best.b1 = q1 * zb; best.b2 = q2 * zb;
        }
    }
}

__global__ __launch_bounds__(256) void mesh_fine_kernel(const MeshArgs A, int64_t *__restrict__ pix_to_face,
                                                        float *__restrict__ zbuf, float *__restrict__ bary)
{
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
    const int T = A.tiles * A.tiles;
    if (tile >= (int64_t)A.N * T) return;
    const int n = (int)(tile / T), t = (int)(tile - (int64_t)n * T);
    const int ty = t / A.tiles, tx = t - ty * A.tiles;
    const int col = tx * DSS_TILE + (lane & 7), row = ty * DSS_TILE + (lane >> 3);
    const float px = pix_to_ndc(A.S - 1 - col, A.S), py = pix_to_ndc(A.S - 1 - row, A.S);
    const int64_t rec0 = A.shared ? (int64_t)n * A.F : 0;   // record id - rec0 = packed face id
    MeshBest best;
    best.z = INFINITY; best.f = INT_MAX; best.b0 = best.b1 = best.b2 = 0.0f;

    const uint32_t beg = A.tile_start[tile], end = A.tile_start[tile + 1];
    for (uint32_t base = beg; base < end; base += 64) {
        const uint32_t mine = base + lane < end ? A.list[base + lane] : 0u;
        const int cnt = (int)min(64u, end - base);
        for (int k = 0; k < cnt; ++k) {
            const uint32_t ri = (uint32_t)__builtin_amdgcn_readlane((int)mine, k);
            mesh_test(A.frec, ri, (int)(ri - rec0), col, row, px, py, best);
        }
    }
    // the camera's large faces: 64 rectangles tested at a time, the ones that meet the tile then one by one
    const uint32_t nl = A.large_count[n];
    const int tc0 = tx * DSS_TILE, tr0 = ty * DSS_TILE;
    for (uint32_t base = 0; base < nl; base += 64) {
        uint32_t mine = 0u;
        bool hit = false;
        if (base + lane < nl) {
            mine = A.large[(size_t)n * A.F + base + lane];
            const float4 r = A.frec[3 * (size_t)mine + 2];
            const int cx = __float_as_int(r.y), cy = __float_as_int(r.z);
            hit = (cx & 0xffff) <= tc0 + DSS_TILE - 1 && (cx >> 16) >= tc0 && (cy & 0xffff) <= tr0 + DSS_TILE - 1 && (cy >> 16) >= tr0;
        }
        unsigned long long m = __ballot(hit);
        while (m) {
            const int k = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t ri = (uint32_t)__builtin_amdgcn_readlane((int)mine, k);
            mesh_test(A.frec, ri, (int)(ri - rec0), col, row, px, py, best);
        }
    }
    if (col < A.S && row < A.S) {
        const size_t o = ((size_t)n * A.S + row) * A.S + col;
        const bool found = best.f != INT_MAX;
        pix_to_face[o] = found ? (int64_t)best.f - A.f_first[A.shared ? 0 : n] : (int64_t)-1;
        zbuf[o] = found ? best.z : -1.0f;
        bary[3 * o] = best.b0; bary[3 * o + 1] = best.b1; bary[3 * o + 2] = best.b2;
    }
}

struct FlatArgs {
    const int64_t *pix_to_face;   // (N,S,S)
    const float *bary;            // (N,S,S,3)
    const float *verts, *face_colors;
    const int64_t *faces, *f_first, *f_num;
    int64_t V, F;
    int S;
    float bg[3];
};

__global__ __launch_bounds__(256) void mesh_flat_shade_kernel(const FlatArgs G, const PhongArgs A, float *__restrict__ rgba)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t SS = (int64_t)G.S * G.S;
    if (i >= A.N * SS) return;
    const int n = (int)(i / SS), m = A.shared ? 0 : n;
    float out[4] = {G.bg[0], G.bg[1], G.bg[2], 0.0f};
    const int64_t fl = G.pix_to_face[i];
    int64_t id[3] = {-1, -1, -1};
    const int64_t f = fl >= 0 && fl < G.f_num[m] ? G.f_first[m] + fl : -1;
    bool ok = f >= 0 && f < G.F;
    if (ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            id[k] = G.faces[3 * f + k];
            ok = ok && id[k] >= 0 && id[k] < G.V;
        }
    }
    if (ok) {
        const float *a = G.verts + 3 * id[0], *b = G.verts + 3 * id[1], *c = G.verts + 3 * id[2];
        const float b0 = G.bary[3 * i], b1 = G.bary[3 * i + 1], b2 = G.bary[3 * i + 2];
        float x[3], u[3], w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = (b0 * a[k] + b1 * b[k]) + b2 * c[k];
            u[k] = b[k] - a[k];
            w[k] = c[k] - a[k];
        }
        const float nrm[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const float len = fmaxf(sqrtf((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]), 1e-30f);
        const float fn[3] = {nrm[0] / len, nrm[1] / len, nrm[2] / len};   // the face normal; below as dss_phong_forward
        float nh[3], v[3];
        unit(fn, nh);
        const float cw[3] = {A.cam[3 * n] - x[0], A.cam[3 * n + 1] - x[1], A.cam[3 * n + 2] - x[2]};
        unit(cw, v);
        float dif[3] = {0.f, 0.f, 0.f}, spec[3] = {0.f, 0.f, 0.f};
        for (int l = 0; l < A.L; ++l) {
            const float *kd = A.kd + ((size_t)n * A.L + l) * 3;
            const float *ks = A.ks + ((size_t)n * A.L + l) * 3;
            const PhongLight t = phong_light(A, n, l, x, nh, v);
            const float D = fmaxf(t.ca, 0.0f);
            const float Sp = powf(t.alpha, A.shininess);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                dif[ch] += kd[ch] * D;
                spec[ch] += ks[ch] * Sp;
            }
        }
        const float *amb = A.ambient + 3 * n;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float col = G.face_colors ? G.face_colors[3 * f + ch] : 1.0f;
            out[ch] = col * (amb[ch] + dif[ch]) + spec[ch];
        }
        out[3] = 1.0f;
    }
    reinterpret_cast<float4 *>(rgba)[i] = make_float4(out[0], out[1], out[2], out[3]);
}

// The regions of the workspace; base == nullptr: the size query
static size_t mesh_carve(MeshArgs &A, void *base, int N, int64_t F, int S)
{
    Bump ws{static_cast<char *>(base), 0};
    const size_t tiles = (size_t)((S + DSS_TILE - 1) / DSS_TILE), NT = (size_t)N * tiles * tiles, NF = (size_t)N * (size_t)F;
    A.frec = ws.take<float4>(3 * NF);
    A.tile_count = ws.take<uint32_t>(NT + (size_t)N);
    A.large_count = A.tile_count ? A.tile_count + NT : nullptr;
    A.tile_start = ws.take<uint32_t>(NT + 1);
    A.large = ws.take<uint32_t>(NF);
    A.list = ws.take<uint32_t>(NF * MESH_BIN_TILES);
    return ws.used;
}

// What the entries refuse alike: the sizes.  N F <= 2^27: record ids and list positions are 32-bit; S <= 32768: a pixel
// rectangle packs into two words, and N tiles^2 stays an int.
static int mesh_sizes(const char *who, int N, int64_t F, int64_t V, int S)
{
    if (N <= 0 || N > 65535 || F < 0 || V < 0 || F >= ((int64_t)1 << 31) || V >= ((int64_t)1 << 31) || S < 1 || S > 32768 ||
        (int64_t)N * F > ((int64_t)1 << 27) || (int64_t)N * V > ((int64_t)1 << 31) ||
        (int64_t)N * ((S + 7) / 8) * ((S + 7) / 8) > ((int64_t)1 << 30)) {
        set_error("%s: bad sizes N=%d F=%lld V=%lld S=%d (N F <= 2^27, N V <= 2^31, S <= 32768)", who, N, (long long)F,
                  (long long)V, S);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    return DSS_OK;
}

}  // namespace dss

using namespace dss;

extern "C" size_t dss_mesh_raster_workspace(int N, int64_t F, int64_t V, int S)
{
    if (mesh_sizes("dss_mesh_raster_workspace", N, F, V, S)) return 0;
    MeshArgs A;
    return mesh_carve(A, nullptr, N, F, S);
}

extern "C" int dss_rasterize_meshes(const float *verts, int64_t V, const int64_t *faces, const int64_t *f_first,
                                    const int64_t *f_num, int64_t F, const float *M, const float *Vm, const float *znear,
                                    const float *zfar, const float *cam_center, int N, int shared_mesh, int cull_backfaces,
                                    int S, int64_t *pix_to_face, float *zbuf, float *bary, float *screen_verts,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "dss_rasterize_meshes";
    int rc = mesh_sizes(who, N, F, V, S);
    if (rc) return rc;
    if (!M || !Vm || !znear || !zfar || !f_first || !f_num || !pix_to_face || !zbuf || !bary || (V > 0 && (!verts || !screen_verts)) ||
        (F > 0 && !faces) || (cull_backfaces && !cam_center)) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    MeshArgs A;
    const size_t need = mesh_carve(A, nullptr, N, F, S);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, need %zu", who, workspace ? workspace_bytes : (size_t)0, need);
        return DSS_ERR_WORKSPACE;
    }
    mesh_carve(A, workspace, N, F, S);
    A.verts = verts; A.faces = faces; A.f_first = f_first; A.f_num = f_num; A.V = V; A.F = F;
    A.M = M; A.Vm = Vm; A.znear = znear; A.zfar = zfar; A.cam = cam_center;
    A.N = N; A.shared = shared_mesh ? 1 : 0; A.cull = cull_backfaces ? 1 : 0; A.S = S; A.tiles = (S + DSS_TILE - 1) / DSS_TILE;
    A.screen_verts = screen_verts;
    hipStream_t st = as_stream(stream);
    const int64_t NT = (int64_t)N * A.tiles * A.tiles, NV = (int64_t)N * V, recs = A.shared ? (int64_t)N * F : F;
    if (hipMemsetAsync(A.tile_count, 0, ((size_t)NT + (size_t)N) * sizeof(uint32_t), st) != hipSuccess) return check_launch(who);
    if (NV > 0) hipLaunchKernelGGL(mesh_vertex_kernel, dim3((unsigned)((NV + 255) / 256)), dim3(256), 0, st, A);
    if (recs > 0) hipLaunchKernelGGL(mesh_face_kernel, dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(1024), 0, st, A);
    if (recs > 0) hipLaunchKernelGGL(mesh_fill_kernel, dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(mesh_fine_kernel, dim3((unsigned)((NT + 3) / 4)), dim3(256), 0, st, A, pix_to_face, zbuf, bary);
    return check_launch(who);
}

extern "C" int dss_mesh_flat_shade(const int64_t *pix_to_face, const float *bary, const float *verts, int64_t V,
                                   const int64_t *faces, const int64_t *f_first, const int64_t *f_num, int64_t F,
                                   const float *face_colors, int N, int shared_mesh, int S, const float *ambient,
                                   const float *diffuse_color, const float *specular_color, const float *light_vec, int L,
                                   int point_lights, const float *cam_center, float shininess, float bg_r, float bg_g,
                                   float bg_b, float *rgba, void *stream)
{
    const char *who = "dss_mesh_flat_shade";
    int rc = mesh_sizes(who, N, F, V, S);
    if (rc) return rc;
    if (L < 0 || L > 65535) { set_error("%s: bad sizes L=%d", who, L); return DSS_ERR_INVALID_ARGUMENT; }
    if (!pix_to_face || !bary || !f_first || !f_num || !ambient || !cam_center || !rgba || (V > 0 && !verts) || (F > 0 && !faces) ||
        (L > 0 && (!diffuse_color || !specular_color || !light_vec))) {
        set_error("%s: NULL tensor pointer", who);
        return DSS_ERR_INVALID_ARGUMENT;
    }
    FlatArgs G;
    G.pix_to_face = pix_to_face; G.bary = bary; G.verts = verts; G.face_colors = face_colors; G.faces = faces;
    G.f_first = f_first; G.f_num = f_num; G.V = V; G.F = F; G.S = S; G.bg[0] = bg_r; G.bg[1] = bg_g; G.bg[2] = bg_b;
    PhongArgs A = {};
    A.N = N; A.shared = shared_mesh ? 1 : 0; A.L = L; A.point_lights = point_lights;
    A.ambient = ambient; A.kd = diffuse_color; A.ks = specular_color; A.lvec = light_vec; A.cam = cam_center;
    A.shininess = shininess;
    const int64_t pix = (int64_t)N * S * S;
    hipLaunchKernelGGL(mesh_flat_shade_kernel, dim3((unsigned)((pix + 255) / 256)), dim3(256), 0, as_stream(stream), G, A, rgba);
    return check_launch(who);
}
