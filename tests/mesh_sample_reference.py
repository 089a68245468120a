"""The surface sampler's rule (include/dss_hip.h, "Surface samples of a triangle mesh") restated in numpy, operation for
operation: what `dss_sample_mesh_surface` must return to the bit.  Philox4x32-10 in uint64 arithmetic, the area keys via
`np.ldexp` / `math.frexp`, the table and the targets in Python integers, `bisect_right` for the face, float32 weights and
points with every intermediate a float32 array.  The backward twice: sequential float32 in ascending entry order (the
yardstick for bits) and float64 (the yardstick for accuracy).  Also the meshes the two test modules share (built on
`mesh_raster_reference.icosphere`).  Checked on the CPU by test_mesh_sample_cpu.py."""
import math
from bisect import bisect_right
from itertools import accumulate

import numpy as np

import mesh_raster_reference as mr

f32 = np.float32
M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


# ---- the generator

def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint64 arrays holding 32-bit words"""
    c = [np.atleast_1d(np.asarray(w, np.uint64)) for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    m32 = np.uint64(M32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]       # 32 x 32 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c


def sample_words(n, S, seed, first_sample=0):
    """r0 .. r3 of the samples first_sample .. first_sample + S - 1 of mesh n"""
    s = np.arange(first_sample, first_sample + S, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((s & np.uint64(M32), s >> np.uint64(32), np.uint64(n), np.uint64(0)), (seed & M32, seed >> 32))


# ---- the area table

def face_lengths(verts, faces):
    """-> len (F,) float32 (0 for an absent face), nrm (F,3) float32 (garbage where len is 0).  faces index verts."""
    verts, faces = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    ok = ((faces >= 0) & (faces < V)).all(1)
    tri = verts[np.clip(faces, 0, max(V - 1, 0))] if V else np.zeros((len(faces), 3, 3), np.float32)
    ok &= np.isfinite(tri).all((1, 2))
    with np.errstate(all="ignore"):
        u, w = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        nrm = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                        u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)
        ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    assert nrm.dtype == np.float32 and ln.dtype == np.float32
    ok &= np.isfinite(ln)
    return np.where(ok, ln, f32(0)), nrm


def area_keys(ln):
    """len (F,) of ONE mesh -> keys, a list of Python ints"""
    ln = np.asarray(ln, np.float32)
    len_max = float(ln.max()) if len(ln) else 0.0
    if not len_max > 0.0:
        return [0] * len(ln)
    _, e = math.frexp(len_max)
    return [int(k) for k in np.floor(np.ldexp(ln.astype(np.float64), 32 - e))]


def cumulate(keys):
    return list(accumulate(keys))


def pick(cum, target):
    """the first f with cum[f] > target"""
    return bisect_right(cum, target)


# ---- the sampler

def sample_mesh(verts, faces, S, seed, n=0, first_sample=0):
    """S samples of ONE mesh (faces (F,3) index verts; n is the mesh's index in its batch, which only enters the counter)
    -> points (S,3) float32, normals (S,3) float32, face_idx (S,) int64, bary (S,3) float32"""
    verts, faces = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ln, nrm = face_lengths(verts, faces)
    cum = cumulate(area_keys(ln))
    total = cum[-1] if cum else 0
    zero = np.zeros((S, 3), np.float32)
    if total == 0 or S == 0:
        return zero, zero.copy(), np.full(S, -1, np.int64), zero.copy()
    r0, r1, r2, r3 = sample_words(n, S, seed, first_sample)
    fi = np.asarray([pick(cum, (((int(a) << 32) | int(b)) * total) >> 64) for a, b in zip(r0, r1)], np.int64)
    u1 = (r2 >> np.uint64(8)).astype(np.float32) * f32(2.0 ** -24)
    u2 = (r3 >> np.uint64(8)).astype(np.float32) * f32(2.0 ** -24)
    su = np.sqrt(u1)
    w0, w1, w2 = f32(1) - su, su * (f32(1) - u2), su * u2
    A, B, C = (verts[faces[fi, k]] for k in range(3))
    points = (w0[:, None] * A + w1[:, None] * B) + w2[:, None] * C
    normals = nrm[fi] / ln[fi][:, None]
    bary = np.stack([w0, w1, w2], -1)
    assert points.dtype == np.float32 and normals.dtype == np.float32 and bary.dtype == np.float32
    return points, normals, fi, bary


def _mesh_faces(faces, first, num, n):
    F = len(faces)
    a, k = int(first[n]), int(num[n])
    return faces[a:a + k] if a >= 0 and k > 0 and a + k <= F else faces[:0]


def sample_batch(verts, faces, first, num, S, seed):
    """packed meshes (faces hold packed vertex ids) -> points (N,S,3), normals (N,S,3), face_idx (N,S), bary (N,S,3)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    out = [sample_mesh(verts, _mesh_faces(faces, first, num, n), S, seed, n) for n in range(len(first))]
    return tuple(np.stack([o[k] for o in out]) if out else np.zeros((0, S) + ((3,) if k != 2 else ()), np.float32 if k != 2 else np.int64)
                 for k in range(4))


# ---- the backward

def backward(verts_count, faces, first, num, face_idx, bary, g_points, dtype=np.float32):
    """grad_verts (V,3): the entries e = 3 (n S + s) + c added in ascending e.  dtype float32: product and sum rounded one
    by one, the order the kernel keeps; float64: the same sum where rounding does not matter."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    grad = np.zeros((verts_count, 3), dtype)
    N, S = face_idx.shape
    for n in range(N):
        fm = _mesh_faces(faces, first, num, n)
        for s in range(S):
            fl = int(face_idx[n, s])
            if fl < 0 or fl >= len(fm):
                continue
            g = np.asarray(g_points[n, s], np.float32).astype(dtype)
            for c in range(3):
                v = int(fm[fl, c])
                if 0 <= v < verts_count:
                    grad[v] = grad[v] + dtype(bary[n, s, c]) * g
    assert grad.dtype == dtype
    return grad


# ---- meshes

def pack(meshes):
    """[(verts, faces with mesh-local vertex ids)] -> packed verts, faces with packed ids, first, num"""
    starts = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])[:-1]]).astype(np.int64)
    verts = np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])
    faces = np.concatenate([np.asarray(f, np.int64).reshape(-1, 3) + s for (_, f), s in zip(meshes, starts)])
    num = np.asarray([len(np.asarray(f).reshape(-1, 3)) for _, f in meshes], np.int64)
    first = np.concatenate([[0], np.cumsum(num)[:-1]]).astype(np.int64)
    return verts, faces, first, num


def icosphere(level, scale=(1.0, 1.0, 1.0)):
    verts, faces = mr.icosphere(level)
    return (verts * np.asarray(scale, np.float32)).astype(np.float32), faces


def triangle():
    return np.asarray([(0.25, -0.5, 0.125), (1.5, 0.25, -0.75), (-0.5, 1.25, 0.5)], np.float32), np.asarray([(0, 1, 2)], np.int64)


def empty_mesh():
    return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)


def degenerate_mesh():
    """collinear, repeated and coincident corners: every len is exactly 0"""
    verts = np.asarray([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0.5, 0.5, 0.5)], np.float32)
    return verts, np.asarray([(0, 1, 2), (0, 0, 3), (3, 3, 3), (1, 2, 1)], np.int64)


def batch_of_five():
    """level 0, an empty mesh, a single triangle, a mesh of only degenerate faces, level 2"""
    return [icosphere(0), empty_mesh(), triangle(), degenerate_mesh(), icosphere(2, (1.0, 0.5, 2.0))]


def hostile_mesh():
    """Everything at once: a level-1 icosphere; a face of len 1 (the largest); a face 2^-12 of it; a face 2^-34 of it
    (key 0: never drawn); faces with vertex id -1 and id V; a face with a NaN vertex.  The vertex rows that only bad faces
    name are NaN.  -> verts, faces, ids of the undrawable faces (absent or key 0)"""
    v, f = mr.icosphere(1)
    v = (v * f32(0.5)).astype(np.float32)
    n0 = len(v)
    extra = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0),                          # len 1
                        (0, 0, 1), (2.0 ** -12, 0, 1), (0, 1, 1),                 # len 2^-12
                        (0, 0, 2), (2.0 ** -34, 0, 2), (0, 1, 2),                 # len 2^-34
                        (np.nan, np.nan, np.nan), (np.nan, np.nan, np.nan), (np.nan, np.nan, np.nan)], np.float32)
    verts = np.concatenate([v, extra])
    V = len(verts)
    big, small, tiny, bad = n0, n0 + 3, n0 + 6, n0 + 9
    more = np.asarray([(bad, bad + 1, -1), (big, big + 1, big + 2), (bad + 1, V, bad + 2), (tiny, tiny + 1, tiny + 2),
                       (0, 1, bad), (small, small + 1, small + 2), (V + 5, -7, 0)], np.int64)
    faces = np.concatenate([f[:40], more, f[40:]])
    undrawable = 40 + np.asarray([0, 2, 3, 4, 6])
    return verts, faces, undrawable
