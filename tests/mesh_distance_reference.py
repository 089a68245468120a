"""The point-triangle distance of include/dss_hip.h (dss_point_face_distance) restated in numpy, twice: float32 in the exact
operation order of the definition (the yardstick for bits) and float64 (the yardstick for accuracy); the gradient as fp64
torch autograd of the same formula; and the scenes of the two test modules (numpy only: an icosahedron subdivided here, a
lattice sheet; no files).

    dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z
    seg(q, P, R): p0 = the lexicographically smaller endpoint, e = p1 - p0, w = q - p0, ee = dot(e, e), we = dot(w, e);
        we <= 0 or ee == 0: r = w;  we >= ee: r = q - p1;  else t = we / ee, r = w - t e;  -> dot(r, r)
    n = (B - A) x (C - A), nn = dot(n, n);  s = dot((R - P) x (q - P), n) for A->B, B->C, C->A;  inside = nn > 0 and all s > 0
    plane = (h h) / nn, h = dot(q - A, n)
    d2 = first minimum under `<` of seg(A,B), seg(B,C), seg(C,A), inside ? plane : +inf, starting from +inf
"""
import numpy as np

EPS = 2.0 ** -23

# Worst c of |d2_f32 - d2_f64| <= c EPS k (d2 + L sqrt(d2) + EPS k L^2), L = sqrt(d2) + the mesh's longest edge, k = the
# conditioning `kappa` of the face that is the answer (1 for a well-shaped triangle, ~aspect for a sliver: the plane term's
# normal is a difference of products), per scene, as measured by
# tests/test_mesh_distance_cpu.py::test_float32_restatement_within_derived_error (which prints them); the bar used anywhere
# is BAR times the scene's value: reference against reference, the margin covers the sampling of queries.  Without k the
# queries above the interiors of the sliver scenes give c = 12 (aspect 100) and 1e4 (aspect 1e4).
ERROR_C = {"ico0": 0.49, "ico2": 0.65, "ico3": 0.83, "ico2_near": 0.83, "ico2_shift": 0.62, "slivers": 0.10, "slivers100": 0.11,
           "degenerate": 0.57, "lattice": 0.0}
BAR = 4.0


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _seg(q, P, R):
    """q (Q,1,3), P, R (1,F,3) -> (Q,F)"""
    sw = (R[..., 0] < P[..., 0]) | ((R[..., 0] == P[..., 0]) & ((R[..., 1] < P[..., 1]) | ((R[..., 1] == P[..., 1]) & (R[..., 2] < P[..., 2]))))
    p0 = np.where(sw[..., None], R, P)
    p1 = np.where(sw[..., None], P, R)
    e = p1 - p0
    w = q - p0
    ee = np.broadcast_to(_dot(e, e), w.shape[:-1])
    we = _dot(w, e)
    with np.errstate(all="ignore"):
        t = we / ee
        r_mid = w - t[..., None] * e
    first = (we <= 0) | (ee == 0)
    second = ~first & (we >= ee)
    r = np.where(first[..., None], w, np.where(second[..., None], q - p1, r_mid))
    return _dot(r, r)


def d2_matrix(q, tri, dtype=np.float32):
    """q (Q,3), tri (F,3,3) -> (Q,F) of the definition, every operation in `dtype`."""
    q = np.asarray(q, dtype)[:, None, :]
    tri = np.asarray(tri, dtype)
    A, B, C = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    with np.errstate(all="ignore"):
        n = _cross(B - A, C - A)
        nn = _dot(n, n)
        s_ab = _dot(_cross(B - A, q - A), n)
        s_bc = _dot(_cross(C - B, q - B), n)
        s_ca = _dot(_cross(A - C, q - C), n)
        inside = (nn > 0) & (s_ab > 0) & (s_bc > 0) & (s_ca > 0)
        h = _dot(q - A, n)
        plane = np.where(inside, (h * h) / nn, np.asarray(np.inf, dtype))
        best = np.full(plane.shape, np.inf, dtype)
        for cand in (_seg(q, A, B), _seg(q, B, C), _seg(q, C, A), plane):
            best = np.where(cand < best, cand, best)
    assert best.dtype == dtype
    return best


def usable_faces(verts, faces):
    """faces with every id in [0, V) and only finite vertices -> (F,) bool"""
    verts, faces = np.asarray(verts), np.asarray(faces)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    fin = np.isfinite(verts[np.clip(faces, 0, max(len(verts) - 1, 0))]).all((1, 2)) if len(verts) else np.zeros(len(faces), bool)
    return ok & fin


def triangles(verts, faces):
    """(F,3,3) with the absent faces' rows as NaN (never an answer)"""
    verts, faces = np.asarray(verts), np.asarray(faces)
    ok = usable_faces(verts, faces)
    tri = np.full((len(faces), 3, 3), np.nan, verts.dtype)
    tri[ok] = verts[faces[ok]]
    return tri


def _pick(D):
    """(rows, cols) -> first minimum per row, NaN never wins; (0, -1) for a row nothing wins"""
    D = np.where(np.isnan(D), np.inf, D)
    if D.shape[1] == 0:
        return np.zeros(D.shape[0], D.dtype), np.full(D.shape[0], -1, np.int64)
    idx = D.argmin(1)
    d = D[np.arange(D.shape[0]), idx]
    found = d < np.inf
    return np.where(found, d, 0).astype(D.dtype), np.where(found, idx, -1).astype(np.int64)


def nearest_face(q, verts, faces, dtype=np.float32, chunk=512, pruned=False):
    """Every query against every face of ONE mesh -> (d2 (Q,), idx (Q,)).  pruned: candidates by a KD-tree over the
    centroids plus the radius bound (large scenes); the result is the same."""
    q, tri = np.asarray(q), triangles(np.asarray(verts), faces)
    if pruned:
        from scipy.spatial import cKDTree
        ok = ~np.isnan(tri).any((1, 2))
        ids = np.nonzero(ok)[0]
        t64 = tri[ok].astype(np.float64)
        cen = t64.mean(1)
        rmax = np.sqrt(((t64 - cen[:, None]) ** 2).sum(-1)).max()
        tree = cKDTree(cen)
        dc, _ = tree.query(q.astype(np.float64))
        d2, idx = np.zeros(len(q), dtype), np.full(len(q), -1, np.int64)
        for i in range(len(q)):
            # the triangle of the nearest centroid is within dc; one whose centroid is beyond dc + rmax is farther than dc
            cand = np.sort(np.asarray(tree.query_ball_point(q[i].astype(np.float64), (dc[i] + rmax) * 1.001 + 1e-6)))
            d, j = _pick(d2_matrix(q[i:i + 1], tri[ids[cand]], dtype))
            d2[i], idx[i] = d[0], ids[cand][j[0]] if j[0] >= 0 else -1
        return d2, idx
    out = [_pick(d2_matrix(q[s:s + chunk], tri, dtype)) for s in range(0, len(q), chunk)]
    if not out:
        return np.zeros(0, dtype), np.zeros(0, np.int64)
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def nearest_point(q, verts, faces, dtype=np.float32, chunk=512):
    """Every face of ONE mesh against every point of ONE cloud -> (d2 (F,), idx (F,)); an absent face gets (0, -1)."""
    q, tri = np.asarray(q), triangles(np.asarray(verts), faces)
    out = [_pick(d2_matrix(q, tri[s:s + chunk], dtype).T) for s in range(0, len(tri), chunk)]
    if not out:
        return np.zeros(0, dtype), np.zeros(0, np.int64)
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def nearest_both(q, verts, faces, dtype=np.float32, chunk=256):
    """both searches of ONE (cloud, mesh) pair from one pass over the distance matrix -> ((d2 (Q,), idx (Q,)), (d2 (F,), idx (F,)))"""
    q, tri = np.asarray(q), triangles(np.asarray(verts), faces)
    pd, pi = [], []
    fd, fi = np.full(len(tri), np.inf, dtype), np.full(len(tri), -1, np.int64)
    for s in range(0, len(q), chunk):
        D = d2_matrix(q[s:s + chunk], tri, dtype)
        d, i = _pick(D)
        pd.append(d), pi.append(i)
        D = np.where(np.isnan(D), np.inf, D)
        j = D.argmin(0)
        m = D[j, np.arange(D.shape[1])]
        better = m < fd                       # strict: an earlier chunk's (smaller) id keeps a tie
        fd, fi = np.where(better, m, fd), np.where(better, j + s, fi)
    found = fi >= 0
    pf = (np.concatenate(pd), np.concatenate(pi)) if pd else (np.zeros(0, dtype), np.zeros(0, np.int64))
    return pf, (np.where(found, fd, 0).astype(dtype), fi)


def loss_fp64(clouds, meshes):
    """point_mesh_face_distance: sum_p d2_p / (|cloud| N) + sum_f d2_f / (|mesh| N), everything in float64"""
    N, total = len(clouds), 0.0
    for q, (v, f) in zip(clouds, meshes):
        (dp, _), (df, _) = nearest_both(np.asarray(q, np.float64), np.asarray(v, np.float64), f, np.float64)
        total += dp.sum() / (len(q) * N) + df.sum() / (len(f) * N)
    return total


def kappa(verts, faces):
    """(F,) conditioning of every face's plane term: (longest edge)^2 / |n|, at least 1; 1 for a face whose float32 normal is
    exactly zero (its plane branch is never taken) and for an absent face"""
    t32 = triangles(np.asarray(verts, np.float32), faces)
    with np.errstate(all="ignore"):
        n32 = _cross(t32[:, 1] - t32[:, 0], t32[:, 2] - t32[:, 0])
        never = ~(_dot(n32, n32) > 0)
        t = t32.astype(np.float64)
        l2 = ((t - np.roll(t, 1, 1)) ** 2).sum(-1).max(1)
        n = np.sqrt((np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) ** 2).sum(-1))
        k = np.where(never | ~(n > 0), 1.0, l2 / np.where(n > 0, n, 1.0))
    return np.maximum(np.nan_to_num(k, nan=1.0), 1.0)


def error_bar(d2_64, longest_edge, c, k=1.0):
    """c EPS k (d2 + L sqrt(d2) + EPS k L^2), L = sqrt(d2) + longest edge, k = kappa of the face in question"""
    r = np.sqrt(d2_64)
    L = r + longest_edge
    return c * EPS * k * (d2_64 + L * r + EPS * k * L * L)


def longest_edge(verts, faces):
    tri = triangles(np.asarray(verts, np.float64), faces)
    tri = tri[~np.isnan(tri).any((1, 2))]
    return float(np.sqrt(((tri - np.roll(tri, 1, 1)) ** 2).sum(-1)).max())


# ---- the gradient: fp64 torch autograd of the same formula, at given pairs
def d2_pairs_torch(q, A, B, C):
    """(M,3) double tensors -> (M,) d2 of the definition, differentiable (the first minimum is selected, not blended)."""
    import torch

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def seg(P, R):
        sw = (R[:, 0] < P[:, 0]) | ((R[:, 0] == P[:, 0]) & ((R[:, 1] < P[:, 1]) | ((R[:, 1] == P[:, 1]) & (R[:, 2] < P[:, 2]))))
        p0, p1 = torch.where(sw[:, None], R, P), torch.where(sw[:, None], P, R)
        e, w = p1 - p0, q - p0
        ee, we = dot(e, e), dot(w, e)
        first = (we <= 0) | (ee == 0)
        second = ~first & (we >= ee)
        t = we / torch.where(ee == 0, torch.ones_like(ee), ee)
        r = torch.where(first[:, None], w, torch.where(second[:, None], q - p1, w - t[:, None] * e))
        return dot(r, r)

    n = torch.linalg.cross(B - A, C - A)
    nn = dot(n, n)
    s = [dot(torch.linalg.cross(R - P, q - P), n) for P, R in ((A, B), (B, C), (C, A))]
    inside = (nn > 0) & (s[0] > 0) & (s[1] > 0) & (s[2] > 0)
    h = dot(q - A, n)
    plane = torch.where(inside, (h * h) / torch.where(nn > 0, nn, torch.ones_like(nn)), torch.full_like(h, float("inf")))
    best = torch.full_like(h, float("inf"))
    for cand in (seg(A, B), seg(B, C), seg(C, A), plane):
        best = torch.where(cand < best, cand, best)
    return best


def gradients_fp64(points, verts, faces, pair_point, pair_face, g):
    """sum_k g[k] d2(points[pair_point[k]], face pair_face[k]) differentiated in double -> (grad_points, grad_verts) numpy"""
    import torch
    p = torch.tensor(np.asarray(points, np.float64), requires_grad=True)
    v = torch.tensor(np.asarray(verts, np.float64), requires_grad=True)
    f = torch.as_tensor(np.asarray(faces)[np.asarray(pair_face)], dtype=torch.int64)
    q = p[torch.as_tensor(np.asarray(pair_point), dtype=torch.int64)]
    d2 = d2_pairs_torch(q, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    (d2 * torch.tensor(np.asarray(g, np.float64))).sum().backward()
    return p.grad.numpy(), v.grad.numpy()


# ---- scenes
def icosphere(level, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(verts (V,3) float32, faces (F,3) int64): an icosahedron subdivided `level` times, 20 * 4^level faces"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.asarray(v) * radius + np.asarray(center, np.float64)).astype(np.float32)
    return verts, np.asarray(f, np.int64)


def lattice_sheet(nx=4, ny=4):
    """nx x ny unit squares in the plane z = 0, each split into two right triangles: ((nx+1)(ny+1) verts, 2 nx ny faces);
    every coordinate an integer, so dyadic queries make every operation of the definition exact."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    verts = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], 1).astype(np.float32)
    f = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            f += [(a, b, c), (a, c, d)]
    return verts, np.asarray(f, np.int64)


def lattice_queries(nx=4, ny=4):
    """dyadic queries: vertices, edge midpoints and quarter points of the sheet, and positions outside it by 1/2, 3 and 50
    cells, each at heights 0, 1/2 and 2"""
    inside = np.arange(0, 4 * nx + 1) / 4.0
    u = np.concatenate([[-50.0, -3.0, -0.5], inside, [nx + 0.5, nx + 3.0, nx + 50.0]])
    insidey = np.arange(0, 4 * ny + 1) / 4.0
    w = np.concatenate([[-50.0, -3.0, -0.5], insidey, [ny + 0.5, ny + 3.0, ny + 50.0]])
    X, Y, Z = np.meshgrid(u, w, np.asarray([0.0, 0.5, 2.0]), indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.float32)


def sphere_queries(rng, n, radius=1.0, center=(0.0, 0.0, 0.0)):
    """a third inside, a third just outside, a third up to 50 radii away"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = n // 3
    r = np.concatenate([rng.uniform(0.0, 0.98, k), rng.uniform(1.0, 1.5, k), rng.uniform(2.0, 50.0, n - 2 * k)])
    return (d * (r * radius)[:, None] + np.asarray(center)).astype(np.float32)


def on_mesh_queries(rng, verts, faces, n_vertices, n_midpoints):
    """queries exactly on vertices and on (fp32-rounded) edge midpoints"""
    vi = rng.choice(len(verts), min(n_vertices, len(verts)), replace=False)
    fi = rng.choice(len(faces), n_midpoints, replace=len(faces) < n_midpoints)
    mids = (verts[faces[fi, 0]] + verts[faces[fi, 1]]) * np.float32(0.5)
    return np.concatenate([verts[vi], mids]).astype(np.float32)


def above_interiors(rng, verts, faces, per_face=8):
    """queries above and below random interior points of every face, at heights from 1e-5 to 0.3: the plane term decides"""
    t = np.asarray(verts, np.float64)[faces]
    w = rng.dirichlet([1.0, 1.0, 1.0], size=(len(faces), per_face))
    base = (w[..., None] * t[:, None]).sum(2)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    h = rng.uniform(-0.3, 0.3, (len(faces), per_face, 1)) * rng.choice([1.0, 1e-2, 1e-4], (len(faces), per_face, 1))
    return (base + h * n[:, None]).reshape(-1, 3).astype(np.float32)


def degenerate_faces(verts):
    """three faces over existing vertices: collinear (a midpoint vertex is appended), two equal vertices, three equal"""
    a, b = verts[0], verts[1]
    verts = np.concatenate([verts, ((a + b) * np.float32(0.5))[None]]).astype(np.float32)
    m = len(verts) - 1
    return verts, np.asarray([(0, m, 1), (2, 2, 3), (4, 4, 4)], np.int64)


def sliver_mesh(rng, n=48, aspect=1e4):
    """n triangles of aspect ~1e4 at random places in the unit cube"""
    o = rng.uniform(-1, 1, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    s = np.cross(d, rng.normal(size=(n, 3)))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    verts = np.stack([o, o + d, o + 0.5 * d + s / aspect], 1).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def cpu_scenes():
    """name -> (queries, verts, faces): the scenes the float32 restatement is measured on (and the GPU module reuses)"""
    rng = np.random.default_rng(20250)
    out = {}
    for name, level in (("ico0", 0), ("ico2", 2), ("ico3", 3)):
        v, f = icosphere(level)
        out[name] = (np.concatenate([sphere_queries(rng, 384), on_mesh_queries(rng, v, f, 64, 32)]), v, f)
    v, f = icosphere(2)
    d = rng.normal(size=(384, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out["ico2_near"] = ((d * (1.0 + rng.uniform(-1e-3, 1e-3, 384))[:, None]).astype(np.float32), v, f)
    v, f = icosphere(2, center=(1000.0, 1000.0, 1000.0))
    out["ico2_shift"] = (sphere_queries(rng, 384, center=(1000.0, 1000.0, 1000.0)), v, f)
    for name, aspect in (("slivers", 1e4), ("slivers100", 1e2)):
        v, f = sliver_mesh(rng, aspect=aspect)
        out[name] = (np.concatenate([rng.uniform(-1.5, 1.5, (512, 3)).astype(np.float32), above_interiors(rng, v, f)]), v, f)
    v, f = icosphere(1)
    v, deg = degenerate_faces(v)
    out["degenerate"] = (np.concatenate([sphere_queries(rng, 256), v[:8]]), v, np.concatenate([f, deg]))
    v, f = lattice_sheet()
    out["lattice"] = (lattice_queries(), v, f)
    return out
