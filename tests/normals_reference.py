"""The two contracts of dss_amd/csrc/normals.hip restated in numpy float32, operation by operation (TEST INFRASTRUCTURE;
numpy only): `disambiguate` (dss_disambiguate_normals) and `orient` (dss_orient_normals), on the packed layout of the
entries, plus the seeded shapes that the CPU and the GPU tests share.  Every product and every sum below is a float32
operation of its own, in the order of the contract, so the GPU results are compared with these bit for bit."""
import numpy as np

TAU = np.array([0.95, 0.8, 0.5, 0.0], np.float32)
F32 = np.float32


def _dot(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z, float32"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unowned(P):
    out = np.zeros((P, 3), F32)
    out[:, 2] = 1.0
    return out


def _clouds(first, num, P):
    for n, (f, s) in enumerate(zip(np.asarray(first, np.int64), np.asarray(num, np.int64))):
        f = int(min(max(f, 0), P))
        s = int(min(max(s, 0), P - f))
        if s:
            yield n, f, s


def disambiguate(points, normals, knn_idx, first, num, mode=0, viewpoint=None):
    """dss_disambiguate_normals -> normals (P,3) float32"""
    pts, nrm = np.asarray(points, F32), np.asarray(normals, F32)
    P = pts.shape[0]
    out = _unowned(P)
    for n, f, s in _clouds(first, num, P):
        p, v = pts[f:f + s], nrm[f:f + s]
        if mode == 0:
            idx = np.asarray(knn_idx, np.int64)[f:f + s]
            kn = min(idx.shape[1], s)
            j = idx[:, :kn]
            ok = (j >= 0) & (j < s)
            with np.errstate(invalid="ignore", over="ignore"):
                d = p[np.clip(j, 0, s - 1)] - p[:, None, :]
            proj = _dot(v[:, None, :], d)
            pos = ((proj > 0) & ok).sum(1)
            flip = 2 * pos < kn
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                d = np.asarray(viewpoint, F32).reshape(-1, 3)[n][None, :] - p
            flip = _dot(v, d) < 0
        out[f:f + s] = np.where(flip[:, None], -v, v)
    return out


def seed_sign_flip(n):
    """the seed rule: of (n.z, n.y, n.x) the first that is positive or negative is made positive -> flip?"""
    for c in (n[2], n[1], n[0]):
        if c > 0:
            return False
        if c < 0:
            return True
    return False


def orient_cloud(normals, points, knn_idx, KP):
    """One cloud alone -> (normals (P,3) float32, stamp (P,) int32, parent (P,) int64, iterations)"""
    n, z = np.asarray(normals, F32), np.asarray(points, F32)[:, 2]
    idx = np.asarray(knn_idx, np.int64)
    P, K = n.shape[0], idx.shape[1]
    kp = min(KP, K, P)
    out, stamp, parent = n.copy(), np.zeros(P, np.int32), np.full(P, -1, np.int64)
    nb = idx[:, 1:max(kp, 1)]
    valid = (nb != np.arange(P)[:, None]) & (nb >= 0) & (nb < P)
    nb = np.clip(nb, 0, P - 1)
    level = it = 0
    while (stamp == 0).any() and it < 5 * P:
        it += 1
        un = np.flatnonzero(stamp == 0)
        oriented_now = False
        if nb.shape[1]:
            j = nb[un]
            # every stamp set so far was set in an earlier iteration: the state is only changed at the end of this one
            ok = valid[un] & (stamp[j] > 0)
            d = _dot(n[un][:, None, :], out[j])
            a = np.abs(d)
            with np.errstate(invalid="ignore"):
                ok &= a >= TAU[level]                       # a NaN never passes
            cand = ok.any(1)
            if cand.any():
                am = np.where(ok, a, F32(-1.0))
                top = am.max(1)
                best = ok & (am == top[:, None])
                jj = np.where(best, j, np.iinfo(np.int64).max).min(1)      # ties to the smallest id
                slot = np.argmax(best & (j == jj[:, None]), 1)
                dsel = d[np.arange(len(un)), slot]
                rows = un[cand]
                flip = dsel[cand] < 0
                out[rows] = np.where(flip[:, None], -n[rows], n[rows])
                stamp[rows] = it
                parent[rows] = jj[cand]
                level = 0
                oriented_now = True
        if oriented_now:
            continue
        if level < 3:
            level += 1
            continue
        zu = z[un]
        real = ~np.isnan(zu)
        s = un[0] if not real.any() else un[real & (zu == zu[real].max())][0]     # NaN loses; ties to the smallest id
        out[s] = -n[s] if seed_sign_flip(n[s]) else n[s]
        stamp[s] = it
        level = 0
    return out, stamp, parent, it


def orient(normals, points, knn_idx, first, num, KP=8):
    """dss_orient_normals -> (normals (P,3) float32, stamp (P,) int32, parent (P,) int64, iterations of every cloud)"""
    nrm, pts, idx = np.asarray(normals, F32), np.asarray(points, F32), np.asarray(knn_idx, np.int64)
    P = nrm.shape[0]
    out, stamp, parent, its = _unowned(P), np.zeros(P, np.int32), np.full(P, -1, np.int64), {}
    for n, f, s in _clouds(first, num, P):
        out[f:f + s], stamp[f:f + s], parent[f:f + s], its[n] = orient_cloud(nrm[f:f + s], pts[f:f + s], idx[f:f + s], KP)
    return out, stamp, parent, its


# ---- neighbour lists and PCA directions on the host ----------------------------------------------------------------------

def knn_lists(points, K):
    """(P,K) int64 lists of one cloud in the (distance, id) order of dss_knn_points, self first; zero-padded behind the
    min(K, P) entries.  Brute force in float64: for the small clouds of the tests."""
    p = np.asarray(points, np.float64)
    P = p.shape[0]
    out = np.zeros((P, K), np.int64)
    kk = min(K, P)
    for s in range(0, P, 1024):
        q = p[s:s + 1024]
        with np.errstate(invalid="ignore"):
            d = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        d[np.isnan(d)] = np.inf
        d[np.arange(len(q)), np.arange(s, s + len(q))] = -1.0      # self first, whatever coincides with it
        out[s:s + 1024, :kk] = np.argsort(d, axis=1, kind="stable")[:, :kk]
    return out


def tree_lists(points, K):
    """`knn_lists` by a KD-tree, for the golden clouds"""
    from scipy.spatial import cKDTree
    p = np.asarray(points, np.float64)
    idx = cKDTree(p).query(p, k=K)[1].astype(np.int64)
    idx[:, 0] = np.arange(len(p))
    return idx


def pca_normals(points, idx, fp32=False):
    """the direction of least variance of every neighbourhood `idx` (P,K) of one cloud, sign as the solver leaves it ->
    (P,3) float32.  Covariances in float64, or with ``fp32`` those of `frames_reference.local_frames_fp32`."""
    import frames_reference
    pts = np.asarray(points, F32)
    first, num = [0], [pts.shape[0]]
    if fp32:
        C, _ = frames_reference.local_frames_fp32(pts, idx, first, num)
        return np.ascontiguousarray(np.linalg.eigh(C)[1][:, :, 0]).astype(F32)
    return np.ascontiguousarray(frames_reference.local_frames_reference(pts, idx, first, num).vec[:, :, 0]).astype(F32)


# ---- seeded shapes ---------------------------------------------------------------------------------------------------------

def fibonacci_sphere(P, centre=(0.0, 0.0, 0.0), radius=1.0):
    """-> (points (P,3) float32, outward unit normals (P,3) float32)"""
    i = np.arange(P) + 0.5
    phi, zc = np.pi * (1.0 + 5.0 ** 0.5) * i, 1.0 - 2.0 * i / P
    r = np.sqrt(1.0 - zc * zc)
    n = np.stack([r * np.cos(phi), r * np.sin(phi), zc], 1)
    return (n * radius + np.asarray(centre)).astype(F32), n.astype(F32)


def torus(P, seed=0, R=1.0, r=0.35):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, P), rng.uniform(0, 2 * np.pi, P)
    n = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    p = np.stack([R * np.cos(u), R * np.sin(u), np.zeros(P)], 1) + r * n
    return p.astype(F32), n.astype(F32)


def random_signs(normals, seed):
    s = np.where(np.random.default_rng(seed).random(normals.shape[0]) < 0.5, -1.0, 1.0).astype(F32)
    return (normals * s[:, None]).astype(F32)


def plane_grid(side=16, seed=3):
    """side x side grid in z = 0 with normals (0,0,+-1) of random sign: every |d| is 1"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    p = np.concatenate([g, np.zeros((side * side, 1))], 1).astype(F32) * F32(0.125)
    return p, random_signs(np.tile(np.array([[0, 0, 1]], F32), (side * side, 1)), seed)


def cube(side=10):
    """six faces of side x side points with their analytic outward normals; the points of a face keep clear of its edges"""
    t = (np.arange(side) + 0.5) / side * 2.0 - 1.0
    a, b = [x.reshape(-1) for x in np.meshgrid(t, t, indexing="ij")]
    pts, nrm = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            p = np.zeros((side * side, 3))
            p[:, axis] = sign
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = a, b
            n = np.zeros((side * side, 3))
            n[:, axis] = sign
            pts.append(p)
            nrm.append(n)
    return np.concatenate(pts).astype(F32), np.concatenate(nrm).astype(F32)


def polyline(P=4000, seed=5):
    """an open, gently bending line in space with unit normals across it, random sign"""
    t = np.linspace(0.0, 1.0, P)
    p = np.stack([t * 40.0, np.sin(6.0 * t), t * 2.0], 1)
    tangent = np.gradient(p, axis=0)
    n = np.cross(tangent, np.array([0.0, 0.0, 1.0]))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return p.astype(F32), random_signs(n.astype(F32), seed)


def outward_share(normals, outward):
    return float((_dot(normals, outward) > 0).mean())
