"""Plain fp64 reference of the PCA frames behind the anisotropic source variance (TEST INFRASTRUCTURE; numpy only).

`dss_local_frames` (local_frames_kernel, setup.hip) restated without any of its shortcuts: the fp32 positions as they are,
everything else in float64, `numpy.linalg.eigh` in place of the fixed-sweep Jacobi and of the branch-free selection.  Unlike
`oracle.local_frames` it takes the cloud-local ids of `dss_knn_points` plus the packed layout, and it follows the entry point
where a cloud has fewer than K points: the first kk = min(K, num[n]) entries of a list, divided by kk.

`local_frames_fp32` is the yardstick of the GPU tests' bound, not a reference: the same pipeline in float32 (differences to the
query point, mean, covariance) with LAPACK's single-precision solver, to see what the number format alone costs."""
from collections import namedtuple

import numpy as np

Frames = namedtuple("Frames", "C lam vec vr6 owned")

# what the entry point writes for a packed slot that no cloud owns and for a neighbourhood of zero (or not normal) trace
CONST_VR6 = np.zeros(6)
CONST_NORMAL = np.array([0.0, 0.0, 1.0])
CONST_CURV = np.zeros(3)

_II, _JJ = (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)


def sym6(m):
    """(P,3,3) symmetric -> (P,6) in the order xx, xy, xz, yy, yz, zz"""
    return m[:, _II, _JJ]


def mat33(v6):
    """(P,6) -> (P,3,3) symmetric"""
    v6 = np.asarray(v6)
    return np.stack([v6[:, [0, 1, 2]], v6[:, [1, 3, 4]], v6[:, [2, 4, 5]]], 1)


def _neighbourhoods(points, knn_idx_local, first, num):
    """per cloud: (slice of its packed slots, kk, packed ids (n, kk) of the list entries that count)"""
    idx = np.asarray(knn_idx_local, np.int64)
    K = idx.shape[1]
    for f, n in zip(np.asarray(first, np.int64), np.asarray(num, np.int64)):
        if n <= 0:
            continue
        kk = int(min(K, n))
        ids = idx[f:f + n, :kk]
        assert (ids >= 0).all() and (ids < n).all(), "a list entry outside its cloud"
        yield slice(int(f), int(f + n)), kk, ids + f


def local_frames_reference(points_f32, knn_idx_local, first, num):
    """-> Frames(C (P,3,3) covariance of the kk list entries about their mean, lam (P,3) ascending eigenvalues, vec (P,3,3)
    eigenvectors in columns (vec[:, :, 0] = e0), vr6 (P,6) = C - lam0 e0 e0^T, owned (P,) bool), all float64.
    Slots outside every cloud: C = 0, lam = 0, e0 = (0,0,1), vr6 = 0, owned = False."""
    pts = np.asarray(points_f32)
    assert pts.dtype == np.float32
    P = pts.shape[0]
    p64 = pts.astype(np.float64)
    C = np.zeros((P, 3, 3))
    lam = np.zeros((P, 3))
    vec = np.tile(np.eye(3)[:, ::-1], (P, 1, 1))      # columns (0,0,1), (0,1,0), (1,0,0)
    owned = np.zeros(P, bool)
    for sl, kk, ids in _neighbourhoods(pts, knn_idx_local, first, num):
        nb = p64[ids]                                  # (n, kk, 3)
        d = nb - nb.mean(1, keepdims=True)
        C[sl] = np.einsum("nka,nkb->nab", d, d) / kk
        lam[sl], vec[sl] = np.linalg.eigh(C[sl])
        owned[sl] = True
    e0 = vec[:, :, 0]
    vr = C - lam[:, 0, None, None] * e0[:, :, None] * e0[:, None, :]
    return Frames(C, lam, vec, sym6(vr), owned)


def local_frames_fp32(points_f32, knn_idx_local, first, num):
    """The whole pipeline in float32, every operation rounded once: differences to the query point, their mean, the
    covariance with 1/kk, then `numpy.linalg.eigh` on the float32 matrix -> (C (P,3,3), lam (P,3)) float32; zeros where no
    cloud owns the slot."""
    pts = np.asarray(points_f32)
    assert pts.dtype == np.float32
    P = pts.shape[0]
    C = np.zeros((P, 3, 3), np.float32)
    lam = np.zeros((P, 3), np.float32)
    for sl, kk, ids in _neighbourhoods(pts, knn_idx_local, first, num):
        ik = np.float32(1.0) / np.float32(kk)
        diff = pts[ids] - pts[sl][:, None, :]          # (n, kk, 3) float32
        mean = np.zeros_like(diff[:, 0])
        for k in range(kk):
            mean = mean + diff[:, k]
        d = diff - (mean * ik)[:, None, :]
        c = np.zeros((diff.shape[0], 3, 3), np.float32)
        for k in range(kk):
            c = c + d[:, k, :, None] * d[:, k, None, :] * ik
        assert c.dtype == np.float32
        C[sl] = c
        lam[sl] = np.linalg.eigh(c)[0]
    return C, lam
