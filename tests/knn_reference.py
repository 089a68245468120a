"""Plain fp64 references of the neighbour statistic behind the variance scale h, stated once for the kNN tests.

Everything here is numpy / scipy on the CPU: a KD-tree over fp64 copies of the points, and an O(P^2) brute force that the
KD-tree itself is checked against (`brute_kth`, `brute_radius_stat`) so that the reference does not rest on scipy alone."""
import numpy as np
from scipy.spatial import cKDTree

# distances: the same pair of points evaluated in fp32 (kernel) and fp64 (here)
DIST_RTOL, DIST_ATOL = 2e-5, 1e-9
MEAN_RTOL = 1e-5


def kth(points, K):
    if points.shape[0] == 0:
        return np.zeros(0, np.float32)
    k = min(K, points.shape[0])
    d, _ = cKDTree(points.astype(np.float64)).query(points.astype(np.float64), k=k)
    d = d.reshape(points.shape[0], -1)
    return (d[:, -1] ** 2).astype(np.float32)


def radius_stat(points, K, r):
    """frnn_grid_points(K, r) followed by `sq_dist[:, :, 1:].max(-1)` (rasterizer.py:317-324): neighbours beyond r come back
    as -1; the statistic is the farthest of the K - 1 nearest non-self neighbours that lies within r, -1 if there is none"""
    P = points.shape[0]
    if P == 0:
        return np.zeros(0, np.float32)
    k = min(K, P)
    d, _ = cKDTree(points.astype(np.float64)).query(points.astype(np.float64), k=k)
    d2 = d.reshape(P, -1)[:, 1:] ** 2
    d2 = np.where(d2 <= float(r) ** 2, d2, -1.0)
    return (d2.max(1) if d2.shape[1] else np.full(P, -1.0)).astype(np.float32)


def sorted_sq(points, K, workers=8):
    """(P, K) squared distances of every point to its K nearest of the cloud, itself first, ascending; zero-padded when the
    cloud has fewer than K points (the layout of the full-list entry); one KD-tree query serves every k <= K"""
    P = points.shape[0]
    out = np.zeros((P, K))
    if P == 0:
        return out
    k = min(K, P)
    p64 = points.astype(np.float64)
    d, _ = cKDTree(p64).query(p64, k=k, workers=workers)
    out[:, :k] = d.reshape(P, -1) ** 2
    return out


def stat_from_sorted(sq, n_points, K, r=None):
    """`kth` / `radius_stat` of a cloud of n_points from its `sorted_sq` table (K <= its width)"""
    k = min(K, n_points)
    if n_points == 0:
        return np.zeros(0, np.float32)
    if r is None or r <= 0:
        return sq[:, k - 1].astype(np.float32)
    d2 = np.where(sq[:, 1:k] <= float(r) ** 2, sq[:, 1:k], -1.0)
    return (d2.max(1) if d2.shape[1] else np.full(n_points, -1.0)).astype(np.float32)


def stat(points, K, r=None):
    """`radius_stat` for r > 0, else the plain K-th distance"""
    return radius_stat(points, K, r) if (r is not None and r > 0) else kth(points, K)


def _brute_sorted_sq(points, K):
    """(P, min(K, P)) smallest squared distances of every point to the cloud, itself included, ascending; O(P^2) fp64"""
    p = points.astype(np.float64)
    out = np.empty((p.shape[0], min(K, p.shape[0])))
    for s in range(0, p.shape[0], 512):
        d2 = ((p[s:s + 512, None, :] - p[None, :, :]) ** 2).sum(-1)
        out[s:s + 512] = np.sort(d2, axis=1)[:, :out.shape[1]]
    return out


def brute_kth(points, K):
    if points.shape[0] == 0:
        return np.zeros(0, np.float32)
    return _brute_sorted_sq(points, K)[:, -1].astype(np.float32)


def brute_radius_stat(points, K, r):
    P = points.shape[0]
    if P == 0:
        return np.zeros(0, np.float32)
    d2 = _brute_sorted_sq(points, K)[:, 1:]
    d2 = np.where(d2 <= float(r) ** 2, d2, -1.0)
    return (d2.max(1) if d2.shape[1] else np.full(P, -1.0)).astype(np.float32)


def view_depth32(cloud, V_n):
    """view depth with the kernel's expression, every operation rounded to fp32 (KnnCamera::kept in knn.hip)"""
    c, V = cloud.astype(np.float32), V_n.astype(np.float32)
    return ((c[:, 0] * V[0, 2] + c[:, 1] * V[1, 2]) + c[:, 2] * V[2, 2]) + np.float32(1.0) * V[3, 2]


def plane_gap(cloud, V_n, znear_n, zfar_n):
    """smallest fp64 distance (in depth units) of a point to one of the camera's two depth planes: a scene whose points
    are meant to lie clearly on one side asserts that this is far above fp32 rounding (1e-6), so that the kept set does
    not depend on how the depth expression is rounded or contracted"""
    if cloud.shape[0] == 0:
        return np.inf
    c, V = cloud.astype(np.float64), V_n.astype(np.float64)
    z = c[:, 0] * V[0, 2] + c[:, 1] * V[1, 2] + c[:, 2] * V[2, 2] + V[3, 2]
    return float(min(np.abs(z - float(znear_n)).min(), np.abs(z - float(zfar_n)).min()))


def view_stat(cloud, V_n, znear_n, zfar_n, K, r=None):
    """The reference's order (rasterizer.py:599, 183-217, 310-326): the camera drops the points outside [znear, zfar]
    (inclusive bounds, depth in fp32 like the kernel so that `ok` is the kernel's set), THEN the neighbours are searched
    among the points it keeps -> (ok (P,) bool, statistic of the kept points (ok.sum(),))"""
    z = view_depth32(cloud, V_n)
    ok = (z >= np.float32(znear_n)) & (z <= np.float32(zfar_n))
    return ok, stat(cloud[ok], K, r)


def view_row(cloud, V_n, znear_n, zfar_n, K, r=None):
    """`view_stat` laid out like the kernel's output: the statistic at the kept points, 0 at the dropped ones"""
    ok, s = view_stat(cloud, V_n, znear_n, zfar_n, K, r)
    row = np.zeros(cloud.shape[0], np.float32)
    row[ok] = s
    return ok, row


def padded_mean_clamp(stats_per_camera, kept_counts, scale, lo, hi, fallback, min_points):
    """h of every camera from the statistic of the points it keeps: fp64 sum of stat * scale over the kept points divided by
    the LARGEST kept count of the batch -- the reference's `h_k.mean(dim=1)` runs over the padded length of the filtered
    batch, the padding contributing zeros (rasterizer.py:326) -- clamped to [lo, hi].  A camera that keeps fewer than
    `min_points` gets `fallback` (`sq_dist[num_points_per_cloud < 7] = 1e-3` fills the whole padded row, :323, and 0.5 * 1e-3
    is the fallback the rasterizer passes).  When no camera keeps anything the reference takes the mean of an empty
    dimension (NaN); this follows renderable_mean_kernel instead, which returns `fallback` for every camera."""
    cmax = max([int(c) for c in kept_counts] + [0])
    out = []
    for s, c in zip(stats_per_camera, kept_counts):
        if int(c) >= min_points and cmax > 0:
            m = float((np.asarray(s, np.float32).astype(np.float64) * float(scale)).sum() / cmax)
        else:
            m = float(fallback)
        out.append(min(max(np.float32(m), np.float32(lo)), np.float32(hi)))
    return np.array(out, np.float32)


def assert_stat_close(got, want, what=""):
    """distances to the project's tolerance; sign pattern (< 0: no neighbour within r) and exact zeros compared exactly"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), (what, "NaN", int(np.isnan(got).sum()))
    assert ((got < 0) == (want < 0)).all(), (what, "sign pattern", int(((got < 0) != (want < 0)).sum()))
    assert ((got == 0) == (want == 0)).all(), (what, "zeros", int(((got == 0) != (want == 0)).sum()))
    bad = ~np.isclose(got, want, rtol=DIST_RTOL, atol=DIST_ATOL)
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(got - want).max()))
