"""Float64 yardstick of sparsity upsampling (the reference: `upsample`, DSS/core/cloud.py:555-632), brute
force numpy, stated once for the CPU and the GPU tests.

One round on a cloud of P points, neighbourhood size K, n_new points to insert:
  neighbours   q_0 .. q_{K-1} = entries 1 .. K of the point's (distance, id) ordered list, self dropped.  The LIST is the
               contract of `dss_knn_points`, whose distances are fp32 in the difference form (dx dx + dy dy) + dz dz: the
               distance matrix here is evaluated in exactly that arithmetic on the fp32 rounding of the positions (numpy
               float32 rounds every operation like the kernel built with -ffp-contract=off) and ordered by a STABLE
               argsort, so ties go to the smaller id.  Everything after the lists is float64.
  candidates   mid_j = (q_j + 2 p) / 3
  sparsity     m_j = min_l |mid_j - q_l|^2 over all l, l = j included
  father       s = max_j m_j, j* = the SMALLEST j that attains it
  selection    the n_new points with the largest s, ties to the smaller id, emitted in ascending (s, descending id) order
  new cloud    [the selected candidates in that order ; the old points]; attributes: (a[q_j*] + 2 a[p]) / 3
It also reports how close every decision was: per point the relative margin between its two best sqrt(m_j), per round the
relative margin of sqrt(s) at the selection cut.
"""
import numpy as np


def sphere_scene(seed, P):
    """Unit sphere with 2 % radial noise (the scenes of tests/golden/ref_upsample.npz) -> (P,3) float32."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, 3, generator=g)
    x = x / x.norm(dim=1, keepdim=True) * (1 + 0.02 * torch.randn(P, 1, generator=g))
    return x.numpy().astype(np.float32)


def knn_lists(pts, K):
    """(P,K) ids of the K nearest OTHER points in (distance, id) order: entries 1 .. K of the self query."""
    p = np.asarray(pts).astype(np.float32)
    P = p.shape[0]
    nb = np.empty((P, K), np.int64)
    for s in range(0, P, 1024):
        d = p[s:s + 1024, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        nb[s:s + 1024] = np.argsort(d2, axis=1, kind="stable")[:, 1:K + 1]
    return nb


def candidates(pts, K):
    """-> dict(nb (P,K), mid (P,K,3), m (P,K), s (P,), father (P,), father_margin (P,))"""
    pts = np.asarray(pts, np.float64)
    P = pts.shape[0]
    nb = knn_lists(pts, K)
    q = pts[nb]
    mid = (q + 2.0 * pts[:, None, :]) / 3.0
    m = np.empty((P, K))
    for s in range(0, P, 2048):
        d = mid[s:s + 2048, :, None, :] - q[s:s + 2048, None, :, :]
        m[s:s + 2048] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(-1)
    father = m.argmax(-1)          # the first maximum: the smallest j
    s_ = m.max(-1)
    if K > 1:
        r = np.sqrt(np.sort(m, -1))
        margin = (r[:, -1] - r[:, -2]) / np.maximum(r[:, -1], 1e-300)
    else:
        margin = np.ones(P)
    return dict(nb=nb, mid=mid, m=m, s=s_, father=father, father_margin=margin)


def emission_order(s, n_new):
    """ids of the n_new points with the largest s (ties to the smaller id) in ascending (s, descending id) order"""
    P = s.shape[0]
    return np.lexsort((-np.arange(P), s))[P - n_new:]


def one_round(pts, n_new, K, attrs=None):
    pts = np.asarray(pts, np.float64)
    c = candidates(pts, K)
    P = pts.shape[0]
    sel = emission_order(c["s"], n_new)
    new = c["mid"][sel, c["father"][sel]]
    r = np.sqrt(np.sort(c["s"]))
    c["cut_margin"] = (r[P - n_new] - r[P - n_new - 1]) / max(r[P - n_new], 1e-300) if 0 < n_new < P else 1.0
    c["sel"], c["new"] = sel, new
    c["points"] = np.concatenate([new, pts], 0)
    if attrs is not None:
        a = np.asarray(attrs, np.float64)
        qa = c["nb"][sel, c["father"][sel]]
        c["attrs"] = np.concatenate([(a[qa] + 2.0 * a[sel]) / 3.0, a], 0)
    return c


def upsample(pts, target, K=16, max_rounds=None):
    """Rounds of n_new = min(remaining, P // 10) until the cloud has `target` points -> (points float64, list of rounds)"""
    pts = np.asarray(pts, np.float64)
    rounds = []
    while pts.shape[0] < target and (max_rounds is None or len(rounds) < max_rounds):
        n_new = min(target - pts.shape[0], pts.shape[0] // 10)
        assert n_new > 0
        rounds.append(one_round(pts, n_new, K))
        pts = rounds[-1]["points"]
    return pts, rounds


def unmatched(new_points, other_cloud, tol=1e-5):
    """how many of `new_points` have no point of `other_cloud` within `tol` (the set comparison of multi-round results)"""
    from scipy.spatial import cKDTree
    d, _ = cKDTree(np.asarray(other_cloud, np.float64)).query(np.asarray(new_points, np.float64))
    return int((d > tol).sum())


def pack_key(sparsity_sq, local_id):
    """The sort key of `dss_upsample_candidates` as a Python integer: float bits of sparsity_sq << 32 | 0xffffffff - id."""
    bits = int(np.asarray(sparsity_sq, np.float32).reshape(()).view(np.uint32))
    return (bits << 32) | (0xFFFFFFFF - int(local_id))


def round_fp32(pts, K):
    """sparsity_sq and father of every point with each operation rounded to fp32 as upsample.hip does -- what the
    kernel must return bit for bit on the same lists; used by the CPU tests to show that the tolerances asked of the kernel
    follow from fp32 arithmetic and not from the kernel at hand"""
    p = np.asarray(pts).astype(np.float32)
    nb = knn_lists(p, K)
    q = p[nb]
    two, three = np.float32(2.0), np.float32(3.0)
    mid = (q + two * p[:, None, :]) / three
    d = mid[:, :, None, :] - q[:, None, :, :]
    m = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(-1)
    assert m.dtype == np.float32
    return m.max(-1), m.argmax(-1)
