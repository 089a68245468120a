"""Operators that change the NUMBER of points of a cloud: `upsample` / `upsample_clouds` insert points where a neighbourhood
is sparsest (DSS/core/cloud.py:555-632), `remove_outliers` drops the points whose neighbourhood is not flat (:363-378).
Both sit on the exact grid kNN (``ops.knn_points``); the K x K sparsity search and the assembly of the grown cloud are the
HIP kernels of ``dss_amd/csrc/upsample.hip``, the curvature test reads ``ops.local_frames``.  DESIGN 4.14 states the
round's contract, tie rules included.  Nothing here is differentiable: the reference uses these tools to re-parametrise
a model between optimiser phases.
"""
from typing import List, Optional, Sequence, Union

import torch
import torch.nn.functional as F

from . import ops
from .cloud import PointClouds3D

_i64 = torch.int64
MAX_KNN = 40            # dss_knn_points: K <= 40, and a round asks for K + 1 (self first)
MAX_ATTR_CHANNELS = 16  # dss_upsample_insert: C <= 16


def _host_ints(x, N: int, name: str) -> List[int]:
    """``x`` (an int, a sequence or a tensor of N integers) as N host integers.  A tensor on the GPU is read back, once:
    pass integers to keep the call free of device-to-host reads."""
    if isinstance(x, torch.Tensor):
        x = x.reshape(-1).tolist()
    if isinstance(x, (int, float)):
        x = [x] * N
    x = [int(v) for v in x]
    if len(x) == 1 and N > 1:
        x = x * N
    if len(x) != N:
        raise ValueError("%s must be one integer or %d of them, got %d" % (name, N, len(x)))
    return x


def _device_ints(values: Sequence[int], device) -> torch.Tensor:
    """(len,) int64 on ``device`` from host integers by fill kernels: no host-to-device copy, which a pageable source
    turns into a stream synchronisation (and which stream capture refuses)."""
    out = torch.empty((len(values),), dtype=_i64, device=device)
    for i, v in enumerate(values):
        out[i].fill_(int(v))
    return out


def _ranges(sizes: Sequence[int], device):
    first, acc = [], 0
    for s in sizes:
        first.append(acc)
        acc += s
    return _device_ints(first, device), _device_ints(sizes, device)


def check_upsample(sizes: Sequence[int], targets: Sequence[int], K: int) -> None:
    """The refusals of `upsample`, from host integers, before anything is launched (ValueError)."""
    if K < 1 or K + 1 > MAX_KNN:
        raise ValueError("upsample: neighborhood_size must be in 1 .. %d (a round searches K + 1 <= %d neighbours), got %d"
                         % (MAX_KNN - 1, MAX_KNN, K))
    for n, (s, t) in enumerate(zip(sizes, targets)):
        if t < s:   # (the reference indexes with a negative count)
            raise ValueError("upsample: cloud %d has %d points, more than its target of %d" % (n, s, t))
        if t > s and s < max(10, K + 1):   # (the reference loops forever once P // 10 == 0)
            raise ValueError("upsample: cloud %d has %d points; growing it needs at least max(10, K + 1) = %d"
                             % (n, s, max(10, K + 1)))


def round_sizes(sizes: Sequence[int], targets: Sequence[int]) -> List[int]:
    """n_new of every cloud in the next round: min(remaining, P_n // 10), every cloud as if it were alone."""
    return [min(t - s, s // 10) for s, t in zip(sizes, targets)]


def _upsample_packed(points, sizes: List[int], targets: List[int], K: int, attrs=None):
    """Rounds on packed clouds until every cloud has its target size -> (points, sizes, attrs).  All sizes of all rounds
    follow from the host integers; no device-to-host read."""
    dev = points.device
    while any(t > s for s, t in zip(sizes, targets)):
        n_new = round_sizes(sizes, targets)
        first, num = _ranges(sizes, dev)
        _, knn_idx = ops.knn_points(points, first, num, K + 1)
        _, father, key = ops.upsample_candidates(points, knn_idx, first, num, K)
        # selection: per cloud ONE ascending integer sort of its keys (unique within a cloud: the id is part of the key);
        # the last n_new of it are the points to split, already in emission order
        sel, f = [], 0
        for s, k in zip(sizes, n_new):
            if k > 0:
                sel.append(torch.sort(key[f:f + s]).indices[s - k:] + f)
            f += s
        sel = torch.cat(sel) if len(sel) > 1 else sel[0]
        new_sizes = [s + k for s, k in zip(sizes, n_new)]
        new_first, new_num = _ranges(new_sizes, dev)
        points, attrs = ops.upsample_insert(points, attrs, knn_idx, father, sel, first, num, new_first, new_num,
                                            _device_ints(n_new, dev), K)
        sizes = new_sizes
    return points, sizes, attrs


def _pack(padded, sizes):
    return torch.cat([padded[n, :s] for n, s in enumerate(sizes)], dim=0) if len(sizes) > 1 else padded[0, :sizes[0]]


def _pad(packed, sizes):
    out = packed.new_zeros((len(sizes), max(sizes)) + tuple(packed.shape[1:]))
    f = 0
    for n, s in enumerate(sizes):
        out[n, :s] = packed[f:f + s]
        f += s
    return out


@torch.no_grad()
def upsample(points, n_points: Union[int, Sequence[int], torch.Tensor], num_points=None, neighborhood_size: int = 16,
             attributes: Optional[List[torch.Tensor]] = None):
    """Grow every cloud of a padded batch to ``n_points`` points by inserting points where a neighbourhood is sparsest,
    a tenth of the cloud per round: `upsample` of DSS/core/cloud.py:555-632 with its signature and padded convention.

    points (N,P,3) padded, ``num_points`` the N lengths (None: all P), ``n_points`` the target size (one for all clouds or
    N of them) -> ``(points_padded (N, max target, 3), num_points (N,) int64 on the device)``; with ``attributes``, a list
    of padded (N,P,C) tensors that ride along (old rows copied, a new row = (a_q + 2 a_p) / 3 of its two parents, not
    renormalised; at most 16 channels in all), the grown attributes are returned as a third value.

    A round: every point proposes the candidate (q_j + 2 p) / 3 among its K = ``neighborhood_size``
    neighbours that lies farthest from all of them; the min(remaining, P_n // 10) points with the sparsest candidates
    are split (ties to the smaller id) and their candidates PREPENDED to the cloud.  Every cloud is processed as if it
    were alone (the reference sorts the padded rows of a ragged batch together); a cloud that has its size is copied.

    Not differentiable (runs under ``torch.no_grad()``).  With sizes given as Python integers the call reads nothing back
    from the device; sizes given as GPU tensors cost one read each.  Raises ValueError, before anything is launched,
    for a target below the current size, a cloud that must grow but has fewer than max(10, K + 1) points, and K outside
    1 .. 39.  GPU tensors only: there is no CPU fallback."""
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("upsample expects padded points (N,P,3)")
    N, K = points.shape[0], int(neighborhood_size)
    sizes = _host_ints(points.shape[1] if num_points is None else num_points, N, "num_points")
    targets = _host_ints(n_points, N, "n_points")
    if any(s < 0 or s > points.shape[1] for s in sizes):
        raise ValueError("num_points must lie in 0 .. P = %d" % points.shape[1])
    check_upsample(sizes, targets, K)
    attributes = None if attributes is None else list(attributes)
    channels = [a.shape[-1] for a in attributes] if attributes else []
    if attributes and (sum(channels) > MAX_ATTR_CHANNELS or any(a.dim() != 3 or tuple(a.shape[:2]) != tuple(points.shape[:2])
                                                                for a in attributes)):
        raise ValueError("attributes must be padded (N,P,C) tensors like the points, with at most %d channels in all"
                         % MAX_ATTR_CHANNELS)
    if not points.is_cuda:
        raise RuntimeError("dss_amd: points is on %s; the HIP path needs GPU tensors (no CPU fallback)" % points.device)
    packed = _pack(points.to(torch.float32), sizes).contiguous()
    attrs = _pack(torch.cat([a.to(torch.float32) for a in attributes], dim=-1), sizes).contiguous() if attributes else None
    packed, sizes, attrs = _upsample_packed(packed, sizes, targets, K, attrs)
    out = (_pad(packed, sizes), _device_ints(sizes, points.device))
    if attributes is None:
        return out
    return out + (list(torch.split(_pad(attrs, sizes), channels, dim=-1)) if attributes else [],)


@torch.no_grad()
def upsample_clouds(point_clouds, n_points: Union[int, Sequence[int], torch.Tensor], neighborhood_size: int = 16) -> PointClouds3D:
    """`upsample` for a ``PointClouds3D``: the positions grow as there, normals are interpolated between the two parents
    of a new point and re-normalised (``F.normalize``, old normals too), features are interpolated.  -> a new container
    (detached tensors; the input is not modified)."""
    pts = point_clouds.points_list()
    N, K = len(pts), int(neighborhood_size)
    sizes = [int(p.shape[0]) for p in pts]
    targets = _host_ints(n_points, N, "n_points")
    check_upsample(sizes, targets, K)
    normals, feats = point_clouds.normals_list(), point_clouds.features_list()
    cn = 3 if normals is not None else 0
    cf = int(feats[0].shape[-1]) if feats is not None else 0
    if cn + cf > MAX_ATTR_CHANNELS:
        raise ValueError("upsample_clouds: normals and features have %d channels together, at most %d ride along"
                         % (cn + cf, MAX_ATTR_CHANNELS))
    if not pts[0].is_cuda:
        raise RuntimeError("dss_amd: the cloud is on %s; the HIP path needs GPU tensors (no CPU fallback)" % pts[0].device)
    packed = torch.cat([p.detach().to(torch.float32) for p in pts], dim=0).contiguous()
    cols = [torch.cat([t.detach().to(torch.float32) for t in lst], dim=0) for lst in (normals, feats) if lst is not None]
    attrs = torch.cat(cols, dim=-1).contiguous() if cols else None
    packed, sizes, attrs = _upsample_packed(packed, sizes, targets, K, attrs)
    split = lambda t: list(torch.split(t, sizes, dim=0))
    return PointClouds3D(split(packed),
                         split(F.normalize(attrs[:, :cn], dim=-1)) if cn else None,
                         split(attrs[:, cn:].contiguous()) if cf else None)


@torch.no_grad()
def remove_outliers(point_clouds, neighborhood_size: int = 16, tolerance: float = 0.05) -> PointClouds3D:
    """Drop the points whose neighbourhood is not flat: `remove_outliers` of DSS/core/cloud.py:363-378.  A point is kept
    iff ``curvature[0] / (curvature[0] + curvature[1] + curvature[2]) < tolerance``, the curvatures being the ascending
    eigenvalues of the covariance of its ``neighborhood_size`` nearest points (itself included) from
    ``ops.knn_points`` and ``ops.local_frames``.  A degenerate neighbourhood (trace 0) is dropped, as the reference's
    ``0 / 0 < tolerance`` is False.  Normals and features follow their points.  Raises ValueError when a cloud has no
    more than ``neighborhood_size`` points (mathHelper.py:57-61).  The sizes of the new clouds are the kept counts:
    the one device-to-host read of this function (the boolean indexing of every cloud)."""
    K = int(neighborhood_size)
    if K < 1 or K > MAX_KNN:
        raise ValueError("remove_outliers: neighborhood_size must be in 1 .. %d, got %d" % (MAX_KNN, K))
    pts = point_clouds.points_list()
    sizes = [int(p.shape[0]) for p in pts]
    for n, s in enumerate(sizes):
        if s <= K:
            raise ValueError("remove_outliers: cloud %d has %d points, the neighbourhood size is %d" % (n, s, K))
    packed = point_clouds.points_packed().detach().to(torch.float32).contiguous()
    first, num = point_clouds.cloud_to_packed_first_idx(), point_clouds.num_points_per_cloud()
    _, knn_idx = ops.knn_points(packed, first, num, K)
    _, _, curvature = ops.local_frames(packed, knn_idx, first, num, return_curvature=True)
    keep = (curvature[:, 0] / curvature.sum(dim=-1)) < float(tolerance)   # NaN (0 / 0) compares False
    keeps = list(torch.split(keep, sizes, dim=0))
    pick = lambda lst: None if lst is None else [t[k] for t, k in zip(lst, keeps)]
    return PointClouds3D(pick(pts), pick(point_clouds.normals_list()), pick(point_clouds.features_list()))
