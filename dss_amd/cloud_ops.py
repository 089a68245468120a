"""Operators on a whole cloud between optimiser phases.  Those that change the NUMBER of points: `upsample` /
`upsample_clouds` insert points where a neighbourhood is sparsest (DSS/core/cloud.py:555-632), `remove_outliers` drops the
points whose neighbourhood is not flat (:363-378).  Both sit on the exact grid kNN (``ops.knn_points``); the K x K sparsity
search and the assembly of the grown cloud are the HIP kernels of ``dss_amd/csrc/upsample.hip``, the curvature test reads
``ops.local_frames``.  DESIGN 4.14 states the round's contract, tie rules included.  Those that CLEAN a cloud:
`denoise_normals` filters the normals over a neighbourhood (:515-552) and `project_to_latent_surface` moves every point
onto a locally fitted implicit surface (RIMLS, :442-513); their kernels are ``dss_amd/csrc/smoothing.hip``, their contract
is DESIGN 4.15.  Nothing here is differentiable: the reference uses these tools to re-parametrise a model between optimiser
phases.  The one that THINS a cloud evenly: `sample_farthest_points` (pytorch3d's call) and `subsample` pick a subset by
farthest point sampling -- every new point the one farthest from those already picked, ties to the smallest id, no point
picked twice -- in one persistent workgroup per cloud (``dss_amd/csrc/sampling.hip``); `subsample` with
``method="random"`` is the reference's `subsample_randomly` (:260-279), which keeps the density of its input.  The one that
gives a cloud its NORMALS: `estimate_normals` (:210-258) takes the PCA direction of every neighbourhood and chooses its sign,
by default so that every connected part shows one side; `orient_normals` does the same for normals that exist
(``dss_amd/csrc/normals.hip``).
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


def _smoothing_inputs(who: str, points, normals, num_points, K: int, search_radius):
    """Shapes, sizes and refusals that the two cleaning tools share -> (points (N,P,3), normals (N,P,3), sizes).  Nothing is
    launched here."""
    if isinstance(points, PointClouds3D):
        if normals is None:
            normals = points.normals_padded()
        if num_points is None:
            num_points = [int(p.shape[0]) for p in points.points_list()]
        points = points.points_padded()
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("%s expects padded points (N,P,3) or a PointClouds3D" % who)
    if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(points.shape):
        raise ValueError("%s expects normals of the points' shape %s" % (who, tuple(points.shape)))
    N, P = points.shape[0], points.shape[1]
    if K < 1 or K + 1 > MAX_KNN:
        raise ValueError("%s: neighborhood_size must be in 1 .. %d (it searches K + 1 <= %d neighbours), got %d"
                         % (who, MAX_KNN - 1, MAX_KNN, K))
    if search_radius is not None and not float(search_radius) > 0.0:
        raise ValueError("%s: search_radius must be positive, got %r" % (who, search_radius))
    sizes = _host_ints(P if num_points is None else num_points, N, "num_points")
    if any(s < 0 or s > P for s in sizes):
        raise ValueError("num_points must lie in 0 .. P = %d" % P)
    if not points.is_cuda or not normals.is_cuda:
        bad = points if not points.is_cuda else normals
        raise RuntimeError("dss_amd: %s is on %s; the HIP path needs GPU tensors (no CPU fallback)"
                           % ("points" if bad is points else "normals", bad.device))
    return points.detach(), normals.detach(), sizes


def _search_radius(points, sizes: Sequence[int], c: float, K: int, search_radius) -> torch.Tensor:
    """(N,) fp32 on the device: ``search_radius`` when given, else min(c K sqrt(diag_n / P_n), 0.2) with diag_n the length
    of the bounding-box diagonal of cloud n alone (cloud.py:449-451, 522-525).  No device-to-host read."""
    if search_radius is not None:
        return torch.full((len(sizes),), float(search_radius), dtype=torch.float32, device=points.device)
    r = torch.full((len(sizes),), 0.2, dtype=torch.float32, device=points.device)   # an empty cloud: unused
    for n, s in enumerate(sizes):
        if s > 0:
            x = points[n, :s].to(torch.float32)
            diag = (x.amax(dim=0) - x.amin(dim=0)).norm()
            r[n] = (float(c * K) * torch.sqrt(diag / float(s))).clamp(max=0.2)
    return r


def _packed_lists(points, normals, sizes, K: int):
    dev = points.device
    pts = _pack(points.to(torch.float32), sizes).contiguous()
    nrm = _pack(normals.to(torch.float32), sizes).contiguous()
    first, num = _ranges(sizes, dev)
    knn_d, knn_idx = ops.knn_points(pts, first, num, K + 1)
    return pts, nrm, first, num, knn_d, knn_idx


@torch.no_grad()
def denoise_normals(points, normals=None, num_points=None, sharpness_sigma: float = 30.0, neighborhood_size: int = 16,
                    search_radius: Optional[float] = None):
    """Bilateral filter of the normals over the ``neighborhood_size`` nearest points: `denoise_normals` of
    DSS/core/cloud.py:515-552 -> normals (N,P,3), unit length, a new tensor; padding rows are zeros.

    points, normals (N,P,3) padded with ``num_points`` the N lengths (None: all P), or a ``PointClouds3D`` (then
    ``normals=None`` takes the cloud's own).  A neighbour counts if it lies within ``search_radius``, by default
    min(4 K sqrt(diag / P_n), 0.2) per cloud; its weight is exp(-((1 - n_j.n) / sharpness_sigma)^2) times
    exp(-|q_j - p|^2 P_n / 2) cut at |q_j - p|^2 <= 32 / P_n.  DESIGN 4.15 states the contract and the two deviations
    from the reference: a neighbour outside the radius contributes nothing (the reference gathers zeros for it), and a
    point without any weight keeps its normalised normal (the reference returns a zero vector).  Every cloud is processed
    as if it were alone.

    Not differentiable.  With sizes given as Python integers the call reads nothing back from the device.  Raises
    ValueError, before anything is launched, for wrong shapes, K outside 1 .. 39, ``search_radius <= 0`` and
    ``sharpness_sigma <= 0``.  GPU tensors only: there is no CPU fallback."""
    K = int(neighborhood_size)
    if not float(sharpness_sigma) > 0.0:
        raise ValueError("denoise_normals: sharpness_sigma must be positive, got %r" % (sharpness_sigma,))
    points, normals, sizes = _smoothing_inputs("denoise_normals", points, normals, num_points, K, search_radius)
    radius = _search_radius(points, sizes, 4.0, K, search_radius)
    pts, nrm, first, num, knn_d, knn_idx = _packed_lists(points, normals, sizes, K)
    out = ops.denoise_normals(pts, nrm, knn_d, knn_idx, first, num, radius, K, float(sharpness_sigma))
    return _pad_to(out, sizes, points.shape[1])


@torch.no_grad()
def project_to_latent_surface(points, normals=None, num_points=None, sharpness_angle: float = 60.0,
                              neighborhood_size: int = 31, max_proj_iters: int = 10, max_est_iter: int = 5,
                              search_radius: Optional[float] = None, return_converged: bool = False):
    """Move every point onto the implicit surface fitted to its neighbourhood (robust implicit MLS):
    `project_to_latent_surface` of DSS/core/cloud.py:442-513 -> points (N,P,3), a new tensor (the input is not modified;
    padding rows are zeros), and with ``return_converged`` also (N,P) bool: the points that stopped moving (a step shorter
    than 5e-4, or no usable neighbourhood; padding rows False).

    ``max_proj_iters`` outer iterations, each ``max_est_iter`` reweighting passes over the ``neighborhood_size`` nearest
    points of the INPUT cloud within ``search_radius`` (default min(16 K sqrt(diag / P_n), 0.2) per cloud); every
    iteration moves the points that have not converged by f grad f of the fitted function, all at once.  ``normals``
    should be filtered first (`denoise_normals`).  ``sharpness_angle`` is accepted and unused, as in the reference.  DESIGN
    4.15 states the arithmetic; it improves planar and gently curved clouds and inflates sparse, strongly curved ones.

    Not differentiable.  The iterations are launched back to back; with sizes given as Python integers nothing is read
    back from the device.  Raises ValueError, before anything is launched, for wrong shapes, K outside 1 .. 39,
    ``max_proj_iters < 1``, ``max_est_iter < 1`` and ``search_radius <= 0``.  GPU tensors only: no CPU fallback."""
    K = int(neighborhood_size)
    if int(max_proj_iters) < 1 or int(max_est_iter) < 1:
        raise ValueError("project_to_latent_surface: max_proj_iters and max_est_iter must be at least 1, got %r and %r"
                         % (max_proj_iters, max_est_iter))
    points, normals, sizes = _smoothing_inputs("project_to_latent_surface", points, normals, num_points, K, search_radius)
    radius = _search_radius(points, sizes, 16.0, K, search_radius)
    pts, nrm, first, num, knn_d, knn_idx = _packed_lists(points, normals, sizes, K)
    live = None
    for _ in range(int(max_proj_iters)):
        pts, live = ops.rimls_step(pts, nrm, knn_d, knn_idx, first, num, radius, K, live, int(max_est_iter))
    out = _pad_to(pts, sizes, points.shape[1])
    if not return_converged:
        return out
    return out, _pad_to(live == 0, sizes, points.shape[1])


def _pad_to(packed, sizes, P: int):
    """`_pad` to a given row count P >= max(sizes)."""
    out = packed.new_zeros((len(sizes), P) + tuple(packed.shape[1:]))
    f = 0
    for n, s in enumerate(sizes):
        out[n, :s] = packed[f:f + s]
        f += s
    return out


def _host_floats(x, N: int, name: str) -> List[float]:
    """`_host_ints` for floats."""
    if isinstance(x, torch.Tensor):
        x = x.reshape(-1).tolist()
    if isinstance(x, (int, float)):
        x = [x] * N
    x = [float(v) for v in x]
    if len(x) == 1 and N > 1:
        x = x * N
    if len(x) != N:
        raise ValueError("%s must be one number or %d of them, got %d" % (name, N, len(x)))
    return x


def check_sampling(who: str, sizes: Sequence[int], counts: Sequence[int], starts: Sequence[int]) -> None:
    """The refusals of the sampling calls, from host integers, before anything is launched (ValueError)."""
    for n, (s, k, c) in enumerate(zip(sizes, counts, starts)):
        if k < 0:
            raise ValueError("%s: cloud %d is asked for %d samples, a negative count" % (who, n, k))
        if c < 0 or c >= max(s, 1):
            raise ValueError("%s: start_idx %d lies outside cloud %d of %d points" % (who, c, n, s))


def _require_gpu_cloud(t) -> None:
    if not t.is_cuda:
        raise RuntimeError("dss_amd: points is on %s; the HIP path needs GPU tensors (no CPU fallback)" % t.device)


@torch.no_grad()
def sample_farthest_points(points, lengths=None, K: Union[int, Sequence[int], torch.Tensor] = 50,
                           start_idx: Union[int, Sequence[int], torch.Tensor] = 0):
    """Farthest point sampling of every cloud, pytorch3d's ``sample_farthest_points`` with a fixed start ->
    ``(selected (N, K_max, 3), idx (N, K_max) int64)``, K_max = max(K): the points of every cloud that were picked, in the
    order of picking, and their cloud-local ids.  Behind the min(K_n, P_n) samples of cloud n: id -1, point 0
    (pytorch3d's padding).

    points (N,P,3) padded with ``lengths`` the N sizes (None: all P), or a ``PointClouds3D`` (its own sizes).  ``K`` and
    ``start_idx`` are one integer or N of them; cloud n starts at its point ``start_idx[n]``.

    The selection: with d[i] the squared distance, in fp32 as ``(dx dx + dy dy) + dz dz``, of point i to the
    nearest point picked so far, the next pick is the point of the largest d, among equals the one of the SMALLEST id, and
    a picked point is never picked again -- so K_n = P_n returns a permutation even when points coincide.  Those are the
    two places where this departs from pytorch3d, which lets its argmax break ties and repeats a point once all distances
    are 0.  A point with a NaN coordinate keeps d = +inf: it is picked second and then never again.  Every cloud is sampled
    as if it were alone, by one persistent workgroup; padding rows are not read.

    Not differentiable.  With integers given as Python integers the call reads nothing back from the device and can be
    captured in a graph; integers given as GPU tensors cost one read each.  Raises ValueError, before anything is launched,
    for wrong shapes, a negative count and a ``start_idx`` outside its cloud.  GPU tensors only: no CPU fallback."""
    who = "sample_farthest_points"
    if isinstance(points, PointClouds3D):
        sizes = [int(p.shape[0]) for p in points.points_list()]
        N, firsts = len(sizes), [sum(sizes[:n]) for n in range(len(sizes))]
        packed = points.points_packed().detach()
    else:
        if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 3:
            raise ValueError("%s expects padded points (N,P,3) or a PointClouds3D" % who)
        N, P = points.shape[0], points.shape[1]
        sizes = _host_ints(P if lengths is None else lengths, N, "lengths")
        if any(s < 0 or s > P for s in sizes):
            raise ValueError("lengths must lie in 0 .. P = %d" % P)
        firsts = [n * P for n in range(N)]   # the padded batch IS a packed array with rows that no cloud owns
        packed = points.detach().reshape(N * P, 3)
    counts, starts = _host_ints(K, N, "K"), _host_ints(start_idx, N, "start_idx")
    check_sampling(who, sizes, counts, starts)
    _require_gpu_cloud(packed)
    dev, K_max = packed.device, max(counts)
    first = _device_ints(firsts, dev)
    idx = ops.farthest_points(packed.to(torch.float32), first, _device_ints(sizes, dev), _device_ints(counts, dev),
                              _device_ints(starts, dev) if any(starts) else None, K_max)
    if packed.shape[0] == 0 or K_max == 0:
        return packed.new_zeros((N, K_max, 3)), idx
    selected = packed[(first[:, None] + idx.clamp(min=0)).clamp(max=packed.shape[0] - 1)]   # (a padding id reads any row)
    return torch.where((idx >= 0)[..., None], selected, torch.zeros_like(selected)), idx


@torch.no_grad()
def subsample(point_clouds, n_points: Union[None, int, Sequence[int], torch.Tensor] = None,
              ratio: Union[None, float, Sequence[float], torch.Tensor] = None, method: str = "farthest",
              start_idx: Union[int, Sequence[int], torch.Tensor] = 0, generator=None) -> PointClouds3D:
    """Thin every cloud of a ``PointClouds3D`` to ``n_points`` points (at most its size) or to ``int(ratio * P_n)`` of
    them -> a new container (detached tensors; the input is not modified).  Normals and features follow their points; the
    rows stand in the order in which they were picked.  Exactly one of ``n_points`` / ``ratio`` (one value or one per cloud).

    ``method="farthest"``: an even subset by farthest point sampling from ``start_idx`` (`sample_farthest_points`: ties to
    the smallest id, no point twice), the inverse of `upsample`.  GPU tensors only.
    ``method="random"``: the reference's `subsample_randomly` (DSS/core/cloud.py:260-279), the first rows of a
    ``torch.randperm(P_n)`` drawn on the cloud's device from ``generator``; it keeps the density of the input.

    Not differentiable.  Raises ValueError, before anything is launched, for a negative count, a ``ratio`` outside [0, 1],
    a ``start_idx`` outside its cloud, both or neither of ``n_points`` / ``ratio`` and an unknown ``method``."""
    if method not in ("farthest", "random"):
        raise ValueError("subsample: method must be 'farthest' or 'random', got %r" % (method,))
    if (n_points is None) == (ratio is None):
        raise ValueError("subsample: give exactly one of n_points and ratio")
    pts = point_clouds.points_list()
    N = len(pts)
    sizes = [int(p.shape[0]) for p in pts]
    if ratio is not None:
        ratios = _host_floats(ratio, N, "ratio")
        if any(not 0.0 <= r <= 1.0 for r in ratios):
            raise ValueError("subsample: ratio must lie in [0, 1], got %r" % (ratio,))
        counts = [int(r * s) for r, s in zip(ratios, sizes)]
    else:
        counts = _host_ints(n_points, N, "n_points")
    starts = _host_ints(start_idx, N, "start_idx") if method == "farthest" else [0] * N
    check_sampling("subsample", sizes, counts, starts)
    counts = [min(k, s) for k, s in zip(counts, sizes)]
    dev = pts[0].device
    if method == "farthest":
        _require_gpu_cloud(pts[0])
        first, num = _ranges(sizes, dev)
        packed = torch.cat([p.detach().to(torch.float32) for p in pts], dim=0).contiguous()
        idx = ops.farthest_points(packed, first, num, _device_ints(counts, dev),
                                  _device_ints(starts, dev) if any(starts) else None, max(counts))
        keep = [idx[n, :k] for n, k in enumerate(counts)]
    else:
        keep = [torch.randperm(s, device=dev, generator=generator)[:k] for s, k in zip(sizes, counts)]
    pick = lambda lst: None if lst is None else [t.detach().index_select(0, k) for t, k in zip(lst, keep)]
    return PointClouds3D(pick(pts), pick(point_clouds.normals_list()), pick(point_clouds.features_list()))


ORIENTATIONS = ("none", "local", "viewpoint", "consistent")


def _normals_points(who: str, points, num_points):
    """Shapes and sizes that the two normal calls share -> (points (N,P,3), sizes).  Nothing is launched here."""
    if isinstance(points, PointClouds3D):
        if num_points is None:
            num_points = [int(p.shape[0]) for p in points.points_list()]
        points = points.points_padded()
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("%s expects padded points (N,P,3) or a PointClouds3D" % who)
    N, P = points.shape[0], points.shape[1]
    sizes = _host_ints(P if num_points is None else num_points, N, "num_points")
    if any(s < 0 or s > P for s in sizes):
        raise ValueError("num_points must lie in 0 .. P = %d" % P)
    return points.detach(), sizes


def _check_neighbourhood(who: str, sizes: Sequence[int], K: int) -> None:
    if K < 1 or K > MAX_KNN:
        raise ValueError("%s: neighborhood_size must be in 1 .. %d, got %d" % (who, MAX_KNN, K))
    for n, s in enumerate(sizes):
        if s <= K:
            raise ValueError("%s: cloud %d has %d points, the neighbourhood size is %d" % (who, n, s, K))


@torch.no_grad()
def estimate_normals(points, num_points=None, neighborhood_size: int = 16, orientation: str = "consistent",
                     orientation_neighbours: int = 8, viewpoint=None, return_curvature: bool = False):
    """Unit normals of a cloud that has none -> normals (N,P,3), a new tensor, padding rows zero; with
    ``return_curvature`` also the ascending eigenvalues (N,P,3) of every neighbourhood's covariance.

    points (N,P,3) padded with ``num_points`` the N lengths (None: all P), or a ``PointClouds3D``.  The direction is the
    axis of least variance of the ``neighborhood_size`` nearest points, the point itself included (``ops.knn_points``,
    ``ops.local_frames``: `estimate_pointcloud_normals` of DSS/utils/mathHelper.py:113-147).  Its sign, by ``orientation``:

    ``"none"``        as the eigen-solver leaves it.
    ``"local"``       the reference's rule (Tombari's majority vote): towards the side on which most of the neighbourhood
                      lies.  Decided per point; on a convex shape nearly every normal ends up pointing inward.
    ``"viewpoint"``   towards ``viewpoint``, (3,) for all clouds or (N,3): for a scan taken from a known position.
    ``"consistent"``  one side of the surface for every connected part: from the highest point, turned
                      upwards, the sign spreads over the ``orientation_neighbours`` nearest points (the point itself
                      counted) to the most parallel neighbours first, a fold being crossed only when nothing else is left.
                      The sign of a whole part rests on its seed -- outward for a closed surface, whose highest point
                      looks up -- and two sheets closer than the neighbourhood radius can be joined.

    Every cloud is processed as if it were alone.  Not differentiable.  With sizes given as Python integers the call reads
    nothing back from the device and can be captured in a graph.  Raises ValueError, before anything is launched, for wrong
    shapes, ``neighborhood_size`` outside 1 .. 40, a cloud with no more than ``neighborhood_size`` points,
    ``orientation_neighbours`` outside 2 .. ``neighborhood_size``, an unknown ``orientation`` and a ``viewpoint`` that is
    missing or superfluous.  GPU tensors only: there is no CPU fallback."""
    who = "estimate_normals"
    K, KP = int(neighborhood_size), int(orientation_neighbours)
    if orientation not in ORIENTATIONS:
        raise ValueError("%s: orientation must be one of %s, got %r" % (who, ", ".join(map(repr, ORIENTATIONS)), orientation))
    if (viewpoint is not None) != (orientation == "viewpoint"):
        raise ValueError("%s: orientation='viewpoint' needs a viewpoint and no other orientation takes one" % who)
    points, sizes = _normals_points(who, points, num_points)
    N = len(sizes)
    _check_neighbourhood(who, sizes, K)
    if KP < 2 or KP > K:
        raise ValueError("%s: orientation_neighbours must be in 2 .. neighborhood_size = %d, got %d" % (who, K, KP))
    if viewpoint is not None:
        viewpoint = torch.as_tensor(viewpoint, dtype=torch.float32)
        if tuple(viewpoint.shape) not in ((3,), (N, 3)):
            raise ValueError("%s: viewpoint must be (3,) or (N,3) = (%d,3), got %s" % (who, N, tuple(viewpoint.shape)))
    _require_gpu_cloud(points)
    dev = points.device
    pts = _pack(points.to(torch.float32), sizes).contiguous()
    first, num = _ranges(sizes, dev)
    _, knn_idx = ops.knn_points(pts, first, num, K)
    _, nrm, curvature = ops.local_frames(pts, knn_idx, first, num, return_curvature=True)
    if orientation == "local":
        nrm = ops.disambiguate_normals(pts, nrm, knn_idx, first, num)
    elif orientation == "viewpoint":
        nrm = ops.disambiguate_normals(pts, nrm, None, first, num, viewpoint.to(dev).expand(N, 3).contiguous())
    elif orientation == "consistent":
        nrm = ops.orient_normals(nrm, pts, knn_idx, first, num, KP)
    out = _pad_to(nrm, sizes, points.shape[1])
    return (out, _pad_to(curvature, sizes, points.shape[1])) if return_curvature else out


@torch.no_grad()
def orient_normals(points, normals, num_points=None, neighborhood_size: int = 8, return_parents: bool = False):
    """One side of the surface for a cloud that already has normals, unsigned or inconsistently signed -> normals
    (N,P,3), a new tensor: every input normal or its negative, padding rows zero; with ``return_parents`` also (N,P)
    int64, the cloud-local id of the neighbour whose sign a point took, -1 for a seed and in the padding.

    points, normals (N,P,3) padded with ``num_points`` the N lengths (None: all P), or a ``PointClouds3D`` (then
    ``normals=None`` takes the cloud's own).  The propagation of `estimate_normals` with ``orientation="consistent"`` over
    the ``neighborhood_size`` nearest points, the point itself counted.  Not differentiable; no
    device-to-host read with host integers.  Raises ValueError, before anything is launched, for wrong shapes,
    ``neighborhood_size`` outside 2 .. 40 and a cloud with no more than ``neighborhood_size`` points.  GPU tensors only:
    there is no CPU fallback."""
    who = "orient_normals"
    K = int(neighborhood_size)
    if isinstance(points, PointClouds3D) and normals is None:
        normals = points.normals_padded()
    points, sizes = _normals_points(who, points, num_points)
    if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(points.shape):
        raise ValueError("%s expects normals of the points' shape %s" % (who, tuple(points.shape)))
    if K < 2 or K > MAX_KNN:
        raise ValueError("%s: neighborhood_size must be in 2 .. %d, got %d" % (who, MAX_KNN, K))
    _check_neighbourhood(who, sizes, K)
    _require_gpu_cloud(points)
    if not normals.is_cuda:
        raise RuntimeError("dss_amd: normals is on %s; the HIP path needs GPU tensors (no CPU fallback)" % normals.device)
    dev = points.device
    pts = _pack(points.to(torch.float32), sizes).contiguous()
    nrm = _pack(normals.detach().to(torch.float32), sizes).contiguous()
    first, num = _ranges(sizes, dev)
    _, knn_idx = ops.knn_points(pts, first, num, K)
    res = ops.orient_normals(nrm, pts, knn_idx, first, num, K, return_parents=return_parents)
    if not return_parents:
        return _pad_to(res, sizes, points.shape[1])
    parents = torch.full((len(sizes), points.shape[1]), -1, dtype=_i64, device=dev)
    f = 0
    for n, s in enumerate(sizes):
        parents[n, :s] = res[1][f:f + s]
        f += s
    return _pad_to(res[0], sizes, points.shape[1]), parents
