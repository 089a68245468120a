"""Minimal packed/padded point-cloud container with the accessor names of pytorch3d's
``Pointclouds`` / DSS's ``PointClouds3D`` (DSS/core/cloud.py) that the splatting hot path calls
(rasterizer.py:155, 194, 236-240, 275-280, 651; renderer.py:57).  pytorch3d itself is absent here
[third party]; any object exposing the same accessors can be passed to ``dss_amd`` instead.
"""
from typing import List, Optional

import torch


def _to_list(x) -> Optional[List[torch.Tensor]]:
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        if x.dim() == 2:
            return [x]
        return [x[i] for i in range(x.shape[0])]
    return list(x)


_RANGES = {}


def _cloud_ranges(sizes, device):
    """(num_points_per_cloud, cloud_to_packed_first_idx) int64 tensors for a tuple of cloud sizes.  A training loop
    builds several containers per iteration with the same sizes: the two tiny tensors (a host-to-device copy each
    time) are made once per (sizes, device) and shared -- they are never written to."""
    key = (sizes, str(device))
    hit = _RANGES.get(key)
    if hit is None:
        if len(_RANGES) > 256:
            _RANGES.clear()
        num = torch.tensor(list(sizes), dtype=torch.int64, device=device)
        hit = _RANGES[key] = (num, torch.cumsum(num, 0) - num)
    return hit


def shared_cloud_ranges(n_views: int, points_per_cloud: int, device):
    """(first_idx, num_points) of one cloud of ``points_per_cloud`` points seen by ``n_views`` cameras (the packed
    layout of Pointclouds.extend), cached like `_cloud_ranges`."""
    num, first = _cloud_ranges((int(points_per_cloud),) * int(n_views), device)
    return first, num


def spatial_order(points: torch.Tensor, bits: int = 10) -> torch.Tensor:
    """Permutation that puts a cloud ``(P, 3)`` into Morton (Z-curve) order of its positions -> int64 ``(P,)``.

    The order of the points of a cloud is free (they are the model's parameters), but it matters to the kernels: waves of
    spatially neighbouring splats hit the same tile counters, list segments and image rows.  Measured at 8 cameras x 1M
    points @1024^2: a uniformly random order runs at 4.26 ms per iteration, the same cloud in this order at 3.43 ms
    (binning 1.01 -> 0.65 ms, backward gather 1.69 -> 1.42 ms).  Scanned or mesh-sampled clouds are usually coherent
    already; apply ``points[spatial_order(points)]`` (and the same permutation to normals / colours) once at load time
    to clouds that are not.  Plain torch ops on the tensor's device; nothing in the renderer depends on it."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("spatial_order expects (P, 3) positions")
    if points.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=points.device)
    p = points.detach().to(torch.float32)
    lo = p.min(0).values
    extent = (p.max(0).values - lo).max().clamp_min(1e-20)
    q = ((p - lo) / extent * float((1 << bits) - 1)).to(torch.int64).clamp_(0, (1 << bits) - 1)

    def spread(v):  # bit i of v -> bit 3 i
        out = torch.zeros_like(v)
        for i in range(bits):
            out |= ((v >> i) & 1) << (3 * i)
        return out
    code = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    return torch.argsort(code, stable=True)


class PointClouds3D:
    def __init__(self, points, normals=None, features=None):
        self._points = _to_list(points)
        self._normals = _to_list(normals)
        self._features = _to_list(features)
        self.device = self._points[0].device if self._points else torch.device("cpu")
        self._num, self._first = _cloud_ranges(tuple(p.shape[0] for p in self._points), self.device)
        self._packed_cache = {}

    def __len__(self):
        return len(self._points)

    def isempty(self) -> bool:
        return len(self._points) == 0 or int(sum(p.shape[0] for p in self._points)) == 0

    def num_points_per_cloud(self):
        return self._num

    def cloud_to_packed_first_idx(self):
        return self._first

    def packed_to_cloud_idx(self):
        return torch.repeat_interleave(torch.arange(len(self), device=self.device), self._num)

    def _packed(self, name):
        lst = getattr(self, "_" + name)
        if lst is None:
            return None
        if len(lst) == 1:
            return lst[0]
        cached = self._packed_cache.get(name)
        # a concatenation first built under torch.no_grad() (e.g. for the kNN statistic) is cut off from autograd:
        # rebuild it when a differentiable one is asked for
        needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in lst)
        if cached is None or (needs_grad and not cached.requires_grad):
            cached = torch.cat(lst, dim=0)
            self._packed_cache[name] = cached
        return cached

    def points_list(self):
        return self._points

    def normals_list(self):
        return self._normals

    def features_list(self):
        return self._features

    def points_packed(self):
        return self._packed("points")

    def normals_packed(self):
        return self._packed("normals")

    def features_packed(self):
        return self._packed("features")

    def _padded(self, lst):
        if lst is None:
            return None
        mx = int(max(t.shape[0] for t in lst))
        if all(t.shape[0] == mx for t in lst):
            return torch.stack(lst, 0)
        out = lst[0].new_zeros((len(lst), mx) + tuple(lst[0].shape[1:]))
        for i, t in enumerate(lst):
            out[i, : t.shape[0]] = t
        return out

    def points_padded(self):
        return self._padded(self._points)

    def normals_padded(self):
        return self._padded(self._normals)

    def features_padded(self):
        return self._padded(self._features)

    def estimate_normals(self, neighborhood_size: int = 16, disambiguate_directions: bool = True,
                         assign_to_self: bool = False, orientation: Optional[str] = None):
        """Normals of every cloud from the PCA of its ``neighborhood_size`` nearest points -> padded (N,P_max,3), the
        method of DSS/core/cloud.py:210-258.  ``disambiguate_directions=True`` is the reference's per-neighbourhood sign
        (``orientation="local"`` of `dss_amd.cloud_ops.estimate_normals`), ``False`` leaves the sign of the eigen-solver
        (``"none"``); ``orientation``, when given, overrides both: ``"consistent"`` is the one that makes the cloud
        renderable (``"viewpoint"`` needs the free function).  ``assign_to_self`` stores the result as the cloud's normals,
        replacing any it had."""
        from . import cloud_ops
        if orientation is None:
            orientation = "local" if disambiguate_directions else "none"
        normals = cloud_ops.estimate_normals(self, neighborhood_size=neighborhood_size, orientation=orientation,
                                             orientation_neighbours=min(8, int(neighborhood_size)))
        if assign_to_self:
            self._normals = [normals[n, :p.shape[0]] for n, p in enumerate(self._points)]
            self._packed_cache.pop("normals", None)
        return normals

    def extend(self, N: int) -> "PointClouds3D":
        """N copies of every cloud (shared autograd graph), like Pointclouds.extend."""
        rep = lambda lst: None if lst is None else [t for t in lst for _ in range(N)]
        return PointClouds3D(rep(self._points), rep(self._normals), rep(self._features))

    def to(self, device):
        mv = lambda lst: None if lst is None else [t.to(device) for t in lst]
        return PointClouds3D(mv(self._points), mv(self._normals), mv(self._features))

    def clone(self) -> "PointClouds3D":
        cp = lambda lst: None if lst is None else [t.clone() for t in lst]
        return PointClouds3D(cp(self._points), cp(self._normals), cp(self._features))

    def get_bounding_boxes(self) -> torch.Tensor:
        """(N, 3, 2) min / max of every cloud (pytorch3d Pointclouds.get_bounding_boxes; losses.py:252)."""
        lo = torch.stack([p.min(0).values for p in self._points])
        hi = torch.stack([p.max(0).values for p in self._points])
        return torch.stack([lo, hi], dim=-1)


class PointCloudsFilters:
    """Per-point boolean filters of a batch of clouds, mirroring `DSS.core.cloud.PointCloudsFilters`
    (DSS/core/cloud.py:284-351): padded 2-D masks ``inmask`` / ``activation`` / ``visibility`` of shape (N, P_max)
    (or (1, 1) = everything on), `set_filter(**masks)`, `filter(point_clouds)` and `filter_with(point_clouds, names)`.
    The rasterizer drops the points whose ``activation`` is off (rasterizer.py:230-234) and stores the per-point
    ``visibility`` of the last render here (rasterizer.py:639-652); the projection regulariser reads ``visibility`` and
    ``inmask`` (losses.py:198-212, 337-340)."""

    _NAMES = ("inmask", "activation", "visibility")

    def __init__(self, device="cpu", inmask=None, activation=None, visibility=None, **kwargs):
        self.device = torch.device(device)
        on = torch.ones(1, 1, dtype=torch.bool)
        for name, value in (("inmask", inmask), ("activation", activation), ("visibility", visibility)) + tuple(kwargs.items()):
            value = on if value is None else torch.as_tensor(value)
            setattr(self, name, value.to(self.device))

    def _tensors(self):
        return {k: v for k, v in vars(self).items() if torch.is_tensor(v)}

    _all_on_cache = {}

    @classmethod
    def all_on(cls, mask) -> bool:
        """True if every entry of ``mask`` is set.  One host synchronisation per (tensor, in-place version): the
        activation mask of a model changes only when points are pruned, but it is consulted several times per
        iteration, and an all-on mask lets every consumer skip its boolean indexing (each one a sync of its own)."""
        hit = cls._all_on_cache.get(id(mask))
        if hit is not None and hit[0] is mask and hit[1] == mask._version:
            return hit[2]
        value = bool(mask.all())
        if len(cls._all_on_cache) > 64:
            cls._all_on_cache.clear()
        cls._all_on_cache[id(mask)] = (mask, mask._version, value)   # keeps the tensor alive: ids are not recycled
        return value

    def set_filter(self, **kwargs):
        """Replace / add filters; each should be a 2-D (padded) mask.  The device follows the new tensors."""
        filters = self._tensors()
        filters.update(kwargs)
        for v in filters.values():
            if torch.is_tensor(v):
                self.device = v.device
        self.__init__(device=self.device, **filters)

    def filter(self, point_clouds):
        return self.filter_with(point_clouds, tuple(self._tensors()))

    def filter_with(self, point_clouds, filter_names):
        """The clouds reduced to the points for which ALL the named filters are on.  One cloud with N-row filters
        gives N clouds (the cloud is broadcast), like the reference's convert_to_tensors_and_broadcast."""
        masks = [getattr(self, k) for k in filter_names if torch.is_tensor(getattr(self, k, None))]
        points = point_clouds.points_list()
        if all(m.dim() == 2 for m in masks):
            p_max = max(p.shape[0] for p in points) if points else 0
            covers = lambda m: m.shape[1] == 1 or m.shape[1] >= p_max
            if len(points) >= max([1] + [m.shape[0] for m in masks]) and all(covers(m) and self.all_on(m) for m in masks):
                return point_clouds      # nothing to drop: no indexing, the tensors (and their identities) are kept
        normals, features = point_clouds.normals_list(), point_clouds.features_list()
        n_out = max([len(points)] + [m.shape[0] for m in masks])
        if any(m.dim() != 2 for m in masks) or any(m.shape[0] not in (1, n_out) for m in masks) or len(points) not in (1, n_out):
            raise ValueError("filters must be 2-D (N, P_max) masks broadcastable to the %d clouds" % n_out)
        pick = lambda lst, b: lst[b if len(lst) > 1 else 0]
        out_p, out_n, out_f = [], [], []
        keeps, done = {}, {}
        # Replicated clouds (Pointclouds.extend: the SAME position / normal tensors N times, per-camera colours) are
        # filtered once per distinct tensor and stay replicated, so the renderer still sees shared geometry.

        def reduced(t, rows, keep):
            k = (id(t), rows)
            if k not in done:
                done[k] = t[keep]
            return done[k]

        for b in range(n_out):
            pts = pick(points, b)
            rows = tuple(b if m.shape[0] > 1 else 0 for m in masks)
            if (rows, pts.shape[0]) not in keeps:
                keep = torch.ones(pts.shape[0], dtype=torch.bool, device=pts.device)
                for m in masks:
                    row = m[b if m.shape[0] > 1 else 0].to(pts.device)
                    if row.shape[0] == 1:
                        row = row.expand(pts.shape[0])
                    if row.shape[0] < pts.shape[0]:
                        raise ValueError("filter of %d entries for a cloud of %d points" % (row.shape[0], pts.shape[0]))
                    keep = keep & row[: pts.shape[0]].bool()   # entries at padded positions are ignored
                keeps[(rows, pts.shape[0])] = keep
            keep = keeps[(rows, pts.shape[0])]
            out_p.append(reduced(pts, rows, keep))
            if normals is not None:
                out_n.append(reduced(pick(normals, b), rows, keep))
            if features is not None:
                out_f.append(reduced(pick(features, b), rows, keep))
        return PointClouds3D(out_p, out_n if normals is not None else None, out_f if features is not None else None)
