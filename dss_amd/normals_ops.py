"""The operators that give estimated normals a sign: the per-neighbourhood and the viewpoint rule
(``dss_disambiguate_normals``) and the propagation of one sign over a whole cloud (``dss_orient_normals``).
Re-exported by `dss_amd.ops` (``ops.disambiguate_normals``, ``ops.orient_normals``); written like the operators of
`sampling_ops.py` and entering the library the same way, through `_lib.call`: tensors checked by `_lib.require_gpu`, no CPU
fallback.  `dss_amd.cloud_ops.estimate_normals` and `orient_normals` are the public calls.
"""
import torch

from . import _lib

_f32, _i32, _i64 = torch.float32, torch.int32, torch.int64
_on_device = _lib.on_device

# Points per cloud whose stamps the propagation kernel keeps in LDS (NORMALS_LDS_POINTS of csrc/normals.hip: 160,000 of a
# compute unit's 163,840 bytes); a larger cloud keeps them in the workspace, slower and correct for any size.
LDS_CAPACITY = 40000
# Entries of a neighbour list, the point itself included, up to which the kernel reads an int32 copy of the lists that it
# makes in the workspace (NORMALS_FAST_LIST); ``min(KP, K)`` above it reads the caller's lists directly, which is slower.
FAST_LIST = 8
THRESHOLDS = (0.95, 0.8, 0.5, 0.0)   # tau of the propagation, by level


def _inputs(who, points, normals, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, need_lists=True):
    points = _lib.require_gpu(points, "points", _f32)
    normals = _lib.require_gpu(normals, "normals", _f32)
    first = _lib.require_gpu(cloud_to_packed_first_idx, "cloud_to_packed_first_idx", _i64)
    num = _lib.require_gpu(num_points_per_cloud, "num_points_per_cloud", _i64)
    if knn_idx is not None or need_lists:
        knn_idx = _lib.require_gpu(knn_idx, "knn_idx", _i64)
    P, N = points.shape[0], first.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or tuple(normals.shape) != (P, 3):
        raise RuntimeError("%s: points and normals must be (P,3), got %s and %s"
                           % (who, tuple(points.shape), tuple(normals.shape)))
    if knn_idx is not None and (knn_idx.dim() != 2 or knn_idx.shape[0] != P or knn_idx.shape[1] < 1):
        raise RuntimeError("%s: knn_idx must be (P,K) for the P = %d packed points, K >= 1, got %s"
                           % (who, P, tuple(knn_idx.shape)))
    if N < 1 or num.shape != (N,):
        raise RuntimeError("%s: cloud_to_packed_first_idx and num_points_per_cloud must be (N,), N >= 1" % who)
    return points, normals, knn_idx, first, num, N, P


def disambiguate_normals(points, normals, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, viewpoint=None):
    """The sign of every normal by a rule of its own point (``dss_disambiguate_normals``) -> normals (P,3), a new tensor.
    ``viewpoint=None``: the local rule -- flip iff fewer than half of the first min(K, P_n) entries of the point's list
    ``knn_idx`` (P,K) (``knn_points``, self first) lie on the positive side, ``(n.x dx + n.y dy) + n.z dz > 0`` in fp32.
    ``viewpoint`` (N,3): flip iff the normal points away from its cloud's viewpoint; ``knn_idx`` may then be None.
    A flip negates the three floats.  Rows that no cloud owns come back as (0,0,1) and are not read."""
    who = "disambiguate_normals"
    points, normals, knn_idx, first, num, N, P = _inputs(who, points, normals, knn_idx, cloud_to_packed_first_idx,
                                                         num_points_per_cloud, need_lists=viewpoint is None)
    if viewpoint is not None:
        viewpoint = _lib.require_gpu(viewpoint, "viewpoint", _f32)
        if tuple(viewpoint.shape) != (N, 3):
            raise RuntimeError("%s: viewpoint must be (N,3) = (%d,3), got %s" % (who, N, tuple(viewpoint.shape)))
    dev = points.device
    with _on_device(dev):
        out = torch.empty((P, 3), dtype=_f32, device=dev)
        if P:   # the entry launches nothing for an empty packed array
            _lib.call("dss_disambiguate_normals", dev, points, normals, knn_idx, first, num, N, P,
                      int(knn_idx.shape[1]) if knn_idx is not None else 1, 0 if viewpoint is None else 1, viewpoint, out)
    return out


def orient_normals(normals, points, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, KP: int = 8,
                   return_stamps: bool = False, return_parents: bool = False):
    """One sign for every connected part of every cloud (``dss_orient_normals``) -> normals (P,3), a new tensor; with
    ``return_stamps`` also stamp (P,) int32, the iteration in which a point was oriented (>= 1), with ``return_parents``
    also parent (P,) int64, the cloud-local id of the neighbour whose sign it took, -1 for a seed.

    The sign spreads from seeds (the highest unoriented point, turned upwards) over the entries 1 .. min(KP, K, P_n) - 1 of
    the lists ``knn_idx`` (P,K) (``knn_points``, self first), in rounds: every unoriented point that has a neighbour
    oriented in an earlier round with ``|n_i . o_j|`` of at least 0.95 takes the sign of its most parallel such neighbour
    (ties to the smallest id); when a round finds nobody the threshold falls to 0.8, 0.5, 0.0, and then a new seed is
    taken.  DESIGN 4.17 states the contract.  Every cloud is oriented as if it were alone by one persistent workgroup;
    rows that no cloud owns come back as (0,0,1), stamp 0, parent -1 and are not read."""
    who = "orient_normals"
    points, normals, knn_idx, first, num, N, P = _inputs(who, points, normals, knn_idx, cloud_to_packed_first_idx,
                                                         num_points_per_cloud)
    KP = int(KP)
    if KP < 1:
        raise RuntimeError("%s: KP must be at least 1, got %d" % (who, KP))
    dev = points.device
    with _on_device(dev):
        out = torch.empty((P, 3), dtype=_f32, device=dev)
        stamp = torch.empty((P,), dtype=_i32, device=dev) if return_stamps else None
        parent = torch.empty((P,), dtype=_i64, device=dev) if return_parents else None
        if P:
            ws = _lib.workspace(dev, _lib.load().dss_orient_normals_workspace(N, P))
            _lib.call("dss_orient_normals", dev, normals, points, knn_idx, first, num, N, P, int(knn_idx.shape[1]), KP, out,
                      stamp, parent, ws, ws.numel())
    res = (out,) + ((stamp,) if return_stamps else ()) + ((parent,) if return_parents else ())
    return res if len(res) > 1 else out
