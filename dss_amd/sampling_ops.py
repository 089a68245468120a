"""The operator that thins a cloud evenly: farthest point sampling of every cloud of a packed batch
(``dss_farthest_points``).  Re-exported by `dss_amd.ops` (``ops.farthest_points``); written like the operators
of `smoothing_ops.py` and entering the library the same way, through `_lib.call`: tensors checked by `_lib.require_gpu`, no
CPU fallback.  `dss_amd.cloud_ops.sample_farthest_points` and `subsample` are the public calls.
"""
import torch

from . import _lib

_f32, _i64 = torch.float32, torch.int64
_on_device = _lib.on_device

# Points per cloud that each register instantiation of the kernel holds, ascending (FPS_INSTANCES of csrc/sampling.hip):
# a cloud runs in the smallest that fits it, a cloud above the last one on the streaming path.
REGISTER_CAPACITIES = (64 * 4, 512 * 4, 1024 * 8, 1024 * 16, 1024 * 24)   # threads * points per thread
MAX_REGISTER_POINTS = REGISTER_CAPACITIES[-1]


def farthest_points(points, cloud_to_packed_first_idx, num_points_per_cloud, n_samples, start=None, K_max: int = 0,
                    return_sqdist: bool = False):
    """Farthest point sampling of every cloud (``dss_farthest_points``) -> idx (N, K_max) int64, cloud-local ids in
    selection order, -1 behind the ``min(n_samples[n], P_n)`` samples of cloud n; with ``return_sqdist`` also sel_sqdist
    (N, K_max) fp32, the squared distance of every sample to the samples before it when it was selected (+inf for the
    first, 0 in the padding).  points (P,3) packed, the ranges and ``n_samples`` (N,) int64, ``start`` (N,) int64 or None
    (every cloud starts at its id 0).  Ties go to the smallest id and a selected point is never selected again; rows that
    no cloud owns are not read."""
    points = _lib.require_gpu(points, "points", _f32)
    first = _lib.require_gpu(cloud_to_packed_first_idx, "cloud_to_packed_first_idx", _i64)
    num = _lib.require_gpu(num_points_per_cloud, "num_points_per_cloud", _i64)
    n_samples = _lib.require_gpu(n_samples, "n_samples", _i64)
    if start is not None:
        start = _lib.require_gpu(start, "start", _i64)
    P, N, K_max = points.shape[0], first.shape[0], int(K_max)
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("points must be (P,3), got %s" % (tuple(points.shape),))
    if num.shape != (N,) or n_samples.shape != (N,) or (start is not None and start.shape != (N,)):
        raise RuntimeError("cloud_to_packed_first_idx, num_points_per_cloud, n_samples and start must be (N,), N=%d" % N)
    if K_max < 0:
        raise RuntimeError("farthest_points: K_max must not be negative, got %d" % K_max)
    dev = points.device
    with _on_device(dev):
        if P == 0:   # the entry launches nothing for an empty packed array: the rows of -1 are made here
            idx = torch.full((N, K_max), -1, dtype=_i64, device=dev)
            sqd = torch.zeros((N, K_max), dtype=_f32, device=dev) if return_sqdist else None
        else:
            idx = torch.empty((N, K_max), dtype=_i64, device=dev)
            sqd = torch.empty((N, K_max), dtype=_f32, device=dev) if return_sqdist else None
            nbytes = _lib.load().dss_farthest_points_workspace(N, P)
            ws = _lib.workspace(dev, nbytes) if nbytes else None
            _lib.call("dss_farthest_points", dev, points, first, num, n_samples, start, N, P, K_max, idx, sqd, ws,
                      ws.numel() if ws is not None else 0)
    return (idx, sqd) if return_sqdist else idx
