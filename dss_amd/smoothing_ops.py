"""The two operators that clean a cloud (DSS/core/cloud.py:442-552): the bilateral filter of the normals
(``dss_denoise_normals``) and one outer iteration of the RIMLS projection (``dss_rimls_step``).  Re-exported by `dss_amd.ops`
(``ops.denoise_normals``, ``ops.rimls_step``); written like the operators of `upsample_ops.py` and entering the library the
same way, through `_lib.call`: tensors checked by `_lib.require_gpu`, no CPU fallback.  `dss_amd.cloud_ops.denoise_normals`
and `project_to_latent_surface` are the public calls.
"""
import torch

from . import _lib

_f32, _u8, _i64 = torch.float32, torch.uint8, torch.int64
_on_device = _lib.on_device


def _smoothing_inputs(points, normals, knn_dists, knn_idx, first, num, radius, K: int):
    """What the two entries share: points, normals (P,3), the lists (P, K + 1) of ``knn_points(K + 1)`` with their
    distances, the cloud ranges and the search radius of every cloud (N,)."""
    points = _lib.require_gpu(points, "points", _f32)
    normals = _lib.require_gpu(normals, "normals", _f32)
    knn_dists = _lib.require_gpu(knn_dists, "knn_dists", _f32)
    knn_idx = _lib.require_gpu(knn_idx, "knn_idx", _i64)
    first = _lib.require_gpu(first, "cloud_to_packed_first_idx", _i64)
    num = _lib.require_gpu(num, "num_points_per_cloud", _i64)
    radius = _lib.require_gpu(radius, "radius", _f32)
    P, N = points.shape[0], first.shape[0]
    lists = (P, int(K) + 1)
    if (points.dim() != 2 or points.shape[1] != 3 or normals.shape != points.shape or tuple(knn_idx.shape) != lists
            or tuple(knn_dists.shape) != lists):
        raise RuntimeError("points and normals must be (P,3), knn_dists and knn_idx (P, K + 1) = (%d, %d), the lists of "
                           "knn_points(K + 1)" % lists)
    if num.shape != (N,) or radius.shape != (N,):
        raise RuntimeError("cloud_to_packed_first_idx, num_points_per_cloud and radius must be (N,), N=%d" % N)
    return points, normals, knn_dists, knn_idx, first, num, radius, N, P, points.device


def denoise_normals(points, normals, knn_dists, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, radius, K: int,
                    sharpness_sigma: float = 30.0):
    """The bilateral filter of the normals (``dss_denoise_normals``, cloud.py:515-552) -> normals (P,3), unit length:
    normalize(sum of wn_j wp_j n_j over the live neighbours); a point without weight keeps its normalised input normal.
    ``knn_dists`` / ``knn_idx``: the lists of ``knn_points(K + 1)``, self first; ``radius`` (N,) per cloud."""
    points, normals, knn_dists, knn_idx, first, num, radius, N, P, dev = _smoothing_inputs(
        points, normals, knn_dists, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, radius, K)
    with _on_device(dev):
        out = torch.empty((P, 3), dtype=_f32, device=dev)
        _lib.call("dss_denoise_normals", dev, points, normals, knn_dists, knn_idx, first, num, radius, N, P, int(K),
                  float(sharpness_sigma), out)
    return out


def rimls_step(points, normals, knn_dists, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, radius, K: int,
               live=None, max_est_iter: int = 5):
    """One outer iteration of the RIMLS projection (``dss_rimls_step``, cloud.py:465-508) -> (points (P,3), live (P,)
    uint8), both new tensors.  ``points`` is the state of the step before; ``normals`` and the lists are those of the
    INPUT cloud in every step; ``live`` (P,) uint8 from the step before, None for the first step."""
    points, normals, knn_dists, knn_idx, first, num, radius, N, P, dev = _smoothing_inputs(
        points, normals, knn_dists, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, radius, K)
    if live is not None:
        live = _lib.require_gpu(live, "live", _u8)
        if live.shape != (P,):
            raise RuntimeError("rimls_step: live must be (P,) uint8, P=%d" % P)
    with _on_device(dev):
        out = torch.empty((P, 3), dtype=_f32, device=dev)
        live_out = torch.empty((P,), dtype=_u8, device=dev)
        _lib.call("dss_rimls_step", dev, points, normals, knn_dists, knn_idx, first, num, radius, live, N, P, int(K),
                  int(max_est_iter), out, live_out)
    return out, live_out
