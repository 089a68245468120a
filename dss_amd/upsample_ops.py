"""The two operators of one sparsity-upsampling round (DSS/core/cloud.py:555-632): the K x K sparsity search
(``dss_upsample_candidates``) and the assembly of the grown cloud (``dss_upsample_insert``).  Re-exported by `dss_amd.ops`
(``ops.upsample_candidates``, ``ops.upsample_insert``); written like the operators there and entering the library the same
way, through `_lib.call`: tensors checked by `_lib.require_gpu`, no CPU fallback.  `dss_amd.cloud_ops.upsample` runs the
rounds.
"""
import torch

from . import _lib

_f32, _i32, _i64 = torch.float32, torch.int32, torch.int64
_on_device = _lib.on_device


def _gpu(dtype, **tensors):
    return [_lib.require_gpu(t, name, dtype) for name, t in tensors.items()]


def _upsample_inputs(points, knn_idx, K: int):
    """What the two upsampling entries share: points (P,3), the neighbour lists (P, K + 1) of ``knn_points(K + 1)``."""
    points = _lib.require_gpu(points, "points", _f32)
    knn_idx = _lib.require_gpu(knn_idx, "knn_idx", _i64)
    P = points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or tuple(knn_idx.shape) != (P, int(K) + 1):
        raise RuntimeError("points must be (P,3) and knn_idx (P, K + 1) = (%d, %d), the lists of knn_points(K + 1)" % (P, int(K) + 1))
    return points, knn_idx, P, points.device


def upsample_candidates(points, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, K: int):
    """The sparsity search of one upsampling round (``dss_upsample_candidates``, cloud.py:599-605) -> (sparsity_sq (P,) =
    max_j min_l |mid_j - q_l|^2, father (P,) int32 = the smallest j that attains it, key (P,) int64 holding the uint64
    ``float bits of sparsity_sq << 32 | 0xffffffff - cloud-local id``, non-negative): an ascending sort of a cloud's keys is
    the round's emission order.  ``knn_idx``: the lists of ``knn_points(K + 1)``, self first."""
    points, knn_idx, P, dev = _upsample_inputs(points, knn_idx, K)
    first, num = _gpu(_i64, cloud_to_packed_first_idx=cloud_to_packed_first_idx, num_points_per_cloud=num_points_per_cloud)
    N = first.shape[0]
    with _on_device(dev):
        sparsity_sq = torch.empty((P,), dtype=_f32, device=dev)
        father = torch.empty((P,), dtype=_i32, device=dev)
        key = torch.empty((P,), dtype=_i64, device=dev)
        _lib.call("dss_upsample_candidates", dev, points, knn_idx, first, num, N, P, int(K), sparsity_sq, father, key)
    return sparsity_sq, father, key


def upsample_insert(points, attrs, knn_idx, father, sel, old_first, old_num, new_first, new_num, n_new, K: int):
    """The grown cloud of one upsampling round (``dss_upsample_insert``, cloud.py:611-625) -> (out_points (P + n_sel, 3),
    out_attrs (P + n_sel, C) or None): per cloud the ``n_new[n]`` candidates of the points ``sel`` (packed ids, in emission
    order) first, then the old rows.  ``attrs`` (P,C), C <= 16, or None: old rows copied, new rows (a_q + 2 a_p) / 3."""
    points, knn_idx, P, dev = _upsample_inputs(points, knn_idx, K)
    father = _lib.require_gpu(father, "father", _i32)
    sel, old_first, old_num, new_first, new_num, n_new = _gpu(_i64, sel=sel, old_first=old_first, old_num=old_num,
                                                              new_first=new_first, new_num=new_num, n_new=n_new)
    N, n_sel = old_first.shape[0], sel.shape[0]
    if father.shape != (P,) or any(t.shape != (N,) for t in (old_num, new_first, new_num, n_new)):
        raise RuntimeError("upsample_insert: father (P,) and five (N,) range tensors, P=%d N=%d" % (P, N))
    C = 0
    if attrs is not None:
        attrs = _lib.require_gpu(attrs, "attrs", _f32)
        if attrs.dim() != 2 or attrs.shape[0] != P:
            raise RuntimeError("upsample_insert: attrs must be (P,C) with P=%d" % P)
        C = attrs.shape[1]
    with _on_device(dev):
        out_points = torch.empty((P + n_sel, 3), dtype=_f32, device=dev)
        out_attrs = torch.empty((P + n_sel, C), dtype=_f32, device=dev) if attrs is not None else None
        _lib.call("dss_upsample_insert", dev, points, attrs, C, knn_idx, father, sel, old_first, old_num, new_first, new_num,
                  n_new, N, int(K), P, P + n_sel, n_sel, out_points, out_attrs)
    return out_points, out_attrs
