"""Operators between TWO sets of packed clouds: the nearest point of cloud n of ``y`` for every point of cloud n of ``x``
(``dss_nearest_points``) and the gradient of the chamfer point term built on it (``dss_chamfer_backward``) -- the 3-D metric of
the reference's loop, ``pytorch3d.loss.chamfer_distance`` in `Trainer.evaluate_3d` (trainer.py:144-171).  Re-exported by
`dss_amd.ops` (``ops.nearest_points``, ``ops.chamfer_backward``); written like the operators there and entering the library
the same way, through `_lib.call`: tensors checked by `_lib.require_gpu`, no CPU fallback.
"""
import torch

from . import _lib

_f32, _i64, _u8 = torch.float32, torch.int64, torch.uint8
_on_device = _lib.on_device


def _gpu(dtype, **tensors):
    return [_lib.require_gpu(t, name, dtype) for name, t in tensors.items()]


def _cross_inputs(x, x_first, x_num, y, y_first, y_num):
    """What the two cross-cloud entries share: the six checked tensors, N, Px, Py and the device."""
    x, y = _gpu(_f32, x=x, y=y)
    xf, xn, yf, yn = _gpu(_i64, x_first=x_first, x_num=x_num, y_first=y_first, y_num=y_num)
    N, Ny = xf.shape[0], yf.shape[0]
    if Ny != N or x.dim() != 2 or y.dim() != 2 or x.shape[1] != 3 or y.shape[1] != 3 or y.device != x.device:
        raise RuntimeError("x (Px,3) and y (Py,3) packed clouds on one device, with as many clouds in y (%d) as in x (%d)" % (Ny, N))
    return x, xf, xn, y, yf, yn, N, x.shape[0], y.shape[0], x.device


def nearest_points(x, x_first, x_num, y, y_first, y_num):
    """Nearest point of cloud n of ``y`` for every point of cloud n of ``x`` (packed clouds) -> (d2 (Px,) squared distance,
    idx (Px,) int64 cloud-local id in y; ties to the smaller id): the K = 1 cross query
    ``pytorch3d.ops.knn_points(x, y, lengths1, lengths2, K=1)`` behind ``chamfer_distance`` (trainer.py:144-171), exact grid
    search in HIP (``dss_nearest_points``).  A query whose target cloud is empty, and a packed slot of no cloud, get (0, -1)."""
    x, xf, xn, y, yf, yn, N, Px, Py, dev = _cross_inputs(x, x_first, x_num, y, y_first, y_num)
    with _on_device(dev):
        d2 = torch.empty((Px,), dtype=_f32, device=dev)
        idx = torch.empty((Px,), dtype=_i64, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_nearest_workspace(N, Py))
        _lib.call("dss_nearest_points", dev, x, xf, xn, Px, y, yf, yn, Py, N, d2, idx, ws, ws.numel())
    return d2, idx


def packed_cloud_ids(first, num, P: int):
    """Cloud of every packed slot -> (P,) int64, -1 for a slot of no cloud (plain torch, no synchronisation)."""
    slot = torch.arange(P, dtype=_i64, device=first.device)[:, None]
    owns = (slot >= first[None]) & (slot < (first + num)[None])
    return torch.where(owns.any(1), owns.to(_u8).argmax(1), torch.full((), -1, dtype=_i64, device=first.device))


def chamfer_order(idx, own_first, own_num, target_first):
    """The contributor list of ``dss_chamfer_backward``: the packed ids of one side sorted by (packed id of their nearest
    point on the other side, own id) -- a stable `torch.sort` of int64 keys; pairs without a neighbour (idx < 0) and slots of
    no cloud go last."""
    cloud = packed_cloud_ids(own_first, own_num, idx.shape[0])
    key = torch.where((cloud >= 0) & (idx >= 0), target_first[cloud.clamp(min=0)] + idx,
                      torch.full((), torch.iinfo(_i64).max, dtype=_i64, device=idx.device))
    return torch.sort(key, stable=True).indices


def chamfer_backward(x, x_first, x_num, y, y_first, y_num, idx_xy, idx_yx, gx, gy, want_x: bool = True, want_y: bool = True):
    """Gradient of the chamfer point term (``dss_chamfer_backward``) with the index lists of `nearest_points` (x in y:
    ``idx_xy``, y in x: ``idx_yx``) held constant, ``gx`` (Px,) / ``gy`` (Py,) = d loss / d squared distance of the two
    searches -> (grad_x (Px,3) or None, grad_y (Py,3) or None), fully written, bitwise reproducible (no atomics: see
    `chamfer_order`)."""
    x, xf, xn, y, yf, yn, N, Px, Py, dev = _cross_inputs(x, x_first, x_num, y, y_first, y_num)
    idx_xy, idx_yx = _gpu(_i64, idx_xy=idx_xy, idx_yx=idx_yx)
    gx, gy = _gpu(_f32, gx=gx, gy=gy)
    if idx_xy.shape != (Px,) or idx_yx.shape != (Py,) or gx.shape != (Px,) or gy.shape != (Py,):
        raise RuntimeError("chamfer_backward: idx_xy, gx (Px,) and idx_yx, gy (Py,) with Px=%d Py=%d" % (Px, Py))
    with _on_device(dev):
        order_yx = chamfer_order(idx_yx, yf, yn, xf) if want_x else None    # who contributes to which x point
        order_xy = chamfer_order(idx_xy, xf, xn, yf) if want_y else None
        grad_x = torch.empty((Px, 3), dtype=_f32, device=dev) if want_x else None
        grad_y = torch.empty((Py, 3), dtype=_f32, device=dev) if want_y else None
        _lib.call("dss_chamfer_backward", dev, x, y, xf, xn, Px, yf, yn, Py, N, idx_xy, idx_yx, order_xy, order_yx, gx, gy,
                  grad_x, grad_y)
    return grad_x, grad_y
