"""Tensor-level operators over the C ABI: ALL seven functions the reference binds in ``DSS._C``
(DSS/csrc/ext.cpp:5-18: ``splat_points``, ``_splat_points_naive``, ``_splat_points_occ_backward``,
``_rasterize_coarse``, ``_rasterize_fine``, ``_splat_points_occ_fast_cuda_backward``, ``_backward_zbuf``), same names and
argument meaning, plus the fused entry points.

All inputs must be GPU tensors; outputs are freshly allocated on the input's device
(rasterize_points.cu:632-637) except ``_backward_zbuf`` which accumulates in place
(rasterize_points.h:388-392).

Every operator reads top to bottom as check, allocate, call: the input helpers below state each repeated contract once,
and ``_lib.call`` is the one place where tensors become pointers, the stream is appended and the status is checked --
so the argument list at each call site is exactly the C prototype's, minus the stream.
"""
from typing import Optional, Tuple

import weakref

import torch

from . import _lib

_f32, _i32, _i64, _u8, _f64 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64
_on_device = _lib.on_device


def _gpu(dtype, **tensors):
    """`_lib.require_gpu` of several tensors of one dtype, in the order given; the keyword is the name in the message."""
    return [_lib.require_gpu(t, name, dtype) for name, t in tensors.items()]


def _ranges(cloud_to_packed_first_idx, num_points_per_cloud):
    """The packed cloud ranges that almost every operator takes -> (first, num, N)."""
    first = _lib.require_gpu(cloud_to_packed_first_idx, "cloud_to_packed_first_idx", _i64)
    num = _lib.require_gpu(num_points_per_cloud, "num_points_per_cloud", _i64)
    return first, num, first.shape[0]


def _as_u8(mask):
    """bool -> uint8 without a copy kernel (same storage, values 0/1)."""
    return mask.view(_u8) if mask.dtype == torch.bool else mask


def _flags(mask, name):
    """Per-point flags for the kernels: bool or uint8 (any other dtype is refused, unlike `_mask_u8`)."""
    return _lib.require_gpu(_as_u8(mask), name, _u8)


def _h_mode(h, N: int, Pw: int, P: int, shared) -> int:
    """What the entries of `h` stand for: 0 = one per cloud, 1 = one per world point, 2 = one per PACKED point (a shared
    cloud whose cameras cull differently: one value per (camera, point) pair).  As many clouds as points reads per cloud."""
    n = h.numel()
    if n == Pw and not (n == N and Pw == N):
        return 1
    if shared and N > 1 and n == P:
        return 2
    if n != N:
        raise RuntimeError("h must have %d (per point), %d (per cloud) or, for a shared cloud, %d (per packed point) entries" % (Pw, N, P))
    return 0


def _check_cameras(M, V, znear, zfar, N):
    if tuple(M.shape) != (N, 4, 4) or tuple(V.shape) != (N, 4, 4) or znear.numel() != N or zfar.numel() != N:
        raise RuntimeError("camera tensors must be M,V (N,4,4) and znear,zfar (N,) with N=%d" % N)


def _dense(t, shape, dtype=_f32) -> bool:
    """whether a caller-owned output buffer is a contiguous `dtype` tensor of `shape` (an int: of that many elements)"""
    return t.dtype == dtype and t.is_contiguous() and (t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == shape)


def _check_raster_inputs(points, ellipse_params, cutoff_thres, radii, first_idx, num_pts):
    # shape checks of RasterizePoints, rasterize_points.h:474-488
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("points must have shape (P, 3), got %s" % (tuple(points.shape),))
    P = points.shape[0]
    if tuple(radii.shape) != (P, 2):
        raise RuntimeError("radii must have shape (%d, 2), got %s" % (P, tuple(radii.shape)))
    if tuple(ellipse_params.shape) != (P, 3):
        raise RuntimeError("ellipse_params must have shape (%d, 3), got %s" % (P, tuple(ellipse_params.shape)))
    if tuple(cutoff_thres.shape) != (P,):
        raise RuntimeError("cutoff_thres must have shape (%d,), got %s" % (P, tuple(cutoff_thres.shape)))
    if first_idx.shape != num_pts.shape or first_idx.dim() != 1:
        raise RuntimeError("cloud_to_packed_first_idx and num_points_per_cloud must both be (N,)")
    return P


def _fragments(dev, N, rows, S, K):
    """the four fragment outputs of a splat: idx, zbuf, qvalue (N,rows,S,K) and occupancy (N,rows,S)"""
    return (torch.empty((N, rows, S, K), dtype=_i32, device=dev), torch.empty((N, rows, S, K), dtype=_f32, device=dev),
            torch.empty((N, rows, S, K), dtype=_f32, device=dev), torch.empty((N, rows, S), dtype=_f32, device=dev))


def splat_points(points, ellipse_params, cutoff_thres, radii, cloud_to_packed_first_idx,
                 num_points_per_cloud, depth_merging_thres: float, image_size: int,
                 points_per_pixel: int, bin_size: Optional[int] = None,
                 max_points_per_bin: Optional[int] = None, *, rows: Optional[Tuple[int, int]] = None,
                 return_visible: bool = False):
    """``DSS._C.splat_points`` (ext.cpp:8, rasterize_points.h:461-525).

    Returns ``(idx int32 (N,S,S,K), zbuf, qvalue f32 (N,S,S,K), occupancy f32 (N,S,S))``.
    ``bin_size == 0`` scans every cloud per tile (the reference's naive mode); any other value
    (or None) builds compacted screen-tile lists.  ``max_points_per_bin`` is accepted for
    signature compatibility and ignored: tile lists are compacted, never truncated.
    ``rows=(row0,row1)`` renders only that row band (outputs are band shaped);
    ``return_visible`` appends the per-point visibility mask (bool (P,)).
    """
    P = _check_raster_inputs(points, ellipse_params, cutoff_thres, radii, cloud_to_packed_first_idx,
                             num_points_per_cloud)
    points, ellipse_params, cutoff_thres, radii = _gpu(_f32, points=points, ellipse_params=ellipse_params,
                                                       cutoff_thres=cutoff_thres, radii=radii)
    dev = points.device
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    S, K = int(image_size), int(points_per_pixel)
    row0, row1, _ = _band(rows, S)
    nrows = max(row1 - row0, 0)
    bs = 1 if bin_size is None else int(bin_size)
    with _on_device(dev):
        idx, zbuf, qv, occ = _fragments(dev, N, nrows, S, K)
        vis = torch.empty((P,), dtype=_u8, device=dev) if return_visible else None
        if nrows == 0:  # a rank whose row band is empty (RowPartition with S < world_size * band): nothing to launch
            if vis is not None:
                vis.zero_()
        else:
            ws = _lib.workspace(dev, _lib.load().dss_splat_forward_workspace(N, P, S, K, bs))
            _lib.call("dss_splat_forward", dev, points, ellipse_params, cutoff_thres, radii, first, num, N, P,
                      float(depth_merging_thres), S, K, bs, row0, row1, idx, zbuf, qv, occ, vis, ws, ws.numel())
    if return_visible:
        return idx, zbuf, qv, occ, vis.view(torch.bool)  # zero-copy reinterpretation (values are 0/1)
    return idx, zbuf, qv, occ


def _splat_points_naive(points, ellipse_params, cutoff_thres, radii, cloud_to_packed_first_idx,
                        num_points_per_cloud, depth_merging_thres, image_size, points_per_pixel):
    """``DSS._C._splat_points_naive`` (ext.cpp:9)."""
    return splat_points(points, ellipse_params, cutoff_thres, radii, cloud_to_packed_first_idx,
                        num_points_per_cloud, depth_merging_thres, image_size, points_per_pixel, 0, 0)


# What the fine pass needs besides the tile lists of `_rasterize_coarse`, and what the lists were built from.  Kept in a
# registry keyed by the buffer's address (not as a Python attribute of the tensor, which views, autograd saves and
# `detach()` drop): any tensor that still refers to this storage finds it; a copy (clone / to) does not and is refused with
# a clear message.  Keyed by the STORAGE address, so that a view with a storage offset still finds its entry.
_bin_registry = {}


def _bin_source(points, radii):
    """identity of the caller's tensors as handed over: address, layout and version counter (a non-contiguous input is
    normalised into a temporary inside the call; comparing the temporary's address would reject the same tensor next time,
    or accept another one that recycled the address)"""
    return tuple((t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version) for t in (points, radii))


def _rasterize_coarse(points, radii, cloud_to_packed_first_idx, num_points_per_cloud, image_size: int, bin_size: int,
                      max_points_per_bin: int):
    """``DSS._C._rasterize_coarse`` (ext.cpp:11, rasterize_points.h:167-203): the binning pass alone.  The reference
    returns a dense ``(N, B, B, M)`` int32 table; here ``bin_points`` is an OPAQUE uint8 tensor (the tile-list workspace
    of ``dss_splat_bin``: per-tile sub-list counters + fixed-capacity id lists over 8x8-pixel tiles) that is only meant
    to be handed to :func:`_rasterize_fine`.  ``bin_size`` / ``max_points_per_bin`` are accepted and ignored (tile size
    and list capacity are chosen by the library; lists never truncate)."""
    src = _bin_source(points, radii)   # what the CALLER handed over (before any normalisation copy)
    points, radii = _gpu(_f32, points=points, radii=radii)
    dev = points.device
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    if points.dim() != 2 or points.shape[1] != 3 or tuple(radii.shape) != (points.shape[0], 2):
        raise RuntimeError("points must be (P,3) and radii (P,2)")
    P, S = points.shape[0], int(image_size)
    with _on_device(dev):
        nbytes = _lib.load().dss_splat_forward_workspace(N, P, S, 1, 1)
        bin_points = torch.empty(nbytes, dtype=_u8, device=dev)
        if P > 0:
            _lib.call("dss_splat_bin", dev, points, radii, first, num, N, P, S, 0, S, bin_points, nbytes)
    _bin_registry[bin_points.untyped_storage().data_ptr()] = (weakref.ref(bin_points), first, num, N, P, S, src)
    if len(_bin_registry) > 64:
        for k in [k for k, v in _bin_registry.items() if v[0]() is None]:
            del _bin_registry[k]
    return bin_points


def _rasterize_fine(points, ellipse_params, cutoff_thres, radii, bin_points, depth_merging_thres: float, image_size: int,
                    bin_size: int, points_per_pixel: int):
    """``DSS._C._rasterize_fine`` (ext.cpp:12, rasterize_points.h:257-285) on the ``bin_points`` of
    :func:`_rasterize_coarse` -> ``(idx, zbuf, qvalue, occupancy)`` like ``splat_points``."""
    meta = _bin_registry.get(bin_points.untyped_storage().data_ptr()) \
        if isinstance(bin_points, torch.Tensor) and bin_points.is_cuda else None
    if meta is None or meta[0]() is None:
        raise RuntimeError("bin_points must be the tensor dss_amd.ops._rasterize_coarse returned, or a view of it (opaque "
                           "tile lists, not the reference's dense (N,B,B,M) table; a clone / device copy is not accepted)")
    whole, first, num, N, P, S, src = meta
    whole = whole()   # the tensor _rasterize_coarse returned (bin_points may be a view of it)
    if int(image_size) != S or points.shape[0] != P:
        raise RuntimeError("bin_points were built for image_size=%d and %d points" % (S, P))
    if src != _bin_source(points, radii):
        raise RuntimeError("bin_points were built from other points / radii tensors (or these were modified since)")
    _check_raster_inputs(points, ellipse_params, cutoff_thres, radii, first, num)
    points, ellipse_params, cutoff_thres, radii = _gpu(_f32, points=points, ellipse_params=ellipse_params,
                                                       cutoff_thres=cutoff_thres, radii=radii)
    dev, K = points.device, int(points_per_pixel)
    with _on_device(dev):
        idx, zbuf, qv, occ = _fragments(dev, N, S, S, K)
        _lib.call("dss_splat_fine", dev, points, ellipse_params, cutoff_thres, radii, first, num, N, P,
                  float(depth_merging_thres), S, K, 0, S, idx, zbuf, qv, occ, None, whole if P > 0 else None, whole.numel())
    return idx, zbuf, qv, occ


def _splat_points_occ_backward(points, radii, grad_occ, cloud_to_packed_first_idx, num_points_per_cloud, radii_s: float,
                               depth_merging_thres: float = 0.0):
    """``DSS._C._splat_points_occ_backward`` on GPU tensors (ext.cpp:10, 16; rasterize_points.cu:672-822): the
    box-supported occupancy surrogate over ALL points handed in -> (P,2).  Not on the training path
    (``backward_occ_fast = True``, rasterizer.py:816).  ``depth_merging_thres`` is unused, as in the reference."""
    points, radii, grad_occ = _gpu(_f32, points=points, radii=radii, grad_occ=grad_occ)
    dev = points.device
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    if points.dim() != 2 or points.shape[1] != 3 or tuple(radii.shape) != (points.shape[0], 2) or first.shape != num.shape:
        raise RuntimeError("points must be (P,3), radii (P,2), first_idx / num_points (N,)")  # rasterize_points.h:357-361
    P = points.shape[0]
    if grad_occ.dim() != 3 or grad_occ.shape[0] != N or grad_occ.shape[1] != grad_occ.shape[2]:
        raise RuntimeError("grad_occ must be (N,S,S) with N=%d, got %s" % (N, tuple(grad_occ.shape)))
    with _on_device(dev):
        grad = torch.empty((P, 2), dtype=_f32, device=dev)
        _lib.call("dss_occ_backward_box", dev, points, radii, grad_occ, first, num, N, P, grad_occ.shape[1],
                  float(radii_s), grad)
    return grad


def _splat_points_occ_fast_cuda_backward(points_sorted, radii_sorted, rs, grad_occ, num_points_per_cloud,
                                         cloud_to_packed_first_idx, points_grid_off=None, grid_params=None):
    """``DSS._C._splat_points_occ_fast_cuda_backward`` (ext.cpp:14, rasterize_points_backward.cu:227-322) -> (P,2) in the
    order of ``points_sorted``.  Every point handed in takes part (the reference passes the visible points only,
    rasterizer.py:863-864, 951-952).  ``points_grid_off`` / ``grid_params`` -- the FRNN grid that only accelerates the
    reference's pixel-centric search -- are accepted and ignored: the gather kernel needs no grid, so the points need
    not be sorted either (and the last-cell bug of :124-126 cannot occur)."""
    all_points = torch.ones(points_sorted.shape[0], dtype=_u8, device=points_sorted.device)
    return occ_backward(points_sorted, radii_sorted, all_points, rs, grad_occ, cloud_to_packed_first_idx,
                        num_points_per_cloud)[:, :2].contiguous()


def backward_radius(radii, visible, cloud_to_packed_first_idx, num_points_per_cloud, radii_s: float):
    """Search radius of the backward pass, rasterizer.py:885-888 -> f32 (N,)."""
    radii = _lib.require_gpu(radii, "radii", _f32)
    dev = radii.device
    vis = _flags(visible, "visible")
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    P = radii.shape[0]
    with _on_device(dev):
        rs = torch.empty((N,), dtype=_f32, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_backward_radius_workspace(N, P))
        _lib.call("dss_backward_radius", dev, radii, vis, first, num, N, P, float(radii_s), rs, ws, ws.numel())
    return rs


def _pixel_strided(t, N, rows, S):
    """(tensor, pixel stride) for an (N,rows,S) float32 GPU view that is dense up to a constant element
    stride per pixel (e.g. ``grad_image[..., 3]``); anything else is made contiguous."""
    if t.is_cuda and t.dtype == _f32 and tuple(t.shape) == (N, rows, S) and t.numel() > 0:
        c = t.stride(2)
        if c >= 1 and t.stride(1) == S * c and t.stride(0) == rows * S * c:
            return t, c
    return _lib.require_gpu(t, "grad_occ", _f32), 1


def occ_backward(points, radii, visible, rs, grad_occ, cloud_to_packed_first_idx, num_points_per_cloud,
                 image_size: Optional[int] = None, rows: Optional[Tuple[int, int]] = None, clip: float = -1.0):
    """Occupancy surrogate gradient -> (P,3) with z column 0.  Replaces the FRNN grid build
    (rasterizer.py:889-950) + ``DSS._C._splat_points_occ_fast_cuda_backward`` (ext.cpp:14).
    ``grad_occ`` may be a strided channel view of an image gradient (read in place).  ``clip > 0`` fuses
    the per-point clip hook (valid only when no zbuf gradient / cross-rank reduction follows)."""
    points, radii = _gpu(_f32, points=points, radii=radii)
    dev = points.device
    vis = _flags(visible, "visible")
    rs = _lib.require_gpu(rs, "rs", _f32)
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    P = points.shape[0]
    S = int(image_size) if image_size is not None else grad_occ.shape[2]
    row0, row1, _ = _band(rows, S)
    if tuple(grad_occ.shape) != (N, row1 - row0, S):
        raise RuntimeError("grad_occ must have shape (%d, %d, %d), got %s" % (N, row1 - row0, S, tuple(grad_occ.shape)))
    if row1 <= row0:  # empty band: no pixel contributes
        return torch.zeros((P, 3), dtype=_f32, device=dev)
    grad_occ, gstride = _pixel_strided(grad_occ, N, row1 - row0, S)
    with _on_device(dev):
        grad = torch.empty((P, 3), dtype=_f32, device=dev)
        _lib.call("dss_occ_backward", dev, points, radii, vis, rs, grad_occ, first, num, N, P, S, row0, row1, gstride,
                  float(clip), grad)
    return grad


def _backward_zbuf(idx, grad_zbuf, point_grad):
    """``DSS._C._backward_zbuf`` (ext.cpp:17): in-place scatter-add.  ``point_grad`` is either the
    reference's (P,1) z-gradient tensor or a (P,3) point-gradient tensor (z column updated)."""
    idx = _lib.require_gpu(idx, "idx", _i32)
    dev = idx.device
    grad_zbuf = _lib.require_gpu(grad_zbuf, "grad_zbuf", _f32)
    if idx.dim() != 4 or idx.shape != grad_zbuf.shape:
        raise RuntimeError("idx and grad_zbuf must both be (N,H,W,K)")
    if not (point_grad.is_cuda and point_grad.dtype == _f32 and point_grad.is_contiguous() and point_grad.dim() == 2):
        raise RuntimeError("point_grad must be a contiguous float32 GPU tensor of shape (P,1) or (P,3)")
    if point_grad.shape[1] not in (1, 3):
        raise RuntimeError("point_grad must have 1 or 3 columns")
    N, H, W, K = idx.shape
    with _on_device(dev):
        if point_grad.shape[1] == 3:
            _lib.call("dss_zbuf_backward", dev, idx, grad_zbuf, N, H, W, K, point_grad)
        else:
            tmp = torch.zeros((point_grad.shape[0], 3), dtype=_f32, device=dev)
            _lib.call("dss_zbuf_backward", dev, idx, grad_zbuf, N, H, W, K, tmp)
            point_grad += tmp[:, 2:3]


def clip_grad_(grad_pts, clip: float):
    """In-place per-point norm clip (rasterizer.py:667-673)."""
    if not (grad_pts.is_cuda and grad_pts.dtype == _f32 and grad_pts.is_contiguous()):
        raise RuntimeError("grad_pts must be a contiguous float32 GPU tensor")
    with _on_device(grad_pts.device):
        _lib.call("dss_clip_grad", grad_pts.device, grad_pts, grad_pts.shape[0], float(clip))
    return grad_pts


def splat_backward(points, radii, visible, idx, grad_occ, grad_zbuf, cloud_to_packed_first_idx,
                   num_points_per_cloud, radii_s: float, clip: float = -1.0, return_rs: bool = False):
    """Whole ``EllipticalRasterizer.backward`` (rasterizer.py:787-977) in one call -> grad (P,3)."""
    points, radii = _gpu(_f32, points=points, radii=radii)
    dev = points.device
    vis = _flags(visible, "visible")
    idx = _lib.require_gpu(idx, "idx", _i32)
    if grad_occ is None:  # (autograd hands over None for an unused output: only then are zeros allocated)
        grad_occ = torch.zeros(idx.shape[:3], dtype=_f32, device=dev)
    if not grad_occ.is_cuda:
        raise RuntimeError("dss_amd: grad_occ must be a GPU tensor (no CPU fallback)")
    if grad_zbuf is not None:
        grad_zbuf = _lib.require_gpu(grad_zbuf, "grad_zbuf", _f32)
    first, num, _ = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    N, S, _, K = idx.shape
    P = points.shape[0]
    grad_occ, gstride = _pixel_strided(grad_occ, N, S, S)
    with _on_device(dev):
        grad = torch.empty((P, 3), dtype=_f32, device=dev)
        rs = torch.empty((N,), dtype=_f32, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_splat_backward_workspace(N, P))
        _lib.call("dss_splat_backward", dev, points, radii, vis, idx, grad_occ, grad_zbuf, first, num, N, P, S, K, gstride,
                  float(radii_s), float(clip), grad, rs, ws, ws.numel())
    return (grad, rs) if return_rs else grad


def blend_forward(idx, qvalue, occupancy, scaler, features, return_wsum: bool = False):
    """Fused weights + NormWeightedCompositor + RGBA assembly (renderer.py:53-78).
    ``features`` is (P,C); returns (N,H,W,C+1) [and the per-pixel weight sum max(sum w, 1e-4)]."""
    idx = _lib.require_gpu(idx, "idx", _i32)
    dev = idx.device
    qvalue, occupancy, scaler, features = _gpu(_f32, qvalue=qvalue, occupancy=occupancy, scaler=scaler, features=features)
    N, H, W, K = idx.shape
    C = features.shape[1]
    with _on_device(dev):
        out = torch.empty((N, H, W, C + 1), dtype=_f32, device=dev)
        wsum = torch.empty((N, H, W), dtype=_f32, device=dev) if return_wsum else None
        _lib.call("dss_blend_forward", dev, idx, qvalue, occupancy, scaler, features, N, H, W, K, C, out, wsum)
    return (out, wsum) if return_wsum else out


def blend_backward(grad_out, idx, qvalue, scaler, num_points: int, geometry=None, wsum=None,
                   image_size: Optional[int] = None, rows: Optional[Tuple[int, int]] = None):
    """-> (grad_features (P,C), grad_occupancy (N,H,W) = strided view ``grad_out[..., C]``).

    ``geometry = (pts_screen, radii, visible, first_idx, num_points_per_cloud)`` selects the
    point-centric gather kernel (no atomics, deterministic); without it the pixel-centric scatter
    kernel is used."""
    grad_out = _lib.require_gpu(grad_out, "grad_out", _f32)
    dev = grad_out.device
    idx = _lib.require_gpu(idx, "idx", _i32)
    qvalue, scaler = _gpu(_f32, qvalue=qvalue, scaler=scaler)
    N, H, W, K = idx.shape
    C = grad_out.shape[-1] - 1
    with _on_device(dev):
        gf = torch.empty((num_points, C), dtype=_f32, device=dev)
        if geometry is None:
            _lib.call("dss_blend_backward_scatter", dev, grad_out, idx, qvalue, scaler, N, H, W, K, C, num_points, gf)
        else:
            pts, radii, vis, first, num = geometry
            pts, radii = _gpu(_f32, pts_screen=pts, radii=radii)
            vis = _flags(vis, "visible")
            first, num, n_clouds = _ranges(first, num)
            if wsum is not None:
                wsum = _lib.require_gpu(wsum, "wsum", _f32)
            S = int(image_size) if image_size is not None else W
            row0, row1, _ = _band(rows, S)
            if H != row1 - row0 or W != S:
                raise RuntimeError("fragment tensors must be (N, %d, %d, K)" % (row1 - row0, S))
            _lib.call("dss_blend_backward", dev, grad_out, idx, qvalue, wsum, scaler, pts, radii, vis, first, num,
                      n_clouds, num_points, S, K, C, row0, row1, gf)
    return gf, grad_out[..., C]


def fuse_projection(N: int, S: int, K: int, C: int, shared: bool, n_world: int, P: int) -> bool:
    """whether `render_backward(..., project=(world, M))` can take the projection backward of a whole-image render of N
    cameras, K fragments per pixel and C feature channels: only for RGB features, clouds that are not shared between
    cameras (or one camera), one world point per screen point, and on the 32-bit-offset variants of the gather (every
    gathered tensor below 4 GB and DSS_OPT_BACKWARD_ADDR64 off, raster_backward.hip).  Otherwise the separate projection
    kernel runs (`project_backward`)."""
    widest = N * S * S * max(K, C + 1) * 4
    return (not shared or N == 1) and C == 3 and n_world == P and widest < (1 << 32) \
        and int(_lib.load().dss_get_option(_lib.OPT_BACKWARD_ADDR64)) != 1


def _band(rows, S):
    """`rows` of the fused entry points: None = whole image; (row0, row1) = contiguous band; (row0, row1, c) = of that
    band only every c-th 8-row tile row starting at row0 (tile-row-cyclic multi-GPU partition, include/dss_hip.h)."""
    if rows is None:
        return 0, int(S), 1
    return int(rows[0]), int(rows[1]), (int(rows[2]) if len(rows) > 2 else 1)


def band_rows(row0: int, row1: int, cycle: int = 1) -> int:
    """rows of a band tensor (dss_band_rows)"""
    if row1 <= row0:
        return 0
    if cycle <= 1:
        return row1 - row0
    full, rem = divmod(row1 - row0, 8 * cycle)
    return full * 8 + min(rem, 8)


def _order_state(ws, state: int, shape, order_refresh: int) -> int:
    """workspace_state of a dss_render_forward call on buffer `ws` under the cached point order (``order_refresh`` = k: the
    order saved by one call serves the next k - 1 calls on the same buffer).  The age lives on the buffer OBJECT: a new
    buffer -- or one whose last call failed and was dropped -- starts with a save."""
    if state not in (0, 1):
        return state
    if order_refresh <= 0:
        # a call without either flag sorts for itself and the library forgets the order this buffer held: the next call
        # with order_refresh > 0 must save again (e.g. two renderers of the same shape, one of them without the option)
        if getattr(ws, "_dss_order_age", None) is not None:
            ws._dss_order_age = None
        return state
    age = getattr(ws, "_dss_order_age", None)
    if age is None or age[0] != shape or age[1] + 1 >= int(order_refresh):
        ws._dss_order_age = (shape, 0)
        return state | _lib.WS_ORDER_SAVE
    ws._dss_order_age = (shape, age[1] + 1)
    return state | _lib.WS_ORDER_REUSE


def render_forward(world, normals, h, M, V, znear, zfar, cloud_to_packed_first_idx, num_points_per_cloud, features,
                   image_size: int, points_per_pixel: int, cutoff_threshold: float, depth_merging_thres: float,
                   antialiasing_sigma: float = 1.0, backface_culling: bool = False, shared_cloud: bool = False,
                   rows: Optional[Tuple[int, int]] = None, out_image: Optional[torch.Tensor] = None,
                   out_visible: Optional[torch.Tensor] = None, vr6=None, frame_normals=None, want_zbuf: bool = True,
                   workspace_state: int = 1, order_refresh: int = 0, band_outputs_only: bool = False,
                   point_outputs=None):
    """Fused forward (setup + binning + fine + blend, ``dss_render_forward``).  ``out_image`` (float32
    (N,rows,S,C+1), 16-byte aligned) / ``out_visible`` (uint8 (P,)) let the caller place these two outputs
    in its own buffer (the multi-GPU step points them into one all-gather send buffer).  ``features`` are the
    packed (P,C) features.  Returns a dict with everything the separate calls produce:
    ``pts_screen, ellipse_params, radii, scaler, cutoff_threshold, valid, idx, zbuf, qvalue, occupancy,
    visible, image, wsum``.  ``want_zbuf=False`` skips the depth plane (``zbuf`` is None): the fused backward never reads it.
    ``workspace_state``: 1 = DSS_WS_CLEAN (default: cached zero-initialised workspace, no memset launch), 0 = DSS_WS_UNKNOWN
    (memset + both launches, lists stay in place), 2 = DSS_WS_BINNED (after a state-0 call with the same inputs: repeat only
    the fine + blend launch; profiling / timing of the dominant kernel).
    ``order_refresh`` = k > 0: renderer-owned cached point order (DSS_WS_ORDER_SAVE / DSS_WS_ORDER_REUSE, above 2M points):
    the screen-cell order that the binning sorts the points into is kept in the workspace of this problem size and reused by
    the next k - 1 calls on it, which then skip the sort (same outputs bit for bit; a stale order only costs locality).
    ``band_outputs_only`` (DSS_WS_BAND_OUTPUTS; with ``rows`` only): ``ellipse_params``, ``scaler`` and ``cutoff_threshold`` are
    written for the splats that meet the band only (zero elsewhere); everything else is unchanged -- what a multi-GPU
    rank asks for: it needs every point's position and radii for the backward, but bins an eighth of the cloud.
    ``point_outputs`` = (ellipse (P,3), scaler (P,), cutoff (P,)): caller-owned buffers for those three outputs."""
    world, normals, h, M, V, znear, zfar = _gpu(_f32, world=world, normals=normals, h=h, M=M, V=V, znear=znear, zfar=zfar)
    dev = world.device
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    features = _lib.require_gpu(features, "features", _f32)
    Pw = world.shape[0]
    _check_cameras(M, V, znear, zfar, N)
    if normals.shape != world.shape:
        raise RuntimeError("normals must match world points")
    P = N * Pw if shared_cloud else Pw
    if features.shape[0] != P:
        raise RuntimeError("features must be packed (P,C) with P=%d, got %s" % (P, tuple(features.shape)))
    h_mode = _h_mode(h, N, Pw, P, shared_cloud)
    S, K, C = int(image_size), int(points_per_pixel), features.shape[1]
    row0, row1, cyc = _band(rows, S)
    nr = band_rows(row0, row1, cyc)
    e = lambda *shape, dtype=_f32: torch.empty(shape, dtype=dtype, device=dev)
    if nr == 0:
        # empty row band (multi-GPU rank without rows): only the per-point setup runs; no fragments, nothing visible
        o = point_setup(world, normals, h, M, V, znear, zfar, first, num, S, cutoff_threshold, antialiasing_sigma,
                        backface_culling, shared_cloud, vr6=vr6, frame_normals=frame_normals)
        vis = torch.zeros(P, dtype=_u8, device=dev) if out_visible is None else out_visible.zero_()
        o.update(idx=e(N, 0, S, K, dtype=_i32), zbuf=e(N, 0, S, K), qvalue=e(N, 0, S, K), occupancy=e(N, 0, S),
                 image=e(N, 0, S, C + 1) if out_image is None else out_image, wsum=e(N, 0, S), visible=vis.view(torch.bool))
        return o
    ws_mode = int(workspace_state) & 0xf
    with _on_device(dev):
        # band_outputs_only: the library writes ellipse / scaler / cutoff only for the splats that meet the band; the rest of
        # those three arrays is handed out ZERO-filled, never as uninitialised device memory (one fill of 20 P bytes)
        if point_outputs is not None:
            # caller-owned (ellipse (P,3), scaler (P,), cutoff (P,)): a multi-GPU step zero-fills them ONCE and hands them to
            # every forward (entries of splats outside the band then hold zeros or the value of an earlier step: defined)
            ell, sca, cut = point_outputs
            if not (_dense(ell, (P, 3)) and _dense(sca, (P,)) and _dense(cut, (P,))) or any(t.device != dev for t in point_outputs):
                raise RuntimeError("point_outputs must be contiguous float32 (P,3), (P,), (P,) tensors on the device")
        elif band_outputs_only and ws_mode != 2:
            z3 = torch.zeros(P * 5, dtype=_f32, device=dev)
            ell, sca, cut = z3[:P * 3].view(P, 3), z3[P * 3:P * 4], z3[P * 4:]
        else:
            ell, sca, cut = e(P, 3), e(P), e(P)
        o = dict(pts_screen=e(P, 3), ellipse_params=ell, radii=e(P, 2), scaler=sca, cutoff_threshold=cut,
                 idx=e(N, nr, S, K, dtype=_i32), zbuf=e(N, nr, S, K) if want_zbuf else None, qvalue=e(N, nr, S, K),
                 occupancy=e(N, nr, S), image=e(N, nr, S, C + 1) if out_image is None else out_image, wsum=e(N, nr, S))
        valid = e(P, dtype=_u8)
        vis = e(P, dtype=_u8) if out_visible is None else out_visible
        img = o["image"]
        if tuple(img.shape) != (N, nr, S, C + 1) or img.dtype != _f32 or img.data_ptr() % 16 \
                or img.stride(3) != 1 or img.stride(2) != C + 1 or img.stride(0) % 4 or img.stride(1) % 4 \
                or tuple(vis.shape) != (P,) or vis.dtype != _u8:
            raise RuntimeError("out_image must be float32 (N,rows,S,C+1), 16-byte aligned, with contiguous rows "
                               "(any camera / row strides that are multiples of 4 floats); out_visible uint8 (P,)")
        vr6, frame_normals = _aniso_args(vr6, frame_normals, Pw)
        # dedicated zero-initialised buffer per problem size: the library keeps it clean (no memset launch)
        tag = ("render_forward" if ws_mode == 1 else "render_forward_binned", N, P, S)
        ws = _lib.clean_workspace(dev, tag, _lib.load().dss_render_forward_workspace(N, P, S, K))
        state = _order_state(ws, int(workspace_state), (N, P, S), order_refresh)
        if band_outputs_only and ws_mode != 2:
            state |= _lib.WS_BAND_OUTPUTS
        try:
            _lib.call("dss_render_forward", dev, world, normals, h if h_mode else None, None if h_mode == 1 else h,
                      vr6, frame_normals, M, V, znear, zfar, first, num, N, P, int(shared_cloud), int(backface_culling), S, K,
                      float(cutoff_threshold), float(antialiasing_sigma), float(depth_merging_thres), row0, row1, cyc,
                      features, C, o["pts_screen"], ell, o["radii"], sca, cut, valid, o["idx"], o["zbuf"], o["qvalue"],
                      o["occupancy"], vis, img, int(img.stride(0)), int(img.stride(1)), o["wsum"], ws, ws.numel(), state)
        except RuntimeError:
            _lib.drop_clean_workspace(dev, tag)
            raise
    o["valid"], o["visible"] = valid.view(torch.bool), vis.view(torch.bool)
    return o


def render_backward(grad_out, idx, qvalue, wsum, scaler, points, radii, visible, cloud_to_packed_first_idx,
                    num_points_per_cloud, radii_s: float, clip: float = -1.0, with_features: bool = True,
                    return_rs: bool = False, image_size: Optional[int] = None,
                    rows: Optional[Tuple[int, int]] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                    gather_only_rs: Optional[torch.Tensor] = None, project=None,
                    grad_out_full: Optional[torch.Tensor] = None, grad_occ_full: Optional[torch.Tensor] = None):
    """Fused backward of renderer + rasterizer (blend backward + median radius + occupancy backward +
    clip) -> (grad_features (P,C) or None, grad_pts_screen (P,3)).  With ``rows`` (multi-GPU band) pass the
    union of the visibility flags and ``clip <= 0``; the results are the band's partial sums.
    ``project=(world (P,3), M (N,4,4))`` also fuses `project_backward` into the launch: the second result is then the
    WORLD-space position gradient (clouds that are not shared between cameras, whole image, 3 feature channels).
    ``gather_only_rs`` = the ``rs`` a preceding identical call returned (and ``out`` = its outputs): re-runs only the
    second stage, the gather kernel (``dss_render_backward_gather``; per-kernel timing).
    ``grad_out_full`` (N,S,S,C+1) with ``rows``: OWNER mode of the band (``dss_render_backward_owned``) -- the position
    gradient of every (camera, point) pair is computed completely, over its whole search window in the full image gradient,
    by the rank whose band holds the image row of the point's centre (zeros on the other ranks), so that clip and projection
    can precede the reduction over the ranks; the feature gradients stay partial sums of the band.
    ``grad_occ_full`` (N,S,S) with ``rows``: the same owner mode fed by the dense plane of the occupancy gradient alone
    (``dss_render_backward_owned_plane``) -- what the ranks of a step with a band-local loss all-gather (`gather_rows`)."""
    grad_out = _lib.require_gpu(grad_out, "grad_out", _f32)
    dev = grad_out.device
    idx = _lib.require_gpu(idx, "idx", _i32)
    qvalue, scaler, points, radii = _gpu(_f32, qvalue=qvalue, scaler=scaler, points=points, radii=radii)
    vis = _flags(visible, "visible")
    first, num, _ = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    if wsum is not None:
        wsum = _lib.require_gpu(wsum, "wsum", _f32)
    N, H, W, K = idx.shape
    C = grad_out.shape[-1] - 1
    P = points.shape[0]
    S = int(image_size) if image_size is not None else W
    row0, row1, cyc = _band(rows, S)
    if W != S or H != band_rows(row0, row1, cyc) or tuple(grad_out.shape[:3]) != (N, H, W):
        raise RuntimeError("render_backward needs idx (N,rows,S,K) and grad_out (N,rows,S,C+1)")
    with _on_device(dev):
        if out is not None:  # caller-provided (P,C) / (P,3) float32 views, e.g. slices of one all-reduce bucket
            gf, gp = out
            if not (_dense(gf, (P, C)) and _dense(gp, (P, 3))):
                raise RuntimeError("out must be contiguous float32 tensors of shape (P,C) and (P,3)")
        else:
            gf = torch.empty((P, C), dtype=_f32, device=dev) if with_features else None
            gp = torch.empty((P, 3), dtype=_f32, device=dev)
        if H == 0:  # empty row band: zero partial sums (the search radius still follows the global visibility)
            if gf is not None:
                gf.zero_()
            gp.zero_()
            if return_rs:
                return gf, gp, backward_radius(radii, vis, first, num, radii_s)
            return gf, gp
        rs = torch.empty((N,), dtype=_f32, device=dev) if gather_only_rs is None else \
            _lib.require_gpu(gather_only_rs, "gather_only_rs", _f32)
        if gather_only_rs is not None and out is None:
            raise RuntimeError("gather_only_rs needs out= (the gradients the full call zero-filled)")
        # entry point by mode: the owner modes take the full-image gradient after grad_out and no projection
        name, head, tail = "dss_render_backward", (grad_out,), (None, None)
        if project is not None:
            w_t, m_t = _gpu(_f32, world=project[0], M=project[1])
            if tuple(w_t.shape) != (P, 3) or tuple(m_t.shape) != (N, 4, 4):
                raise RuntimeError("project=(world (P,3), M (N,4,4)) with P=%d N=%d, got %s %s"
                                   % (P, N, tuple(w_t.shape), tuple(m_t.shape)))
            tail = (w_t, m_t)
        ws = _lib.workspace(dev, _lib.load().dss_render_backward_workspace(N, P, S))
        if grad_occ_full is not None:
            if project is not None or gather_only_rs is not None or grad_out_full is not None:
                raise RuntimeError("grad_occ_full (owner mode of a band) excludes project=, gather_only_rs= and grad_out_full=")
            plane = _lib.require_gpu(grad_occ_full, "grad_occ_full", _f32)
            if tuple(plane.shape) != (N, S, S):
                raise RuntimeError("grad_occ_full must be (N,S,S) = %s, got %s" % ((N, S, S), tuple(plane.shape)))
            name, head, tail = "dss_render_backward_owned_plane", (grad_out, plane), ()
        elif grad_out_full is not None:
            if project is not None or gather_only_rs is not None:
                raise RuntimeError("grad_out_full (owner mode of a band) excludes project= and gather_only_rs=")
            full = _lib.require_gpu(grad_out_full, "grad_out_full", _f32)
            if tuple(full.shape) != (N, S, S, C + 1) or not full.is_contiguous():
                raise RuntimeError("grad_out_full must be contiguous (N,S,S,C+1)")
            name, head, tail = "dss_render_backward_owned", (grad_out, full), ()
        _lib.call(name if gather_only_rs is None else "dss_render_backward_gather", dev, *head, idx, qvalue, wsum, scaler,
                  points, radii, vis, first, num, N, P, S, K, C, row0, row1, cyc, float(radii_s), float(clip), gf, gp, rs,
                  *tail, ws, ws.numel())
    return (gf, gp, rs) if return_rs else (gf, gp)


def gather_rows(src, row_pos, n_images: int, rows: int, row_floats: int, out=None):
    """``dss_gather_rows``: rows of an all-gathered (position, camera, row_floats) float32 buffer put in image order ->
    dense (n_images, rows, row_floats); ``row_pos`` int32 (rows,) = position of image row r in ``src``."""
    src = _lib.require_gpu(src, "src", _f32)
    dev = src.device
    row_pos = _lib.require_gpu(row_pos, "row_pos", _i32)
    if row_pos.numel() != rows or src.numel() % (n_images * row_floats):
        raise RuntimeError("gather_rows: row_pos must have %d entries and src whole (camera, row) slices" % rows)
    with _on_device(dev):
        if out is None:
            out = torch.empty((n_images, rows, row_floats), dtype=_f32, device=dev)
        elif not _dense(out, n_images * rows * row_floats):
            raise RuntimeError("gather_rows: out must be a contiguous float32 tensor of %d elements" % (n_images * rows * row_floats))
        _lib.call("dss_gather_rows", dev, src, row_pos, int(n_images), int(rows), int(row_floats), out)
    return out


class FusedPlan:
    """Host-lean form of ``render_forward`` + ``render_backward`` for one problem shape (the drop-in renderer's hot path,
    DSS/core/renderer.py:36-82 + rasterizer.py:584-664): ONE arena allocation per forward carved into the 13 output
    tensors (only the ones somebody reads become tensor objects), the workspace looked up once, the ~45 arguments of the
    two C entry points prebuilt with only the pointers refreshed per call.  Same kernels, same results; the general
    functions above stay the reference for argument checking (a plan is only built from inputs they would accept)."""

    _ALIGN = 256

    def __init__(self, device, N, Pw, P, S, K, C, shared, per_point_h, aniso, backface, cutoff, sigma, thr, want_zbuf=True):
        self.lib = _lib.load()
        self.dev, self.N, self.Pw, self.P, self.S, self.K, self.C = device, N, Pw, P, S, K, C
        # per_point_h: 0 = one h per cloud, 1 = per world point, 2 = per PACKED point (shared cloud, cameras that cull differently)
        self.shared, self.per_point_h, self.aniso = bool(shared), int(per_point_h), bool(aniso)
        off = [0]

        def take(nbytes):
            o = off[0]
            off[0] += (int(nbytes) + self._ALIGN - 1) // self._ALIGN * self._ALIGN
            return o
        px = N * S * S
        self.layout = {}   # name -> (offset, bytes, dtype, shape)
        for name, nbytes, dt, shape in (
                ("image", px * (C + 1) * 4, _f32, (N, S, S, C + 1)), ("pts_screen", P * 12, _f32, (P, 3)),
                ("ellipse_params", P * 12, _f32, (P, 3)), ("radii", P * 8, _f32, (P, 2)), ("scaler", P * 4, _f32, (P,)),
                ("cutoff_threshold", P * 4, _f32, (P,)), ("valid", P, _u8, (P,)), ("visible", P, _u8, (P,)),
                ("idx", px * K * 4, _i32, (N, S, S, K)), ("qvalue", px * K * 4, _f32, (N, S, S, K)),
                ("occupancy", px * 4, _f32, (N, S, S)), ("wsum", px * 4, _f32, (N, S, S))) + (
                (("zbuf", px * K * 4, _f32, (N, S, S, K)),) if want_zbuf else ()):
            self.layout[name] = (take(nbytes), int(nbytes), dt, shape)
        self.total = off[0]
        self.want_zbuf = want_zbuf
        self.order_refresh = 0   # k > 0: cached point order, see render_forward (set by the rasterizer that owns the plan)
        self.force_state = None  # workspace_state passed as is (a caller that captures the saving and the reusing call as graphs)
        self.fwd_ws_bytes = self.lib.dss_render_forward_workspace(N, P, S, K)
        self.bwd_ws_bytes = self.lib.dss_render_backward_workspace(N, P, S)
        self.tag = ("render_forward", N, P, S)
        self.consts = (int(shared), int(backface), S, K, float(cutoff), float(sigma), float(thr))
        self._o = {k: v[0] for k, v in self.layout.items()}

    @staticmethod
    def lean_input(t, dtype=_f32):
        return t is not None and t.is_cuda and t.dtype == dtype and t.is_contiguous()

    def view(self, arena, name):
        o, n, dt, shape = self.layout[name]
        return arena[o:o + n].view(dt).view(shape)

    def image(self, arena):
        """the (N,S,S,C+1) image at offset 0 of the arena"""
        n, shape = self.layout["image"][1], self.layout["image"][3]
        return arena[:n].view(_f32).view(shape)

    def forward(self, world, normals, h, M, V, znear, zfar, first, num, feats, vr6=None, frame_n=None, ws=None):
        """-> arena (uint8): every output of dss_render_forward at its offset (see `view`).  `ws`: a caller-owned forward
        workspace under the DSS_WS_CLEAN contract (zero-filled once, `fwd_ws_bytes` long) instead of the cached per-stream
        one -- a captured graph bakes the workspace address into its launches and must own the buffer."""
        lib, dev, o = self.lib, self.dev, self._o
        N, P, S, K, C = self.N, self.P, self.S, self.K, self.C
        shared, backface, _, _, cutoff, sigma, thr = self.consts
        own_ws = ws is not None
        with _on_device(dev):
            arena = torch.empty(self.total, dtype=_u8, device=dev)
            if not own_ws:
                ws = _lib.clean_workspace(dev, self.tag, self.fwd_ws_bytes)
            b = arena.data_ptr()
            hp = h.data_ptr()
            rc = lib.dss_render_forward(
                world.data_ptr(), normals.data_ptr(), hp if self.per_point_h else None, None if self.per_point_h == 1 else hp,
                None if vr6 is None else vr6.data_ptr(), None if frame_n is None else frame_n.data_ptr(),
                M.data_ptr(), V.data_ptr(), znear.data_ptr(), zfar.data_ptr(), first.data_ptr(), num.data_ptr(), N, P,
                shared, backface, S, K, cutoff, sigma, thr, 0, S, 1, feats.data_ptr(), C,
                b + o["pts_screen"], b + o["ellipse_params"], b + o["radii"], b + o["scaler"], b + o["cutoff_threshold"],
                b + o["valid"], b + o["idx"], (b + o["zbuf"]) if self.want_zbuf else None, b + o["qvalue"], b + o["occupancy"],
                b + o["visible"], b + o["image"], 0, 0, b + o["wsum"], ws.data_ptr(), ws.numel(),
                self.force_state if self.force_state is not None else _order_state(ws, 1, (N, P, S), self.order_refresh),
                torch.cuda.current_stream(dev).cuda_stream)
            if rc:
                if own_ws:
                    ws.zero_()   # (a failed call may leave counters behind: restore the contract's state)
                else:
                    _lib.drop_clean_workspace(dev, self.tag)
        _lib.check(rc, "dss_render_forward")
        return arena

    def backward(self, arena, g_image, first, num, radii_s, clip, world=None, M=None, ws=None):
        """-> (grad_features (P,C), grad_pts (P,3)) -- world-space position gradients when (world, M) are given (fused
        projection, see render_backward).  `ws`: a caller-owned backward workspace (`bwd_ws_bytes`), see `forward`."""
        lib, dev, o = self.lib, self.dev, self._o
        N, P, S, K, C = self.N, self.P, self.S, self.K, self.C
        with _on_device(dev):
            if C == 3:
                both = torch.empty((2, P, 3), dtype=_f32, device=dev)
                gf, gp = both[0], both[1]
            else:
                gf = torch.empty((P, C), dtype=_f32, device=dev)
                gp = torch.empty((P, 3), dtype=_f32, device=dev)
            rs = torch.empty((N,), dtype=_f32, device=dev)
            if ws is None:
                ws = _lib.workspace(dev, self.bwd_ws_bytes)
            b = arena.data_ptr()
            rc = lib.dss_render_backward(
                g_image.data_ptr(), b + o["idx"], b + o["qvalue"], b + o["wsum"], b + o["scaler"], b + o["pts_screen"],
                b + o["radii"], b + o["visible"], first.data_ptr(), num.data_ptr(), N, P, S, K, C, 0, S, 1, float(radii_s),
                float(clip), gf.data_ptr(), gp.data_ptr(), rs.data_ptr(), None if world is None else world.data_ptr(),
                None if M is None else M.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "dss_render_backward")
        return gf, gp


def _aniso_args(vr6, frame_normals, Pw):
    """(vr6, frame_normals) of the anisotropic source variance, checked, or (None, None)."""
    if vr6 is None:
        return None, None
    vr6, fn = _gpu(_f32, vr6=vr6, frame_normals=frame_normals)
    if tuple(vr6.shape) != (Pw, 6) or tuple(fn.shape) != (Pw, 3):
        raise RuntimeError("anisotropic mode needs vr6 (%d,6) and frame_normals (%d,3)" % (Pw, Pw))
    return vr6, fn


def local_frames(points, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, return_curvature: bool = False):
    """PCA frames of the K-neighbourhoods (``knn_idx`` from ``knn_points``, self included) -> anisotropic source
    variance ``vr6 (P,6)`` (xx,xy,xz,yy,yz,zz) and frame normals ``(P,3)`` (rasterizer.py:256-291 +
    mathHelper.py:34-92 with neighborhood_size = 8)."""
    points = _lib.require_gpu(points, "points", _f32)
    dev = points.device
    knn_idx = _lib.require_gpu(knn_idx, "knn_idx", _i64)
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    P, K = knn_idx.shape
    if points.shape[0] != P:
        raise RuntimeError("knn_idx must be (P,K) for the P packed points")
    with _on_device(dev):
        vr6 = torch.empty((P, 6), dtype=_f32, device=dev)
        fn = torch.empty((P, 3), dtype=_f32, device=dev)
        cv = torch.empty((P, 3), dtype=_f32, device=dev) if return_curvature else None
        _lib.call("dss_local_frames", dev, points, knn_idx, first, num, N, P, int(K), vr6, fn, cv)
    return (vr6, fn, cv) if return_curvature else (vr6, fn)


def point_setup(world, normals, h, M, V, znear, zfar, cloud_to_packed_first_idx, num_points_per_cloud,
                image_size: int, cutoff_threshold: float, antialiasing_sigma: float = 1.0,
                backface_culling: bool = False, shared_cloud: bool = False, vr6=None, frame_normals=None):
    """Fused culling + projection + EWA per-point setup (rasterizer.py:183-254, 443-565, 614).

    ``h`` is either per point ``(Pw,)`` or per cloud ``(N,)``; with ``vr6`` / ``frame_normals`` (``local_frames``)
    the anisotropic source variance is used instead and ``h`` is ignored.  Returns a dict with
    ``pts_screen (P,3), ellipse_params (P,3), radii (P,2), scaler (P,), cutoff_threshold (P,),
    valid bool (P,)``.
    """
    world, normals, h, M, V, znear, zfar = _gpu(_f32, world=world, normals=normals, h=h, M=M, V=V, znear=znear, zfar=zfar)
    dev = world.device
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    Pw = world.shape[0]
    _check_cameras(M, V, znear, zfar, N)
    if normals.shape != world.shape:
        raise RuntimeError("normals must match world points")
    P = N * Pw if shared_cloud else Pw
    h_mode = _h_mode(h, N, Pw, P, shared_cloud)
    with _on_device(dev):
        e = lambda *shape: torch.empty(shape, dtype=_f32, device=dev)
        out = dict(pts_screen=e(P, 3), ellipse_params=e(P, 3), radii=e(P, 2), scaler=e(P), cutoff_threshold=e(P))
        valid = torch.empty((P,), dtype=_u8, device=dev)
        vr6, frame_normals = _aniso_args(vr6, frame_normals, Pw)
        _lib.call("dss_point_setup", dev, world, normals, h if h_mode else None, None if h_mode == 1 else h, vr6,
                  frame_normals, M, V, znear, zfar, first, num, N, P, int(shared_cloud), int(backface_culling),
                  int(image_size), float(cutoff_threshold), float(antialiasing_sigma), *out.values(), valid)   # (`out` is in the entry's order)
    out["valid"] = valid.view(torch.bool)
    return out


def _projection_inputs(world, M, V, cloud_to_packed_first_idx, num_points_per_cloud, grad_screen, valid):
    """What `project_backward` and `camera_backward` share: the checked inputs, N, Pw and the device."""
    world, M, V = _gpu(_f32, world=world, M=M, V=V)
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    grad_screen = _lib.require_gpu(grad_screen, "grad_screen", _f32)
    return world, M, V, first, num, grad_screen, _flags(valid, "valid"), N, world.shape[0], world.device


def project_backward(world, M, V, cloud_to_packed_first_idx, num_points_per_cloud, grad_screen, valid,
                     shared_cloud: bool = False, clip: float = -1.0, grad_features=None, out=None):
    """grad of (NDC x, NDC y, view z) w.r.t. the world points -> (Pw,3).  ``clip > 0`` applies the per-point norm
    clip of ``clip_grad_`` to ``grad_screen`` on the fly (multi-GPU: the clip comes after the all-reduce).
    ``grad_features`` (P,C): also sums the per-camera feature gradients of a shared cloud over its cameras in the same
    launch (``dss_project_backward_features``) -> (grad_world (Pw,3), grad_features_world (Pw,C)).
    ``out`` = (grad_world, grad_features_world) to write into (contiguous float32, e.g. two views of one all-reduce
    buffer)."""
    world, M, V, first, num, grad_screen, vis, N, Pw, dev = _projection_inputs(
        world, M, V, cloud_to_packed_first_idx, num_points_per_cloud, grad_screen, valid)
    with _on_device(dev):
        gw = torch.empty((Pw, 3), dtype=_f32, device=dev) if out is None else out[0]
        if out is not None and not _dense(gw, (Pw, 3)):
            raise RuntimeError("out[0] must be a contiguous float32 (Pw,3) tensor")
        lead = (world, M, V, first, num, N, Pw, int(shared_cloud), grad_screen, vis, float(clip), gw)
        if grad_features is None:
            _lib.call("dss_project_backward", dev, *lead)
            return gw
        gfeat = _lib.require_gpu(grad_features, "grad_features", _f32)
        P = N * Pw if shared_cloud else Pw
        if gfeat.dim() != 2 or gfeat.shape[0] != P:
            raise RuntimeError("grad_features must be packed (P,C) with P=%d, got %s" % (P, tuple(gfeat.shape)))
        C = gfeat.shape[1]
        gfw = torch.empty((Pw, C), dtype=_f32, device=dev) if out is None else out[1]
        if out is not None and not _dense(gfw, (Pw, C)):
            raise RuntimeError("out[1] must be a contiguous float32 (Pw,C) tensor")
        _lib.call("dss_project_backward_features", dev, *lead, gfeat, C, gfw)
    return gw, gfw


def camera_backward(world, M, V, cloud_to_packed_first_idx, num_points_per_cloud, grad_screen, valid,
                    shared_cloud: bool = False, clip: float = -1.0):
    """grad of (NDC x, NDC y, view z) w.r.t. the camera matrices (``dss_camera_backward``; the counterpart of
    `project_backward`, same inputs) -> (grad_M (N,4,4), grad_V (N,4,4)), fully written, bitwise reproducible.  From
    there plain torch autograd carries on to ``R``, ``T``, ``fov``, ... of the camera object."""
    world, M, V, first, num, grad_screen, vis, N, Pw, dev = _projection_inputs(
        world, M, V, cloud_to_packed_first_idx, num_points_per_cloud, grad_screen, valid)
    P = N * Pw if shared_cloud else Pw
    if tuple(M.shape) != (N, 4, 4) or tuple(V.shape) != (N, 4, 4) or tuple(grad_screen.shape) != (P, 3) or vis.numel() != P:
        raise RuntimeError("camera_backward: need M, V (N,4,4), grad_screen (P,3), valid (P,) with N=%d P=%d" % (N, P))
    with _on_device(dev):
        gM = torch.empty((N, 4, 4), dtype=_f32, device=dev)
        gV = torch.empty((N, 4, 4), dtype=_f32, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_camera_backward_workspace(N, P))
        _lib.call("dss_camera_backward", dev, world, M, V, first, num, N, Pw, int(shared_cloud), grad_screen, vis,
                  float(clip), gM, gV, ws, ws.numel())
    return gM, gV


def _knn_inputs(points, cloud_to_packed_first_idx, num_points_per_cloud):
    """What the kNN entries share: the three checked tensors, N, P and the device."""
    points = _lib.require_gpu(points, "points", _f32)
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    return points, first, num, N, points.shape[0], points.device


def knn_kth_sqdist(points, cloud_to_packed_first_idx, num_points_per_cloud, K: int = 7, radius=None):
    """K-th smallest squared distance of every point to its own cloud (self included) -> (P,).
    Exact grid search in HIP; replaces frnn.frnn_grid_points / pytorch3d.ops.knn_points for the
    variance-scale statistic (rasterizer.py:310-321, 366-383).  ``radius`` > 0 (``dss_knn_kth_sqdist_radius``): the
    fixed-radius semantics of the reference's DEFAULT search, ``frnn_grid_points(K, r = frnn_radius = 0.2)`` -- the largest of
    the K - 1 neighbour distances that lie within ``radius``, -1 for a point that has no neighbour there."""
    points, first, num, N, P, dev = _knn_inputs(points, cloud_to_packed_first_idx, num_points_per_cloud)
    with _on_device(dev):
        out = torch.empty((P,), dtype=_f32, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_knn_workspace(N, P))
        if radius is not None and radius > 0:
            _lib.call("dss_knn_kth_sqdist_radius", dev, points, first, num, N, P, int(K), float(radius), out, ws, ws.numel())
        else:
            _lib.call("dss_knn_kth_sqdist", dev, points, first, num, N, P, int(K), out, ws, ws.numel())
    return out


def knn_points(points, cloud_to_packed_first_idx, num_points_per_cloud, K: int):
    """Self kNN of packed clouds -> (dists (P,K) squared, idx (P,K) int64 cloud-local), ascending, the point itself
    first, zero-padded for clouds with fewer than K points: the packed form of
    ``pytorch3d.ops.knn_points(p, p, lengths, lengths, K)`` used by the regularisers (losses.py:157-180)."""
    points, first, num, N, P, dev = _knn_inputs(points, cloud_to_packed_first_idx, num_points_per_cloud)
    with _on_device(dev):
        dists = torch.empty((P, int(K)), dtype=_f32, device=dev)
        idx = torch.empty((P, int(K)), dtype=_i64, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_knn_workspace(N, P))
        _lib.call("dss_knn_points", dev, points, first, num, N, P, int(K), dists, idx, ws, ws.numel())
    return dists, idx


def cloud_mean_clamp(values, cloud_to_packed_first_idx, num_points_per_cloud, scale: float, lo: float, hi: float,
                     fallback: float, min_points: int):
    """Per-cloud clamp(mean(values*scale), lo, hi) -> (N,), deterministic."""
    values = _lib.require_gpu(values, "values", _f32)
    dev = values.device
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    with _on_device(dev):
        out = torch.empty((N,), dtype=_f32, device=dev)
        _lib.call("dss_cloud_mean_clamp", dev, values, first, num, N, float(scale), float(lo), float(hi), float(fallback),
                  int(min_points), out)
    return out


def renderable_mean_clamp(values, world, V, znear, zfar, cloud_to_packed_first_idx, num_points_per_cloud, shared_cloud: bool,
                          scale: float, lo: float, hi: float, fallback: float, min_points: int):
    """``cloud_mean_clamp`` under the reference's depth culling for MASKED clouds (``dss_renderable_mean_clamp``): per camera
    the mean over the points it keeps (view z in [znear, zfar]), divided by the LARGEST kept count of the batch like the
    reference's mean over the padded clouds (rasterizer.py:183-217, 320-326) -> (N,).  ``values``: (Pw,) one per world point,
    or (N, Pw) per (camera, point) from `knn_kth_sqdist_view` (a shared cloud in the reference's exact order)."""
    values, world, V, znear, zfar = _gpu(_f32, values=values, world=world, V=V, znear=znear, zfar=zfar)
    dev = values.device
    first, num, n_clouds = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    N, Pw = V.shape[0], world.shape[0]
    per_cam = values.dim() == 2
    if (tuple(values.shape) != ((N, Pw) if per_cam else (Pw,))) or n_clouds != N or znear.numel() != N or zfar.numel() != N:
        raise RuntimeError("renderable_mean_clamp: values (Pw,) or (N,Pw); V, znear, zfar, first_idx, num_points per camera")
    with _on_device(dev):
        out = torch.empty((N,), dtype=_f32, device=dev)
        ws = _lib.workspace(dev, 512 * N)
        _lib.call("dss_renderable_mean_clamp", dev, values, world, V, znear, zfar, first, num, N, int(shared_cloud),
                  float(scale), float(lo), float(hi), float(fallback), int(min_points), Pw if per_cam else 0, out,
                  ws, ws.numel())
    return out


def knn_kth_sqdist_view(points, cloud_to_packed_first_idx, num_points_per_cloud, K: int, V, znear, zfar, shared_cloud: bool,
                        radius=None):
    """`knn_kth_sqdist` in the reference's order under depth culling (``dss_knn_kth_sqdist_view``): every camera drops the
    points outside its [znear, zfar] BEFORE the neighbour search (rasterizer.py:599, 183-217, 310-326).  ``shared_cloud``:
    one cloud, N cameras -> (N, P) (row c: among the points camera c keeps; 0 for the ones it drops); else cloud n belongs to
    camera n -> (P,).  Packed slots outside every cloud (before ``first_idx[0]``, between clouds, behind the last one) are 0,
    in every row."""
    points, first, num, N, P, dev = _knn_inputs(points, cloud_to_packed_first_idx, num_points_per_cloud)
    V, znear, zfar = _gpu(_f32, V=V, znear=znear, zfar=zfar)
    n_cams = V.shape[0]
    with _on_device(dev):
        out = torch.empty((n_cams, P) if shared_cloud else (P,), dtype=_f32, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_knn_workspace(N, P))
        _lib.call("dss_knn_kth_sqdist_view", dev, points, first, num, N, P, int(K),
                  float(radius) if radius is not None else -1.0, V, znear, zfar, n_cams, int(shared_cloud), out,
                  ws, ws.numel())
    return out


def _phong_common(world, normals, rgb, first, num, shared_cloud, ambient, diffuse_color, specular_color, light_vec,
                  point_lights, cam_center, shininess, grad_out=None, who=None):
    """What the four Phong operators share -> (dev, N, Pw, P, L, lead): the checked inputs as the argument list that every
    one of their entries begins with (the backward entries after `grad_out`, checked here under the operator's name `who`)."""
    world, normals, rgb = _gpu(_f32, world=world, normals=normals, rgb=rgb)
    first, num, N = _ranges(first, num)
    Pw = world.shape[0]
    P = N * Pw if shared_cloud else Pw
    amb, kd, ks, lv, cam = _gpu(_f32, ambient=ambient, diffuse_color=diffuse_color, specular_color=specular_color,
                                light_vec=light_vec, cam_center=cam_center)
    L = kd.shape[1] if kd.dim() == 3 else 0
    if tuple(rgb.shape) != (P, 3) or normals.shape != world.shape or tuple(amb.shape) != (N, 3) \
            or tuple(kd.shape) != (N, L, 3) or tuple(ks.shape) != (N, L, 3) or tuple(lv.shape) != (N, L, 3) \
            or tuple(cam.shape) != (N, 3):
        raise RuntimeError("phong: need rgb (P,3), ambient / cam_center (N,3), light tensors (N,L,3)")
    lead = (world, normals, rgb, first, num, N, Pw, int(shared_cloud), amb, kd, ks, lv, L, int(point_lights), cam,
            float(shininess))
    if who is not None:
        grad_out = _lib.require_gpu(grad_out, "grad_out", _f32)
        if tuple(grad_out.shape) != (P, 3):
            raise RuntimeError("%s: grad_out must be (P,3)" % who)
        lead = (grad_out,) + lead
    return world.device, N, Pw, P, L, lead


def phong_forward(world, normals, rgb, cloud_to_packed_first_idx, num_points_per_cloud, ambient, diffuse_color,
                  specular_color, light_vec, point_lights: bool, cam_center, shininess: float = 64.0,
                  shared_cloud: bool = False):
    """Phong shading of the points (LightingTexture.forward, texture.py:65-125; lighting.py:10-172) -> (P,3).
    Per-camera clouds: the row of a packed point that no cloud owns is zeros.  A shared cloud with ``num[n] < Pw`` (which
    `shared_cloud_ranges` never produces) leaves the rows of that camera's missing pairs unspecified."""
    dev, N, Pw, P, L, lead = _phong_common(
        world, normals, rgb, cloud_to_packed_first_idx, num_points_per_cloud, shared_cloud, ambient, diffuse_color,
        specular_color, light_vec, point_lights, cam_center, shininess)
    with _on_device(dev):
        out = torch.empty((P, 3), dtype=_f32, device=dev)
        _lib.call("dss_phong_forward", dev, *lead, out)
    return out


def phong_backward(grad_out, world, normals, rgb, cloud_to_packed_first_idx, num_points_per_cloud, ambient,
                   diffuse_color, specular_color, light_vec, point_lights: bool, cam_center, shininess: float = 64.0,
                   shared_cloud: bool = False):
    """-> (grad_world (Pw,3), grad_normals (Pw,3), grad_rgb (P,3)).  Per-camera clouds: a packed point that no cloud owns
    gets zeros in all three.  A shared cloud with ``num[n] < Pw`` (which `shared_cloud_ranges` never produces) leaves the
    rows of ``grad_rgb`` of that camera's missing pairs unspecified; the other two sum the cameras that own the point."""
    dev, N, Pw, P, L, lead = _phong_common(
        world, normals, rgb, cloud_to_packed_first_idx, num_points_per_cloud, shared_cloud, ambient, diffuse_color,
        specular_color, light_vec, point_lights, cam_center, shininess, grad_out, "phong_backward")
    with _on_device(dev):
        gw = torch.empty((Pw, 3), dtype=_f32, device=dev)
        gn = torch.empty((Pw, 3), dtype=_f32, device=dev)
        gc = torch.empty((P, 3), dtype=_f32, device=dev)
        _lib.call("dss_phong_backward", dev, *lead, gw, gn, gc)
    return gw, gn, gc


def phong_backward_camera(grad_out, world, normals, rgb, cloud_to_packed_first_idx, num_points_per_cloud, ambient,
                          diffuse_color, specular_color, light_vec, point_lights: bool, cam_center, shininess: float = 64.0,
                          shared_cloud: bool = False):
    """-> grad_cam (N,3): the shading's gradient w.r.t. the camera centres (``dss_phong_backward_camera``; same inputs as
    `phong_backward`), bitwise reproducible."""
    dev, N, Pw, P, L, lead = _phong_common(
        world, normals, rgb, cloud_to_packed_first_idx, num_points_per_cloud, shared_cloud, ambient, diffuse_color,
        specular_color, light_vec, point_lights, cam_center, shininess, grad_out, "phong_backward_camera")
    with _on_device(dev):
        gcam = torch.empty((N, 3), dtype=_f32, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_camera_backward_workspace(N, P))
        _lib.call("dss_phong_backward_camera", dev, *lead, gcam, ws, ws.numel())
    return gcam


def phong_backward_lights(grad_out, world, normals, rgb, cloud_to_packed_first_idx, num_points_per_cloud, ambient,
                          diffuse_color, specular_color, light_vec, point_lights: bool, cam_center, shininess: float = 64.0,
                          shared_cloud: bool = False, needs=(True, True, True, True)):
    """-> (grad_ambient (N,3), grad_diffuse, grad_specular, grad_light_vec (N,L,3)): the shading's gradient w.r.t. the
    lights (``dss_phong_backward_lights``; same inputs as `phong_backward`), bitwise reproducible.  ``ambient`` is the
    (N,3) sum over lights, and so is its gradient.  ``needs``: the outputs to compute; the others are returned as None."""
    dev, N, Pw, P, L, lead = _phong_common(
        world, normals, rgb, cloud_to_packed_first_idx, num_points_per_cloud, shared_cloud, ambient, diffuse_color,
        specular_color, light_vec, point_lights, cam_center, shininess, grad_out, "phong_backward_lights")
    with _on_device(dev):
        outs = [torch.empty(shape, dtype=_f32, device=dev) if need else None
                for need, shape in zip(needs, ((N, 3), (N, L, 3), (N, L, 3), (N, L, 3)))]
        ws = _lib.workspace(dev, _lib.load().dss_phong_backward_lights_workspace(N, P, L))
        _lib.call("dss_phong_backward_lights", dev, *lead, *outs, ws, ws.numel())
    return tuple(outs)


def _mask_u8(mask, name, P, dev):
    if mask is None:
        return None
    mask = _lib.require_gpu(mask, name)
    if mask.numel() != P:
        raise RuntimeError("dss_amd: %s must have one entry per packed point (%d), got %d" % (name, P, mask.numel()))
    return _nonzero_u8(mask)


def _nonzero_u8(mask):
    """Flags of any dtype as 0 / 1 bytes, true where the reference's ``.bool()`` is: ``!= 0`` (0.5 and 256.0 are true; a
    cast to uint8 would make them 0).  bool keeps its bytes: no conversion kernel."""
    if mask.dtype != torch.bool:
        mask = mask != 0
    return mask.contiguous().view(torch.uint8)


def _knn_lists(knn_dists, knn_idx, P, need_dists=True):
    knn_idx = _lib.require_gpu(knn_idx, "knn_idx", _i64)
    if knn_idx.dim() != 2 or knn_idx.shape[0] != P:
        raise RuntimeError("dss_amd: knn_idx must be (P, K) with P = %d, got %s" % (P, tuple(knn_idx.shape)))
    if need_dists:
        knn_dists = _lib.require_gpu(knn_dists, "knn_dists", _f32)
        if knn_dists.shape != knn_idx.shape:
            raise RuntimeError("dss_amd: knn_dists %s and knn_idx %s differ" % (tuple(knn_dists.shape), tuple(knn_idx.shape)))
    return knn_dists, knn_idx, int(knn_idx.shape[1])


def _grad_loss(grad_loss, numel, shape_text):
    """the optional upstream gradient of a per-point loss"""
    if grad_loss is not None:
        grad_loss = _lib.require_gpu(grad_loss, "grad_loss", _f32)
        if grad_loss.numel() != numel:
            raise RuntimeError("dss_amd: grad_loss must be %s" % shape_text)
    return grad_loss


def mollify_normals(normals, knn_dists, knn_idx, keep, cloud_to_packed_first_idx, num_points_per_cloud):
    """Robust normal mollification of the regularisers (SurfaceLoss._denoise_normals with get_phi weights,
    losses.py:181-222, 262-278) on the packed neighbour lists of :func:`knn_points` -> (P,3).  ``keep`` (P,) bool marks
    the points whose own normal is kept (visibility & inmask); None mollifies every point."""
    normals = _lib.require_gpu(normals, "normals", _f32)
    dev, P = normals.device, normals.shape[0]
    knn_dists, knn_idx, K = _knn_lists(knn_dists, knn_idx, P)
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    keep = _mask_u8(keep, "keep", P, dev)
    with _on_device(dev):
        out = torch.empty_like(normals)
        _lib.call("dss_mollify_normals", dev, normals, knn_dists, knn_idx, keep, first, num, N, P, K, out)
    return out


def projection_loss(points, mollified, knn_dists, knn_idx, visible, cloud_to_packed_first_idx, num_points_per_cloud,
                    sharpness_sigma: float, grad_loss=None, want_loss: bool = True, want_grad: bool = False):
    """ProjectionLoss.compute (losses.py:296-392) per packed point -> (loss (P,) or None, grad_points (P,3) or None);
    grad_points = d loss_i / d p_i * grad_loss_i (grad_loss None = ones)."""
    points, mollified = _gpu(_f32, points=points, mollified=mollified)
    dev, P = points.device, points.shape[0]
    knn_dists, knn_idx, K = _knn_lists(knn_dists, knn_idx, P)
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    visible = _mask_u8(visible, "visible", P, dev)
    grad_loss = _grad_loss(grad_loss, P, "(P,)")
    with _on_device(dev):
        loss = torch.empty((P,), dtype=_f32, device=dev) if want_loss else None
        grad = torch.empty((P, 3), dtype=_f32, device=dev) if want_grad else None
        _lib.call("dss_projection_loss", dev, points, mollified, knn_dists, knn_idx, visible, first, num, N, P, K,
                  float(sharpness_sigma), grad_loss, loss, grad)
    return loss, grad


def repulsion_loss(points, mollified, knn_idx, cloud_to_packed_first_idx, num_points_per_cloud, sharpness_sigma: float,
                   filter_scale: float, grad_loss=None, want_loss: bool = True, want_grad: bool = False):
    """RepulsionLoss.compute (losses.py:395-492) per packed point -> (loss (P,3) or None, grad_points (P,3) or None)."""
    points, mollified = _gpu(_f32, points=points, mollified=mollified)
    dev, P = points.device, points.shape[0]
    _, knn_idx, K = _knn_lists(None, knn_idx, P, need_dists=False)
    first, num, N = _ranges(cloud_to_packed_first_idx, num_points_per_cloud)
    grad_loss = _grad_loss(grad_loss, 3 * P, "(P,3)")
    with _on_device(dev):
        loss = torch.empty((P, 3), dtype=_f32, device=dev) if want_loss else None
        grad = torch.empty((P, 3), dtype=_f32, device=dev) if want_grad else None
        ws = _lib.workspace(dev, 24 * N)
        _lib.call("dss_repulsion_loss", dev, points, mollified, knn_idx, first, num, N, P, K, float(sharpness_sigma),
                  float(filter_scale), grad_loss, loss, grad, ws, ws.numel())
    return loss, grad


def _check_target_rgb(target_rgb):
    if not isinstance(target_rgb, torch.Tensor) or not target_rgb.is_cuda or target_rgb.dtype != _f32:
        raise RuntimeError("dss_amd: target_rgb must be a float32 GPU tensor (no CPU fallback)")


def _grad_total(grad_total):
    """the optional device scalar that scales an image-loss gradient -> float32 (1,) or None"""
    return None if grad_total is None else _lib.require_gpu(grad_total, "grad_total", _f32).reshape(1)


def _image_loss_args(rgba, target_rgb, target_mask):
    rgba = _lib.require_gpu(rgba, "rgba", _f32)
    if rgba.dim() != 4 or rgba.shape[-1] != 4:
        raise RuntimeError("dss_amd: rgba must be (N,H,W,4), got %s" % (tuple(rgba.shape),))
    N, H, W, _ = rgba.shape
    _check_target_rgb(target_rgb)
    if tuple(target_rgb.shape) != (N, H, W, 3):
        raise RuntimeError("dss_amd: target_rgb must be (N,H,W,3) = %s (a permuted NCHW view is fine), got %s"
                           % ((N, H, W, 3), tuple(target_rgb.shape)))
    target_mask = _lib.require_gpu(target_mask, "target_mask", _f32).reshape(N, H, W)
    return rgba, target_rgb, target_mask, N, H, W


def image_loss_forward(rgba, target_rgb, target_mask, lambda_rgb: float, lambda_silhouette: float):
    """Trainer.calc_dr_loss (trainer.py:332-372) on the rendered (N,H,W,4) image -> (losses (4,) = total, weighted rgb
    term, weighted silhouette term, IoU term; sums (N+1,5) float64 for :func:`image_loss_backward`).  ``target_rgb``
    (N,H,W,3) may be any strided view (e.g. ``img.permute(0, 2, 3, 1)``); no host synchronisation."""
    rgba, target_rgb, target_mask, N, H, W = _image_loss_args(rgba, target_rgb, target_mask)
    dev = rgba.device
    with _on_device(dev):
        losses = torch.empty((4,), dtype=_f32, device=dev)
        sums = torch.empty((N + 1, 5), dtype=_f64, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_image_loss_workspace(N, H, W))
        _lib.call("dss_image_loss_forward", dev, rgba, target_rgb, *target_rgb.stride(), target_mask, N, H, W,
                  float(lambda_rgb), float(lambda_silhouette), sums, losses, ws, ws.numel())
    return losses, sums


def image_loss_backward(rgba, target_rgb, target_mask, lambda_rgb: float, lambda_silhouette: float, sums, grad_total=None):
    """Gradient of the total image loss w.r.t. the rendered image, (N,H,W,4), scaled by the device scalar
    ``grad_total`` (None = 1)."""
    rgba, target_rgb, target_mask, N, H, W = _image_loss_args(rgba, target_rgb, target_mask)
    dev = rgba.device
    sums = _lib.require_gpu(sums, "sums", _f64)
    if tuple(sums.shape) != (N + 1, 5):
        raise RuntimeError("dss_amd: sums must be (N+1,5) from image_loss_forward")
    grad_total = _grad_total(grad_total)
    with _on_device(dev):
        grad = torch.empty_like(rgba)
        _lib.call("dss_image_loss_backward", dev, rgba, target_rgb, *target_rgb.stride(), target_mask, N, H, W,
                  float(lambda_rgb), float(lambda_silhouette), sums, grad_total, grad)
    return grad


def points_inmask(points, M, mask_img, visible=None):
    """In-mask filter of the regularisers (point_modeling.py:183-208): bool (P,) = visible & any over the views of
    (target mask bilinearly sampled at the point's projection != 0).  ``points`` (P,3) world positions of one cloud,
    ``M`` (N,4,4) full projection matrices, ``mask_img`` (N,H,W) or (N,1,H,W)."""
    points, M = _gpu(_f32, points=points, M=M)
    dev, P, N = points.device, points.shape[0], M.shape[0]
    if not isinstance(mask_img, torch.Tensor) or not mask_img.is_cuda:
        raise RuntimeError("dss_amd: mask_img must be a GPU tensor (no CPU fallback)")
    if mask_img.dim() == 4:
        mask_img = mask_img[:, 0]
    if mask_img.dim() != 3 or mask_img.shape[0] != N:
        raise RuntimeError("dss_amd: mask_img must be (N,H,W) or (N,1,H,W) with N = %d views, got %s" % (N, tuple(mask_img.shape)))
    mask_img = mask_img.to(_f32).contiguous()
    visible = _mask_u8(visible, "visible", P, dev)
    with _on_device(dev):
        out = torch.empty((P,), dtype=torch.uint8, device=dev)
        _lib.call("dss_points_inmask", dev, points, M, mask_img, visible, N, P, mask_img.shape[1], mask_img.shape[2], out)
    return out.view(torch.bool)   # the kernel writes 0 / 1


_band_row_cache = {}


def _band_row_index(row0, row1, cyc, device):
    """image rows of the tile-row-cyclic band (row0, row1, cyc), in band order, as a cached int64 device tensor"""
    key = (row0, row1, cyc, device)
    t = _band_row_cache.get(key)
    if t is None:
        if len(_band_row_cache) > 64:
            _band_row_cache.clear()
        rows = [r0 + i for r0 in range(row0, row1, 8 * cyc) for i in range(8) if r0 + i < row1]
        t = _band_row_cache[key] = torch.tensor(rows, dtype=_i64, device=device)
    return t


def band_targets(target_rgb, target_mask, rows):
    """The rows ``rows`` of the targets of a band loss, gathered ONCE (a tile-row-cyclic band costs two index_select launches
    per call otherwise): pass the result as ``band_targets=`` to `image_loss_band_sums` / `image_loss_band_backward` while the
    targets stay the same."""
    row0, row1, cyc = _band(rows, None)
    N, H, W = target_rgb.shape[0], target_rgb.shape[1], target_rgb.shape[2]
    target_mask = target_mask.to(_f32).reshape(N, H, W)
    if cyc > 1:
        ri = _band_row_index(row0, row1, cyc, target_rgb.device)
        return target_rgb.index_select(1, ri).contiguous(), target_mask.index_select(1, ri).contiguous()
    return target_rgb[:, row0:row1], target_mask[:, row0:row1]


def _band_args(rgba_band, target_rgb, target_mask, rows, band_targets=None, keep_strides=False):
    """Row band of an image loss: the band render (N,rows,W,4) against the FULL targets (N,H,W,3) / (N,H,W); returns the
    tensors plus the targets' band and the image stride of its mask.  ``rows`` = (row0, row1) for a contiguous band (views of
    the targets, no copy) or (row0, row1, cycle) for a tile-row-cyclic one (`RowPartition(cyclic=True).rows`: the owned
    rows of the targets are gathered once per call).  ``keep_strides``: the band has been vetted by `_strided_band` and is
    taken as it is (not made contiguous)."""
    if not keep_strides:
        rgba_band = _lib.require_gpu(rgba_band, "rgba_band", _f32)
    row0, row1, cyc = _band(rows, None)
    want = band_rows(row0, row1, cyc)
    if rgba_band.dim() != 4 or rgba_band.shape[-1] != 4 or rgba_band.shape[1] != want:
        raise RuntimeError("dss_amd: rgba_band must be (N, %d, W, 4) for rows %s, got %s" % (want, tuple(rows), tuple(rgba_band.shape)))
    N, nr, W, _ = rgba_band.shape
    _check_target_rgb(target_rgb)
    H = target_rgb.shape[1]
    if target_rgb.dim() != 4 or tuple(target_rgb.shape) != (N, H, W, 3) or not (0 <= row0 <= row1 <= H):
        raise RuntimeError("dss_amd: target_rgb must be the full (N,H,W,3) target with 0 <= row0 <= row1 <= H")
    target_mask = _lib.require_gpu(target_mask, "target_mask", _f32).reshape(N, H, W)
    if band_targets is not None:
        band_rgb, band_mask = band_targets
        if tuple(band_rgb.shape) != (N, nr, W, 3) or tuple(band_mask.shape) != (N, nr, W):
            raise RuntimeError("dss_amd: band_targets must be (N,%d,W,3) and (N,%d,W)" % (nr, nr))
        return rgba_band, band_rgb, band_mask, target_mask, N, nr, W, H, int(band_mask.stride(0))
    if cyc > 1:
        ri = _band_row_index(row0, row1, cyc, rgba_band.device)
        band_rgb = target_rgb.index_select(1, ri)
        band_mask = target_mask.index_select(1, ri)
        return rgba_band, band_rgb, band_mask, target_mask, N, nr, W, H, nr * W
    band_rgb = target_rgb[:, row0:row1]
    band_mask = target_mask[:, row0:row1]
    return rgba_band, band_rgb, band_mask, target_mask, N, nr, W, H, H * W


def image_loss_band_sums(rgba_band, target_rgb, target_mask, rows, band_targets=None):
    """Per-image sums of ``Trainer.calc_dr_loss`` over the row band ``rows = (row0, row1)`` -> float64 (N+1,5) whose
    first N rows are filled; all-reduce (SUM) ``sums[:N]`` over the ranks, then :func:`image_loss_from_sums`."""
    rgba_band, band_rgb, band_mask, _keep, N, nr, W, H, mstride = _band_args(rgba_band, target_rgb, target_mask, rows, band_targets)
    dev = rgba_band.device
    with _on_device(dev):
        sums = torch.zeros((N + 1, 5), dtype=_f64, device=dev)
        if nr > 0:
            ws = _lib.workspace(dev, _lib.load().dss_image_loss_workspace(N, nr, W))
            _lib.call("dss_image_loss_band_sums", dev, rgba_band, band_rgb, *band_rgb.stride(), band_mask, mstride, N, nr, W,
                      sums, ws, ws.numel())
    return sums


def image_loss_from_sums(sums, image_size, lambda_rgb: float, lambda_silhouette: float):
    """Totals row + losses (4,) from the (all-reduced) per-image sums; ``image_size = (H, W)`` of the FULL image."""
    sums = _lib.require_gpu(sums, "sums", _f64)
    N = sums.shape[0] - 1
    dev = sums.device
    with _on_device(dev):
        losses = torch.empty((4,), dtype=_f32, device=dev)
        _lib.call("dss_image_loss_from_sums", dev, sums, N, int(image_size[0]), int(image_size[1]), float(lambda_rgb),
                  float(lambda_silhouette), losses)
    return losses


def image_loss_band_backward(rgba_band, target_rgb, target_mask, rows, lambda_rgb: float, lambda_silhouette: float, sums,
                             grad_total=None, band_targets=None):
    """The band ``rows`` of d total / d rgba, (N,rows,W,4), from the reduced ``sums`` (after image_loss_from_sums)."""
    rgba_band, band_rgb, band_mask, _keep, N, nr, W, H, mstride = _band_args(rgba_band, target_rgb, target_mask, rows, band_targets)
    dev = rgba_band.device
    sums = _lib.require_gpu(sums, "sums", _f64)
    grad_total = _grad_total(grad_total)
    with _on_device(dev):
        grad = torch.empty_like(rgba_band)
        if nr > 0:
            _lib.call("dss_image_loss_band_backward", dev, rgba_band, band_rgb, *band_rgb.stride(), band_mask, mstride,
                      N, nr, W, H, float(lambda_rgb), float(lambda_silhouette), sums, grad_total, grad)
    return grad


def _strided_band(rgba_band):
    """-> (tensor, camera stride, row stride) of an (N, rows, W, 4) float32 band whose pixels and rows of pixels are contiguous
    (the (row, camera, col, channel) send buffer of the multi-GPU renderer through its (N, rows, W, 4) view); (t, 0, 0) for a
    dense band; anything else is copied"""
    if not isinstance(rgba_band, torch.Tensor) or not rgba_band.is_cuda or rgba_band.dtype != _f32:
        raise RuntimeError("dss_amd: rgba_band must be a float32 GPU tensor (no CPU fallback)")
    if rgba_band.dim() != 4 or rgba_band.shape[-1] != 4:
        raise RuntimeError("dss_amd: rgba_band must be (N,rows,W,4), got %s" % (tuple(rgba_band.shape),))
    if rgba_band.is_contiguous():
        return rgba_band, 0, 0
    sn, sh, sw, sc = rgba_band.stride()
    if sc == 1 and sw == 4 and sn % 4 == 0 and sh % 4 == 0 and sh >= 4 * rgba_band.shape[2] and rgba_band.data_ptr() % 16 == 0:
        return rgba_band, int(sn), int(sh)
    return rgba_band.contiguous(), 0, 0


def image_loss_band_partials(rgba_band, target_rgb, target_mask, rows, band_targets=None, out=None):
    """First launch of the two-launch band loss (``dss_image_loss_band_partials``): the block partials of the band's five
    per-image sums -> float64 (N, 64, 5).  All-reduce THEM (SUM) over the ranks, then `image_loss_band_backward_partials`.
    ``rgba_band`` may be the strided (N, rows, W, 4) view of a (row, camera, col, channel) buffer (no copy).
    ``out``: a caller-owned buffer of that shape (a step that replays as a graph all-reduces a static one)."""
    view, rsn, rsh = _strided_band(rgba_band)
    _c, band_rgb, band_mask, _keep, N, nr, W, H, mstride = _band_args(view, target_rgb, target_mask, rows, band_targets,
                                                                      keep_strides=True)
    dev = view.device
    with _on_device(dev):
        n = _lib.load().dss_image_loss_band_partials_count(N)
        part = torch.empty((N, n // (5 * N), 5), dtype=_f64, device=dev) if out is None else out
        if not _dense(part, n, _f64):
            raise RuntimeError("dss_amd: out must be a contiguous float64 tensor of %d elements" % n)
        strides = band_rgb.stride() if nr > 0 else (0, 0, 0, 0)
        _lib.call("dss_image_loss_band_partials", dev, view, band_rgb, *strides, band_mask, mstride, N, nr, W, rsn, rsh, part)
    return part


def image_loss_band_backward_partials(rgba_band, target_rgb, target_mask, rows, lambda_rgb: float, lambda_silhouette: float,
                                      partials, grad_total=None, band_targets=None, want_sums: bool = False, alpha_out=None):
    """Second launch: from the ALL-REDUCED partials -> (band of d total / d rgba (N,rows,W,4) dense, losses (4,) = total,
    weighted rgb term, weighted silhouette term, IoU term[, sums (N+1,5) float64]) -- identical bits on every rank.
    ``alpha_out`` (N, rows, W) float32, last dimension contiguous (any camera / row strides): receives the alpha channel of
    the gradient a second time -- the send buffer of the owner form's alpha-plane exchange, no extraction copy."""
    view, rsn, rsh = _strided_band(rgba_band)
    _c, band_rgb, band_mask, _keep, N, nr, W, H, mstride = _band_args(view, target_rgb, target_mask, rows, band_targets,
                                                                      keep_strides=True)
    dev = view.device
    partials = _lib.require_gpu(partials, "partials", _f64)
    if partials.numel() != _lib.load().dss_image_loss_band_partials_count(N):
        raise RuntimeError("dss_amd: partials must come from image_loss_band_partials")
    grad_total = _grad_total(grad_total)
    asn, ash = 0, 0
    if alpha_out is not None:
        if tuple(alpha_out.shape) != (N, nr, W) or alpha_out.dtype != _f32 or not alpha_out.is_cuda or (nr > 0 and alpha_out.stride(2) != 1):
            raise RuntimeError("dss_amd: alpha_out must be a float32 GPU tensor (N,%d,%d) with contiguous rows" % (nr, W))
        asn, ash = int(alpha_out.stride(0)), int(alpha_out.stride(1))
    with _on_device(dev):
        grad = torch.empty((N, nr, W, 4), dtype=_f32, device=dev)
        losses = torch.empty((4,), dtype=_f32, device=dev)
        sums = torch.empty((N + 1, 5), dtype=_f64, device=dev) if want_sums else None
        strides = band_rgb.stride() if nr > 0 else (0, 0, 0, 0)
        _lib.call("dss_image_loss_band_backward_partials", dev, view, band_rgb, *strides, band_mask, mstride, N, nr, W, H,
                  float(lambda_rgb), float(lambda_silhouette), partials, grad_total, grad, losses, sums, rsn, rsh,
                  alpha_out, asn, ash)
    return (grad, losses, sums) if want_sums else (grad, losses)


# The cross-cloud operators (nearest point in ANOTHER cloud, the chamfer backward on it) live in cross_cloud.py and go
# through the same boundary (`_lib.call`); they are operators of this module like the ones above.
from .cross_cloud import chamfer_backward, chamfer_order, nearest_points, packed_cloud_ids  # noqa: E402,F401
# likewise the operators between a cloud and a triangle mesh (mesh_ops.py: nearest face, nearest point of a face, backward)
from .mesh_ops import face_point_distance, mesh_distance_backward, mesh_distance_orders, point_face_distance  # noqa: E402,F401
# and the meshes' way to target images (mesh_ops.py: hard rasteriser, flat shader)
from .mesh_ops import rasterize_meshes, shade_mesh_flat  # noqa: E402,F401
# and the points on a mesh's surface (mesh_ops.py: the sampler and its backward; the public calls are
# dss_amd.mesh_sampling.sample_points_from_meshes and sample_mesh_evenly)
from .mesh_ops import mesh_sample_backward, mesh_sample_order, sample_mesh_surface  # noqa: E402,F401
# likewise the two kernels of an upsampling round (upsample_ops.py; the rounds themselves are dss_amd.cloud_ops.upsample)
from .upsample_ops import upsample_candidates, upsample_insert  # noqa: E402,F401
# and the two kernels that clean a cloud (smoothing_ops.py; the public calls are dss_amd.cloud_ops.denoise_normals and
# project_to_latent_surface)
from .smoothing_ops import denoise_normals, rimls_step  # noqa: E402,F401
# and the kernel that thins a cloud evenly (sampling_ops.py; the public calls are dss_amd.cloud_ops.sample_farthest_points
# and subsample)
from .sampling_ops import farthest_points  # noqa: E402,F401
# and the two kernels that give estimated normals a sign (normals_ops.py; the public calls are
# dss_amd.cloud_ops.estimate_normals and orient_normals)
from .normals_ops import disambiguate_normals, orient_normals  # noqa: E402,F401
