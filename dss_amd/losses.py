"""Point-cloud regularisers of the training iteration, mirroring DSS/training/losses.py.

`ProjectionLoss` and `RepulsionLoss` (reference losses.py:281-392, :395-492, both on `SurfaceLoss` :145-278) keep the
reference's constructor arguments, call signature (``loss(point_clouds, points_filter=..., rebuild_knn=True)``),
reduction handling (`BaseLoss` :24-62) and results; the Trainer builds them with ``reduction='mean',
filter_scale=2.0, knn_k=12`` (trainer.py:134-137).  The arithmetic runs in three HIP kernels on the packed neighbour
lists of `dss_knn_points` (dss_amd/csrc/regularizers.hip) instead of ~40 padded torch tensors; the neighbour search
itself replaces `pytorch3d.ops.knn_points`.  As in the reference, only the points receive a gradient (every weight is
computed under no_grad there).
"""
from typing import Optional

import torch
from torch import autograd

from . import neighbours, ops


class _Neighbourhood:
    """Self-query neighbour lists of a batch of clouds (the reference's `knn_tree`, losses.py:155-179), packed."""

    def __init__(self, point_clouds, K: int):
        self.first = point_clouds.cloud_to_packed_first_idx()
        self.num = point_clouds.num_points_per_cloud()
        self.K = int(K)
        self.dists, self.idx = neighbours.self_knn(point_clouds.points_packed(), self.first, self.num,
                                                   [p.shape[0] for p in point_clouds.points_list()], self.K)

    def matches(self, point_clouds) -> bool:
        num = point_clouds.num_points_per_cloud()
        return num.shape == self.num.shape and bool(torch.equal(num, self.num))


def _packed_mask(mask, point_clouds) -> Optional[torch.Tensor]:
    """(N, Pmax) padded or (P,) packed bool mask -> packed (P,) bool.  A mask with more rows than clouds (one row per
    camera of a shared cloud) is OR-ed over the rows like losses.py:203-206."""
    if mask is None:
        return None
    sizes = [p.shape[0] for p in point_clouds.points_list()]   # host-side sizes: no device synchronisation
    P = sum(sizes)
    if mask.dim() == 1:
        if mask.numel() != P:
            raise ValueError("Incompatible point clouds ({} points) and mask {}".format(P, tuple(mask.shape)))
        return mask.bool()
    if mask.shape[0] != len(point_clouds):
        if len(point_clouds) == 1 and mask.shape[0] > 1:
            mask = mask.any(dim=0, keepdim=True)
        else:
            raise ValueError("Incompatible point clouds {} and mask {}".format(len(point_clouds), tuple(mask.shape)))
    if len(sizes) == 1:
        return mask[0, : sizes[0]].bool()
    return torch.cat([mask[b, :n] for b, n in enumerate(sizes)]).bool()


class _Projection(autograd.Function):
    @staticmethod
    def forward(ctx, points, mollified, dists, idx, visible, first, num, sigma):
        loss, _ = ops.projection_loss(points, mollified, dists, idx, visible, first, num, sigma)
        ctx.save_for_backward(points, mollified, dists, idx, first, num)
        ctx.visible, ctx.sigma = visible, sigma
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        points, mollified, dists, idx, first, num = ctx.saved_tensors
        _, grad = ops.projection_loss(points, mollified, dists, idx, ctx.visible, first, num, ctx.sigma,
                                      grad_loss=grad_loss.contiguous(), want_loss=False, want_grad=True)
        return (grad,) + (None,) * 7


class _Repulsion(autograd.Function):
    @staticmethod
    def forward(ctx, points, mollified, idx, first, num, sigma, filter_scale):
        loss, _ = ops.repulsion_loss(points, mollified, idx, first, num, sigma, filter_scale)
        ctx.save_for_backward(points, mollified, idx, first, num)
        ctx.sigma, ctx.filter_scale = sigma, filter_scale
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        points, mollified, idx, first, num = ctx.saved_tensors
        _, grad = ops.repulsion_loss(points, mollified, idx, first, num, ctx.sigma, ctx.filter_scale,
                                     grad_loss=grad_loss.contiguous(), want_loss=False, want_grad=True)
        return (grad,) + (None,) * 6


class SurfaceLoss(torch.nn.Module):
    """Shared state of the two regularisers (reference `SurfaceLoss` + `BaseLoss`)."""

    def __init__(self, reduction: str = "mean", knn_k: int = 33, filter_scale: float = 1.0, sharpness_sigma: float = 0.75):
        super().__init__()
        self.reduction = reduction
        self.channel_dim = None
        self.knn_tree = None
        self.knn_k = knn_k
        neighbours.request_lists(knn_k)   # the renderer's kNN for `h` will now produce lists this loss can reuse
        self.filter_scale = filter_scale
        self.sharpness_sigma = sharpness_sigma

    def _reduce(self, loss, reduction=None):  # losses.py:42-52
        reduction = reduction or self.reduction
        if reduction == "none":
            return loss
        if reduction == "sum":
            return torch.sum(loss)
        if reduction == "mean":
            return torch.mean(loss)
        raise ValueError("Invalid reduction method ({})".format(reduction))

    def forward(self, *args, **kwargs):  # losses.py:54-61
        reduction = kwargs.pop("reduction", self.reduction)
        self.channel_dim = kwargs.pop("channel_dim", self.channel_dim)
        loss = self.compute(*args, **kwargs)
        if self.channel_dim is not None:
            loss = torch.sum(loss, dim=self.channel_dim)
        return self._reduce(loss, reduction=reduction)

    def _neighbourhood(self, point_clouds, rebuild_knn, kwargs):
        self.sharpness_sigma = kwargs.get("sharpness_sigma", self.sharpness_sigma)
        self.filter_scale = kwargs.get("filter_scale", self.filter_scale)
        self.knn_tree = kwargs.get("knn_tree", self.knn_tree)
        if self.knn_tree is not None and not isinstance(self.knn_tree, _Neighbourhood):
            raise TypeError("knn_tree must be the packed neighbourhood of a dss_amd loss (its `.knn_tree`), not a padded "
                            "pytorch3d result; pass rebuild_knn=True to search again")
        if rebuild_knn or self.knn_tree is None or not self.knn_tree.matches(point_clouds):
            self.knn_tree = _Neighbourhood(point_clouds, self.knn_k)
        return self.knn_tree

    @staticmethod
    def _mollified(point_clouds, nb, points_filter):
        keep = None
        if points_filter is not None:
            vis, inm = getattr(points_filter, "visibility", None), getattr(points_filter, "inmask", None)
            if vis is not None and inm is not None:
                # losses.py:198-206: AND first (same view), then OR over the views of a shared cloud
                both = (vis.bool() & inm.bool()) if vis.shape == inm.shape else None
                keep = _packed_mask(both, point_clouds) if both is not None else \
                    _packed_mask(vis, point_clouds) & _packed_mask(inm, point_clouds)
        return ops.mollify_normals(point_clouds.normals_packed().detach(), nb.dists, nb.idx, keep, nb.first, nb.num)


class ProjectionLoss(SurfaceLoss):
    """Weighted squared distance of every point to the planes of its neighbours (reference :281-392), (P,) before the
    reduction."""

    def compute(self, point_clouds, points_filter=None, rebuild_knn=False, **kwargs):
        nb = self._neighbourhood(point_clouds, rebuild_knn, kwargs)
        mollified = self._mollified(point_clouds, nb, points_filter)
        visible = None if points_filter is None else _packed_mask(points_filter.visibility, point_clouds)
        return _Projection.apply(point_clouds.points_packed(), mollified, nb.dists, nb.idx, visible, nb.first, nb.num,
                                 float(self.sharpness_sigma))


class RepulsionLoss(SurfaceLoss):
    """exp(-|tangential offset to the weighted neighbourhood|) per coordinate (reference :395-492), (P,3) before the
    reduction."""

    def compute(self, point_clouds, points_filter=None, rebuild_knn=True, **kwargs):
        nb = self._neighbourhood(point_clouds, rebuild_knn, kwargs)
        mollified = self._mollified(point_clouds, nb, points_filter)
        return _Repulsion.apply(point_clouds.points_packed(), mollified, nb.idx, nb.first, nb.num,
                                float(self.sharpness_sigma), float(self.filter_scale))


class _ImageLoss(autograd.Function):
    """total, loss_dr_rgb, loss_dr_silhouette, IoU term; only the total is differentiable (the others are what the
    Trainer logs)."""

    @staticmethod
    def forward(ctx, rgba, img, mask_img, lambda_rgb, lambda_silhouette):
        losses, sums = ops.image_loss_forward(rgba, img, mask_img, lambda_rgb, lambda_silhouette)
        ctx.save_for_backward(rgba, img, mask_img, sums)
        ctx.lambdas = (lambda_rgb, lambda_silhouette)
        total, rest = losses[0], losses[1:]
        ctx.mark_non_differentiable(rest)
        return total, rest

    @staticmethod
    def backward(ctx, grad_total, _grad_rest):
        rgba, img, mask_img, sums = ctx.saved_tensors
        grad = ops.image_loss_backward(rgba, img, mask_img, ctx.lambdas[0], ctx.lambdas[1], sums,
                                       grad_total=grad_total.contiguous())
        return grad, None, None, None, None


def calc_dr_loss(rgba_pred, img, mask_img, lambda_dr_rgb: float = 1.0, lambda_dr_silhouette: float = 1.0):
    """The image loss of `Trainer.calc_dr_loss` (trainer.py:332-372) on the renderer's (N,H,W,4) output
    (``img_pred = rgba[..., :3]``, ``mask_img_pred = rgba[..., 3]``): masked L1 on RGB + silhouette L1 + 0.01 IoU, as
    one reduction pass and, in backward, one gradient pass (dss_amd/csrc/image_loss.hip).

    ``img`` (N,H,W,3) float (a permuted NCHW view is fine, as in trainer.py:306), ``mask_img`` (N,H,W) or (N,1,H,W).
    Returns the Trainer's dictionary entries: ``loss`` (differentiable), ``loss_dr_rgb``, ``loss_dr_silhouette``, plus
    ``loss_iou`` -- device scalars, no host synchronisation."""
    if mask_img.dtype != torch.float32:
        mask_img = mask_img.float()
    total, rest = _ImageLoss.apply(rgba_pred, img, mask_img, float(lambda_dr_rgb), float(lambda_dr_silhouette))
    return {"loss": total, "loss_dr_rgb": rest[0], "loss_dr_silhouette": rest[1], "loss_iou": rest[2]}


class _ChamferSide:
    """One argument of `chamfer_distance` as packed clouds: ``src`` is the tensor autograd sees (padded (N,P,3), or the
    packed (P,3) of a `PointClouds3D`), ``pack`` / ``unpack_grad`` move between it and the packed (P,3) the kernels take."""

    def __init__(self, points, lengths, normals, name):
        if hasattr(points, "points_packed"):
            self.src = points.points_packed()
            self.sizes = [int(p.shape[0]) for p in points.points_list()]   # host-side sizes: no device synchronisation
            self.sel, self.padded_shape = None, None
            normals = points.normals_packed()
        elif torch.is_tensor(points):
            if points.dim() != 3:
                raise ValueError("Expected points to be of shape (N, P, D)")
            if points.shape[2] != 3:
                raise ValueError("dss_amd.losses.chamfer_distance is built for 3-D points, got D = %d" % points.shape[2])
            N, P = points.shape[0], points.shape[1]
            if lengths is not None and (lengths.dim() != 1 or lengths.shape[0] != N):
                raise ValueError("Expected lengths to be of shape (N,)")
            if normals is not None and (normals.dim() != 3 or normals.shape[:2] != points.shape[:2]):
                raise ValueError("Expected normals to be of shape (N, P, 3")
            self.src = points
            self.sizes = [P] * N if lengths is None else [int(v) for v in lengths.tolist()]
            if any(s > P for s in self.sizes):
                raise ValueError("%s_lengths exceed the padded size %d" % (name, P))
            self.padded_shape = tuple(points.shape)
            self.sel = None
            if any(s != P for s in self.sizes):   # flat positions of the valid entries of the padded tensor
                self.sel = torch.cat([torch.arange(n * P, n * P + s, device=points.device) for n, s in enumerate(self.sizes)])
        else:
            raise ValueError("The input pointclouds should be either Pointclouds objects or torch.Tensor of shape (minibatch, "
                             "num_points, 3).")
        if len(self.sizes) == 0 or any(s <= 0 for s in self.sizes):
            raise ValueError("chamfer_distance: %s has an empty cloud (sizes %s): its mean distance is undefined" % (name, self.sizes))
        dev = self.src.device
        self.num = torch.tensor(self.sizes, dtype=torch.int64, device=dev)
        first, run = [], 0
        for s in self.sizes:
            first.append(run)
            run += s
        self.first = torch.tensor(first, dtype=torch.int64, device=dev)
        self.P = run
        self.normals = None if normals is None else self.pack(normals.detach())

    def pack(self, t):
        if self.padded_shape is None:
            return t.contiguous()
        flat = t.reshape(-1, t.shape[-1])
        return flat.contiguous() if self.sel is None else flat.index_select(0, self.sel)

    def unpack_grad(self, g):
        if self.padded_shape is None:
            return g
        if self.sel is None:
            return g.view(self.padded_shape)
        return g.new_zeros((self.padded_shape[0] * self.padded_shape[1], 3)).index_copy_(0, self.sel, g).view(self.padded_shape)

    def per_point(self, per_cloud):
        return torch.repeat_interleave(per_cloud, self.num, output_size=self.P)

    def cloud_sums(self, v):
        """(P,) -> (N,) per-cloud sums in a fixed order (no atomics)."""
        if all(s == self.sizes[0] for s in self.sizes):
            return v.view(len(self.sizes), self.sizes[0]).sum(1)
        return torch.stack([c.sum() for c in v.split(self.sizes)])


def _normal_term(own, near):   # 1 - |cos|, F.cosine_similarity(dim = 1, eps = 1e-6)
    return 1 - torch.abs(torch.nn.functional.cosine_similarity(own, near, dim=1, eps=1e-6))


class _Chamfer(autograd.Function):
    """Both nearest-point searches, the normal term and the reductions as ONE node; backward = dss_chamfer_backward."""

    @staticmethod
    def forward(ctx, x_src, y_src, sx, sy, weights, batch_reduction, point_reduction):
        x, y = sx.pack(x_src.detach()), sy.pack(y_src.detach())
        d2x, idx_xy = ops.nearest_points(x, sx.first, sx.num, y, sy.first, sy.num)
        d2y, idx_yx = ops.nearest_points(y, sy.first, sy.num, x, sx.first, sx.num)
        N = len(sx.sizes)
        # d (result) / d (squared distance of a point of cloud n), per side: weight, point and batch reduction
        kx = torch.ones(N, dtype=x.dtype, device=x.device) if weights is None else weights.to(x.dtype).reshape(N)
        ky = kx
        if point_reduction == "mean":
            kx, ky = kx / sx.num, ky / sy.num
        if batch_reduction == "mean":
            div = weights.sum() if weights is not None else N
            kx, ky = kx / div, ky / div
        cx, cy = sx.per_point(kx), sy.per_point(ky)
        cham = sx.cloud_sums(d2x * cx) + sy.cloud_sums(d2y * cy)
        cham_normals = None
        if sx.normals is not None and sy.normals is not None:
            # the neighbours' normals: one row gather each (dss_gather_rows), rows = packed ids of the nearest points
            near_x = ops.gather_rows(sy.normals, (idx_xy + sx.per_point(sy.first)).to(torch.int32), 1, sx.P, 3)[0]
            near_y = ops.gather_rows(sx.normals, (idx_yx + sy.per_point(sx.first)).to(torch.int32), 1, sy.P, 3)[0]
            cham_normals = sx.cloud_sums(_normal_term(sx.normals, near_x) * cx) + sy.cloud_sums(_normal_term(sy.normals, near_y) * cy)
        if batch_reduction is not None:
            cham = cham.sum()
            cham_normals = None if cham_normals is None else cham_normals.sum()
        ctx.save_for_backward(x, y, idx_xy, idx_yx, kx, ky)
        ctx.sides = (sx, sy)
        if cham_normals is not None:
            ctx.mark_non_differentiable(cham_normals)
        return cham, cham_normals

    @staticmethod
    def backward(ctx, grad_cham, _grad_normals):
        x, y, idx_xy, idx_yx, kx, ky = ctx.saved_tensors
        sx, sy = ctx.sides
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx, gy = sx.per_point(grad_cham * kx), sy.per_point(grad_cham * ky)   # grad_cham: () or (N,)
        grad_x, grad_y = ops.chamfer_backward(x, sx.first, sx.num, y, sy.first, sy.num, idx_xy, idx_yx, gx, gy, want_x, want_y)
        return (sx.unpack_grad(grad_x) if want_x else None, sy.unpack_grad(grad_y) if want_y else None, None, None, None, None, None)


class _MeshSide:
    """The meshes of `point_mesh_face_distance` as packed arrays: ``verts`` (V,3) is the tensor autograd sees, ``faces``
    (F,3) holds packed vertex ids, ``first`` / ``num`` (N,) the faces of every mesh."""

    def __init__(self, meshes):
        if isinstance(meshes, (tuple, list)) and len(meshes) == 2 and isinstance(meshes[0], (tuple, list)):
            verts_list, faces_list = meshes
            if len(verts_list) != len(faces_list) or len(verts_list) == 0:
                raise ValueError("point_mesh_face_distance: (verts, faces) must be two lists of equal, non-zero length")
            self.sizes = [int(f.shape[0]) for f in faces_list]
            self.verts = torch.cat(list(verts_list), 0)
            starts, run = [], 0
            for v in verts_list:
                starts.append(run)
                run += int(v.shape[0])
            self.faces = torch.cat([f.to(torch.int64) + s for f, s in zip(faces_list, starts)], 0)
        elif hasattr(meshes, "verts_packed") and hasattr(meshes, "faces_packed"):
            self.verts, self.faces = meshes.verts_packed(), meshes.faces_packed().to(torch.int64)
            if hasattr(meshes, "faces_list"):   # host-side sizes: no device synchronisation
                self.sizes = [int(f.shape[0]) for f in meshes.faces_list()]
            else:                               # (an object without host-side sizes costs one host read per call)
                self.sizes = [int(v) for v in meshes.num_faces_per_mesh().tolist()]
        else:
            raise ValueError("point_mesh_face_distance: meshes must offer pytorch3d's packed accessors or be a (verts, faces) "
                             "pair of lists")
        if len(self.sizes) == 0 or any(s <= 0 for s in self.sizes) or self.verts.shape[0] == 0:
            raise ValueError("point_mesh_face_distance: an empty mesh (faces %s, %d vertices): its mean distance is undefined"
                             % (self.sizes, self.verts.shape[0]))
        dev = self.verts.device
        if hasattr(meshes, "mesh_to_faces_packed_first_idx"):
            self.first, self.num = meshes.mesh_to_faces_packed_first_idx().to(torch.int64), meshes.num_faces_per_mesh().to(torch.int64)
        else:
            first, run = [], 0
            for s in self.sizes:
                first.append(run)
                run += s
            self.first = torch.tensor(first, dtype=torch.int64, device=dev)
            self.num = torch.tensor(self.sizes, dtype=torch.int64, device=dev)
        self.F = sum(self.sizes)


class _PointMeshFace(autograd.Function):
    """Both searches and the reductions as ONE node; backward = dss_mesh_distance_backward."""

    @staticmethod
    def forward(ctx, p_src, verts, sp, sm):
        pts, v = sp.pack(p_src.detach()), verts.detach().contiguous()
        d2p, idx_pf = ops.point_face_distance(pts, sp.first, sp.num, v, sm.faces, sm.first, sm.num)
        d2f, idx_fp = ops.face_point_distance(pts, sp.first, sp.num, v, sm.faces, sm.first, sm.num)
        N = len(sp.sizes)
        kp = 1.0 / (sp.num.to(pts.dtype) * N)     # d loss / d (squared distance of a point of cloud n)
        kf = 1.0 / (sm.num.to(pts.dtype) * N)
        cp = sp.per_point(kp)
        cf = torch.repeat_interleave(kf, sm.num, output_size=sm.F)
        loss = (d2p * cp).sum() + (d2f * cf).sum()
        ctx.save_for_backward(pts, v, idx_pf, idx_fp, cp, cf)
        ctx.sides = (sp, sm)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        pts, v, idx_pf, idx_fp, cp, cf = ctx.saved_tensors
        sp, sm = ctx.sides
        want_p, want_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gp, gv = ops.mesh_distance_backward(pts, sp.first, sp.num, v, sm.faces, sm.first, sm.num, idx_pf, idx_fp,
                                            grad_loss * cp, grad_loss * cf, want_p, want_v)
        return (sp.unpack_grad(gp) if want_p else None, gv if want_v else None, None, None)


def point_mesh_face_distance(meshes, pcls, min_triangle_area=None):
    """``pytorch3d.loss.point_mesh_face_distance`` on the HIP path: for cloud n against mesh n,
    ``sum_p d2_p / (|cloud(p)| N) + sum_f d2_f / (|mesh(f)| N)`` with d2_p the squared distance of a point to its nearest
    face (``dss_point_face_distance``) and d2_f of a face to its nearest point (``dss_face_point_distance``), under the one
    distance of include/dss_hip.h.  One autograd node, differentiable w.r.t. the points and the vertices (face assignment
    held constant, deterministic).

    ``meshes``: any object with pytorch3d's ``verts_packed() / faces_packed() / mesh_to_faces_packed_first_idx() /
    num_faces_per_mesh()`` (``faces_packed()`` already holds packed vertex ids, so the two vertex accessors
    ``mesh_to_verts_packed_first_idx() / num_verts_per_mesh()`` are not read; ``faces_list()``, when offered, spares a host
    read of the sizes), or a ``(verts, faces)`` pair of lists (faces then hold mesh-local vertex ids).  ``pcls``: a `dss_amd.cloud.PointClouds3D` or a padded (N,P,3) tensor, as in
    `chamfer_distance`.  An empty cloud or mesh raises ValueError.  ``min_triangle_area`` is accepted and ignored: the
    distance treats a degenerate triangle as the union of its edges and needs no threshold (pytorch3d's absolute 5e-3
    turns small valid triangles into edge sets)."""
    del min_triangle_area
    sm = _MeshSide(meshes)
    try:
        sp = _ChamferSide(pcls, None, None, "pcls")
    except ValueError as e:
        raise ValueError(str(e).replace("chamfer_distance", "point_mesh_face_distance"))
    if len(sp.sizes) != len(sm.sizes):
        raise ValueError("point_mesh_face_distance: %d clouds against %d meshes" % (len(sp.sizes), len(sm.sizes)))
    return _PointMeshFace.apply(sp.src, sm.verts, sp, sm)


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                     batch_reduction="mean", point_reduction: str = "mean"):
    """``pytorch3d.loss.chamfer_distance`` -- the 3-D metric of `Trainer.evaluate_3d` (trainer.py:144-171,
    ``chamfer_distance(target, model)`` -> ``chamfer_point``, ``chamfer_normal``) -- on the HIP path: both nearest-point
    searches (``dss_nearest_points``), the gather of the neighbours' normals and the backward (``dss_chamfer_backward``).

    ``x``, ``y``: padded float32 (N,P,3) tensors with optional ``*_lengths`` (N,) and ``*_normals`` (N,P,3), or
    `dss_amd.cloud.PointClouds3D` (lengths and normals then come from the clouds).  ``weights`` (N,), ``batch_reduction`` in
    ("mean", "sum", None), ``point_reduction`` in ("mean", "sum") as in pytorch3d.  Returns ``(cham_dist, cham_normals)``;
    ``cham_normals`` = mean of 1 - |cos| between a point's normal and its nearest neighbour's (eps 1e-6), None unless both
    sides have normals.  One autograd node: ``cham_dist`` is differentiable w.r.t. the points of x and y (index lists held
    constant, deterministic), ``cham_normals`` carries no graph.  An empty cloud on either side raises ValueError."""
    if batch_reduction is not None and batch_reduction not in ("mean", "sum"):
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    sx, sy = _ChamferSide(x, x_lengths, x_normals, "x"), _ChamferSide(y, y_lengths, y_normals, "y")
    N = len(sx.sizes)
    if len(sy.sizes) != N:
        raise ValueError("y does not have the correct shape.")
    if weights is not None:
        if weights.size(0) != N:
            raise ValueError("weights must be of shape (N,).")
        if not (weights >= 0).all():
            raise ValueError("weights cannot be negative.")
        if weights.sum() == 0.0:   # pytorch3d: a zero that keeps the graph
            per_cloud = torch.stack([c.sum() for c in sx.pack(sx.src).split(sx.sizes)]) * weights.reshape(N)
            zero = (per_cloud.sum() if batch_reduction is not None else per_cloud) * 0.0
            return zero, zero
    return _Chamfer.apply(sx.src, sy.src, sx, sy, weights, batch_reduction, point_reduction)
