"""The reference's evaluation row (scripts/evaluatePointClouds.py:52,103-132) for one predicted cloud, on the GPU: chamfer
and Hausdorff distance against a ground-truth cloud (``ops.nearest_points``), mean and spread of the point-to-face
distance against a ground-truth mesh (``ops.point_face_distance``; the reference reads that column from
``*_point2mesh_distance.xyz`` files an outside tool wrote)."""
import torch

from . import ops


def _one_cloud(t, name):
    if hasattr(t, "points_packed"):
        t = t.points_packed()
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("evaluate_cloud: %s must be a (P,3) tensor or a single cloud" % name)
    t = t.detach().to(torch.float32).contiguous()
    if t.shape[0] == 0:
        raise ValueError("evaluate_cloud: %s is empty" % name)
    dev = t.device
    return t, torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), t.shape[0], dtype=torch.int64, device=dev)


def evaluate_cloud(pred, gt_cloud=None, gt_mesh=None, gt_samples=None, seed=0):
    """The reference script's row for ``pred`` (P,3) -> dict of 0-dim device tensors (no host read):

    ``"CD"``         mean squared nearest-point distance pred -> gt plus gt -> pred (with ``gt_cloud`` (Q,3); without one,
                     with ``gt_mesh`` and an int ``gt_samples``, against that many surface samples of the mesh:
                     `ops.sample_mesh_surface` under ``seed``)
    ``"hausdorff"``  the two maxima of those squared distances, SUMMED as evaluatePointClouds.py:114-115 does (a quirk of the
                     script, kept: the textbook Hausdorff distance is their maximum, of unsquared distances)
    ``"p2f avg"``, ``"p2f std"``  mean and population standard deviation of sqrt(d2) from `ops.point_face_distance`
                     (with ``gt_mesh`` = (verts (V,3), faces (F,3)))
    Keys whose ground truth is not given are absent."""
    x, xf, xn = _one_cloud(pred, "pred")
    row = {}
    if gt_cloud is None and gt_mesh is not None and gt_samples is not None:
        verts, faces = gt_mesh
        dev = x.device
        faces = faces.to(torch.int64).contiguous()
        gt_cloud = ops.sample_mesh_surface(verts.detach().to(torch.float32).contiguous(), faces,
                                           torch.zeros(1, dtype=torch.int64, device=dev),
                                           torch.full((1,), faces.shape[0], dtype=torch.int64, device=dev), int(gt_samples),
                                           int(seed), want_normals=False, want_bary=False)[0][0]
    if gt_cloud is not None:
        y, yf, yn = _one_cloud(gt_cloud, "gt_cloud")
        d_xy, _ = ops.nearest_points(x, xf, xn, y, yf, yn)
        d_yx, _ = ops.nearest_points(y, yf, yn, x, xf, xn)
        row["CD"] = d_xy.mean() + d_yx.mean()
        row["hausdorff"] = d_xy.max() + d_yx.max()
    if gt_mesh is not None:
        verts, faces = gt_mesh
        verts = verts.detach().to(torch.float32).contiguous()
        faces = faces.to(torch.int64).contiguous()
        if faces.dim() != 2 or faces.shape[0] == 0:
            raise ValueError("evaluate_cloud: gt_mesh has no face")
        dev = x.device
        ff = torch.zeros(1, dtype=torch.int64, device=dev)
        fn = torch.full((1,), faces.shape[0], dtype=torch.int64, device=dev)
        d2, _ = ops.point_face_distance(x, xf, xn, verts, faces, ff, fn)
        d = d2.sqrt()
        row["p2f avg"] = d.mean()
        row["p2f std"] = d.std(unbiased=False)
    return row
