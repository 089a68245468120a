"""Operators on packed triangle meshes.  Between packed clouds and packed meshes: the nearest face of mesh n for every point of cloud n
(``dss_point_face_distance``), the nearest point of cloud n for every face of mesh n (``dss_face_point_distance``) and the
gradient of both (``dss_mesh_distance_backward``) -- the p2f columns of the reference's evaluation row
(scripts/evaluatePointClouds.py:52,103-132) and ``pytorch3d.loss.point_mesh_face_distance``.  The distance is defined once
in include/dss_hip.h.  Re-exported by `dss_amd.ops`; written like `cross_cloud.py` and entering the library the same way,
through `_lib.call`: tensors checked by `_lib.require_gpu`, no CPU fallback.

Meshes to target images (``dss_rasterize_meshes``, ``dss_mesh_flat_shade``): `rasterize_meshes`, `shade_mesh_flat` -- the
hard rasteriser and the flat shader of the reference's data script (scripts/create_mvr_data_from_mesh.py:148-219), forward
only, under the coverage and depth rule stated once in include/dss_hip.h.

Points on a mesh's surface (``dss_sample_mesh_surface``, ``dss_mesh_sample_backward``): `sample_mesh_surface`,
`mesh_sample_backward` -- the area-weighted sampler of that script's ground-truth cloud (:174-181), under the rule stated
once in include/dss_hip.h: integer area keys and a counter-based generator, so a result is a function of the inputs and
the seed alone.
"""
import torch

from . import _lib
from .cross_cloud import packed_cloud_ids

_f32, _i64 = torch.float32, torch.int64
_on_device = _lib.on_device
_NO_KEY = torch.iinfo(_i64).max


def _gpu(dtype, **tensors):
    return [_lib.require_gpu(t, name, dtype) for name, t in tensors.items()]


def _mesh_inputs(points, p_first, p_num, verts, faces, f_first, f_num):
    """What the three entries share: the seven checked tensors, N, P, V, F and the device."""
    points, verts = _gpu(_f32, points=points, verts=verts)
    pf, pn, faces, ff, fn = _gpu(_i64, p_first=p_first, p_num=p_num, faces=faces, f_first=f_first, f_num=f_num)
    N = pf.shape[0]
    if (points.dim() != 2 or verts.dim() != 2 or faces.dim() != 2 or points.shape[1] != 3 or verts.shape[1] != 3 or faces.shape[1] != 3
            or pf.dim() != 1 or pn.shape != pf.shape or ff.shape != pf.shape or fn.shape != pf.shape
            or verts.device != points.device or faces.device != points.device):
        raise RuntimeError("points (P,3), verts (V,3) float32 and faces (F,3) int64 on one device, with as many meshes (%s) as "
                           "clouds (%d)" % (tuple(ff.shape), N))
    return points, pf, pn, verts, faces, ff, fn, N, points.shape[0], verts.shape[0], faces.shape[0], points.device


def point_face_distance(points, p_first, p_num, verts, faces, f_first, f_num):
    """Nearest face of mesh n for every point of cloud n -> (d2 (P,) squared distance, idx (P,) int64 mesh-local face id;
    ties to the smaller id).  ``faces`` holds PACKED vertex ids.  A point of no cloud, a point with a NaN position and a
    point whose mesh has no usable face get (0, -1); a face with a vertex id outside [0, V) or a non-finite vertex is
    absent.  Exact grid search over the centroids in HIP (``dss_point_face_distance``)."""
    points, pf, pn, verts, faces, ff, fn, N, P, V, F, dev = _mesh_inputs(points, p_first, p_num, verts, faces, f_first, f_num)
    with _on_device(dev):
        d2 = torch.empty((P,), dtype=_f32, device=dev)
        idx = torch.empty((P,), dtype=_i64, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_point_face_workspace(N, F))
        _lib.call("dss_point_face_distance", dev, points, pf, pn, P, verts, V, faces, ff, fn, F, N, d2, idx, ws, ws.numel())
    return d2, idx


def face_point_distance(points, p_first, p_num, verts, faces, f_first, f_num):
    """Nearest point of cloud n for every face of mesh n, under the same distance -> (d2 (F,), idx (F,) int64 cloud-local
    point id; ties to the smaller id).  A face of no mesh, an absent face and a face whose cloud has no usable point get
    (0, -1).  One wavefront per face over the cloud's point grid (``dss_face_point_distance``)."""
    points, pf, pn, verts, faces, ff, fn, N, P, V, F, dev = _mesh_inputs(points, p_first, p_num, verts, faces, f_first, f_num)
    with _on_device(dev):
        d2 = torch.empty((F,), dtype=_f32, device=dev)
        idx = torch.empty((F,), dtype=_i64, device=dev)
        ws = _lib.workspace(dev, _lib.load().dss_nearest_workspace(N, P))
        _lib.call("dss_face_point_distance", dev, points, pf, pn, P, verts, V, faces, ff, fn, F, N, d2, idx, ws, ws.numel())
    return d2, idx


def _pair_targets(idx, own_first, own_num, target_first, n_target):
    """Packed id on the other side that every slot of one side names -> (own,) int64, -1 where there is none."""
    cloud = packed_cloud_ids(own_first, own_num, idx.shape[0])
    tgt = target_first[cloud.clamp(min=0)] + idx
    return torch.where((cloud >= 0) & (idx >= 0) & (tgt >= 0) & (tgt < n_target), tgt, torch.full_like(tgt, -1))


def mesh_distance_orders(faces, V, idx_pf, idx_fp, p_first, p_num, f_first, f_num, want_points=True, want_verts=True):
    """The two contributor lists of ``dss_mesh_distance_backward`` (stable `torch.sort` of int64 keys, as
    `cross_cloud.chamfer_order`): ``order_f`` (F,) = the packed face ids by (packed id of their point, own id);
    ``order_v`` (3 (P + F),) = the entries 3 pair + corner by (packed id of the vertex at that corner, entry)."""
    P, F = idx_pf.shape[0], idx_fp.shape[0]
    point_of_face = _pair_targets(idx_fp, f_first, f_num, p_first, P)
    order_f = order_v = None
    if want_points:
        order_f = torch.sort(torch.where(point_of_face >= 0, point_of_face, torch.full_like(point_of_face, _NO_KEY)),
                             stable=True).indices
    if want_verts:
        face_of_point = _pair_targets(idx_pf, p_first, p_num, f_first, F)
        pair_face = torch.cat([face_of_point, torch.where(point_of_face >= 0, torch.arange(F, dtype=_i64, device=faces.device),
                                                          torch.full_like(point_of_face, -1))])
        if F > 0:
            vid = faces[pair_face.clamp(min=0)]                     # (P + F, 3); rows of pairs that do not exist are masked below
        else:
            vid = torch.full((P, 3), -1, dtype=_i64, device=faces.device)
        key = torch.where((pair_face >= 0)[:, None] & (vid >= 0) & (vid < V), vid, torch.full_like(vid, _NO_KEY))
        order_v = torch.sort(key.reshape(-1), stable=True).indices
    return order_f, order_v


def mesh_distance_backward(points, p_first, p_num, verts, faces, f_first, f_num, idx_pf, idx_fp, g_p, g_f,
                           want_points: bool = True, want_verts: bool = True):
    """Gradient of the two searches (``dss_mesh_distance_backward``) with their index lists (`point_face_distance`:
    ``idx_pf``, `face_point_distance`: ``idx_fp``) held constant, ``g_p`` (P,) / ``g_f`` (F,) = d loss / d squared
    distance -> (grad_points (P,3) or None, grad_verts (V,3) or None), fully written, bitwise reproducible (no atomics:
    see `mesh_distance_orders`)."""
    points, pf, pn, verts, faces, ff, fn, N, P, V, F, dev = _mesh_inputs(points, p_first, p_num, verts, faces, f_first, f_num)
    idx_pf, idx_fp = _gpu(_i64, idx_pf=idx_pf, idx_fp=idx_fp)
    g_p, g_f = _gpu(_f32, g_p=g_p, g_f=g_f)
    if idx_pf.shape != (P,) or g_p.shape != (P,) or idx_fp.shape != (F,) or g_f.shape != (F,):
        raise RuntimeError("mesh_distance_backward: idx_pf, g_p (P,) and idx_fp, g_f (F,) with P=%d F=%d" % (P, F))
    with _on_device(dev):
        order_f, order_v = mesh_distance_orders(faces, V, idx_pf, idx_fp, pf, pn, ff, fn, want_points, want_verts)
        grad_points = torch.empty((P, 3), dtype=_f32, device=dev) if want_points else None
        grad_verts = torch.empty((V, 3), dtype=_f32, device=dev) if want_verts else None
        _lib.call("dss_mesh_distance_backward", dev, points, pf, pn, P, verts, V, faces, ff, fn, F, N, idx_pf, idx_fp, order_f,
                  order_v, g_p, g_f, grad_points, grad_verts)
    return grad_points, grad_verts


def _mesh_cameras(who, verts, faces, f_first, f_num, N, shared_mesh):
    verts, = _gpu(_f32, verts=verts)
    faces, ff, fn = _gpu(_i64, faces=faces, f_first=f_first, f_num=f_num)
    if (verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or ff.dim() != 1 or fn.shape != ff.shape
            or ff.shape[0] != (1 if shared_mesh else N) or faces.device != verts.device):
        raise RuntimeError("%s: verts (V,3) float32 and faces (F,3) int64 on one device, f_first / f_num (%s,), got %s"
                           % (who, "1" if shared_mesh else "N=%d" % N, tuple(ff.shape)))
    return verts, faces, ff, fn


def _one_device(who, dev, **tensors):
    """the entry dereferences every pointer on `dev`: a tensor of another GPU is refused here"""
    for name, t in tensors.items():
        if t.device != dev:
            raise RuntimeError("%s: %s is on %s, verts on %s" % (who, name, t.device, dev))


def rasterize_meshes(verts, faces, f_first, f_num, M, V, znear, zfar, cam_center, image_size: int, shared_mesh: bool = True,
                     cull_backfaces: bool = False):
    """Hard rasterisation of packed meshes for N cameras (``dss_rasterize_meshes``) -> ``pix_to_face`` (N,S,S) int64 =
    the mesh-local id of the nearest covering face or -1, ``zbuf`` (N,S,S) its view depth or -1, ``bary`` (N,S,S,3) its
    perspective-correct barycentrics or 0, ``screen_verts`` (N,V,3) = (NDC x, NDC y, view z) of every vertex under every
    camera.  ``faces`` holds PACKED vertex ids; ``shared_mesh``: f_first / f_num (1,), all cameras see that one mesh,
    otherwise (N,) and camera n sees mesh n.  ``M`` / ``V`` (N,4,4) are the full projection and world-to-view matrices
    (row-vector convention), ``cam_center`` (N,3) is read for ``cull_backfaces`` only.  Inclusive edges, ties to the
    smaller id, no clipping: the rule of include/dss_hip.h, bitwise reproducible."""
    M, V, znear, zfar, cam_center = _gpu(_f32, M=M, V=V, znear=znear, zfar=zfar, cam_center=cam_center)
    N, S = M.shape[0], int(image_size)
    if M.shape != (N, 4, 4) or V.shape != (N, 4, 4) or znear.shape != (N,) or zfar.shape != (N,) or cam_center.shape != (N, 3):
        raise RuntimeError("rasterize_meshes: M, V (N,4,4), znear, zfar (N,), cam_center (N,3) with N=%d" % N)
    verts, faces, ff, fn = _mesh_cameras("rasterize_meshes", verts, faces, f_first, f_num, N, shared_mesh)
    _one_device("rasterize_meshes", verts.device, f_first=ff, f_num=fn, M=M, V=V, znear=znear, zfar=zfar, cam_center=cam_center)
    nV, nF, dev = verts.shape[0], faces.shape[0], verts.device
    with _on_device(dev):
        nbytes = _lib.load().dss_mesh_raster_workspace(N, nF, nV, S)
        if nbytes == 0:
            _lib.check(-1, "dss_mesh_raster_workspace")
        pix_to_face = torch.empty((N, S, S), dtype=_i64, device=dev)
        zbuf = torch.empty((N, S, S), dtype=_f32, device=dev)
        bary = torch.empty((N, S, S, 3), dtype=_f32, device=dev)
        screen_verts = torch.empty((N, nV, 3), dtype=_f32, device=dev)
        ws = _lib.workspace(dev, nbytes)
        _lib.call("dss_rasterize_meshes", dev, verts, nV, faces, ff, fn, nF, M, V, znear, zfar, cam_center, N, int(shared_mesh),
                  int(cull_backfaces), S, pix_to_face, zbuf, bary, screen_verts, ws, ws.numel())
    return pix_to_face, zbuf, bary, screen_verts


def shade_mesh_flat(pix_to_face, bary, verts, faces, f_first, f_num, cam_center, ambient, diffuse_color, specular_color,
                    light_vec, point_lights: bool, shininess: float = 64.0, background=(1.0, 1.0, 1.0), face_colors=None,
                    shared_mesh: bool = True):
    """Flat shading of `rasterize_meshes`' fragments (``dss_mesh_flat_shade``) -> ``rgba`` (N,S,S,4): on a covered pixel
    ``colour * (ambient + diffuse) + specular`` of ``dss_phong_forward``'s formula at the interpolated world position with
    the face normal normalize((B - A) x (C - A)), alpha 1; elsewhere ``background`` and alpha 0.  ``ambient`` (N,3),
    ``diffuse_color`` / ``specular_color`` / ``light_vec`` (N,L,3) as `phong_forward` takes them; ``face_colors`` (F,3)
    per packed face, default white.  Colours are not clamped."""
    pix_to_face, = _gpu(_i64, pix_to_face=pix_to_face)
    bary, cam_center, ambient, kd, ks, lv = _gpu(_f32, bary=bary, cam_center=cam_center, ambient=ambient,
                                                 diffuse_color=diffuse_color, specular_color=specular_color, light_vec=light_vec)
    N, S = pix_to_face.shape[0], pix_to_face.shape[-1]
    L = kd.shape[1] if kd.dim() == 3 else -1
    if (pix_to_face.shape != (N, S, S) or bary.shape != (N, S, S, 3) or cam_center.shape != (N, 3) or ambient.shape != (N, 3)
            or kd.shape != (N, L, 3) or ks.shape != (N, L, 3) or lv.shape != (N, L, 3)):
        raise RuntimeError("shade_mesh_flat: pix_to_face (N,S,S), bary (N,S,S,3), cam_center, ambient (N,3), light tensors "
                           "(N,L,3) with N=%d" % N)
    verts, faces, ff, fn = _mesh_cameras("shade_mesh_flat", verts, faces, f_first, f_num, N, shared_mesh)
    _one_device("shade_mesh_flat", verts.device, f_first=ff, f_num=fn, pix_to_face=pix_to_face, bary=bary, cam_center=cam_center,
                ambient=ambient, diffuse_color=kd, specular_color=ks, light_vec=lv)
    if face_colors is not None:
        face_colors, = _gpu(_f32, face_colors=face_colors)
        if face_colors.shape != (faces.shape[0], 3):
            raise RuntimeError("shade_mesh_flat: face_colors must be (F,3)")
        _one_device("shade_mesh_flat", verts.device, face_colors=face_colors)
    bg = [float(c) for c in background]
    if len(bg) != 3:
        raise RuntimeError("shade_mesh_flat: background must have 3 components")
    dev = verts.device
    with _on_device(dev):
        rgba = torch.empty((N, S, S, 4), dtype=_f32, device=dev)
        _lib.call("dss_mesh_flat_shade", dev, pix_to_face, bary, verts, verts.shape[0], faces, ff, fn, faces.shape[0], face_colors,
                  N, int(shared_mesh), S, ambient, kd, ks, lv, L, int(bool(point_lights)), cam_center, float(shininess), *bg, rgba)
    return rgba


def _sample_meshes(who, faces, f_first, f_num):
    faces, ff, fn = _gpu(_i64, faces=faces, f_first=f_first, f_num=f_num)
    if faces.dim() != 2 or faces.shape[1] != 3 or ff.dim() != 1 or fn.shape != ff.shape:
        raise RuntimeError("%s: faces (F,3) int64, f_first / f_num (N,), got %s, %s, %s" % (who, tuple(faces.shape), tuple(ff.shape),
                                                                                           tuple(fn.shape)))
    _one_device(who, faces.device, f_first=ff, f_num=fn)
    return faces, ff, fn


def sample_mesh_surface(verts, faces, f_first, f_num, num_samples: int, seed: int, want_normals: bool = True,
                        want_bary: bool = True):
    """``num_samples`` area-weighted random points of every mesh of a packed batch (``dss_sample_mesh_surface``) ->
    ``points`` (N,S,3), ``normals`` (N,S,3) = the unit normal (B - A) x (C - A) of the sample's face or None, ``face_idx``
    (N,S) int64 mesh-local, ``bary`` (N,S,3) the weights of the face's three corners or None.  ``faces`` holds PACKED vertex
    ids.  Philox4x32-10 on (sample, mesh) under the 64-bit ``seed`` and integer area keys: the rule of include/dss_hip.h, a
    function of the inputs and the seed alone, bitwise reproducible.  A face with a bad vertex id or a non-finite vertex is
    absent and a face below 2^-32 of its mesh's largest is never drawn; a mesh with nothing to sample gets points, normals
    and bary 0 and face_idx -1."""
    verts, = _gpu(_f32, verts=verts)
    faces, ff, fn = _sample_meshes("sample_mesh_surface", faces, f_first, f_num)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError("sample_mesh_surface: verts must be (V,3), got %s" % (tuple(verts.shape),))
    _one_device("sample_mesh_surface", verts.device, faces=faces)
    N, S, V, F, dev = ff.shape[0], int(num_samples), verts.shape[0], faces.shape[0], verts.device
    if S < 0:
        raise RuntimeError("sample_mesh_surface: num_samples must not be negative, got %d" % S)
    with _on_device(dev):
        if N == 0 or S == 0 or F == 0:   # nothing to launch: the rows of a mesh with nothing to sample are made here
            points = torch.zeros((N, S, 3), dtype=_f32, device=dev)
            normals = torch.zeros((N, S, 3), dtype=_f32, device=dev) if want_normals else None
            bary = torch.zeros((N, S, 3), dtype=_f32, device=dev) if want_bary else None
            return points, normals, torch.full((N, S), -1, dtype=_i64, device=dev), bary
        nbytes = _lib.load().dss_mesh_sample_workspace(N, F)
        if nbytes == 0:
            _lib.check(-1, "dss_mesh_sample_workspace")
        points = torch.empty((N, S, 3), dtype=_f32, device=dev)
        normals = torch.empty((N, S, 3), dtype=_f32, device=dev) if want_normals else None
        face_idx = torch.empty((N, S), dtype=_i64, device=dev)
        bary = torch.empty((N, S, 3), dtype=_f32, device=dev) if want_bary else None
        ws = _lib.workspace(dev, nbytes)
        _lib.call("dss_sample_mesh_surface", dev, verts, V, faces, ff, fn, F, N, S, int(seed) & 0xFFFFFFFFFFFFFFFF, points, normals,
                  face_idx, bary, ws, ws.numel())
    return points, normals, face_idx, bary


def mesh_sample_order(faces, f_first, f_num, V, face_idx):
    """The contributor list of ``dss_mesh_sample_backward`` (stable `torch.sort` of int64 keys, as `mesh_distance_orders`):
    the entries 3 (n S + s) + corner by (packed id of the vertex at that corner, entry), entries of no face last."""
    F = faces.shape[0]
    f = f_first[:, None] + face_idx
    ok = (face_idx >= 0) & (face_idx < f_num[:, None]) & (f >= 0) & (f < F)
    if F > 0:
        vid = faces[f.clamp(min=0, max=F - 1)]                      # (N,S,3); rows of samples without a face are masked below
    else:
        vid = torch.full(tuple(face_idx.shape) + (3,), -1, dtype=_i64, device=faces.device)
    key = torch.where(ok[..., None] & (vid >= 0) & (vid < V), vid, torch.full_like(vid, _NO_KEY))
    return torch.sort(key.reshape(-1), stable=True).indices


def mesh_sample_backward(faces, f_first, f_num, V: int, face_idx, bary, g_points):
    """Gradient of `sample_mesh_surface`'s points w.r.t. the vertices (``dss_mesh_sample_backward``) with ``face_idx`` and
    ``bary`` held constant, ``g_points`` (N,S,3) = d loss / d points -> grad_verts (V,3), fully written, bitwise
    reproducible (no atomics: see `mesh_sample_order`).  The normals carry no gradient."""
    faces, ff, fn = _sample_meshes("mesh_sample_backward", faces, f_first, f_num)
    face_idx, = _gpu(_i64, face_idx=face_idx)
    bary, g_points = _gpu(_f32, bary=bary, g_points=g_points)
    N, V, dev = ff.shape[0], int(V), faces.device
    S = face_idx.shape[1] if face_idx.dim() == 2 else -1
    if face_idx.shape != (N, S) or bary.shape != (N, S, 3) or g_points.shape != (N, S, 3) or V < 0:
        raise RuntimeError("mesh_sample_backward: face_idx (N,S), bary and g_points (N,S,3) with N=%d, V >= 0" % N)
    _one_device("mesh_sample_backward", dev, face_idx=face_idx, bary=bary, g_points=g_points)
    with _on_device(dev):
        if N == 0 or V == 0 or S == 0 or faces.shape[0] == 0:
            return torch.zeros((V, 3), dtype=_f32, device=dev)
        order = mesh_sample_order(faces, ff, fn, V, face_idx)
        grad_verts = torch.empty((V, 3), dtype=_f32, device=dev)
        _lib.call("dss_mesh_sample_backward", dev, faces, ff, fn, faces.shape[0], N, S, V, face_idx, bary, order, g_points, grad_verts)
    return grad_verts
