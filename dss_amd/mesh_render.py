"""Target images from a triangle mesh: what the reference's data script renders per view
(scripts/create_mvr_data_from_mesh.py:148-219 -- pytorch3d's MeshRasterizer with blur_radius 0 and HardFlatShader, a hard
mask, a dense depth map with zfar off the surface), on the GPU through `ops.rasterize_meshes` and `ops.shade_mesh_flat`.
Forward only: a target image needs no gradient.  The script's ground-truth cloud (:174-181) is
`dss_amd.mesh_sampling.sample_points_from_meshes`; file formats stay with the caller."""
import torch

from . import ops
from .texture import PointLights


def _mesh_tensors(meshes, N, dev):
    """-> verts (V,3), faces (F,3) packed ids, f_first, f_num, shared"""
    if isinstance(meshes, (tuple, list)):
        verts, faces = meshes
        if not torch.is_tensor(verts) or not torch.is_tensor(faces):
            raise TypeError("render_mesh_targets: (verts, faces) must be tensors")
        f_first = torch.zeros(1, dtype=torch.int64, device=dev)
        f_num = torch.full((1,), faces.shape[0], dtype=torch.int64, device=dev)
        return verts, faces, f_first, f_num, True
    verts, faces = meshes.verts_packed(), meshes.faces_packed()
    f_first, f_num = meshes.mesh_to_faces_packed_first_idx(), meshes.num_faces_per_mesh()
    if f_first.shape[0] == 1:
        return verts, faces, f_first, f_num, True
    if f_first.shape[0] != N:
        raise ValueError("render_mesh_targets: need 1 or %d meshes for %d cameras" % (N, N))
    return verts, faces, f_first, f_num, False


def render_mesh_targets(meshes, cameras, lights, image_size: int = 512, shininess: float = 64, background=(1.0, 1.0, 1.0),
                        face_colors=None, cull_backfaces: bool = False):
    """``meshes`` = (verts (V,3), faces (F,3)) -- one mesh seen by every camera -- or an object with pytorch3d's packed
    accessors (``verts_packed``, ``faces_packed``, ``mesh_to_faces_packed_first_idx``, ``num_faces_per_mesh``) holding 1
    or N meshes; ``cameras``: N `FoVPerspectiveCameras`; ``lights``: `PointLights` or `DirectionalLights` ->

    ``rgba`` (N,S,S,4) float32: flat-shaded colour, unclamped, ``background`` off the surface; alpha = the mask
    ``mask`` (N,S,S) bool, ``depth`` (N,S,S) = view depth, zfar off the mask (the script's ``dense_depths``)
    ``pix_to_face`` (N,S,S) int64, mesh-local, -1 off the mask.
    Everything stays on the device; CPU tensors are refused."""
    N = len(cameras)
    verts = meshes[0] if isinstance(meshes, (tuple, list)) else meshes.verts_packed()
    if not torch.is_tensor(verts) or not verts.is_cuda:
        raise RuntimeError("render_mesh_targets: the mesh is on %s; the HIP path needs GPU tensors (no CPU fallback)"
                           % (verts.device if torch.is_tensor(verts) else type(verts)))
    dev = verts.device
    verts, faces, f_first, f_num, shared = _mesh_tensors(meshes, N, dev)
    cameras, lights = cameras.to(dev), lights.to(dev)
    f32 = lambda t, *shape: t.detach().to(dev, torch.float32).expand(*shape).contiguous()
    M = f32(cameras.get_full_projection_transform().get_matrix(), N, 4, 4)
    V = f32(cameras.get_world_to_view_transform().get_matrix(), N, 4, 4)
    znear, zfar = f32(cameras.znear.reshape(-1), N), f32(cameras.zfar.reshape(-1), N)
    cam = f32(cameras.get_camera_center().reshape(-1, 3), N, 3)
    verts = verts.detach().to(torch.float32).contiguous()
    faces, f_first, f_num = (t.to(dev, torch.int64).contiguous() for t in (faces, f_first, f_num))
    pix_to_face, zbuf, bary, _ = ops.rasterize_meshes(verts, faces, f_first, f_num, M, V, znear, zfar, cam, int(image_size),
                                                      shared_mesh=shared, cull_backfaces=cull_backfaces)
    amb, kd, ks, vec = (t.detach() for t in lights._packed(N))
    rgba = ops.shade_mesh_flat(pix_to_face, bary, verts, faces, f_first, f_num, cam, amb, kd, ks, vec,
                               isinstance(lights, PointLights), float(shininess), background, face_colors, shared_mesh=shared)
    mask = pix_to_face >= 0
    depth = torch.where(mask, zbuf, zfar.view(N, 1, 1).expand_as(zbuf))
    return rgba, mask, depth, pix_to_face
