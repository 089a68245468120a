"""Points and normals on a triangle mesh's surface: the ground-truth cloud of the reference's data script
(scripts/create_mvr_data_from_mesh.py:174-181, ``sample_points_from_meshes(meshes, 20000, return_normals=True)``), the
initial cloud of config.py:179, and the even sample the reference goes to MeshLab for -- on the GPU through
`ops.sample_mesh_surface`, under the rule of include/dss_hip.h: a result is a function of the mesh and a
64-bit seed alone.  CPU tensors are refused."""
import torch
from torch import autograd

from . import ops
from .mesh_render import _mesh_tensors


def _packed_meshes(meshes, who):
    """-> verts (V,3) as given (it may require grad), faces, f_first, f_num (N,) int64 on the device of verts"""
    pair = isinstance(meshes, (tuple, list))
    verts = meshes[0] if pair else meshes.verts_packed()
    if not torch.is_tensor(verts) or not verts.is_cuda:
        raise RuntimeError("%s: the mesh is on %s; the HIP path needs GPU tensors (no CPU fallback)"
                           % (who, verts.device if torch.is_tensor(verts) else type(verts)))
    dev = verts.device
    N = 1 if pair else int(meshes.num_faces_per_mesh().shape[0])
    verts, faces, f_first, f_num, _ = _mesh_tensors(meshes, N, dev)
    faces, f_first, f_num = (t.to(dev, torch.int64).contiguous() for t in (faces, f_first, f_num))
    return verts, faces, f_first, f_num


def _draw_seed(seed, generator):
    """one 63-bit draw on the CPU (no device sync; `torch.manual_seed` governs it) unless a seed is given"""
    if seed is not None:
        return int(seed)
    return int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator, dtype=torch.int64, device="cpu").item())


class _SamplePoints(autograd.Function):
    """`ops.sample_mesh_surface` and `ops.mesh_sample_backward` as one node: face_idx and bary are constants of the
    backward, the normals carry no gradient."""

    @staticmethod
    def forward(ctx, verts, faces, f_first, f_num, num_samples, seed, want_normals):
        points, normals, face_idx, bary = ops.sample_mesh_surface(verts.detach().contiguous(), faces, f_first, f_num, num_samples,
                                                                  seed, want_normals=want_normals, want_bary=True)
        ctx.save_for_backward(faces, f_first, f_num, face_idx, bary)
        ctx.V = verts.shape[0]
        ctx.mark_non_differentiable(face_idx)
        if normals is not None:
            ctx.mark_non_differentiable(normals)
        return points, normals, face_idx

    @staticmethod
    def backward(ctx, g_points, g_normals, g_face_idx):
        if g_points is None:
            return (None,) * 7
        faces, f_first, f_num, face_idx, bary = ctx.saved_tensors
        grad_verts = ops.mesh_sample_backward(faces, f_first, f_num, ctx.V, face_idx, bary, g_points.contiguous())
        return (grad_verts,) + (None,) * 6


def _sample(who, meshes, num_samples, want_normals, seed, generator):
    verts, faces, f_first, f_num = _packed_meshes(meshes, who)
    seed = _draw_seed(seed, generator)
    verts = verts if verts.dtype == torch.float32 else verts.to(torch.float32)
    if verts.requires_grad and torch.is_grad_enabled():
        return _SamplePoints.apply(verts, faces, f_first, f_num, int(num_samples), seed, bool(want_normals))
    points, normals, face_idx, _ = ops.sample_mesh_surface(verts.detach().contiguous(), faces, f_first, f_num, int(num_samples),
                                                           seed, want_normals=want_normals, want_bary=False)
    return points, normals, face_idx


def sample_points_from_meshes(meshes, num_samples: int = 10000, return_normals: bool = False, return_face_idx: bool = False,
                              seed=None, generator=None):
    """``pytorch3d.ops.sample_points_from_meshes`` on the HIP path: ``num_samples`` points of every mesh, drawn uniformly
    over its surface -> ``points`` (N,S,3)[, ``normals`` (N,S,3) unit face normals][, ``face_idx`` (N,S) int64 mesh-local,
    -1 where a mesh has nothing to sample], in pytorch3d's order with ``face_idx`` last.

    ``meshes``: ``(verts (V,3), faces (F,3))`` -- one mesh -- or an object with pytorch3d's packed accessors
    (``verts_packed``, ``faces_packed``, ``mesh_to_faces_packed_first_idx``, ``num_faces_per_mesh``).  ``seed``: the 64-bit
    seed of the rule; None: one 63-bit draw of ``torch.randint`` on the CPU from ``generator`` or torch's default generator,
    so `torch.manual_seed` governs reproducibility and nothing waits for the device.  The same mesh and seed give the same
    bits on every call.  If ``verts`` requires grad the points are differentiable w.r.t. the vertices (face and weights
    held constant, deterministic).  Departures from pytorch3d: the draws are this project's own (same distribution); the
    NORMALS CARRY NO GRADIENT (pytorch3d's face normals are differentiable); an empty mesh or non-finite vertices do
    not raise -- a face that cannot be used is left out, and a mesh with nothing to sample yields zeros."""
    points, normals, face_idx = _sample("sample_points_from_meshes", meshes, num_samples, return_normals, seed, generator)
    out = (points,) + ((normals,) if return_normals else ()) + ((face_idx,) if return_face_idx else ())
    return out[0] if len(out) == 1 else out


def sample_mesh_evenly(meshes, num_samples: int, oversample: int = 5, seed=None, return_normals: bool = False):
    """An even (blue-noise-like) sample of every mesh, the one the reference calls MeshLab for: ``oversample *
    num_samples`` surface samples (`sample_points_from_meshes`), of which `ops.farthest_points` keeps ``num_samples`` ->
    ``points`` (N,num_samples,3)[, ``normals``], in selection order."""
    K, M = int(num_samples), int(oversample) * int(num_samples)
    if K < 0 or int(oversample) < 1:
        raise ValueError("sample_mesh_evenly: num_samples >= 0 and oversample >= 1, got %d, %d" % (K, int(oversample)))
    points, normals, _ = _sample("sample_mesh_evenly", meshes, M, return_normals, seed, None)
    N, dev = points.shape[0], points.device
    first = torch.arange(N, dtype=torch.int64, device=dev) * M
    full = lambda v: torch.full((N,), v, dtype=torch.int64, device=dev)
    keep = ops.farthest_points(points.detach().reshape(N * M, 3), first, full(M), full(K), K_max=K)
    keep = keep.clamp(min=0)[..., None].expand(N, K, 3)
    points = torch.gather(points, 1, keep)
    return (points, torch.gather(normals, 1, keep)) if return_normals else points
