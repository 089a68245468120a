"""CPU: differentiable cameras -- the matrix caches never serve a freed autograd graph, the fp64 reference of the camera
gradients agrees with torch.autograd, and the two new entry points validate their arguments without a device."""
import ctypes
import math

import pytest
import torch

import camera_reference as cref
from dss_amd import _lib
from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform


def _cams(R, T, fov):
    return FoVPerspectiveCameras(znear=0.1, zfar=50.0, fov=fov, R=R, T=T)


def _camera_loss(cams, pts):
    return ((cams.get_full_projection_transform().get_matrix() ** 2).sum()
            + cams.get_world_to_view_transform().get_matrix().sum()
            + cams.get_camera_center().sum() + cams.transform_points(pts).sum())


def test_two_iterations_on_differentiable_cameras():
    """Training iterations on one camera object whose R, T, fov require grad: every backward() succeeds and the gradients
    are those of freshly built cameras (the cached matrices used to carry the first iteration's graph: "Trying to backward
    through the graph a second time")."""
    R0, T0 = look_at_view_transform(2.0, [20.0, -35.0], [40.0, 130.0])
    R, T = R0.clone().requires_grad_(True), T0.clone().requires_grad_(True)
    fov = torch.tensor([60.0, 45.0], requires_grad=True)
    cams = _cams(R, T, fov)
    pts = torch.randn(7, 3, generator=torch.Generator().manual_seed(0)) * 0.3
    for it in range(3):
        for t in (R, T, fov):
            t.grad = None
        _camera_loss(cams, pts).backward()
        Rf, Tf, ff = (t.detach().clone().requires_grad_(True) for t in (R, T, fov))
        _camera_loss(_cams(Rf, Tf, ff), pts).backward()
        for a, b in ((R, Rf), (T, Tf), (fov, ff)):
            assert a.grad is not None and torch.equal(a.grad, b.grad), it
        if it == 1:
            # (iterations 0 and 1 see the same tensors at the same versions -- the case the caches used to serve with a
            # freed graph; an optimiser step in place bumps the versions, which always rebuilt the matrices)
            with torch.no_grad():
                T -= 0.01 * T.grad
                fov -= 0.01 * fov.grad


def test_cameras_without_grad_keep_their_matrix_cache():
    R, T = look_at_view_transform(2.0, 30.0, 45.0)
    cams = _cams(R, T, 60.0)
    for get in (cams.get_full_projection_transform, cams.get_world_to_view_transform, cams.get_projection_transform):
        assert get() is get()
    # differentiable cameras under no_grad are cached too (nothing to differentiate), and not served when grad is on
    Rg = R.clone().requires_grad_(True)
    cg = _cams(Rg, T, 60.0)
    with torch.no_grad():
        a = cg.get_full_projection_transform()
        assert cg.get_full_projection_transform() is a and not a.get_matrix().requires_grad
    b = cg.get_full_projection_transform()
    assert b is not a and b.get_matrix().requires_grad


def _random_case(N, sizes, shared, seed):
    g = torch.Generator().manual_seed(seed)
    R, T = look_at_view_transform(2.2, [10.0 + 17 * k for k in range(N)], [30.0 + 50 * k for k in range(N)])
    cams = _cams(R, T, 60.0)
    M = cams.get_full_projection_transform().get_matrix().double()
    V = cams.get_world_to_view_transform().get_matrix().double()
    Pw = sizes[0] if shared else sum(sizes)
    world = (torch.rand(Pw, 3, generator=g, dtype=torch.float64) - 0.5)
    num = torch.tensor(sizes, dtype=torch.int64)
    first = torch.cumsum(num, 0) - num
    P = int(num.sum())
    grad = torch.randn(P, 3, generator=g, dtype=torch.float64) * 0.05
    valid = torch.rand(P, generator=g) > 0.33
    return world, M, V, first, num, grad, valid, cams


@pytest.mark.parametrize("shared,clip", [(False, -1.0), (False, 0.05), (True, -1.0), (True, 0.05)])
def test_reference_closed_forms_match_autograd(shared, clip):
    N = 3
    sizes = [41] * N if shared else [41, 0, 17]
    world, M, V, first, num, grad, valid, _ = _random_case(N, sizes, shared, 1)
    gM, gV, aM, aV = cref.camera_backward(world, M, V, first, num, grad, valid, shared, clip)
    rM, rV = cref.camera_backward_autograd(world, M, V, first, num, grad, valid, shared, clip)
    assert (gM - rM).abs().max() <= 1e-13 * aM.max() and (gV - rV).abs().max() <= 1e-13 * aV.max()
    assert gM[:, :, 2].abs().max() == 0 and gV[:, :, [0, 1, 3]].abs().max() == 0
    assert (aM >= gM.abs() - 1e-15).all() and (aV >= gV.abs() - 1e-15).all()
    if not shared:
        assert gM[1].abs().max() == 0 and gV[1].abs().max() == 0       # the empty cloud


@pytest.mark.parametrize("point_lights", [True, False])
@pytest.mark.parametrize("shared", [True, False])
def test_reference_shading_term_matches_autograd(point_lights, shared):
    N, L = 2, 2
    sizes = [33] * N if shared else [33, 12]
    world, _M, _V, first, num, _g, _v, cams = _random_case(N, sizes, shared, 2)
    g = torch.Generator().manual_seed(3)
    P = int(num.sum())
    normals = torch.randn(world.shape[0], 3, generator=g, dtype=torch.float64)
    rgb = torch.rand(P, 3, generator=g, dtype=torch.float64)
    grad_out = torch.randn(P, 3, generator=g, dtype=torch.float64)
    amb = torch.rand(N, 3, generator=g, dtype=torch.float64)
    kd, ks = (torch.rand(N, L, 3, generator=g, dtype=torch.float64) for _ in range(2))
    lvec = torch.randn(N, L, 3, generator=g, dtype=torch.float64) * 2
    cam = cams.get_camera_center().double()
    shininess = 8.0
    gc, ac = cref.phong_backward_camera(grad_out, world, normals, first, num, ks, lvec, point_lights, cam, shininess, shared)
    rc = cref.phong_backward_camera_autograd(grad_out, world, normals, rgb, first, num, amb, kd, ks, lvec, point_lights, cam,
                                             shininess, shared)
    assert ac.max() > 0 and (gc - rc).abs().max() <= 1e-12 * ac.max()
    z, _ = cref.phong_backward_camera(grad_out, world, normals, first, num, ks * 0, lvec, point_lights, cam, shininess, shared)
    assert z.abs().max() == 0


def test_pose_gradients_reach_R_T_through_the_matrices():
    """grad_M / grad_V of the reference, chained through compose / _world_to_view / _projection by autograd, equal the
    gradients of the projection written directly in R, T (the path `ops.camera_backward`'s outputs take on the GPU)."""
    N, sizes = 2, [25, 25]
    world, _M, _V, first, num, grad, valid, _ = _random_case(N, sizes, True, 4)
    R0, T0 = look_at_view_transform(2.2, [10.0, 27.0], [30.0, 80.0])
    leaves = [t.double().clone().requires_grad_(True) for t in (R0, T0)]
    s = 1.0 / math.tan(math.radians(60.0) / 2)

    def direct(R, T):
        out = []
        for n in range(N):
            v = world[:sizes[n]] @ R[n] + T[n]
            out.append(torch.stack([s * v[:, 0] / v[:, 2], s * v[:, 1] / v[:, 2], v[:, 2]], 1))
        return torch.cat(out)
    (direct(*leaves) * grad * valid[:, None]).sum().backward()
    R, T = (t.detach().float().requires_grad_(True) for t in leaves)
    cams = _cams(R, T, 60.0)
    M = cams.get_full_projection_transform().get_matrix()
    V = cams.get_world_to_view_transform().get_matrix()
    gM, gV, _, _ = cref.camera_backward(world, M.detach(), V.detach(), first, num, grad, valid, True)
    torch.autograd.backward([M, V], [gM.float(), gV.float()])
    assert (R.grad.double() - leaves[0].grad).abs().max() <= 1e-5 * leaves[0].grad.abs().max()
    assert (T.grad.double() - leaves[1].grad).abs().max() <= 1e-5 * leaves[1].grad.abs().max()


def test_entry_points_validate_without_a_device():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)     # never dereferenced: every call below fails before a launch
    sizes = [lib.dss_camera_backward_workspace(n, p) for n in (1, 2, 8) for p in (0, 1, 1000, 32684, 1 << 20, 1 << 25)]
    assert all(s > 0 for s in sizes)
    for n in (1, 8):
        row = [lib.dss_camera_backward_workspace(n, p) for p in (0, 1, 5, 1000, 32684, 99790, 1 << 20, (1 << 20) + 1, 1 << 25)]
        assert row == sorted(row)
    for p in (0, 1000, 1 << 25):
        col = [lib.dss_camera_backward_workspace(n, p) for n in (1, 2, 5, 8, 64)]
        assert col == sorted(col)
    need = lib.dss_camera_backward_workspace(2, 1000)
    cam_args = lambda **kw: [kw.get("world", fake), fake, fake, fake, fake, 2, 500, 1, fake, fake, -1.0,
                             kw.get("grad_M", fake), fake, kw.get("ws", fake), kw.get("nbytes", need), None]
    for kw in (dict(world=None), dict(grad_M=None), dict(ws=None), dict(nbytes=need - 1)):
        assert lib.dss_camera_backward(*cam_args(**kw)) == -1, kw
        assert b"dss_camera_backward" in lib.dss_last_error(), kw
    bad = cam_args()
    bad[5] = 0
    assert lib.dss_camera_backward(*bad) == -1 and b"dss_camera_backward" in lib.dss_last_error()
    ph_args = lambda **kw: [kw.get("grad_out", fake)] + [fake] * 5 + [2, 500, 1] + [fake] * 4 + [1, 1, fake, 64.0,
                            kw.get("grad_cam", fake), kw.get("ws", fake), kw.get("nbytes", need), None]
    for kw in (dict(grad_out=None), dict(grad_cam=None), dict(ws=None), dict(nbytes=need - 1)):
        assert lib.dss_phong_backward_camera(*ph_args(**kw)) == -1, kw
        assert b"dss_phong_backward_camera" in lib.dss_last_error(), kw
