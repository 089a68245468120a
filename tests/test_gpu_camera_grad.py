"""GPU: gradients w.r.t. the cameras -- `ops.camera_backward` / `ops.phong_backward_camera` against the fp64 reference
(`tests/camera_reference.py`), bitwise reproducibility, and the public path (R.grad / T.grad after loss.backward()) tied to
the point gradient that is already pinned to the oracle.

Error bookkeeping of the kernel tests: every output entry is compared with its fp64 value RELATIVE TO ``A = sum_p |term|``
of that entry (the sum itself may cancel); the bar is ``1e-5 * A``, the bar of ``points.grad`` / ``colors.grad`` in
test_gpu_sharded.py.  Each test prints the largest observed ratio."""
import numpy as np
import pytest
import torch

import camera_reference as cref
import scenes
from dss_amd import ops
from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
from dss_amd.cloud import PointClouds3D
from dss_amd.losses import calc_dr_loss
from dss_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting
from dss_amd.renderer import NormWeightedCompositor, SurfaceSplattingRenderer
from dss_amd.texture import DirectionalLights, LightingTexture, PointLights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-5


def _case(sizes, shared, seed, all_invalid=None):
    """random points in a ball in front of N look-at cameras, random screen gradients, about a third of the pairs invalid
    -> CPU tensors (world, M, V, first, num, grad_screen, valid)"""
    N = len(sizes)
    g = torch.Generator().manual_seed(seed)
    R, T = look_at_view_transform(2.2, [10.0 + 17 * k for k in range(N)], [30.0 + 47 * k for k in range(N)])
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T)
    M = cams.get_full_projection_transform().get_matrix().contiguous()
    V = cams.get_world_to_view_transform().get_matrix().contiguous()
    Pw = sizes[0] if shared else sum(sizes)
    world = torch.rand(Pw, 3, generator=g) - 0.5
    num = torch.tensor(sizes, dtype=torch.int64)
    first = torch.cumsum(num, 0) - num
    P = int(num.sum())
    grad = torch.randn(P, 3, generator=g) * 0.05
    valid = torch.rand(P, generator=g) > 0.33
    if all_invalid is not None:
        valid[int(first[all_invalid]):int(first[all_invalid] + num[all_invalid])] = False
    return world, M, V, first, num, grad, valid


def _gpu(*ts):
    return [t.to(DEV) for t in ts]


def _check_camera(case, shared, clip, tag):
    world, M, V, first, num, grad, valid = case
    gM, gV = ops.camera_backward(*_gpu(world, M, V, first, num, grad, valid), shared_cloud=shared, clip=clip)
    rM, rV, aM, aV = cref.camera_backward(world, M, V, first, num, grad, valid, shared, clip)
    worst = 0.0
    for got, ref, A in ((gM, rM, aM), (gV, rV, aV)):
        got = got.cpu().double()
        assert tuple(got.shape) == tuple(ref.shape)
        assert (got[A == 0] == 0).all(), "%s: entries without a term must be exact zeros" % tag
        ratio = ((got - ref).abs()[A > 0] / A[A > 0])
        worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
    print("camera_backward %-34s clip %5.2f: max |err| / A = %.3e" % (tag, clip, worst))
    assert worst <= BAR, (tag, clip, worst)
    return gM, gV


@pytest.mark.parametrize("clip", [-1.0, 0.05])
def test_camera_backward_against_fp64(clip):
    _check_camera(_case([32684], False, 11), False, clip, "1 x 32,684")
    # 99,790 is not a multiple of 64 (nor of 4): wavefronts and 16-byte groups straddle cameras in the packed order
    _check_camera(_case([99790] * 8, True, 12), True, clip, "8 x 99,790 shared")
    gM, gV = _check_camera(_case([1000, 37, 5003, 777, 2501], False, 13, all_invalid=2), False, clip,
                           "5 clouds, one without a valid point")
    assert (gM[2] == 0).all() and (gV[2] == 0).all()
    world, M, V, first, num, grad, valid = _case([0, 0], False, 14)                     # Pw == 0
    gM, gV = ops.camera_backward(*_gpu(world, M, V, first, num, grad, valid), shared_cloud=False, clip=clip)
    assert tuple(gM.shape) == (2, 4, 4) and (gM == 0).all() and (gV == 0).all()


def test_camera_backward_8_x_1m():
    _check_camera(_case([1_000_000] * 8, True, 15), True, 0.05, "8 x 1,000,000 shared")


def test_camera_backward_is_bitwise_reproducible():
    for sizes, shared in (([32684], False), ([99790] * 8, True), ([1000, 37, 5003, 777, 2501], False)):
        world, M, V, first, num, grad, valid = _gpu(*_case(sizes, shared, 21))
        a = ops.camera_backward(world, M, V, first, num, grad, valid, shared_cloud=shared, clip=0.05)
        b = ops.camera_backward(world, M, V, first, num, grad, valid, shared_cloud=shared, clip=0.05)
        # an unrelated launch in between (it also reuses the per-stream workspace for other sizes)
        ops.camera_backward(*_gpu(*_case([4099], False, 22)), shared_cloud=False)
        torch.randn(1 << 20, device=DEV).sum()
        c = ops.camera_backward(world, M, V, first, num, grad, valid, shared_cloud=shared, clip=0.05)
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        # a misaligned view of the same gradients takes the scalar loads: same sums in the same order
        pad = torch.zeros(grad.numel() + 1, device=DEV)
        pad[1:] = grad.reshape(-1)
        d = ops.camera_backward(world, M, V, first, num, pad[1:].view(-1, 3), valid, shared_cloud=shared, clip=0.05)
        assert pad[1:].data_ptr() % 16 != 0 and torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])


def _phong_case(sizes, shared, seed, L=2):
    world, _M, _V, first, num, _g, _v = _case(sizes, shared, seed)
    N = len(sizes)
    g = torch.Generator().manual_seed(seed + 100)
    P = int(num.sum())
    normals = torch.nn.functional.normalize(world + 0.3 * torch.randn(world.shape[0], 3, generator=g), dim=1)
    rgb = torch.rand(P, 3, generator=g)
    grad_out = torch.randn(P, 3, generator=g)
    amb = torch.rand(N, 3, generator=g)
    kd, ks = torch.rand(N, L, 3, generator=g), torch.rand(N, L, 3, generator=g)
    R, T = look_at_view_transform(2.2, [10.0 + 17 * k for k in range(N)], [30.0 + 47 * k for k in range(N)])
    cam = FoVPerspectiveCameras(R=R, T=T).get_camera_center().contiguous()
    # lights around the cameras: the highlights face the viewer, the specular chain carries weight
    lvec = cam[:, None, :] * 1.1 + 0.5 * torch.randn(N, L, 3, generator=g)
    return world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out


@pytest.mark.parametrize("point_lights", [True, False])
@pytest.mark.parametrize("sizes,shared", [([20011] * 3, True), ([30011, 20313, 24000], False)])
def test_phong_backward_camera_against_fp64(sizes, shared, point_lights):
    """Cloud sizes: with shininess 64 a single TERM of this sum is conditioned far worse than the bar.  alpha^63 turns the
    ~3e-7 absolute fp32 rounding of alpha = v^ . r into a relative error of 63 * 3e-7 ~ 2e-5 of the term, whatever kernel
    evaluates it (the kernel restates phong_kernel's fp32 arithmetic on purpose).  The roundings of different pairs are
    independent, so the error of the sum is ~2e-5 * A / sqrt(n_eff), n_eff = the pairs inside the specular lobe (a few
    per cent of a cloud): clouds of >= 20,000 points put the format's own error at ~2e-6 and leave the bar to the
    reduction.  The same formula in plain fp32 torch on the CPU shows the figures: 0.8 - 3.2e-6 at these sizes, 1.8e-5
    (point lights) / 2.8e-5 (directional) for a 313-point cloud -- where the kernel measured 1.9e-5, i.e. the format."""
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = _phong_case(sizes, shared, 31)
    shin = 64.0
    args = _gpu(grad_out, world, normals, rgb, first, num, amb, kd, ks, lvec)
    got = ops.phong_backward_camera(*args, point_lights, cam.to(DEV), shin, shared).cpu().double()
    ref, A = cref.phong_backward_camera(grad_out, world, normals, first, num, ks, lvec, point_lights, cam, shin, shared)
    assert (A > 0).all()
    worst = float(((got - ref).abs() / A).max())
    print("phong_backward_camera %s %s: max |err| / A = %.3e"
          % ("shared" if shared else "per-camera", "point" if point_lights else "directional", worst))
    assert worst <= BAR, worst
    again = ops.phong_backward_camera(*args, point_lights, cam.to(DEV), shin, shared).cpu().double()
    assert torch.equal(got, again)
    args[8] = torch.zeros_like(args[8])                                                  # ks = 0: no specular term
    zero = ops.phong_backward_camera(*args, point_lights, cam.to(DEV), shin, shared)
    assert (zero == 0).all()
    # the same pairs, seen from the points: sum_p gw = - (the camera's share of dss_phong_backward's grad_world) when the
    # lights are directional (no other path from the shading to the positions)
    if not point_lights:
        args[8] = ks.to(DEV)
        gw, _gn, _gc = ops.phong_backward(*args, point_lights, cam.to(DEV), shin, shared)
        assert ((-gw.double().sum(0).cpu()) - got.sum(0)).abs().max() <= 1e-4 * A.sum(0).max()


# ---------------------------------------------------------------------------------------------------------------------
# the public path
def _settings(S, clip=0.05):
    return PointsRasterizationSettings(backface_culling=False, cutoff_threshold=1.0, Vrk_invariant=True,
                                       radii_backward_scaler=5, image_size=S, points_per_pixel=5, bin_size=None,
                                       clip_pts_grad=clip)


def _bunny():
    pts, nrm = scenes.load_cloud("bunny")
    pts = scenes.normalize_unit_sphere(pts)
    pts, nrm = scenes.upsample_jitter(pts, nrm, 4, seed=0)
    return pts, nrm, (0.5 + 0.5 * nrm).astype(np.float32), scenes.global_h(pts)


def _renderer(cams, S, **kw):
    return SurfaceSplattingRenderer(SurfaceSplatting(cameras=cams, raster_settings=_settings(S)), NormWeightedCompositor(), **kw)


def _target(pts, nrm, col, h, S, pose):
    R, T = look_at_view_transform(*pose)
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T, device=DEV)
    with torch.no_grad():
        img = _renderer(cams, S, fused=True)(PointClouds3D(*[[torch.from_numpy(a).to(DEV)] for a in (pts, nrm, col)]),
                                             Vrk_h=torch.tensor([h], device=DEV))
    return img[..., :3].contiguous(), img[..., 3].contiguous()


def _pose_grads(pts, nrm, col, h, S, pose, target, fused, camera_grad=True, clouds=1):
    """one render + calc_dr_loss + backward -> (R.grad, T.grad, points.grad, colors.grad, R, T)"""
    R, T = look_at_view_transform(*pose)
    R, T = R.to(DEV).requires_grad_(camera_grad), T.to(DEV).requires_grad_(camera_grad)
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T, device=DEV)
    P = [torch.from_numpy(pts).to(DEV).requires_grad_(True) for _ in range(clouds)]
    C = [torch.from_numpy(col).to(DEV).requires_grad_(True) for _ in range(clouds)]
    nr = torch.from_numpy(nrm).to(DEV)
    img = _renderer(cams, S, fused=fused)(PointClouds3D(P, [nr] * clouds, C), Vrk_h=torch.tensor([h] * clouds, device=DEV))
    calc_dr_loss(img, target[0], target[1], 1.0, 1.0)["loss"].backward()
    return R.grad, T.grad, [p.grad for p in P], [c.grad for c in C], R.detach(), T.detach()


def _check_pose_identity(Rg, Tg, Pg, R, pts, tag):
    """T.grad[n] = sum_p g_view(n,p), R.grad[n] = sum_p x_p^T g_view(n,p) with g_view = points.grad_p @ inverse(R[n]^T):
    the rasterizer depends on the camera through the view coordinates x R + T only (raw colours)."""
    x = torch.from_numpy(pts).double()
    worst = 0.0
    for n in range(R.shape[0]):
        gview = Pg[n].cpu().double() @ torch.linalg.inv(R[n].cpu().double().T)
        t_ref, t_abs = gview.sum(0), gview.abs().sum(0)
        outer = x[:, :, None] * gview[:, None, :]
        r_ref, r_abs = outer.sum(0), outer.abs().sum(0)
        worst = max(worst, float(((Tg[n].cpu().double() - t_ref).abs() / t_abs).max()),
                    float(((Rg[n].cpu().double() - r_ref).abs() / r_abs).max()))
    print("pose identity %-28s: max |err| / sum|contribution| = %.3e" % (tag, worst))
    assert worst <= BAR, (tag, worst)


def test_pose_gradients_end_to_end_bunny_512():
    pts, nrm, col, h = _bunny()
    S = 512
    target = _target(pts, nrm, col, h, S, (2.0, 33.0, 41.0))
    pose = (2.05, 30.0, 45.0)
    out = {}
    for fused in (True, False):
        Rg, Tg, Pg, Cg, R, T = out[fused] = _pose_grads(pts, nrm, col, h, S, pose, target, fused)
        assert Rg is not None and Tg is not None and torch.isfinite(Rg).all() and Rg.abs().max() > 0
        _check_pose_identity(Rg, Tg, Pg, R, pts, "fused" if fused else "unfused")
    # fused and unfused camera gradients agree to the same bar (scale: the summed absolute contributions, >= |sum|)
    x = torch.from_numpy(pts).double()
    gview = out[False][2][0].cpu().double() @ torch.linalg.inv(out[False][4][0].cpu().double().T)
    assert ((out[True][1][0] - out[False][1][0]).cpu().double().abs() / gview.abs().sum(0)).max() <= BAR
    assert ((out[True][0][0] - out[False][0][0]).cpu().double().abs()
            / (x[:, :, None] * gview[:, None, :]).abs().sum(0)).max() <= BAR

    # points.grad / colors.grad do not depend on whether the cameras are differentiated
    rel = lambda a, b: float((a - b).norm() / b.norm())
    for fused in (True, False):
        _, _, Pd, Cd, _, _ = _pose_grads(pts, nrm, col, h, S, pose, target, fused, camera_grad=False)
        Pg, Cg = out[fused][2], out[fused][3]
        if fused:
            # one camera, RGB: with detached cameras the projection backward runs in the gather's epilogue; camera gradients
            # switch that fusion off (the reduction needs the screen-space gradient): same arithmetic, other kernel
            assert rel(Pg[0], Pd[0]) <= 1e-5 and rel(Cg[0], Cd[0]) <= 1e-5
        else:
            assert torch.equal(Pg[0], Pd[0]) and torch.equal(Cg[0], Cd[0])      # the same kernels run


def test_pose_gradients_per_camera_clouds_and_shared_cloud():
    pts, nrm = scenes.load_cloud("teapot")
    pts = scenes.normalize_unit_sphere(pts)
    col, h, S = (0.5 + 0.5 * nrm).astype(np.float32), scenes.global_h(pts), 128
    target = _target(pts, nrm, col, h, S, (2.0, [27.0, 18.0], [41.0, 135.0]))
    pose = (2.05, [25.0, 20.0], [45.0, 130.0])
    for fused in (True, False):
        Rg, Tg, Pg, Cg, R, T = _pose_grads(pts, nrm, col, h, S, pose, target, fused, clouds=2)   # N per-camera clouds
        _check_pose_identity(Rg, Tg, Pg, R, pts, "2 clouds %s" % ("fused" if fused else "unfused"))
    # a cloud shared by the two cameras never fuses the projection: the same kernels run with and without camera gradients
    for fused in (True, False):
        a = _pose_grads(pts, nrm, col, h, S, pose, target, fused, camera_grad=True)
        b = _pose_grads(pts, nrm, col, h, S, pose, target, fused, camera_grad=False)
        assert a[0] is not None and b[0] is None
        assert torch.equal(a[2][0], b[2][0]) and torch.equal(a[3][0], b[3][0])
        if fused:
            ref = a
    assert ((ref[0] - a[0]).abs().max() <= 1e-4 * ref[0].abs().max())     # (fused vs unfused, loose: summed over cancelling pairs)


def test_compact_culled_carries_camera_gradients():
    """`compact_culled=True` (the reference's drop-the-culled-points order) renders through the unfused nodes: supported."""
    pts, nrm = scenes.load_cloud("teapot")
    pts = scenes.normalize_unit_sphere(pts)
    col, h, S = (0.5 + 0.5 * nrm).astype(np.float32), scenes.global_h(pts), 128
    target = _target(pts, nrm, col, h, S, (2.0, 27.0, 41.0))
    R, T = look_at_view_transform(2.05, 25.0, 45.0)
    R, T = R.to(DEV).requires_grad_(True), T.to(DEV).requires_grad_(True)
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T, device=DEV)
    rast = SurfaceSplatting(cameras=cams, raster_settings=_settings(S), compact_culled=True)
    P = torch.from_numpy(pts).to(DEV).requires_grad_(True)
    cloud = PointClouds3D([P], [torch.from_numpy(nrm).to(DEV)], [torch.from_numpy(col).to(DEV)])
    img = SurfaceSplattingRenderer(rast, NormWeightedCompositor())(cloud)
    calc_dr_loss(img, target[0], target[1], 1.0, 1.0)["loss"].backward()
    _check_pose_identity(R.grad, T.grad, [P.grad], R.detach(), pts, "compact_culled")


@pytest.mark.parametrize("lights_cls", [PointLights, DirectionalLights])
def test_shading_path_adds_the_chain_of_grad_cam(lights_cls):
    """With LightingTexture and ks > 0, R.grad / T.grad = the geometry-only value (same colours, camera centre detached)
    + grad_cam (`ops.phong_backward_camera`) chained through get_camera_center()."""
    pts, nrm = scenes.load_cloud("teapot")
    pts = scenes.normalize_unit_sphere(pts)
    col, h, S = (0.5 + 0.5 * nrm).astype(np.float32), scenes.global_h(pts), 128
    target = _target(pts, nrm, col, h, S, (2.0, 27.0, 41.0))
    R0, T0 = look_at_view_transform(2.05, 25.0, 45.0)
    vec = (-R0[0] @ T0[0]) * (1.2 if lights_cls is PointLights else 1.0) + torch.tensor([0.2, 0.1, -0.1])
    lights = lights_cls(ambient_color=((0.4, 0.4, 0.4),), diffuse_color=((0.3, 0.3, 0.3),), specular_color=((0.6, 0.5, 0.4),),
                        device=DEV, **{lights_cls._vec: (tuple(vec.tolist()),)})
    P, nr, C = (torch.from_numpy(a).to(DEV) for a in (pts, nrm, col))
    hv = torch.tensor([h], device=DEV)

    def run(detach_centre, leaf_colours=False):
        R, T = R0.to(DEV).requires_grad_(True), T0.to(DEV).requires_grad_(True)
        cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T, device=DEV)
        tex_cams = FoVPerspectiveCameras(znear=0.1, R=R.detach(), T=T.detach(), device=DEV) if detach_centre else cams
        shaded = LightingTexture(cameras=tex_cams, lights=lights)(PointClouds3D([P], [nr], [C]), shininess=16)
        feats = shaded.features_packed()
        if leaf_colours:
            feats = feats.detach().requires_grad_(True)
            shaded = PointClouds3D([P], [nr], [feats])
        img = _renderer(cams, S, fused=True)(shaded, Vrk_h=hv)
        calc_dr_loss(img, target[0], target[1], 1.0, 1.0)["loss"].backward()
        return R, T, feats

    Rf, Tf, _ = run(False)
    Rgeo, Tgeo, g_leaf = run(True, leaf_colours=True)
    one = torch.zeros(1, dtype=torch.int64, device=DEV)
    cnt = torch.full((1,), P.shape[0], dtype=torch.int64, device=DEV)
    amb, kd, ks, lv = lights._packed(1)
    Rc, Tc = R0.to(DEV).requires_grad_(True), T0.to(DEV).requires_grad_(True)
    centre = FoVPerspectiveCameras(znear=0.1, R=Rc, T=Tc, device=DEV).get_camera_center()
    gcam = ops.phong_backward_camera(g_leaf.grad, P, nr, C, one, cnt, amb, kd, ks, lv, lights_cls is PointLights,
                                     centre.detach().contiguous(), 16.0, False)
    centre.backward(gcam)
    assert gcam.abs().max() > 0 and Rc.grad.abs().max() > 0
    for full, geo, chain, name in ((Rf.grad, Rgeo.grad, Rc.grad, "R"), (Tf.grad, Tgeo.grad, Tc.grad, "T")):
        scale = max(float(full.abs().max()), float(chain.abs().max()))
        err = float((full - geo - chain).abs().max())
        print("shading chain %s (%s): |full - geometry - chain| = %.3e of %.3e, chain / full = %.3e"
              % (name, lights_cls.__name__, err, scale, float(chain.abs().max() / full.abs().max())))
        assert err <= 1e-5 * scale


def test_options_without_camera_gradients_refuse():
    from dss_amd.distributed import RowPartition
    pts, nrm = scenes.load_cloud("teapot")
    pts = scenes.normalize_unit_sphere(pts)
    col, h, S = (0.5 + 0.5 * nrm).astype(np.float32), scenes.global_h(pts), 128
    P, nr, C = (torch.from_numpy(a).to(DEV) for a in (pts, nrm, col))
    hv = torch.tensor([h], device=DEV)
    R0, T0 = look_at_view_transform(2.0, 25.0, 45.0)
    det = FoVPerspectiveCameras(znear=0.1, R=R0, T=T0, device=DEV)
    plain = _renderer(det, S, fused=True)(PointClouds3D([P], [nr], [C]), Vrk_h=hv)
    graphed = _renderer(det, S, graphed=True)
    for _ in range(2):   # capture, then the steady-state replay: as before
        assert torch.equal(graphed(PointClouds3D([P], [nr], [C]), Vrk_h=hv), plain)
    # the same camera object starts to require grad: the graphed renderer must refuse, not replay without the gradient
    det.T.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="graphed=True"):
        graphed(PointClouds3D([P], [nr], [C]), Vrk_h=hv)
    with torch.no_grad():                                   # nothing to differentiate: served as before
        assert torch.equal(graphed(PointClouds3D([P], [nr], [C]), Vrk_h=hv), plain)
    cams = FoVPerspectiveCameras(znear=0.1, R=R0.to(DEV).requires_grad_(True), T=T0.to(DEV), device=DEV)
    with pytest.raises(NotImplementedError, match="graphed=True"):
        _renderer(cams, S, graphed=True)(PointClouds3D([P], [nr], [C]), Vrk_h=hv)
    # (row partitions with detached cameras: test_gpu_sharded.py / test_gpu_rccl_world1.py, unchanged)
    rast = SurfaceSplatting(cameras=cams, raster_settings=_settings(S))
    with pytest.raises(NotImplementedError, match="row_partition"):
        rast.render_fused(PointClouds3D([P], [nr], [C]), Vrk_h=hv, row_partition=RowPartition(S, 2, 0))


def test_memo_and_two_iterations_on_the_gpu():
    """`_prepare`'s memo serves detached cameras only: two iterations with differentiable cameras both backward, and a
    camera that starts to require grad after a memoised call gets its gradient."""
    pts, nrm = scenes.load_cloud("teapot")
    pts = scenes.normalize_unit_sphere(pts)
    col, h, S = (0.5 + 0.5 * nrm).astype(np.float32), scenes.global_h(pts), 128
    target = _target(pts, nrm, col, h, S, (2.0, 27.0, 41.0))
    P, nr, C = (torch.from_numpy(a).to(DEV) for a in (pts, nrm, col))
    hv = torch.tensor([h], device=DEV)
    R0, T0 = look_at_view_transform(2.05, 25.0, 45.0)
    cams = FoVPerspectiveCameras(znear=0.1, R=R0, T=T0, device=DEV)
    renderer = _renderer(cams, S, fused=True)
    a = renderer(PointClouds3D([P], [nr], [C]), Vrk_h=hv)
    assert renderer.rasterizer._prepare_memo is not None
    assert not renderer(PointClouds3D([P], [nr], [C]), Vrk_h=hv).requires_grad
    cams.T.requires_grad_(True)
    grads = []
    for it in range(2):
        cams.T.grad = None
        img = renderer(PointClouds3D([P], [nr], [C]), Vrk_h=hv)
        assert (img - a).abs().max() <= 1e-6        # (the general node instead of the lean plan: the same kernels)
        calc_dr_loss(img, target[0], target[1], 1.0, 1.0)["loss"].backward()
        grads.append(cams.T.grad.clone())
    assert grads[0].abs().max() > 0 and torch.equal(grads[0], grads[1])


def _rotation(w):
    """exp of the skew matrix of w (3,): a small rotation offset, differentiable"""
    z = torch.zeros((), device=w.device)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    return torch.matrix_exp(K)


def test_pose_recovery_property():
    """40 Adam steps on T and on a small rotation offset composed with R, from a pose a few degrees and a few percent of
    the distance off: the loss and the translation error end below where they started (sign and wiring)."""
    pts, nrm = scenes.load_cloud("teapot")
    pts = scenes.normalize_unit_sphere(pts)
    col, h, S = (0.5 + 0.5 * nrm).astype(np.float32), scenes.global_h(pts), 256
    true_pose = (2.0, 25.0, 40.0)
    target = _target(pts, nrm, col, h, S, true_pose)
    R_true, T_true = (t.to(DEV) for t in look_at_view_transform(*true_pose))
    P, nr, C = (torch.from_numpy(a).to(DEV) for a in (pts, nrm, col))
    hv = torch.tensor([h], device=DEV)
    with torch.no_grad():
        R_start = (R_true[0] @ _rotation(torch.tensor([0.04, -0.05, 0.03], device=DEV)))[None]     # ~ 4 degrees
    T = (T_true + torch.tensor([[0.06, -0.05, 0.08]], device=DEV)).requires_grad_(True)           # ~ 5 % of the distance
    w = torch.zeros(3, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([T, w], lr=2e-3)
    rasterizer = SurfaceSplatting(raster_settings=_settings(S))
    renderer = SurfaceSplattingRenderer(rasterizer, NormWeightedCompositor(), fused=True)
    losses, t_err = [], []
    for it in range(40):
        opt.zero_grad()
        cams = FoVPerspectiveCameras(znear=0.1, R=(R_start[0] @ _rotation(w))[None], T=T, device=DEV)
        img = renderer(PointClouds3D([P], [nr], [C]), Vrk_h=hv, cameras=cams)
        loss = calc_dr_loss(img, target[0], target[1], 1.0, 1.0)["loss"]
        loss.backward()
        assert T.grad is not None and w.grad is not None and torch.isfinite(T.grad).all() and torch.isfinite(w.grad).all()
        losses.append(float(loss.detach()))
        t_err.append(float((T.detach() - T_true).norm()))
        opt.step()
    t_err.append(float((T.detach() - T_true).norm()))
    print("pose recovery: loss %.4f -> %.4f, |T - T_true| %.4f -> %.4f" % (losses[0], losses[-1], t_err[0], t_err[-1]))
    assert losses[-1] < losses[0] and t_err[-1] < t_err[0]
