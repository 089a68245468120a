"""GPU: gradients w.r.t. the lights -- `ops.phong_backward_lights` against the fp64 reference (`tests/light_reference.py`),
exact zeros, bitwise reproducibility, and the public path: `.grad` of the tensors a user builds PointLights /
DirectionalLights from, after a loss on the shaded colours or on the rendered image.

Error bookkeeping as in test_gpu_camera_grad.py: every output entry is compared with its fp64 value RELATIVE TO
``A = sum_p |term|`` of that entry; the bar is that file's ``BAR = 1e-5``.  Each test prints the largest observed ratio per
output.  Cloud sizes: `test_phong_backward_camera_against_fp64` explains why, at shininess 64, clouds below ~20,000 points
are limited by the fp32 format and not by the kernel; the specular-dependent outputs (grad_specular, grad_light_vec) are
checked on clouds of at least that size.  The same formula in plain fp32 torch on the CPU
(``light_reference.phong_backward_lights(..., dtype=torch.float32)``) on the cases below: ambient <= 5e-10, diffuse <= 4e-9,
specular 1.8e-6 - 4.0e-6, light_vec 1.9e-7 - 7.8e-7.  The kernel measured on an MI355X: ambient <= 1.5e-9, diffuse <= 4.6e-9,
specular 1.7e-6 - 4.4e-6, light_vec 2.0e-7 - 7.9e-7 -- the format's figures; through the module (32,000-point bunny, 3 cameras)
specular_color 6.4e-7, the others <= 2.5e-9."""
import math

import numpy as np
import pytest
import torch

import light_reference as lref
import scenes
from dss_amd import ops
from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
from dss_amd.cloud import PointClouds3D
from dss_amd.losses import calc_dr_loss
from dss_amd.texture import DirectionalLights, LightingTexture, PointLights
from test_gpu_camera_grad import BAR, _bunny, _gpu, _phong_case, _renderer
from test_gpu_shading import _torch_phong

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("grad_ambient", "grad_diffuse", "grad_specular", "grad_light_vec")


def _call(case, point_lights, shared, shin=64.0, **kw):
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    return ops.phong_backward_lights(*_gpu(grad_out, world, normals, rgb, first, num, amb, kd, ks, lvec), point_lights,
                                     cam.to(DEV), shin, shared, **kw)


def _reference(case, point_lights, shared, shin=64.0):
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    return lref.phong_backward_lights(grad_out, world, normals, rgb, first, num, kd, ks, lvec, point_lights, cam, shin, shared)


def _check(got, ref, A, tag):
    worst = []
    for name, g, r, a in zip(NAMES, got, ref, A):
        g = g.cpu().double()
        assert tuple(g.shape) == tuple(r.shape), name
        assert (g[a == 0] == 0).all(), "%s %s: entries without a term must be exact zeros" % (tag, name)
        ratio = (g - r).abs()[a > 0] / a[a > 0]
        worst.append(float(ratio.max()) if ratio.numel() else 0.0)
    print("phong_backward_lights %-40s max |err| / A: %s" % (tag, "  ".join("%s %.3e" % (n[5:], w) for n, w in zip(NAMES, worst))))
    for name, w in zip(NAMES, worst):
        assert w <= BAR, (tag, name, w)


@pytest.mark.parametrize("point_lights", [True, False])
@pytest.mark.parametrize("sizes,shared", [([20011] * 3, True), ([30011, 20313, 24000], False)])
def test_phong_backward_lights_against_fp64(sizes, shared, point_lights):
    case = _phong_case(sizes, shared, 31)
    tag = "%s %s" % ("shared" if shared else "per-camera", "point" if point_lights else "directional")
    got = _call(case, point_lights, shared)
    ref, A = _reference(case, point_lights, shared)
    assert all(float(a.min()) > 0 for a in A)
    _check(got, ref, A, tag)
    # ks = 0: the outputs that do not read the specular colour keep their bits (grad_specular = sum g S is one of them);
    # grad_light_vec keeps the diffuse chain only, and nothing at all once kd = 0 as well
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    no_ks = (world, normals, rgb, first, num, amb, kd, torch.zeros_like(ks), lvec, cam, grad_out)
    got0 = _call(no_ks, point_lights, shared)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], got0[:3]))
    ref0, A0 = _reference(no_ks, point_lights, shared)
    _check(got0, ref0, A0, tag + ", ks = 0")
    dark = (world, normals, rgb, first, num, amb, torch.zeros_like(kd), torch.zeros_like(ks), lvec, cam, grad_out)
    gotd = _call(dark, point_lights, shared)
    assert (gotd[3] == 0).all() and torch.equal(gotd[0], got[0]) and torch.equal(gotd[1], got[1])


def test_exact_zeros_and_null_outputs():
    # a camera whose cloud is empty gets zero rows; the others are unaffected by it
    sizes = [20011, 0, 20500]
    case = _phong_case(sizes, False, 33)
    got = _call(case, True, False)
    ref, A = _reference(case, True, False)
    _check(got, ref, A, "3 clouds, one empty")
    assert all((g[1] == 0).all() for g in got)
    # NULL outputs: the ones asked for keep their bits
    for needs in ((True, False, False, False), (False, True, False, True), (False, False, True, False)):
        part = _call(case, True, False, needs=needs)
        for need, p, g in zip(needs, part, got):
            assert (p is None) != need and (p is None or torch.equal(p, g))
    # Pw == 0
    empty = _phong_case([0, 0], False, 34)
    z = _call(empty, False, False)
    assert [tuple(t.shape) for t in z] == [(2, 3)] + [(2, 2, 3)] * 3 and all((t == 0).all() for t in z)
    # L == 0: no light outputs to write (N,0,3); out = rgb * ambient, whose gradient is still delivered
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    none = (world, normals, rgb, first, num, amb, kd[:, :0], ks[:, :0], lvec[:, :0], cam, grad_out)
    z = _call(none, True, False)
    assert [tuple(t.shape) for t in z] == [(3, 3)] + [(3, 0, 3)] * 3
    assert torch.equal(z[0], got[0])
    zero_g = (world, normals, rgb, first, num, amb, kd[:, :0], ks[:, :0], lvec[:, :0], cam, torch.zeros_like(grad_out))
    assert (_call(zero_g, True, False)[0] == 0).all()
    zero_g = (world, normals, rgb, first, num, amb, kd, ks, lvec, cam, torch.zeros_like(grad_out))
    assert all((t == 0).all() for t in _call(zero_g, True, False))


def test_phong_backward_lights_is_bitwise_reproducible():
    # 99,790 is not a multiple of 64: wavefronts straddle cameras in the packed order
    for sizes, shared, point_lights in (([99790] * 8, True, True), ([99790] * 8, True, False),
                                        ([30011, 20313, 24000], False, True)):
        case = _phong_case(sizes, shared, 41)
        a = _call(case, point_lights, shared)
        b = _call(case, point_lights, shared)
        # unrelated launches in between (one of them reuses the per-stream workspace for other sizes)
        _call(_phong_case([4099], False, 42, L=3), True, False)
        torch.randn(1 << 20, device=DEV).sum()
        c = _call(case, point_lights, shared)
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        if shared:
            ref, A = _reference(case, point_lights, shared)
            _check(a, ref, A, "8 x 99,790 shared %s" % ("point" if point_lights else "directional"))


# ---------------------------------------------------------------------------------------------------------------------
# the public path
def _learnable_lights(cls, vec, requires_grad=True):
    """a lights batch of 1 with L = 2, built from leaf tensors on the device"""
    leaves = dict(ambient_color=torch.tensor([[[0.25, 0.3, 0.2], [0.1, 0.05, 0.15]]]),
                  diffuse_color=torch.tensor([[[0.5, 0.4, 0.45], [0.2, 0.3, 0.25]]]),
                  specular_color=torch.tensor([[[0.6, 0.5, 0.4], [0.3, 0.35, 0.3]]]))
    leaves[cls._vec] = vec
    leaves = {k: v.to(DEV).requires_grad_(requires_grad) for k, v in leaves.items()}
    return cls(device=DEV, **leaves), leaves


def _three_views():
    R, T = look_at_view_transform(2.0, [25.0, 10.0, 40.0], [45.0, 150.0, 260.0])
    centre = FoVPerspectiveCameras(R=R, T=T).get_camera_center()
    # two lights near the first two cameras: highlights face a viewer, the specular chain carries weight
    vec = (centre[:2] * 1.1 + torch.tensor([[0.2, 0.1, -0.1], [-0.15, 0.2, 0.1]]))[None]
    return R, T, vec


@pytest.mark.parametrize("cls", [PointLights, DirectionalLights])
def test_module_light_gradients_match_fp64_autograd(cls):
    """LightingTexture on a cloud of 32,000 points shared by N = 3 cameras, a lights batch of 1 broadcast to the cameras:
    `.grad` of the four leaves = fp64 autograd of `_torch_phong` (which sums over cameras, and over lights for the ambient
    colour), within the bar relative to the summed absolute terms.  Without the feature every `.grad` is None."""
    pts, nrm, col, _h = _bunny()
    R, T, vec = _three_views()
    N, Pw, shin = 3, len(pts), 64.0
    assert Pw >= 20000
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T, device=DEV)
    lights, leaves = _learnable_lights(cls, vec)
    P, nr, C = (torch.from_numpy(a).to(DEV) for a in (pts, nrm, col))
    shaded = LightingTexture(cameras=cams, lights=lights)(PointClouds3D([P], [nr], [C]), shininess=shin).features_packed()
    go = torch.randn(N * Pw, 3, generator=torch.Generator().manual_seed(5))
    (shaded * go.to(DEV)).sum().backward()

    names = ("ambient_color", "diffuse_color", "specular_color", cls._vec)
    ref_leaves = [leaves[k].detach().cpu().double().requires_grad_(True) for k in names]
    amb, kd, ks, lv = (t.expand(N, 2, 3) for t in ref_leaves)
    cam = cams.get_camera_center().cpu().double()
    x, m, c = (torch.from_numpy(a).double().repeat(N, 1) for a in (pts, nrm, col))
    batch = torch.arange(N).repeat_interleave(Pw)
    ref = _torch_phong(x, m, c, batch, amb.sum(1), kd, ks, lv, cls is PointLights, cam, shin)
    (ref * go.double()).sum().backward()
    first, num = torch.arange(N) * Pw, torch.full((N,), Pw)
    _g, A = lref.phong_backward_lights(go, x[:Pw], m[:Pw], c, first, num, kd.detach(), ks.detach(), lv.detach(),
                                       cls is PointLights, cam, shin, True)
    scale = [A[0].sum(0)[None, None].expand(1, 2, 3)] + [a.sum(0)[None] for a in A[1:]]     # summed over the cameras
    worst = []
    for k, r, a in zip(names, ref_leaves, scale):
        got = leaves[k].grad
        assert got is not None and tuple(got.shape) == (1, 2, 3), k
        worst.append(float(((got.cpu().double() - r.grad).abs() / a).max()))
    print("module %-17s max |err| / A: %s" % (cls.__name__, "  ".join("%s %.3e" % kw for kw in zip(names, worst))))
    assert max(worst) <= BAR, worst


def _teapot():
    pts, nrm = scenes.load_cloud("teapot")
    pts = scenes.normalize_unit_sphere(pts)
    return pts, nrm, (0.5 + 0.5 * nrm).astype(np.float32), scenes.global_h(pts)


@pytest.mark.parametrize("cls", [PointLights, DirectionalLights])
def test_image_loss_reaches_the_lights_and_detached_lights_launch_nothing(cls, monkeypatch):
    """texture -> fused renderer -> image loss: the four leaves get finite non-zero gradients; with lights that do not
    require grad `ops.phong_backward_lights` is never called (the backward launches what it launched before)."""
    pts, nrm, col, h = _teapot()
    S = 128
    R, T, vec = _three_views()
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T, device=DEV)
    P, nr = (torch.from_numpy(a).to(DEV) for a in (pts, nrm))
    hv = torch.tensor([h] * 3, device=DEV)             # the shaded cloud comes back as one cloud per camera
    target_rgb = torch.full((3, S, S, 3), 0.35, device=DEV)
    target_mask = torch.ones((3, S, S), device=DEV)
    calls = []
    real = ops.phong_backward_lights
    monkeypatch.setattr(ops, "phong_backward_lights", lambda *a, **kw: calls.append(1) or real(*a, **kw))

    def run(requires_grad):
        lights, leaves = _learnable_lights(cls, vec, requires_grad)
        C = torch.from_numpy(col).to(DEV).requires_grad_(True)
        shaded = LightingTexture(cameras=cams, lights=lights)(PointClouds3D([P], [nr], [C]), shininess=16)
        img = _renderer(cams, S, fused=True)(shaded, Vrk_h=hv)
        calc_dr_loss(img, target_rgb, target_mask, 1.0, 1.0)["loss"].backward()
        return leaves, C.grad

    leaves, c_on = run(True)
    assert len(calls) == 1
    for k, v in leaves.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and float(v.grad.abs().max()) > 0, k
    leaves, c_off = run(False)
    assert len(calls) == 1 and all(v.grad is None for v in leaves.values())
    assert torch.equal(c_on, c_off)            # the point gradients do not depend on whether the lights are learnable


def test_light_recovery_property():
    """One directional light: from a direction 31 degrees off and a wrong diffuse colour, 100 Adam steps on those two
    tensors only.  The image loss and the angle to the true direction each decrease by at least half (sign and wiring; no
    final value is asserted).  Measured curve, every 20 steps: loss 0.286, 0.025, 0.012, 0.0039, 0.0008, 0.0014; angle 31.1,
    3.3, 1.1, 0.55, 0.09, 0.00 degrees."""
    pts, nrm, col, h = _teapot()
    S = 128
    R, T = look_at_view_transform(2.0, [25.0, 15.0], [40.0, 170.0])
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T, device=DEV)
    P, nr, C = (torch.from_numpy(a).to(DEV) for a in (pts, nrm, col))
    hv = torch.tensor([h] * 2, device=DEV)             # the shaded cloud comes back as one cloud per camera
    renderer = _renderer(cams, S, fused=True)
    true_dir = torch.tensor([[[0.4, 0.8, 0.45]]], device=DEV)
    fixed = dict(ambient_color=((0.2, 0.2, 0.2),), specular_color=((0.2, 0.2, 0.2),), device=DEV)

    def render(direction, diffuse):
        lights = DirectionalLights(diffuse_color=diffuse, direction=direction, **fixed)
        shaded = LightingTexture(cameras=cams, lights=lights)(PointClouds3D([P], [nr], [C]), shininess=32)
        return renderer(shaded, Vrk_h=hv)

    with torch.no_grad():
        target = render(true_dir, torch.tensor([[[0.7, 0.6, 0.5]]], device=DEV))
    target_rgb, target_mask = target[..., :3].contiguous(), target[..., 3].contiguous()
    direction = torch.tensor([[[0.75, 0.55, 0.15]]], device=DEV, requires_grad=True)
    diffuse = torch.tensor([[[0.3, 0.3, 0.3]]], device=DEV, requires_grad=True)
    angle = lambda: math.degrees(math.acos(min(1.0, float(torch.nn.functional.cosine_similarity(
        direction.detach().reshape(3), true_dir.reshape(3), dim=0)))))
    opt = torch.optim.Adam([direction, diffuse], lr=2e-2)
    losses, angles = [], []
    for it in range(100):
        opt.zero_grad()
        loss = calc_dr_loss(render(direction, diffuse), target_rgb, target_mask, 1.0, 1.0)["loss"]
        loss.backward()
        assert torch.isfinite(direction.grad).all() and torch.isfinite(diffuse.grad).all()
        losses.append(float(loss.detach()))
        angles.append(angle())
        opt.step()
    with torch.no_grad():
        losses.append(float(calc_dr_loss(render(direction, diffuse), target_rgb, target_mask, 1.0, 1.0)["loss"]))
    angles.append(angle())
    print("light recovery: step   loss   angle(deg)")
    for it in range(0, 101, 10):
        print("light recovery: %4d  %.5f  %6.2f" % (it, losses[it], angles[it]))
    assert losses[-1] <= 0.5 * losses[0], (losses[0], losses[-1])
    assert angles[-1] <= 0.5 * angles[0], (angles[0], angles[-1])
