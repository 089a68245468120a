"""fp64 CPU reference of the camera gradients (TEST INFRASTRUCTURE; plain torch, no product code).

Two closed forms, each with the sums of the ABSOLUTE terms next to the sums themselves (the error of a kernel is measured
against ``A = sum_p |term|``, not against a sum that may cancel), and for each a straightforward differentiable fp64
restatement of the forward that `torch.autograd` differentiates (`tests/test_camera_grad_cpu.py` compares the two):

* the projection (pytorch3d ``Transform3d.transform_points`` in the row-vector convention): for camera ``n`` and a point
  with homogeneous world position ``x``: ``clip = x @ M[n]``, ``ndc = clip.xy / clip.w``, ``view_z = (x @ V[n]).z``;
* the Phong shading of ``dss_amd/csrc/shading.hip``'s header, whose specular term sees the camera centre through
  ``v^ = normalize(camera - x)``.
"""
import torch

F64 = torch.float64


def _ranges(first, num):
    return [(int(f), int(f) + int(c)) for f, c in zip(first.tolist(), num.tolist())]


def clip_screen_grad(g, clip):
    """the per-point norm clip hook of DSS/core/rasterizer.py:667-673 on (P,3) fp64 gradients (clip <= 0: none)"""
    if clip is None or clip <= 0:
        return g
    nrm = g.norm(dim=1, keepdim=True)
    return g / nrm.clamp_min(1e-12) * nrm.clamp_max(clip)


def _world_of(world, lo, hi, first_n, shared):
    return world[lo - first_n:hi - first_n] if shared else world[lo:hi]


def project(world, M, V, first, num, shared):
    """differentiable (P,3) = (ndc_x, ndc_y, view_z) of every packed (camera, point) pair, fp64"""
    out = []
    for n, (lo, hi) in enumerate(_ranges(first, num)):
        x = _world_of(world, lo, hi, lo, shared)
        xh = torch.cat([x, torch.ones_like(x[:, :1])], 1)
        c = xh @ M[n]
        v = xh @ V[n]
        out.append(torch.stack([c[:, 0] / c[:, 3], c[:, 1] / c[:, 3], v[:, 2]], 1))
    return torch.cat(out, 0) if out else world.new_zeros((0, 3))


def camera_backward(world, M, V, first, num, grad_screen, valid, shared=False, clip=-1.0):
    """closed forms -> (grad_M, grad_V, abs_M, abs_V), each (N,4,4) fp64; abs_* = the sums of the absolute terms"""
    world, M, V, g = world.to(F64), M.to(F64), V.to(F64), grad_screen.to(F64)
    g = clip_screen_grad(g, clip) * valid.to(F64)[:, None]
    N = M.shape[0]
    gM, gV, aM, aV = (torch.zeros(N, 4, 4, dtype=F64) for _ in range(4))
    for n, (lo, hi) in enumerate(_ranges(first, num)):
        x = _world_of(world, lo, hi, lo, shared)
        xh = torch.cat([x, torch.ones_like(x[:, :1])], 1)
        c = xh @ M[n]
        w = c[:, 3]
        nx, ny = c[:, 0] / w, c[:, 1] / w
        gx, gy, gz = g[lo:hi, 0], g[lo:hi, 1], g[lo:hi, 2]
        cols = {0: gx / w, 1: gy / w, 3: -(gx * nx + gy * ny) / w}
        for col, a in cols.items():
            t = xh * a[:, None]
            gM[n, :, col], aM[n, :, col] = t.sum(0), t.abs().sum(0)
        t = xh * gz[:, None]
        gV[n, :, 2], aV[n, :, 2] = t.sum(0), t.abs().sum(0)
    return gM, gV, aM, aV


def camera_backward_autograd(world, M, V, first, num, grad_screen, valid, shared=False, clip=-1.0):
    """the same two gradients from torch.autograd of `project` -> (grad_M, grad_V)"""
    M = M.to(F64).clone().requires_grad_(True)
    V = V.to(F64).clone().requires_grad_(True)
    g = clip_screen_grad(grad_screen.to(F64), clip) * valid.to(F64)[:, None]
    (project(world.to(F64), M, V, first, num, shared) * g).sum().backward()
    return M.grad, V.grad


def _normalize(u):
    return u / u.norm(dim=-1, keepdim=True).clamp_min(1e-6)          # F.normalize, eps 1e-6


def phong(world, normals, rgb, first, num, ambient, kd, ks, lvec, point_lights, cam, shininess, shared):
    """differentiable fp64 shading (P,3): rgb * (ambient + sum_l kd relu(n^.d^)) + sum_l ks (relu(v^.r) [n^.d^ > 0])^s"""
    out = []
    for n, (lo, hi) in enumerate(_ranges(first, num)):
        x = _world_of(world, lo, hi, lo, shared)
        nh = _normalize(_world_of(normals, lo, hi, lo, shared))
        v = _normalize(cam[n][None] - x)
        dif = torch.zeros_like(x)
        spec = torch.zeros_like(x)
        for l in range(kd.shape[1]):
            u = lvec[n, l][None] - x if point_lights else lvec[n, l][None].expand_as(x)
            d = _normalize(u)
            ca = (nh * d).sum(1, keepdim=True)
            r = -d + 2.0 * ca * nh
            alpha = torch.relu((v * r).sum(1, keepdim=True)) * (ca > 0)
            dif = dif + kd[n, l][None] * torch.relu(ca)
            spec = spec + ks[n, l][None] * alpha ** shininess
        out.append(rgb[lo:hi] * (ambient[n][None] + dif) + spec)
    return torch.cat(out, 0)


def phong_backward_camera(grad_out, world, normals, first, num, ks, lvec, point_lights, cam, shininess, shared, dtype=F64):
    """closed form -> (grad_cam (N,3), abs_cam (N,3)) fp64: per pair gv = sum_l ga0_l r_l with
    ga0 = (g . ks) s alpha^(s-1) on lit, facing fragments; gw = (gv - v^ (v^ . gv)) / |w|, w = camera - x
    (`dtype=torch.float32`: the same formula in plain fp32 torch, to see what the number format alone costs)"""
    world, normals, g, ks, lvec, cam = (t.to(dtype) for t in (world, normals, grad_out, ks, lvec, cam))
    N = cam.shape[0]
    gc, ac = torch.zeros(N, 3, dtype=F64), torch.zeros(N, 3, dtype=F64)
    for n, (lo, hi) in enumerate(_ranges(first, num)):
        x = _world_of(world, lo, hi, lo, shared)
        nh = _normalize(_world_of(normals, lo, hi, lo, shared))
        w = cam[n][None] - x
        wn = w.norm(dim=1, keepdim=True)
        v = w / wn.clamp_min(1e-6)
        gv = torch.zeros_like(x)
        for l in range(ks.shape[1]):
            u = lvec[n, l][None] - x if point_lights else lvec[n, l][None].expand_as(x)
            d = _normalize(u)
            ca = (nh * d).sum(1, keepdim=True)
            r = -d + 2.0 * ca * nh
            a0 = (v * r).sum(1, keepdim=True)
            on = (ca > 0) & (a0 > 0)
            gs = (g[lo:hi] * ks[n, l][None]).sum(1, keepdim=True)
            ga0 = torch.where(on, gs * shininess * a0.clamp_min(0) ** (shininess - 1.0), torch.zeros_like(a0))
            gv = gv + ga0 * r
        gw = torch.where(wn > 1e-6, (gv - v * (v * gv).sum(1, keepdim=True)) / wn.clamp_min(1e-6), gv * 1e6)
        gc[n], ac[n] = gw.sum(0).to(F64), gw.to(F64).abs().sum(0)
    return gc, ac


def phong_backward_camera_autograd(grad_out, world, normals, rgb, first, num, ambient, kd, ks, lvec, point_lights, cam,
                                   shininess, shared):
    cam = cam.to(F64).clone().requires_grad_(True)
    a = [t.to(F64) for t in (world, normals, rgb)]
    b = [t.to(F64) for t in (ambient, kd, ks, lvec)]
    out = phong(a[0], a[1], a[2], first, num, b[0], b[1], b[2], b[3], point_lights, cam, shininess, shared)
    (out * grad_out.to(F64)).sum().backward()
    return cam.grad
