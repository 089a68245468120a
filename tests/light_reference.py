"""fp64 CPU reference of the light gradients (TEST INFRASTRUCTURE; plain torch, no product code).

The closed form of the shading's gradient w.r.t. the four light tensors, each sum with the sum of its ABSOLUTE terms next
to it (the error of a kernel is measured against ``A = sum_p |term|``, not against a sum that may cancel), and the same
gradients from `torch.autograd` of `camera_reference.phong`, the differentiable fp64 restatement of the forward
(`tests/test_light_grad_cpu.py` compares the two, and both with the reference's own code through
``tests/golden/ref_light_grads.npz``).

Notation of ``dss_amd/csrc/shading.hip``: for the pair (camera n, point p) and light l, g = grad_out, c = rgb,
u = location - x or direction, d^ = normalize(u), ca = n^ . d^, r = -d^ + 2 ca n^, a0 = v^ . r,
D = relu(ca), S = (relu(a0) [ca > 0]) ^ s:

    grad_ambient[n]     = sum_p g c                     grad_diffuse[n][l] = sum_p g c D
    grad_specular[n][l] = sum_p g S
    grad_light_vec[n][l] = sum_p J(u)^T gdv,   gdv = -ga0 v^ + gca n^,   ga0 = [ca > 0][a0 > 0] (g . ks) s a0^(s-1),
                           gca = [ca > 0] (g c . kd) + 2 ga0 (v^ . n^),   J(u)^T y = (y - d^ (d^ . y)) / |u|   (|u| > 1e-6)
"""
import torch

from camera_reference import F64, _normalize, _ranges, _world_of, phong


def phong_backward_lights(grad_out, world, normals, rgb, first, num, kd, ks, lvec, point_lights, cam, shininess, shared,
                          dtype=F64):
    """closed form -> ((grad_ambient (N,3), grad_diffuse, grad_specular, grad_light_vec (N,L,3)), (abs_* likewise)) fp64
    (`dtype=torch.float32`: the same formula in plain fp32 torch, to see what the number format alone costs)"""
    world, normals, rgb, g, kd, ks, lvec, cam = (t.to(dtype) for t in (world, normals, rgb, grad_out, kd, ks, lvec, cam))
    N, L = cam.shape[0], kd.shape[1]
    grads = [torch.zeros(N, 3, dtype=F64)] + [torch.zeros(N, L, 3, dtype=F64) for _ in range(3)]
    sums = [torch.zeros_like(t) for t in grads]

    def put(k, idx, terms):
        grads[k][idx], sums[k][idx] = terms.to(F64).sum(0), terms.to(F64).abs().sum(0)

    for n, (lo, hi) in enumerate(_ranges(first, num)):
        x = _world_of(world, lo, hi, lo, shared)
        nh = _normalize(_world_of(normals, lo, hi, lo, shared))
        v = _normalize(cam[n][None] - x)
        gc = g[lo:hi] * rgb[lo:hi]
        put(0, n, gc)
        for l in range(L):
            u = lvec[n, l][None] - x if point_lights else lvec[n, l][None].expand_as(x)
            un = u.norm(dim=1, keepdim=True)
            d = u / un.clamp_min(1e-6)
            ca = (nh * d).sum(1, keepdim=True)
            r = -d + 2.0 * ca * nh
            a0 = (v * r).sum(1, keepdim=True)
            lit = ca > 0
            alpha = a0.clamp_min(0) * lit
            put(1, (n, l), gc * ca.clamp_min(0))
            put(2, (n, l), g[lo:hi] * alpha ** shininess)
            gd = (gc * kd[n, l][None]).sum(1, keepdim=True)
            gs = (g[lo:hi] * ks[n, l][None]).sum(1, keepdim=True)
            ga0 = torch.where(lit & (a0 > 0), gs * shininess * alpha ** (shininess - 1.0), torch.zeros_like(a0))
            gca = torch.where(lit, gd, torch.zeros_like(gd)) + 2.0 * ga0 * (v * nh).sum(1, keepdim=True)
            gdv = -ga0 * v + gca * nh
            gu = torch.where(un > 1e-6, (gdv - d * (d * gdv).sum(1, keepdim=True)) / un.clamp_min(1e-6), gdv * 1e6)
            put(3, (n, l), gu)
    return tuple(grads), tuple(sums)


def phong_backward_lights_autograd(grad_out, world, normals, rgb, first, num, ambient, kd, ks, lvec, point_lights, cam,
                                   shininess, shared):
    """the same four gradients from torch.autograd of `camera_reference.phong`"""
    leaves = [t.to(F64).clone().requires_grad_(True) for t in (ambient, kd, ks, lvec)]
    a = [t.to(F64) for t in (world, normals, rgb, cam)]
    out = phong(a[0], a[1], a[2], first, num, leaves[0], leaves[1], leaves[2], leaves[3], point_lights, a[3], shininess,
                shared)
    (out * grad_out.to(F64)).sum().backward()
    return tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in leaves)
