"""Generates tests/golden/ref_point_grads.npz: the gradients that the REFERENCE's own shading hands to the POINTS.

`diffuse` / `specular` (DSS/core/lighting.py:10-77, :80-172) run UNMODIFIED, imported from where they lie (the route of
`make_golden_light_grads.py`: `make_golden_setup.py`'s stubs for the absent third-party packages and the same stand-in
for pytorch3d's `convert_to_tensors_and_broadcast`), in fp64 with requires_grad on the positions, the normals and the base
colours, combined as LightingTexture.forward combines them (`points_rgb * (ambient + diffuse) + specular`,
texture.py:118-122, the ambient colour summed over lights, :48-52).  Three clouds of 300 / 37 / 129 random points with
L = 2 lights each, un-normalised normals (every 7th scaled by 30) and a fixed upstream gradient; a FOURTH cloud of special
rows built from exactly representable numbers (axis-aligned vectors, powers of two), so that an fp32 kernel and this fp64
run take the same branch at each kink.  Its camera is at (0,0,4), its lights are (0,0,2) and (2,0,0) (location or
direction), and unless stated the point is the origin, so v^ = d^_0 = (0,0,1) and d^_1 = (1,0,0):

    a  normal (0,2,0)        ca == 0 exactly for both lights
    b  normal (4,0,0)        light 1: ca = 1 > 0 and r = (1,0,0), a0 = v^ . r == 0 exactly (light 0: ca == 0)
    c  normal (0,0,-1)       light 0: ca = -1 < 0 while v^ . r = 1 > 0: the specular term is gated off
    d  normal (0,1,2^-20)    light 0: a grazing pair, ca = 2^-20 (in fp32 exactly; in fp64 2^-20 / (1 + 2^-41));
                             light 1: ca == 0
    e  normal (0,0,0)        a zero normal
    f  normal (0,0,3e-7)     |m| below the clamp: n^ = m * 1e6 of length 0.3, gradient g * 1e6
    g  point (0,0,2)         at point light 0's location (u = 0), normal (1,0,0)
    h  point (0,0,4)         at its camera's centre (w = 0), normal (0,0,-1)

A special row at which the reference yields a non-finite value in any case is dropped from the fixture (`special_tags`
names the rows kept).  Dropped rows: none -- F.normalize clamps its denominator, and torch's relu / pow have zero
subgradients at the kinks, so every row above is finite.

Every input is an fp32-representable number stored as fp64 (the per-light ambient colours are multiples of 2^-12, so their
sum over lights is fp32-representable too): a test that casts the inputs to fp32 hands the kernel the same numbers.
Cases: point and directional lights at shininess 1, 24 and 64; per case `shaded`, `grad_points`, `grad_normals`,
`grad_rgb` -- arrays only.

    python tests/golden/make_golden_point_grads.py
"""
import importlib
import os

import numpy as np
import torch

import make_golden_setup  # noqa: F401  (installs the stubs and puts the reference on sys.path; writes nothing on import)
from make_golden_light_grads import _ctb

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64
SHININESS = (1.0, 24.0, 64.0)
# Seed: an entry of a normalisation Jacobian, z_i - h_i (h . z), may cancel; two fp64 evaluations of it then agree to
# eps x the cancellation only.  Of the seeds 20 ... 31 this one cancels least (closed form vs autograd <= 6e-14 of the sum
# of absolute terms), which leaves the CPU test's 1e-12 its meaning.
SEED = 20

SPECIAL = (  # tag, point, normal
    ("a", (0.0, 0.0, 0.0), (0.0, 2.0, 0.0)),
    ("b", (0.0, 0.0, 0.0), (4.0, 0.0, 0.0)),
    ("c", (0.0, 0.0, 0.0), (0.0, 0.0, -1.0)),
    ("d", (0.0, 0.0, 0.0), (0.0, 1.0, 2.0 ** -20)),
    ("e", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    ("f", (0.0, 0.0, 0.0), (0.0, 0.0, float(np.float32(3e-7)))),
    ("g", (0.0, 0.0, 2.0), (1.0, 0.0, 0.0)),
    ("h", (0.0, 0.0, 4.0), (0.0, 0.0, -1.0)),
)


def _inputs(special, seed=SEED):
    """-> dict of fp64 tensors holding fp32-representable numbers; `special`: the rows of the fourth cloud"""
    g = torch.Generator().manual_seed(seed)
    f32 = lambda fn, *s: fn(*s, generator=g, dtype=torch.float32)
    num = [300, 37, 129, len(special)]
    R, N, L = sum(num[:3]), 4, 2
    P = sum(num)
    pts = f32(torch.randn, P, 3) * 0.6
    nrm = f32(torch.randn, P, 3)
    nrm[::7] *= 30.0                      # un-normalised normals, like bunny-8000.ply
    rgb = f32(torch.rand, P, 3)
    grad_out = f32(torch.randn, P, 3)
    amb = torch.randint(0, 1229, (N, L, 3), generator=g).float() / 4096.0   # < 0.3; exact sums over lights in fp32
    kd, ks = f32(torch.rand, N, L, 3), f32(torch.rand, N, L, 3)
    vec, cam = f32(torch.randn, N, L, 3) * 2.0, f32(torch.randn, N, 3) * 3.0
    for k, (_tag, x, m) in enumerate(special):
        pts[R + k], nrm[R + k] = torch.tensor(x), torch.tensor(m)
    vec[3] = torch.tensor([[0.0, 0.0, 2.0], [2.0, 0.0, 0.0]])
    cam[3] = torch.tensor([0.0, 0.0, 4.0])
    t = dict(points=pts, normals=nrm, rgb=rgb, grad_out=grad_out, ambient_color=amb, diffuse_color=kd, specular_color=ks,
             light_vec=vec, cam_center=cam)
    return {k: v.to(F64) for k, v in t.items()}, num


def _run(lighting, t, num, tag, shininess):
    pts, nrm, rgb = (t[k].clone().requires_grad_(True) for k in ("points", "normals", "rgb"))
    P = pts.shape[0]
    batch = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(num)])
    vec = t["light_vec"]
    direction = vec[batch] - pts[:, None, :] if tag == "point" else vec[batch]
    dif = lighting.diffuse(normals=nrm, color=t["diffuse_color"][batch], direction=direction)
    spc = lighting.specular(points=pts, normals=nrm, direction=direction, color=t["specular_color"][batch],
                            camera_position=t["cam_center"][batch], shininess=torch.full((P,), shininess, dtype=F64))
    shaded = rgb * (torch.sum(t["ambient_color"], dim=1)[batch] + dif) + spc
    assert shaded.dtype == F64
    (shaded * t["grad_out"]).sum().backward()
    return shaded.detach(), pts.grad, nrm.grad, rgb.grad


def main():
    import pytorch3d.renderer as p3r  # the stub
    p3r.convert_to_tensors_and_broadcast = _ctb
    import pytorch3d.renderer.lighting as _pl  # stub submodule: its DirectionalLights / PointLights are inert bases
    p3r.lighting = _pl
    lighting = importlib.import_module("DSS.core.lighting")
    lighting.convert_to_tensors_and_broadcast = _ctb

    special = list(SPECIAL)
    while True:                            # drop the special rows at which the reference is not finite, then run again
        t, num = _inputs(special)
        R = sum(num[:3])
        runs = {(tag, s): _run(lighting, t, num, tag, s) for tag in ("point", "directional") for s in SHININESS}
        finite = torch.stack([torch.isfinite(a[R:]).all(1) for r in runs.values() for a in r]).all(0)
        if bool(finite.all()):
            break
        print("dropped (non-finite in the reference):", [sp[0] for sp, ok in zip(special, finite.tolist()) if not ok])
        special = [sp for sp, ok in zip(special, finite.tolist()) if ok]
    assert all(bool(torch.isfinite(a).all()) for r in runs.values() for a in r)
    assert all(bool((v.float().double() == v).all()) for v in t.values())
    assert bool((t["ambient_color"].sum(1).float().double() == t["ambient_color"].sum(1)).all())
    out = {k: v.numpy() for k, v in t.items()}
    out.update(num=np.asarray(num, np.int64), shininess=np.asarray(SHININESS, np.float64),
               special_tags=np.frombuffer("".join(sp[0] for sp in special).encode(), dtype=np.uint8).copy())
    for (tag, s), r in runs.items():
        for name, a in zip(("shaded", "grad_points", "grad_normals", "grad_rgb"), r):
            out["%s_s%d_%s" % (tag, int(s), name)] = a.numpy()
    np.savez_compressed(os.path.join(HERE, "ref_point_grads.npz"), **out)
    print("ref_point_grads.npz", {k: getattr(v, "shape", v) for k, v in out.items()})


if __name__ == "__main__":
    main()
