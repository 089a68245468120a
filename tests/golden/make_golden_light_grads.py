"""Generates tests/golden/ref_light_grads.npz: the gradients that the REFERENCE's own shading hands to its lights.

The reference keeps the lights on the autograd tape: `apply_lighting` (DSS/core/texture.py:25-63) calls `diffuse` /
`specular` (DSS/core/lighting.py:10-77, :80-172) on the tensor properties of PointLights / DirectionalLights (:175-302;
point lights: direction = location - point, :270-276) and LightingTexture.forward combines them as
`points_rgb * (ambient + diffuse) + specular` (texture.py:118-122), the ambient colour summed over lights (:48-52).  This
script runs those two functions UNMODIFIED, imported from where they lie, in fp64 with requires_grad on the four light
tensors, for three clouds of a few hundred points with two lights each and a fixed upstream gradient, once as point lights
and once as directional lights, and stores the inputs and the four gradients -- arrays only.

The reference module is imported the way `make_golden_setup.py::lighting_vectors` imports it (that module's stubs for the
absent third-party packages, and the same stand-in for pytorch3d's `convert_to_tensors_and_broadcast`, which broadcasts
dim 0).

    python tests/golden/make_golden_light_grads.py
"""
import importlib
import os

import numpy as np
import torch

import make_golden_setup  # noqa: F401  (installs the stubs and puts the reference on sys.path; writes nothing on import)

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64


def _ctb(*args, device="cpu", dtype=torch.float32):
    ts = [a if torch.is_tensor(a) else torch.as_tensor(a, dtype=dtype) for a in args]
    n = max(t.shape[0] if t.dim() > 0 else 1 for t in ts)
    out = []
    for t in ts:
        if t.dim() == 0:
            t = t.reshape(1)
        out.append(t.expand((n,) + tuple(t.shape[1:])) if t.shape[0] == 1 and n > 1 else t)
    return out


def main():
    import pytorch3d.renderer as p3r  # the stub
    p3r.convert_to_tensors_and_broadcast = _ctb
    import pytorch3d.renderer.lighting as _pl  # stub submodule: its DirectionalLights / PointLights are inert bases
    p3r.lighting = _pl
    lighting = importlib.import_module("DSS.core.lighting")
    lighting.convert_to_tensors_and_broadcast = _ctb

    g = torch.Generator().manual_seed(11)
    num = [300, 420, 260]
    P, N, L = sum(num), 3, 2
    shininess = 24.0
    pts = torch.randn(P, 3, generator=g, dtype=F64) * 0.6
    nrm = torch.randn(P, 3, generator=g, dtype=F64)
    nrm[::7] *= 30.0                      # un-normalised normals, like bunny-8000.ply
    rgb = torch.rand(P, 3, generator=g, dtype=F64)
    grad_out = torch.randn(P, 3, generator=g, dtype=F64)
    batch = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(num)])
    amb = torch.rand(N, L, 3, generator=g, dtype=F64) * 0.3        # (N,L,3): summed over lights like texture.py:48-52
    kd = torch.rand(N, L, 3, generator=g, dtype=F64)
    ks = torch.rand(N, L, 3, generator=g, dtype=F64)
    vec = torch.randn(N, L, 3, generator=g, dtype=F64) * 2.0
    cam = torch.randn(N, 3, generator=g, dtype=F64) * 3.0
    out = dict(points=pts.numpy(), normals=nrm.numpy(), rgb=rgb.numpy(), grad_out=grad_out.numpy(),
               num=np.asarray(num, np.int64), ambient_color=amb.numpy(), diffuse_color=kd.numpy(),
               specular_color=ks.numpy(), light_vec=vec.numpy(), cam_center=cam.numpy(), shininess=np.float64(shininess))
    for tag in ("point", "directional"):
        leaves = [t.clone().requires_grad_(True) for t in (amb, kd, ks, vec)]
        a, d, s, v = leaves
        direction = v[batch] - pts[:, None, :] if tag == "point" else v[batch]
        dif = lighting.diffuse(normals=nrm, color=d[batch], direction=direction)
        spc = lighting.specular(points=pts, normals=nrm, direction=direction, color=s[batch],
                                camera_position=cam[batch], shininess=torch.full((P,), shininess, dtype=F64))
        ambient = torch.sum(a, dim=1)[batch]
        shaded = rgb * (ambient + dif) + spc
        assert shaded.dtype == F64
        (shaded * grad_out).sum().backward()
        out[tag + "_shaded"] = shaded.detach().numpy()
        for name, t in zip(("ambient_color", "diffuse_color", "specular_color", "light_vec"), leaves):
            out["%s_grad_%s" % (tag, name)] = t.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "ref_light_grads.npz"), **out)
    print("ref_light_grads.npz", {k: getattr(v, "shape", v) for k, v in out.items()})


if __name__ == "__main__":
    main()
