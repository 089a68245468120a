"""CPU: differentiable lights -- the fp64 closed form of the light gradients (`tests/light_reference.py`) agrees with
torch.autograd of the restated forward AND with the gradients the reference's own `diffuse` / `specular` hand to its lights
(`tests/golden/ref_light_grads.npz`); the light classes keep the user's tensors on the graph; the new entry point validates
its arguments without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import light_reference as lref
from dss_amd import _lib
from dss_amd.texture import DirectionalLights, PointLights

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_light_grads.npz")
# fp64 round-off: a gradient is a sum of a few hundred terms of ~10 operations each, compared relative to the sum of the
# absolute terms; 1e-12 is ~ 5000 eps
ROUND_OFF = 1e-12


def _case(sizes, shared, seed, L=2):
    g = torch.Generator().manual_seed(seed)
    N = len(sizes)
    Pw = sizes[0] if shared else sum(sizes)
    num = torch.tensor(sizes, dtype=torch.int64)
    first = torch.cumsum(num, 0) - num
    P = int(num.sum())
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    world, normals = r(Pw, 3) * 0.5, r(Pw, 3)
    rgb, grad_out = torch.rand(P, 3, generator=g, dtype=F64), r(P, 3)
    amb, kd, ks = (torch.rand(*s, generator=g, dtype=F64) for s in ((N, 3), (N, L, 3), (N, L, 3)))
    return world, normals, rgb, first, num, amb, kd, ks, r(N, L, 3) * 2, r(N, 3) * 3, grad_out


@pytest.mark.parametrize("point_lights", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("L", [2, 0])
def test_closed_form_matches_autograd(point_lights, shared, L):
    sizes = [37] * 3 if shared else [37, 0, 21]
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = _case(sizes, shared, 5, L)
    shininess = 8.0
    got, A = lref.phong_backward_lights(grad_out, world, normals, rgb, first, num, kd, ks, lvec, point_lights, cam, shininess,
                                        shared)
    ref = lref.phong_backward_lights_autograd(grad_out, world, normals, rgb, first, num, amb, kd, ks, lvec, point_lights,
                                              cam, shininess, shared)
    for g, r, a in zip(got, ref, A):
        assert g.shape == r.shape and (a >= g.abs() - 1e-15).all()
        if g.numel():
            assert (g - r).abs().max() <= ROUND_OFF * a.max()
    if L:
        assert all(float(a.max()) > 0 for a in A)
    if not shared:
        assert all(float(g[1].abs().max()) == 0 for g in got if g.numel())     # the empty cloud


@pytest.mark.parametrize("tag", ["point", "directional"])
def test_closed_form_matches_the_reference_code(tag):
    """ref_light_grads.npz: autograd through the reference's own lighting.py / texture.py arithmetic, fp64"""
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[k])
    num = t("num")
    first = torch.cumsum(num, 0) - num
    got, A = lref.phong_backward_lights(t("grad_out"), t("points"), t("normals"), t("rgb"), first, num, t("diffuse_color"),
                                        t("specular_color"), t("light_vec"), tag == "point", t("cam_center"),
                                        float(z["shininess"]), False)
    assert num.numel() == 3 and z["diffuse_color"].shape == (3, 2, 3) and z[tag + "_grad_light_vec"].dtype == np.float64
    # the ambient colour is summed over lights (texture.py:48-52): every light's ambient gets the camera's gradient
    ref_amb = t(tag + "_grad_ambient_color")
    assert (ref_amb - got[0][:, None, :]).abs().max() <= ROUND_OFF * A[0].max()
    for k, name in ((1, "diffuse_color"), (2, "specular_color"), (3, "light_vec")):
        ref = t("%s_grad_%s" % (tag, name))
        assert float(ref.abs().max()) > 0 and (got[k] - ref).abs().max() <= ROUND_OFF * A[k].max(), name
    # ... and the restated forward is the reference's forward
    amb = t("ambient_color").sum(1)
    out = lref.phong(t("points"), t("normals"), t("rgb"), first, num, amb, t("diffuse_color"), t("specular_color"),
                     t("light_vec"), tag == "point", t("cam_center"), float(z["shininess"]), False)
    assert (out - t(tag + "_shaded")).abs().max() <= 1e-13


@pytest.mark.parametrize("cls", [PointLights, DirectionalLights])
def test_light_tensors_stay_on_the_graph(cls):
    """a tensor handed to the constructor is still the user's leaf after .to() / .clone() / _packed(): the sum over lights of
    the ambient colour and the broadcast of a batch of 1 to N cameras are differentiated by autograd itself"""
    g = torch.Generator().manual_seed(9)
    leaves = dict(ambient_color=torch.rand(1, 2, 3, generator=g), diffuse_color=torch.rand(2, 3, generator=g),
                  specular_color=torch.rand(1, 2, 3, generator=g))
    leaves[cls._vec] = torch.randn(1, 2, 3, generator=g)
    for v in leaves.values():
        v.requires_grad_(True)
    lights = cls(**leaves)
    N = 3
    w = [torch.randn(N, 3, generator=g)] + [torch.randn(N, 2, 3, generator=g) for _ in range(3)]
    for variant in (lights, lights.to("cpu"), lights.clone(), lights.clone().to(torch.device("cpu"))):
        for v in leaves.values():
            v.grad = None
        packed = variant._packed(N)
        assert [tuple(p.shape) for p in packed] == [(N, 3)] + [(N, 2, 3)] * 3
        assert all(p.requires_grad and p.is_contiguous() for p in packed)
        sum((p * wi).sum() for p, wi in zip(packed, w)).backward()
        assert torch.allclose(leaves["ambient_color"].grad, w[0].sum(0)[None, None].expand(1, 2, 3))
        assert torch.allclose(leaves["diffuse_color"].grad, w[1].sum(0))
        assert torch.allclose(leaves["specular_color"].grad, w[2].sum(0)[None])
        assert torch.allclose(leaves[cls._vec].grad, w[3].sum(0)[None])
    # a per-camera batch, fp64 leaves and nested sequences: converted, not detached / accepted as before
    kd = torch.rand(N, 2, 3, generator=g, dtype=F64).requires_grad_(True)
    p = cls(diffuse_color=kd, specular_color=((0.1, 0.2, 0.3), (0.3, 0.2, 0.1)))._packed(N)
    assert p[1].dtype == torch.float32 and not p[2].requires_grad
    p[1].sum().backward()
    assert kd.grad is not None and float(kd.grad.min()) == 1.0


def test_lights_entry_point_validates_without_a_device():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)     # never dereferenced: every call below fails before a launch
    q = lib.dss_phong_backward_lights_workspace
    assert q(0, 10, 1) == 0 and q(1, -1, 1) == 0 and q(1, 10, -1) == 0
    assert q(2, 1000, 0) == q(2, 1000, 1) > 0 and q(2, 1000, 3) >= 3 * q(2, 1000, 1) - 512
    for L in (0, 1, 2, 5):
        row = [q(8, p, L) for p in (0, 1, 5, 1000, 32684, 99790, 1 << 20, (1 << 20) + 1, 1 << 25)]
        assert row == sorted(row) and row[-1] == q(8, 1 << 30, L)      # capped: at most 512 partials per camera and light
    assert q(8, 1 << 25, 2) == 8 * 2 * 512 * 16 * 4
    need = q(2, 1000, 2)
    args = lambda **kw: [kw.get("grad_out", fake)] + [fake] * 5 + [kw.get("N", 2), 500, 1] + [fake] * 4 \
        + [kw.get("L", 2), 1, fake, 64.0, fake, None, fake, None, kw.get("ws", fake), kw.get("nbytes", need), None]
    for kw in (dict(grad_out=None), dict(ws=None), dict(nbytes=need - 1), dict(N=0), dict(L=-1), dict(N=65536)):
        assert lib.dss_phong_backward_lights(*args(**kw)) == -1, kw
        assert b"dss_phong_backward_lights" in lib.dss_last_error(), kw
