"""GPU: the shading's POINT side -- `ops.phong_forward` / `ops.phong_backward` (`phong_kernel<false/true>`) against the
fp64 closed form of `tests/shading_reference.py` and against the gradients of the reference's own `diffuse` / `specular`
(``tests/golden/ref_point_grads.npz``), entry by entry.

Error bookkeeping: every entry of `out`, `grad_world`, `grad_normals` and `grad_rgb` is compared with its fp64 value
RELATIVE TO ``A = sum |term|`` of that entry (a term: one (camera, light) contribution, after its own normalisation
Jacobian), ``|got - ref| <= bar * A`` (+ `shading_reference.UNDERFLOW` = 1e-30 absolute, for the terms fp32 cannot hold at
all); entries without a term must be exact zeros.  Each test prints the largest observed ratio per output.

The bars (`shading_reference.BARS`): for every (case, light kind, shininess) the same formula ran in plain fp32 torch on the
CPU against fp64; a bar is 4 x that figure rounded up to one significant digit (the kernel's operation order and its powf
differ from torch's by a few ulp; `tests/test_shading_points_cpu.py` shows that each of ten wrong formulas lies at least
10 x beyond a bar, and re-measures the figures).  The figures differ this much between cases because a single entry of a
normalisation Jacobian, z_i - h_i (h . z), may cancel: the worst-conditioned entry of a case sets its figure.

fp32 torch on the CPU / bar / kernel on an MI355X, largest |err| / A per output:

    case           lights       s  out                       grad_world                grad_normals              grad_rgb
    fixture        point        1  5.8e-07/3e-06/5.8e-07   2.4e-05/1e-04/2.1e-06   3.0e-05/2e-04/4.9e-06   3.2e-07/2e-06/3.2e-07
    fixture        point       24  3.2e-06/2e-05/2.0e-06   2.4e-05/1e-04/6.4e-06   3.6e-05/2e-04/2.6e-05   3.2e-07/2e-06/3.2e-07
    fixture        point       64  6.6e-06/3e-05/4.7e-06   2.4e-05/1e-04/1.0e-05   1.8e-05/8e-05/1.8e-05   3.2e-07/2e-06/3.2e-07
    fixture        directional  1  7.0e-07/3e-06/6.2e-07   7.1e-06/3e-05/1.4e-05   1.4e-05/6e-05/6.2e-06   3.1e-07/2e-06/3.1e-07
    fixture        directional 24  2.1e-06/9e-06/2.7e-06   2.5e-05/1e-04/4.6e-05   5.9e-06/3e-05/5.6e-06   3.1e-07/2e-06/3.1e-07
    fixture        directional 64  5.4e-06/3e-05/5.4e-06   3.6e-05/2e-04/4.7e-05   1.1e-05/5e-05/2.4e-05   3.1e-07/2e-06/3.1e-07
    ragged         point       12  1.7e-06/7e-06/2.5e-06   5.9e-05/3e-04/1.0e-05   2.1e-05/9e-05/1.3e-05   5.8e-07/3e-06/5.8e-07
    ragged         point       64  5.0e-06/3e-05/1.1e-05   5.9e-05/3e-04/2.0e-05   1.5e-05/7e-05/1.6e-05   5.8e-07/3e-06/5.8e-07
    ragged         directional 12  2.3e-06/1e-05/2.1e-06   3.3e-05/2e-04/3.3e-05   4.5e-05/2e-04/3.0e-05   3.6e-07/2e-06/3.6e-07
    ragged         directional 64  5.8e-06/3e-05/5.8e-06   3.2e-05/2e-04/3.2e-05   1.3e-04/6e-04/2.2e-04   3.6e-07/2e-06/3.6e-07
    gap            point       12  2.4e-06/1e-05/1.4e-06   1.2e-04/5e-04/1.1e-05   2.5e-04/1e-03/1.9e-05   2.4e-07/1e-06/2.5e-07
    gap            point       64  4.0e-06/2e-05/4.0e-06   1.2e-04/5e-04/1.1e-05   2.2e-05/9e-05/1.7e-05   2.4e-07/1e-06/2.5e-07
    gap            directional 12  2.3e-06/1e-05/2.3e-06   6.9e-05/3e-04/4.3e-05   2.0e-05/8e-05/1.4e-05   1.9e-07/8e-07/2.0e-07
    gap            directional 64  5.1e-06/3e-05/5.8e-06   7.6e-05/4e-04/7.1e-05   4.7e-05/2e-04/9.8e-06   1.9e-07/8e-07/2.0e-07
    shared3        point       12  2.5e-06/2e-05/3.1e-06   5.6e-06/3e-05/5.3e-06   8.2e-06/4e-05/3.4e-06   6.7e-07/3e-06/6.7e-07
    shared3        point       64  8.7e-06/4e-05/8.7e-06   1.8e-05/8e-05/1.8e-05   2.6e-05/2e-04/1.7e-05   6.7e-07/3e-06/6.7e-07
    shared3        directional 12  1.9e-06/8e-06/2.4e-06   4.9e-05/2e-04/4.9e-05   8.8e-06/4e-05/9.4e-06   8.2e-07/4e-06/8.2e-07
    shared3        directional 64  4.8e-06/2e-05/1.0e-05   2.5e-05/1e-04/2.6e-05   2.0e-05/9e-05/1.9e-05   8.2e-07/4e-06/8.2e-07
    shared1        point       12  1.7e-06/7e-06/1.7e-06   9.7e-06/4e-05/4.8e-06   1.6e-05/7e-05/8.6e-06   3.4e-07/2e-06/2.7e-07
    shared1        point       64  2.9e-06/2e-05/2.9e-06   9.7e-06/4e-05/9.7e-06   1.6e-05/7e-05/1.4e-05   3.4e-07/2e-06/2.7e-07
    shared1        directional 12  2.2e-06/9e-06/2.2e-06   8.3e-05/4e-04/5.9e-05   1.5e-05/7e-05/7.2e-06   2.7e-07/2e-06/3.6e-07
    shared1        directional 64  9.9e-06/4e-05/9.9e-06   7.5e-05/4e-04/5.6e-05   1.4e-05/6e-05/1.3e-05   2.7e-07/2e-06/3.6e-07
    single         point       12  3.0e-06/2e-05/3.0e-06   1.6e-05/7e-05/2.7e-05   2.1e-05/9e-05/2.1e-05   1.4e-07/6e-07/1.6e-07
    single         point       64  4.4e-06/2e-05/4.5e-06   1.6e-05/7e-05/2.7e-05   1.2e-05/5e-05/8.2e-06   1.4e-07/6e-07/1.6e-07
    single         directional 12  7.5e-07/3e-06/1.2e-06   3.7e-05/2e-04/3.7e-05   1.5e-05/7e-05/1.2e-05   1.4e-07/6e-07/1.4e-07
    single         directional 64  2.5e-06/1e-05/4.2e-06   1.8e-05/8e-05/1.7e-05   1.3e-05/6e-05/9.6e-06   1.4e-07/6e-07/1.4e-07
    L0             point       12  5.8e-08/3e-07/5.8e-08   0.0e+00/0e+00/0.0e+00   0.0e+00/0e+00/0.0e+00   5.9e-08/3e-07/5.9e-08
    L0             point       64  5.8e-08/3e-07/5.8e-08   0.0e+00/0e+00/0.0e+00   0.0e+00/0e+00/0.0e+00   5.9e-08/3e-07/5.9e-08
    L0             directional 12  5.8e-08/3e-07/5.8e-08   0.0e+00/0e+00/0.0e+00   0.0e+00/0e+00/0.0e+00   5.9e-08/3e-07/5.9e-08
    L0             directional 64  5.8e-08/3e-07/5.8e-08   0.0e+00/0e+00/0.0e+00   0.0e+00/0e+00/0.0e+00   5.9e-08/3e-07/5.9e-08
    L1             point       12  2.3e-06/1e-05/1.7e-06   1.4e-05/6e-05/6.9e-06   8.4e-06/4e-05/6.7e-06   6.3e-07/3e-06/6.3e-07
    L1             point       64  2.6e-06/2e-05/2.6e-06   1.6e-05/7e-05/1.6e-05   7.6e-04/4e-03/7.5e-04   6.3e-07/3e-06/6.3e-07
    L1             directional 12  1.9e-06/8e-06/1.9e-06   2.4e-05/1e-04/2.4e-05   4.6e-05/2e-04/1.4e-05   4.0e-07/2e-06/4.8e-07
    L1             directional 64  9.3e-06/4e-05/9.3e-06   2.3e-05/1e-04/2.3e-05   1.3e-05/6e-05/1.1e-05   4.0e-07/2e-06/4.8e-07
    L3             point       12  2.2e-06/9e-06/2.3e-06   9.4e-06/4e-05/4.7e-06   1.5e-05/6e-05/5.5e-06   3.0e-07/2e-06/2.6e-07
    L3             point       64  1.1e-05/5e-05/1.1e-05   3.3e-05/2e-04/3.3e-05   9.3e-05/4e-04/5.4e-05   3.0e-07/2e-06/2.6e-07
    L3             directional 12  2.8e-06/2e-05/2.8e-06   3.1e-05/2e-04/7.0e-05   2.3e-05/1e-04/5.5e-06   2.1e-07/9e-07/2.0e-07
    L3             directional 64  5.7e-06/3e-05/5.8e-06   2.2e-05/9e-05/2.5e-05   2.1e-05/9e-05/2.1e-05   2.1e-07/9e-07/2.0e-07
    shared_partial point       12  2.5e-06/2e-05/3.1e-06   7.9e-06/4e-05/5.3e-06   8.2e-06/4e-05/3.4e-06   6.7e-07/3e-06/6.7e-07
    shared_partial point       64  8.7e-06/4e-05/8.7e-06   1.8e-05/8e-05/1.8e-05   2.6e-05/2e-04/1.7e-05   6.7e-07/3e-06/6.7e-07
    shared_partial directional 12  1.9e-06/8e-06/2.4e-06   5.7e-05/3e-04/5.7e-05   8.8e-06/4e-05/9.4e-06   8.2e-07/4e-06/8.2e-07
    shared_partial directional 64  2.8e-06/2e-05/1.0e-05   2.5e-05/1e-04/2.6e-05   2.0e-05/9e-05/1.9e-05   8.2e-07/4e-06/8.2e-07
    scaled         point       12  3.2e-06/2e-05/3.2e-06   1.9e-05/8e-05/1.7e-05   2.1e-05/9e-05/7.8e-06   7.2e-07/3e-06/7.2e-07
    scaled         point       64  9.9e-06/4e-05/9.9e-06   4.0e-05/2e-04/4.0e-05   1.5e-05/6e-05/1.5e-05   7.2e-07/3e-06/7.2e-07
    scaled         directional 12  2.7e-06/2e-05/2.9e-06   2.0e-05/9e-05/1.9e-05   1.4e-04/6e-04/1.3e-04   3.0e-07/2e-06/2.6e-07
    scaled         directional 64  1.4e-05/6e-05/1.4e-05   2.9e-05/2e-04/2.9e-05   8.2e-05/4e-04/3.2e-05   3.0e-07/2e-06/2.6e-07

    scaled normals (test_the_length_of_a_normal_does_not_matter): out vs unscaled | factor x grad_normals | |m . grad_normals|
    scaled         point       12  3.1e-06/2e-05/3.1e-06   2.0e-05/9e-05/7.6e-06   4.5e-06/2e-05/4.2e-08
    scaled         point       64  9.7e-06/4e-05/9.7e-06   1.5e-05/6e-05/1.6e-05   4.2e-06/2e-05/4.2e-08
    scaled         directional 12  2.7e-06/2e-05/2.8e-06   1.5e-04/6e-04/1.4e-04   4.4e-06/2e-05/5.2e-08
    scaled         directional 64  1.4e-05/6e-05/1.4e-05   8.7e-05/4e-04/3.4e-05   8.3e-06/4e-05/4.2e-08

    the three kernels (test_the_three_phong_kernels_agree): |sum| / summed A
    ragged         point       12  3.1e-09/2e-08/1.5e-09
    ragged         directional 12  2.7e-08/2e-07/1.5e-08
    shared3        point       12  1.4e-09/6e-09/2.2e-09
    shared3        directional 12  4.6e-09/2e-08/8.9e-09
    big            point       64  2.8e-09/2e-08/7.0e-10
    big            directional 64  1.7e-08/7e-08/5.9e-09
    big_shared3    point       64  5.0e-10/3e-09/5.6e-10
    big_shared3    directional 64  2.8e-09/2e-08/1.7e-09

    the module (test_module_point_gradients_match_fp64_autograd; bars derived at run time): bar/kernel
    per-camera     PointLights         3e-05/6.1e-06  9e-05/2.1e-05  8e-05/2.0e-05  3e-06/6.1e-07
    per-camera     DirectionalLights   3e-05/6.0e-06  2e-04/2.8e-05  8e-05/2.4e-05  2e-06/3.8e-07
    shared         PointLights         5e-05/1.4e-05  2e-04/3.7e-05  2e-04/3.7e-05  6e-07/1.8e-07
    shared         DirectionalLights   2e-05/1.5e-05  2e-04/3.0e-05  1e-04/2.5e-05  6e-07/1.8e-07

The kernel evaluates the normalisation Jacobian in fp64 from its fp32 inputs (`normalize_backward`) because of this test.
With the Jacobian in fp32 seven comparisons lay beyond their bars, each at ONE entry, the one whose Jacobian cancels most
(kappa = the magnitude before the cancellation over A; the median entry has 1.8): fixture point s=64 grad_normals, point
186 z, kappa 1768: 1.1e-4 against the bar 8e-5; shared3 point s=12 grad_normals, point 185 y, kappa 629: 6.1e-5 against
4e-5; shared3 directional s=64 grad_world, point 109 x, kappa 1257: 1.3e-4 against 1e-4; single point s=12 / 64
grad_world, point 38 x, kappa 1899: 9.0e-5 against 7e-5 ("shared_partial" repeats "shared3").  An fp32 restatement of the
kernel on the CPU, operation for operation, reproduced those figures to the digit, and with the Jacobian alone in fp64 it
gave 1.8e-5, 3.4e-6, 2.6e-5 and 2.7e-5: the roundings of 1 / |u|, h and h . g inside the Jacobian were what the
cancellation amplified, not the kernel's inputs to it.
"""
import numpy as np
import pytest
import torch

import shading_reference as sr
from dss_amd import _lib, ops
from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
from dss_amd.cloud import PointClouds3D
from dss_amd.texture import DirectionalLights, LightingTexture, PointLights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KIND_SHIN = [(k, s) for k in sr.KINDS for s in (12.0, 64.0)]


def _dev(case):
    return [t.to(DEV) if t.dtype == torch.int64 else t.float().to(DEV) for t in case]


def _kernels(case, shared, kind, shin):
    """-> (out, grad_world, grad_normals, grad_rgb) of the two operators"""
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = _dev(case)
    out = ops.phong_forward(world, normals, rgb, first, num, amb, kd, ks, lvec, kind == "point", cam, shin, shared)
    back = ops.phong_backward(grad_out, world, normals, rgb, first, num, amb, kd, ks, lvec, kind == "point", cam, shin, shared)
    return (out,) + tuple(back)


def _check(tag, got, ref, A, bars, own=None):
    """the per-entry check of every comparison here (`own`: compare out / grad_rgb on these packed rows only)"""
    worst = []
    for name, g, r, a in zip(sr.OUTPUTS, got, ref, A):
        g = g.detach().cpu()
        if own is not None and name in ("out", "grad_rgb"):
            g, r, a = g[own], r[own], a[own]
        w, zeros_ok = sr.entry_ratio(g, r, a)
        assert zeros_ok, "%s %s: entries without a term must be exact zeros" % (tag, name)
        worst.append(w)
    print("phong points %-34s max |err| / A: %s" % (tag, "  ".join("%s %.1e (bar %.0e)" % (n, w, b)
                                                                     for n, w, b in zip(sr.OUTPUTS, worst, bars))))
    for name, w, b in zip(sr.OUTPUTS, worst, bars):
        assert w <= b, (tag, name, w, b)


@pytest.fixture(scope="module")
def golden():
    z = np.load(sr.GOLDEN)
    return z, sr.fixture_case(z)


@pytest.mark.parametrize("shin", [1.0, 24.0, 64.0])
@pytest.mark.parametrize("kind", sr.KINDS)
def test_against_the_reference_codes_gradients(golden, kind, shin):
    """ref_point_grads.npz: 300 / 37 / 129 points and the eight special rows (kinks and clamped normalisations)"""
    z, (case, shared) = golden
    got = _kernels(case, shared, kind, shin)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    _vals, A = sr.run_case(case, shared, kind, shin)
    _check("fixture %s s=%d" % (kind, shin), got, sr.fixture_expected(z, kind, shin), A, sr.BARS[("fixture", kind, int(shin))])


@pytest.mark.parametrize("kind,shin", KIND_SHIN)
@pytest.mark.parametrize("name", list(sr.LAYOUTS))
def test_layouts_against_the_closed_form(name, kind, shin):
    case, shared = sr.layout_case(name)
    got = _kernels(case, shared, kind, shin)
    vals, A = sr.run_case(case, shared, kind, shin)
    # a shared cloud whose camera owns fewer than Pw points leaves that camera's missing rows unspecified
    own = sr.owned_rows(case, shared) if shared else None
    _check("%s %s s=%d" % (name, kind, shin), got, vals, A, sr.BARS[(name, kind, int(shin))], own)
    if case[6].shape[1] == 0:          # L = 0: out = rgb * ambient, grad_rgb = g * ambient, nothing reaches x or m
        world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = _dev(case)
        amb_of = amb[torch.repeat_interleave(torch.arange(len(num), device=DEV), num)]
        assert torch.equal(got[0], rgb * amb_of) and torch.equal(got[3], grad_out * amb_of)
        assert (got[1] == 0).all() and (got[2] == 0).all()


@pytest.mark.parametrize("kind", sr.KINDS)
def test_rows_that_no_cloud_owns_are_zeros(kind):
    """the gap layout on memory that held NaN: the caching allocator hands the freed blocks to the operators' outputs"""
    case, shared = sr.layout_case("gap")
    own = sr.owned_rows(case, shared)
    assert int((~own).sum()) == 64 + 36 + 63
    for _ in range(2):
        junk = [torch.full((case[0].shape[0], 3), float("nan"), device=DEV) for _ in range(4)]
        del junk
        for t in _kernels(case, shared, kind, 64.0):
            assert bool((t[~own.to(DEV)] == 0).all()) and bool(torch.isfinite(t).all())


@pytest.mark.parametrize("kind,shin", KIND_SHIN)
def test_the_length_of_a_normal_does_not_matter(kind, shin):
    """"scaled" = "ragged" with every normal times a factor in [1e-3, 1e3]: `out` stays (against the UNSCALED fp64 value),
    grad_normals divides by the factor, and m . grad_normals = 0"""
    case, shared = sr.layout_case("scaled")
    got = _kernels(case, shared, kind, shin)
    ratios, bars = sr.scale_ratios(got[0], got[2], kind, shin), sr.SCALE_BARS[(kind, int(shin))]
    print("phong points scaled normals %s s=%d: out %.1e (bar %.0e)  factor x grad_normals %.1e (bar %.0e)  "
          "|m . grad_normals| %.1e (bar %.0e)" % ((kind, shin) + tuple(x for rb in zip(ratios, bars) for x in rb)))
    assert all(r <= b for r, b in zip(ratios, bars)), (ratios, bars)


@pytest.mark.parametrize("name,kind,shin", sr.IDENTITY_CASES, ids=["%s-%s-%d" % c for c in sr.IDENTITY_CASES])
def test_the_three_phong_kernels_agree(name, kind, shin):
    """translation: sum_p grad_world (phong_kernel) + sum_n grad_cam (phong_camera_partial_kernel) + sum_{n,l}
    grad_light_vec (phong_light_partial_kernel, point lights) = 0 relative to the summed absolute terms of the three.
    At shininess 64 one cloud of 20,011 points (test_gpu_camera_grad.py: the smallest at which such a sum is not limited
    by the format)."""
    case, shared = sr.identity_case(name)
    args = _dev(case)
    point = kind == "point"
    gw, _gn, _gc = ops.phong_backward(args[10], *args[:9], point, args[9], float(shin), shared)
    gcam = ops.phong_backward_camera(args[10], *args[:9], point, args[9], float(shin), shared)
    glv = ops.phong_backward_lights(args[10], *args[:9], point, args[9], float(shin), shared,
                                    needs=(False, False, False, True))[3]
    ratio, bar = sr.identity_ratio(case, shared, kind, float(shin), gw, gcam, glv), sr.IDENTITY_BARS[(name, kind, shin)]
    print("phong points three kernels %s %s s=%d: |sum| / A = %.1e (bar %.0e)" % (name, kind, shin, ratio, bar))
    assert ratio <= bar, (ratio, bar)


def _pair_case(N, Pw, shared, L, seed=5):
    """A case (in the order of `sr.layout_case`) in which every (camera, point, light) is lit with a0 > 0: the points near
    the origin with normals about +z, the cameras and the lights (locations or directions alike) above them.  Not shared:
    N clouds of ONE point each (Pw = N)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    P = N * Pw if shared else Pw
    up = torch.tensor([0.0, 0.0, 1.0])
    world, normals = 0.2 * r(Pw, 3), 1.7 * (up + 0.2 * r(Pw, 3))
    rgb, grad_out = u(P, 3), r(P, 3)
    amb, kd, ks = u(N, 3) * 0.5, u(N, L, 3), u(N, L, 3)
    lvec, cam = 2.5 * up + 0.4 * r(N, L, 3), 3.0 * up + 0.4 * r(N, 3)
    per = Pw if shared else 1
    first, num = torch.arange(N, dtype=torch.int64) * per, torch.full((N,), per, dtype=torch.int64)
    return (world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out), shared


def _all_lit(case, shared, point):
    """ca > 0.5 and a0 > 0.5 for every (camera, point, light) of the case (fp64, on the CPU)"""
    world, normals, _rgb, first, num, _amb, _kd, _ks, lvec, cam, _g = [t.double() if t.is_floating_point() else t for t in case]
    unit = lambda t: torch.nn.functional.normalize(t, dim=1)
    for n in range(len(num)):
        rows = slice(0, int(num[n])) if shared else slice(int(first[n]), int(first[n] + num[n]))
        x, nh = world[rows], unit(normals[rows])
        v = unit(cam[n][None] - x)
        for l in range(lvec.shape[1]):
            d = unit(lvec[n, l][None] - x if point else lvec[n, l][None].expand_as(x))
            ca = (nh * d).sum(1, keepdim=True)
            a0 = (v * (-d + 2.0 * ca * nh)).sum(1)
            if not (float(ca.min()) > 0.5 and float(a0.min()) > 0.5):
                return False
    return True


def _three_kernels(case, shared, point, shin):
    """-> grad_world (Pw,3), grad_cam (N,3), (grad_ambient, grad_diffuse, grad_specular, grad_light_vec)"""
    args = _dev(case)
    a = (args[10], *args[:9], point, args[9], float(shin), shared)
    return ops.phong_backward(*a)[0], ops.phong_backward_camera(*a), ops.phong_backward_lights(*a)


@pytest.mark.parametrize("shin", [12.0, 64.0])
def test_one_pair_links_the_three_kernels_bit_for_bit(shin):
    """With a single pair per camera every reduction tree adds one value to zeros, so the pair's gw = J(w)^T gv and
    gu = J(u)^T gdv of phong_kernel<true>, phong_camera_partial_kernel and phong_light_partial_kernel (one statement of
    the arithmetic: csrc/phong.h) meet under `torch.equal`: grad_world = 0 - gu - gw per camera in turn."""
    # three clouds of one point each, two directional lights: only the view direction reaches the position
    case, shared = _pair_case(3, 3, False, 2)
    assert _all_lit(case, shared, False)
    gw, gcam, _gl = _three_kernels(case, shared, False, shin)
    assert bool((gw != 0).all()) and bool((gcam != 0).all())
    assert torch.equal(gw, -gcam)
    # the same layout, one point light: the light's location moves with the point as well
    case, shared = _pair_case(3, 3, False, 1)
    assert _all_lit(case, shared, True)
    gw, gcam, gl = _three_kernels(case, shared, True, shin)
    assert bool((gw != 0).all()) and bool((gcam != 0).all()) and bool((gl[3] != 0).all())
    assert torch.equal(gw, -(gl[3][:, 0] + gcam))
    # one point shared by two cameras, directional lights: the cameras in order
    case, shared = _pair_case(2, 1, True, 2)
    assert _all_lit(case, shared, False)
    gw, gcam, _gl = _three_kernels(case, shared, False, shin)
    assert bool((gw != 0).all()) and bool((gcam != 0).all())
    assert torch.equal(gw[0], -(gcam[0] + gcam[1]))


@pytest.mark.parametrize("kind,shin", KIND_SHIN)
def test_one_pair_links_the_specular_gradient_to_the_forward_bit_for_bit(kind, shin):
    """ambient 0, kd = 0, ks = 1: `out` of phong_kernel<false> is S of the pair's one light, and grad_specular of
    phong_light_partial_kernel is grad_out * S, one light at a time"""
    case, shared = _pair_case(3, 3, False, 2)
    point = kind == "point"
    assert _all_lit(case, shared, point)
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    case = (world, normals, rgb, first, num, amb * 0, kd * 0, ks * 0 + 1, lvec, cam, grad_out)
    g_spec = _three_kernels(case, shared, point, shin)[2][2]
    assert bool((g_spec != 0).all())
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = _dev(case)
    for l in range(2):
        one = slice(l, l + 1)
        S = ops.phong_forward(world, normals, rgb, first, num, amb, kd[:, one], ks[:, one], lvec[:, one], point, cam, shin,
                              shared)
        assert bool((S != 0).all()) and torch.equal(g_spec[:, l], grad_out * S)


@pytest.mark.parametrize("name", ["ragged", "shared3"])
def test_null_outputs_and_reproducibility(name):
    case, shared = sr.layout_case(name)
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = _dev(case)
    dev, N, Pw, P, L, lead = ops._phong_common(world, normals, rgb, first, num, shared, amb, kd, ks, lvec, True, cam, 64.0,
                                               grad_out, "phong_backward")
    shapes = ((Pw, 3), (Pw, 3), (P, 3))

    def call(needs):
        outs = [torch.full(s, 7.0, device=DEV) if need else None for need, s in zip(needs, shapes)]
        _lib.call("dss_phong_backward", dev, *lead, *outs)
        return outs

    full = call((True, True, True))
    assert all(bool((t != 7.0).any()) for t in full)
    for needs in ((False, True, True), (True, False, True), (True, True, False),
                  (True, False, False), (False, True, False), (False, False, True)):
        for need, part, whole in zip(needs, call(needs), full):
            assert (part is None) != need and (part is None or torch.equal(part, whole))
    call((False, False, False))                                   # nothing asked for: nothing written, no error
    # an unrelated launch in between
    other, other_shared = sr.layout_case("L3")
    _kernels(other, other_shared, "directional", 12.0)
    torch.randn(1 << 20, device=DEV).sum()
    assert all(torch.equal(a, b) for a, b in zip(call((True, True, True)), full))


# ---------------------------------------------------------------------------------------------------------------------
# the public path
@pytest.mark.parametrize("cls", [PointLights, DirectionalLights])
@pytest.mark.parametrize("shared", [False, True], ids=["per-camera", "shared"])
def test_module_point_gradients_match_fp64_autograd(cls, shared):
    """LightingTexture, per-camera clouds [300, 37, 129] or one cloud of 321 points shared by 3 cameras, shininess 64 (the
    module's default): `.grad` of points, normals and colours per entry against autograd of `camera_reference.phong`.  The
    bars are derived as everywhere: 4 x what fp32 torch loses on these very inputs, rounded up (here at run time: the
    camera centres come from the module)."""
    N, L, shin = 3, 2, 64.0
    sizes = [321] if shared else [300, 37, 129]
    g = torch.Generator().manual_seed(17)
    R, T = look_at_view_transform(2.0, [25.0, 10.0, 40.0], [45.0, 150.0, 260.0])
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T, device=DEV)
    centre = cams.get_camera_center().cpu()
    leaf = lambda t: t.to(DEV).requires_grad_(True)
    X = [leaf(torch.randn(n, 3, generator=g) * 0.5) for n in sizes]
    M = [torch.randn(n, 3, generator=g) for n in sizes]
    for m in M:
        m[::5] *= 20.0
    M = [leaf(m) for m in M]
    C = [leaf(torch.rand(n, 3, generator=g)) for n in sizes]
    amb, kd, ks = (torch.rand(N, L, 3, generator=g) * sc for sc in (0.25, 1.0, 1.0))
    vec = centre[:, None, :] * 1.1 + 0.5 * torch.randn(N, L, 3, generator=g)     # highlights face the viewers
    lights = cls(ambient_color=amb.to(DEV), diffuse_color=kd.to(DEV), specular_color=ks.to(DEV), device=DEV,
                 **{cls._vec: vec.to(DEV)})
    tex = LightingTexture(cameras=cams, lights=lights)
    Pw = sum(sizes)
    P = N * Pw if shared else Pw
    go = torch.randn(P, 3, generator=g)

    def run(**kw):
        for t in X + M + C:
            t.grad = None
        shaded = tex(PointClouds3D(X, M, C), shininess=shin, **kw).features_packed()
        (shaded * go.to(DEV)).sum().backward()
        return [shaded.detach()] + [torch.cat([t.grad for t in ts]) for ts in (X, M, C) if ts[0].grad is not None]

    got = run()
    num = torch.tensor([Pw] * N if shared else sizes, dtype=torch.int64)
    first = torch.cumsum(num, 0) - num
    cat = lambda ts: torch.cat([t.detach().cpu() for t in ts])
    rgb = cat(C).repeat(N, 1) if shared else cat(C)
    packed = [t.detach().cpu() for t in lights._packed(N)]
    case = (cat(X), cat(M), rgb, first, num, packed[0], packed[1], packed[2], packed[3], centre, go)
    vals, A = sr.run_case(case, shared, "point" if cls is PointLights else "directional", shin)
    auto = sr.phong_points_autograd(go, *case[:9], cls is PointLights, centre, shin, shared)
    v32, _ = sr.run_case(case, shared, "point" if cls is PointLights else "directional", shin, dtype=torch.float32)
    fold = (lambda t: t.reshape(N, Pw, 3).sum(0)) if shared else (lambda t: t)     # one colour leaf under N cameras
    ref = [auto[0], auto[1], auto[2], fold(auto[3])]
    A = [A[0], A[1], A[2], fold(A[3])]
    v32 = [v32[0], v32[1], v32[2], fold(v32[3])]
    bars = [sr.round_up_1sig(4 * sr.entry_ratio(f, r, a)[0]) for f, r, a in zip(v32, ref, A)]
    _check("module %s %s" % (cls.__name__, "shared" if shared else "per-camera"), got, ref, A, bars)
    # a non-contiguous view as points_rgb: the bits of the contiguous call
    wide = torch.rand(P, 4, generator=g).to(DEV)
    a, b = run(points_rgb=wide[:, :3]), run(points_rgb=wide[:, :3].contiguous())
    assert not wide[:, :3].is_contiguous() and len(a) == len(b) == 3 and float(a[1].abs().max()) > 0
    assert all(torch.equal(x, y) for x, y in zip(a, b))
