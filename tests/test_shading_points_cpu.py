"""CPU: the yardstick of the shading's point gradients (`tests/shading_reference.py`) is pinned from three sides before
`tests/test_gpu_shading_points.py` measures the kernel with it.

* Agreement: the fp64 closed form, torch.autograd of `camera_reference.phong` and the gradients of the reference's own
  `diffuse` / `specular` (``tests/golden/ref_point_grads.npz``, special rows included) agree to 1e-12 of every entry's sum
  of absolute terms, on every case of the GPU test.
* Identities: translating points, cameras and point lights together changes nothing, and the shading does not depend on
  the length of a normal.
* Discrimination: ten wrong versions of the closed form -- each a one-line mutation of a copy kept here -- go through the
  GPU test's per-entry check with the GPU test's bars, and each exceeds a bar at least tenfold on one of its cases.
* The bars of the GPU test are tied to what plain fp32 torch loses on the same formula.
* The C ABI refuses bad arguments before any launch.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import camera_reference as cref
import light_reference as lref
import shading_reference as sr
from dss_amd import _lib

F64 = torch.float64
# fp64 round-off: an entry is a sum of a few terms of ~30 operations each, compared relative to the sum of the absolute
# terms; 1e-12 is ~ 5000 eps (the seeds keep the cancellation inside a normalisation Jacobian below that, see LAYOUTS)
ROUND_OFF = 1e-12
CASES = [("fixture", k, s) for k in sr.KINDS for s in (1.0, 24.0, 64.0)] \
    + [(name, k, s) for name in sr.LAYOUTS for k in sr.KINDS for s in (12.0, 64.0)]
_id = lambda c: "%s-%s-%d" % c


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return sr.fixture_case(np.load(sr.GOLDEN)) if name == "fixture" else sr.layout_case(name)


@functools.lru_cache(maxsize=None)
def _ref(name, kind, shin):
    case, shared = _inputs(name)
    return sr.run_case(case, shared, kind, shin)


@pytest.mark.parametrize("name,kind,shin", CASES, ids=[_id(c) for c in CASES])
def test_closed_form_autograd_and_reference_code_agree(name, kind, shin):
    case, shared = _inputs(name)
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    vals, A = _ref(name, kind, shin)
    auto = sr.phong_points_autograd(grad_out, world, normals, rgb, first, num, amb, kd, ks, lvec, kind == "point", cam,
                                    shin, shared)
    others = [("autograd", auto)]
    if name == "fixture":
        z = np.load(sr.GOLDEN)
        assert z["special_tags"].tobytes() == b"abcdefgh" and int(z["num"][3]) == 8 and z["light_vec"].shape == (4, 2, 3)
        others.append(("reference code", sr.fixture_expected(z, kind, shin)))
    for who, other in others:
        for out_name, v, a, o in zip(sr.OUTPUTS, vals, A, other):
            assert (a >= v.abs() * (1 - 1e-15)).all()
            worst, zeros_ok = sr.entry_ratio(o, v, a)
            assert zeros_ok and worst <= ROUND_OFF, (who, out_name, worst)
    # rows that no cloud owns: zeros in every output (for a shared cloud: the pairs that a camera does not own)
    own = sr.owned_rows(case, shared)
    assert all(float(t[~own].abs().sum()) == 0 for t in (vals[0], vals[3], A[0], A[3]))
    if not shared:
        assert all(float(t[~own].abs().sum()) == 0 for t in (vals[1], vals[2], A[1], A[2]))
    if kd.shape[1] == 0:
        g, c = grad_out.to(F64), rgb.to(F64)
        n_of = torch.repeat_interleave(torch.arange(len(num)), num)
        assert torch.equal(vals[0][own], c[own] * amb.to(F64)[n_of]) and torch.equal(vals[3][own], g[own] * amb.to(F64)[n_of])
        assert float(vals[1].abs().sum()) == 0 and float(vals[2].abs().sum()) == 0


@pytest.mark.parametrize("name,kind,shin", CASES, ids=[_id(c) for c in CASES])
def test_translation_and_scale_identities(name, kind, shin):
    """sum_p grad_world + sum_n grad_cam (+ sum_{n,l} grad_light_vec for point lights) = 0, against the summed absolute
    terms of the three closed forms; m_p . grad_normals_p = 0 wherever |m_p| is not clamped."""
    case, shared = _inputs(name)
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    vals, A = _ref(name, kind, shin)
    gcam, acam = cref.phong_backward_camera(grad_out, world, normals, first, num, ks, lvec, kind == "point", cam, shin, shared)
    total, scale = vals[1].sum(0) + gcam.sum(0), A[1].sum(0) + acam.sum(0)
    if kind == "point":
        gl, al = lref.phong_backward_lights(grad_out, world, normals, rgb, first, num, kd, ks, lvec, True, cam, shin, shared)
        total, scale = total + gl[3].sum((0, 1)), scale + al[3].sum((0, 1))
    assert (total.abs() <= ROUND_OFF * scale).all(), (total, scale)
    m = normals.to(F64)
    free = m.norm(dim=1) > 1e-6
    assert ((m * vals[2]).sum(1).abs()[free] <= ROUND_OFF * (m.abs() * A[2]).sum(1)[free]).all()


@pytest.mark.parametrize("name,kind,shin", CASES, ids=[_id(c) for c in CASES])
def test_bars_follow_the_fp32_figures(name, kind, shin):
    """A bar is 4 x what the closed form loses in plain fp32 torch, rounded up to one significant digit.  The table was
    filled on one CPU; another one may round a few entries differently, so the tie is asserted as figure <= bar / 2 and
    bar <= 4 x figure rounded up, times 3."""
    case, shared = _inputs(name)
    vals, A = _ref(name, kind, shin)
    v32, _ = sr.run_case(case, shared, kind, shin, dtype=torch.float32)
    figs = []
    for out_name, v, a, f, bar in zip(sr.OUTPUTS, vals, A, v32, sr.BARS[(name, kind, int(shin))]):
        fig, zeros_ok = sr.entry_ratio(f, v, a)
        figs.append(fig)
        assert zeros_ok, out_name
        assert fig <= bar / 2 and bar <= 3 * sr.round_up_1sig(4 * fig), (out_name, fig, bar)
    print("fp32 torch %-28s max |err| / A: %s" % (_id((name, kind, shin)),
                                                   "  ".join("%s %.1e" % (n, f) for n, f in zip(sr.OUTPUTS, figs))))


# ---------------------------------------------------------------------------------------------------------------------
# discrimination
MUTATIONS = ("gca_without_2_ga0_vn", "ga0_without_lit", "ga0_without_a0_gate", "jacobian_without_projection",
             "point_light_chain_sign", "no_view_chain", "clamped_scale_1", "skip_last_shared_camera", "lights_of_camera_0",
             "rgb_row_wi")


def _mutant(mut, grad_out, world, normals, rgb, first, num, ambient, kd, ks, lvec, point_lights, cam, shininess, shared,
            dtype=F64):
    """A COPY of `shading_reference.phong_points` (values only) with one mutation switched on by name; `mut=None` is the
    closed form itself (asserted below)."""
    world, normals, rgb, g_all, ambient, kd, ks, lvec, cam = (
        t.to(F64) for t in (world, normals, rgb, grad_out, ambient, kd, ks, lvec, cam))
    Pw, P, L, s = world.shape[0], rgb.shape[0], kd.shape[1], float(shininess)
    vals = [torch.zeros(k, 3, dtype=F64) for k in (P, Pw, Pw, P)]

    def jt(y, z):
        yn = y.norm(dim=1, keepdim=True)
        h = y / yn.clamp_min(1e-6)
        proj = z if mut == "jacobian_without_projection" else z - h * (h * z).sum(1, keepdim=True)
        return torch.where(yn > 1e-6, proj / yn.clamp_min(1e-6), z * (1.0 if mut == "clamped_scale_1" else 1e6))

    ranges = cref._ranges(first, num)
    for n, (lo, hi) in enumerate(ranges):
        if mut == "skip_last_shared_camera" and shared and n == len(ranges) - 1:
            continue
        rows = slice(lo, hi)
        wr = slice(0, hi - lo) if shared else rows
        x, m, c, g = world[wr], normals[wr], rgb[wr if (mut == "rgb_row_wi" and shared) else rows], g_all[rows]
        ln = 0 if mut == "lights_of_camera_0" else n
        nh = cref._normalize(m)
        w = cam[n][None] - x
        v = cref._normalize(w)
        vals[0][rows] += c * ambient[ln][None]
        vals[3][rows] += g * ambient[ln][None]
        for l in range(L):
            u = lvec[ln, l][None] - x if point_lights else lvec[ln, l][None].expand_as(x)
            d = cref._normalize(u)
            ca = (nh * d).sum(1, keepdim=True)
            r = -d + 2.0 * ca * nh
            a0 = (v * r).sum(1, keepdim=True)
            lit = ca > 0
            alpha = a0.clamp_min(0) * lit
            D = ca.clamp_min(0)
            vals[0][rows] += c * kd[ln, l][None] * D
            vals[0][rows] += ks[ln, l][None] * alpha ** s
            vals[3][rows] += g * kd[ln, l][None] * D
            gd = (g * c * kd[ln, l][None]).sum(1, keepdim=True)
            gs = (g * ks[ln, l][None]).sum(1, keepdim=True)
            if mut == "ga0_without_lit":
                ga0 = torch.where(a0 > 0, gs * s * a0.clamp_min(0) ** (s - 1.0), torch.zeros_like(a0))
            elif mut == "ga0_without_a0_gate":
                ga0 = torch.where(lit, gs * s * a0 ** (s - 1.0), torch.zeros_like(a0))
            else:
                ga0 = torch.where(lit & (a0 > 0), gs * s * alpha ** (s - 1.0), torch.zeros_like(a0))
            gca = torch.where(lit, gd, torch.zeros_like(gd))
            if mut != "gca_without_2_ga0_vn":
                gca = gca + 2.0 * ga0 * (v * nh).sum(1, keepdim=True)
            gdv = -ga0 * v + gca * nh
            vals[2][wr] += jt(m, 2.0 * ca * ga0 * v + gca * d)
            if mut != "no_view_chain":
                vals[1][wr] -= jt(w, ga0 * r)
            if point_lights:
                vals[1][wr] -= jt(u, gdv) * (-1.0 if mut == "point_light_chain_sign" else 1.0)
    return tuple(vals)


def test_the_copy_is_the_closed_form():
    for name, kind, shin in (("fixture", "point", 24.0), ("shared_partial", "directional", 64.0), ("gap", "point", 12.0)):
        case, shared = _inputs(name)
        vals, _A = _ref(name, kind, shin)
        copy = sr.run_case(case, shared, kind, shin, fn=_mutant_none)
        assert all(torch.equal(a, b) for a, b in zip(vals, copy))


def _mutant_none(*args, **kw):
    return _mutant(None, *args, **kw)


@pytest.mark.parametrize("mut", MUTATIONS)
def test_the_per_entry_check_kills_the_mutant(mut):
    """the mutant's output through `entry_ratio` with the GPU test's bars: some output of some case is beyond 10 x its bar
    (entries that are non-zero where no term exists are counted and printed, not relied on)"""
    best, where, nonzero = 0.0, None, 0
    for name, kind, shin in CASES:
        case, shared = _inputs(name)
        vals, A = _ref(name, kind, shin)
        got = sr.run_case(case, shared, kind, shin, fn=functools.partial(_mutant, mut))
        own = sr.owned_rows(case, shared)
        for out_name, g, v, a, bar in zip(sr.OUTPUTS, got, vals, A, sr.BARS[(name, kind, int(shin))]):
            if out_name in ("out", "grad_rgb"):     # the GPU test compares these on owned rows only
                g, v, a = g[own], v[own], a[own]
            worst, zeros_ok = sr.entry_ratio(g, v, a)
            nonzero += not zeros_ok
            if bar > 0 and worst / bar > best:
                best, where = worst / bar, (name, kind, int(shin), out_name)
    print("mutant %-28s exceeds a bar %.3g-fold at %s; non-zero where no term exists in %d comparisons"
          % (mut, best, where, nonzero))
    assert best >= 10.0, (mut, best, where)


# ---------------------------------------------------------------------------------------------------------------------
def test_phong_entry_points_validate_without_a_device():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)     # never dereferenced: every call below fails before a launch

    def args(backward, N=2, Pw=500, L=2, null=(), out=fake, grad_out=fake):
        ins = [None if k in null else fake for k in range(5)]            # world, normals, rgb, first_idx, num_pts
        lights = [None if 5 + k in null else fake for k in range(4)]     # ambient, kd, ks, light_vec
        cam = None if 9 in null else fake
        a = ins + [N, Pw, 0] + lights + [L, 1, cam, 64.0]
        return [grad_out] + a + [fake, fake, fake, None] if backward else a + [out, None]

    for backward, fn, who in ((False, lib.dss_phong_forward, b"dss_phong_forward"),
                              (True, lib.dss_phong_backward, b"dss_phong_backward")):
        bad = [dict(N=0), dict(N=-1), dict(Pw=-1), dict(L=-1)] + [dict(null=(k,)) for k in range(10)]
        bad.append(dict(grad_out=None) if backward else dict(out=None))
        for kw in bad:
            assert fn(*args(backward, **kw)) == -1, (who, kw)
            assert who in lib.dss_last_error(), (who, kw)
        # nothing to do is not an error, whatever the pointers: Pw == 0 returns before any of them is looked at
        assert fn(*args(backward, Pw=0, null=tuple(range(10)), out=None, grad_out=None)) == 0
        # L == 0 needs no light tensors: the NULL check passes them ... and the next refusal is the output's
        assert fn(*args(backward, L=0, null=(6, 7, 8), out=None, grad_out=None)) == -1
        assert b"NULL" in lib.dss_last_error() and b"tensor pointer" not in lib.dss_last_error()
