"""fp64 CPU reference of the shading's POINT gradients (TEST INFRASTRUCTURE; plain torch, no product code).

The closed form of ``dss_phong_forward`` / ``dss_phong_backward`` (`dss_amd/csrc/shading.hip`): the shaded colours and
the gradients w.r.t. the world positions, the normals and the base colours, each ENTRY with the sum of its ABSOLUTE terms
next to it (the error of a kernel is measured against ``A = sum |term|`` of that entry, not against a sum that may cancel).
`tests/test_shading_points_cpu.py` compares it with `torch.autograd` of `camera_reference.phong` and with the gradients
the reference's own `diffuse` / `specular` produce (``tests/golden/ref_point_grads.npz``).

Notation of the kernel: for the pair (camera n, world point wi; packed row p) and light l, g = grad_out[p], c = rgb[p],
m = normal, n^ = m / max(|m|, 1e-6), w = camera - x, v^ = normalize(w), u = location - x or direction, d^ = normalize(u),
ca = n^ . d^, r = -d^ + 2 ca n^, a0 = v^ . r, D = relu(ca), S = (relu(a0) [ca > 0]) ^ s:

    out[p]      = c amb + sum_l c kd D + sum_l ks S                                  terms: c amb | c kd_l D_l | ks_l S_l
    grad_rgb[p] = g amb + sum_l g kd D                                               terms: g amb | g kd_l D_l
    ga0 = [ca > 0][a0 > 0] (g . ks) s a0^(s-1),   gca = [ca > 0] (g c . kd) + 2 ga0 (v^ . n^),   gdv = -ga0 v^ + gca n^
    grad_normals[wi] = sum_n sum_l J(m)^T (2 ca ga0 v^ + gca d^)                     terms: one per (n, l)
    grad_world[wi]   = - sum_n sum_l ( J(w)^T (ga0 r)  +  [point lights] J(u)^T gdv )   terms: two per (n, l), one per chain
    J(y)^T z = (z - h (h . z)) / |y|,  h = y / |y|    (|y| > 1e-6;   otherwise z * 1e6: the clamped denominator)

A term of grad_normals / grad_world is taken AFTER its own normalisation Jacobian (J is linear, so the kernel's one
Jacobian per camera over the sum of the lights is the sum of these).  Rows that no cloud owns are zeros in every output.
A shared cloud (``shared``): world point wi of camera n is packed row ``first[n] + wi`` for ``wi < num[n]``.
"""
import math
import os

import torch

from camera_reference import F64, _normalize, _ranges

# fp32 cannot hold a term below its subnormal range: alpha^(s-1) of a pair far outside the specular lobe (alpha = 0.15,
# s = 64: 1e-52) is a non-zero term in fp64 and an exact zero (or a subnormal with a few bits) in fp32, whatever kernel
# evaluates it.  The absolute error of that is at most 2^-126 (the smallest normal) times the factors that follow it
# (s (g . ks) |r| / max(|w|, 1e-6) <= 1e8 on any case here), so <= 1e-30 -- thirty orders of magnitude below any entry's A.
UNDERFLOW = 1e-30


def _jt(y, z):
    """J(y)^T z of y / max(|y|, 1e-6)"""
    yn = y.norm(dim=1, keepdim=True)
    h = y / yn.clamp_min(1e-6)
    return torch.where(yn > 1e-6, (z - h * (h * z).sum(1, keepdim=True)) / yn.clamp_min(1e-6), z * 1e6)


def phong_points(grad_out, world, normals, rgb, first, num, ambient, kd, ks, lvec, point_lights, cam, shininess, shared,
                 dtype=F64):
    """closed form -> ((out (P,3), grad_world (Pw,3), grad_normals (Pw,3), grad_rgb (P,3)), (A_* likewise)), all fp64
    (`dtype=torch.float32`: the same formula in plain fp32 torch, to see what the number format alone costs)"""
    world, normals, rgb, g_all, ambient, kd, ks, lvec, cam = (
        t.to(dtype) for t in (world, normals, rgb, grad_out, ambient, kd, ks, lvec, cam))
    Pw, P, L, s = world.shape[0], rgb.shape[0], kd.shape[1], float(shininess)
    vals = [torch.zeros(k, 3, dtype=dtype) for k in (P, Pw, Pw, P)]
    sums = [torch.zeros(k, 3, dtype=F64) for k in (P, Pw, Pw, P)]

    def add(k, rows, term, sign=1.0):
        vals[k][rows] += sign * term
        sums[k][rows] += term.to(F64).abs()

    for n, (lo, hi) in enumerate(_ranges(first, num)):
        rows = slice(lo, hi)
        wr = slice(0, hi - lo) if shared else rows
        x, m, c, g = world[wr], normals[wr], rgb[rows], g_all[rows]
        nh = _normalize(m)
        w = cam[n][None] - x
        v = _normalize(w)
        add(0, rows, c * ambient[n][None])
        add(3, rows, g * ambient[n][None])
        for l in range(L):
            u = lvec[n, l][None] - x if point_lights else lvec[n, l][None].expand_as(x)
            d = _normalize(u)
            ca = (nh * d).sum(1, keepdim=True)
            r = -d + 2.0 * ca * nh
            a0 = (v * r).sum(1, keepdim=True)
            lit = ca > 0
            alpha = a0.clamp_min(0) * lit
            D = ca.clamp_min(0)
            add(0, rows, c * kd[n, l][None] * D)
            add(0, rows, ks[n, l][None] * alpha ** s)
            add(3, rows, g * kd[n, l][None] * D)
            gd = (g * c * kd[n, l][None]).sum(1, keepdim=True)
            gs = (g * ks[n, l][None]).sum(1, keepdim=True)
            ga0 = torch.where(lit & (a0 > 0), gs * s * alpha ** (s - 1.0), torch.zeros_like(a0))
            gca = torch.where(lit, gd, torch.zeros_like(gd)) + 2.0 * ga0 * (v * nh).sum(1, keepdim=True)
            gdv = -ga0 * v + gca * nh
            add(2, wr, _jt(m, 2.0 * ca * ga0 * v + gca * d))
            add(1, wr, _jt(w, ga0 * r), -1.0)
            if point_lights:
                add(1, wr, _jt(u, gdv), -1.0)
    return tuple(t.to(F64) for t in vals), tuple(sums)


def phong_backward_points(*args, **kw):
    """-> ((grad_world, grad_normals, grad_rgb), (A_world, A_normals, A_rgb)) of `phong_points`"""
    vals, sums = phong_points(*args, **kw)
    return vals[1:], sums[1:]


def phong_points_autograd(grad_out, world, normals, rgb, first, num, ambient, kd, ks, lvec, point_lights, cam, shininess,
                          shared):
    """the same four tensors from `camera_reference.phong` and torch.autograd (rows that no cloud owns: zeros)"""
    from camera_reference import phong
    x, m, c = (t.to(F64).clone().requires_grad_(True) for t in (world, normals, rgb))
    a = [t.to(F64) for t in (ambient, kd, ks, lvec, cam)]
    owned = torch.cat([torch.arange(lo, hi) for lo, hi in _ranges(first, num)] + [torch.zeros(0, dtype=torch.int64)])
    out = torch.zeros(rgb.shape[0], 3, dtype=F64)
    if owned.numel():
        o = phong(x, m, c, first, num, a[0], a[1], a[2], a[3], point_lights, a[4], shininess, shared)
        out[owned] = o.detach()
        (o * grad_out.to(F64)[owned]).sum().backward()
    return (out,) + tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in (x, m, c))


def entry_ratio(got, ref, A):
    """The per-entry check of the CPU and the GPU test -> (largest (|got - ref| - UNDERFLOW) / A over the entries with
    A > 0, whether every entry with A == 0 is an exact zero).  A non-finite entry counts as an infinite ratio."""
    got = got.detach().cpu().to(F64)
    assert tuple(got.shape) == tuple(ref.shape) == tuple(A.shape)
    zeros_ok = bool((got[A == 0] == 0).all())
    err = ((got - ref).abs() - UNDERFLOW).clamp_min(0)[A > 0] / A[A > 0]
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    return (float(err.max()) if err.numel() else 0.0), zeros_ok


def round_up_1sig(x):
    """x rounded up to one significant digit (how a bar is derived from a measured figure)"""
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x))
    return float("%de%d" % (math.ceil(x / 10.0 ** e - 1e-9), e))


# ---------------------------------------------------------------------------------------------------------------------
# the cases that tests/test_shading_points_cpu.py and tests/test_gpu_shading_points.py share
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_point_grads.npz")
OUTPUTS = ("out", "grad_world", "grad_normals", "grad_rgb")
KINDS = ("point", "directional")
# name -> (Pw, first, num, shared, L, seed); every cloud boundary lies inside a wavefront, every layout but "single" and
# "L*" spans more than one 256-thread block.  Seeds: an entry of a normalisation Jacobian, z_i - h_i (h . z), may cancel, and
# two fp64 evaluations of it then agree to eps x the cancellation only; of the seeds 1 ... 8 each layout takes one at which
# the closed form and autograd agree to <= 1.5e-13 A, which leaves the CPU test's 1e-12 its meaning.
LAYOUTS = {
    "ragged": (466, [0, 300, 300, 337], [300, 0, 37, 129], False, 2, 3),   # per-camera clouds, one of them empty
    "gap": (500, [64, 400], [300, 37], False, 2, 3),                       # rows [0,64), [364,400), [437,500): no owner
    "shared3": (321, [0, 321, 642], [321, 321, 321], True, 2, 3),
    "shared1": (321, [0], [321], True, 2, 6),
    "single": (257, [0], [257], False, 2, 4),
    "L0": (260, [0, 70], [70, 190], False, 0, 3),
    "L1": (260, [0, 70], [70, 190], False, 1, 5),
    "L3": (260, [0, 70], [70, 190], False, 3, 1),
    "shared_partial": (321, [0, 321, 642], [321, 200, 321], True, 2, 3),   # camera 1 owns 200 of the 321 points
    "scaled": (466, [0, 300, 300, 337], [300, 0, 37, 129], False, 2, 3),   # "ragged", each normal x [1e-3, 1e3]
}


def layout_case(name, seed=None):
    """-> (world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out), shared: fp32 CPU tensors, seeded"""
    Pw, first, num, shared, L, own_seed = LAYOUTS[name]
    seed = own_seed if seed is None else seed
    N = len(num)
    P = N * Pw if shared else Pw
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    world, normals = r(Pw, 3) * 0.5, r(Pw, 3)
    normals[::5] *= 20.0
    rgb, grad_out = u(P, 3), r(P, 3)
    amb, kd, ks = u(N, 3) * 0.5, u(N, 3, 3)[:, :L].contiguous(), u(N, 3, 3)[:, :L].contiguous()
    lvec, cam = (r(N, 3, 3) * 2)[:, :L].contiguous(), r(N, 3) * 3
    if name == "scaled":
        normals = normals * scale_factors(Pw)[:, None]
    i64 = lambda a: torch.tensor(a, dtype=torch.int64)
    return (world, normals, rgb, i64(first), i64(num), amb, kd, ks, lvec, cam, grad_out), shared


def scale_factors(Pw):
    """the per-point factors in [1e-3, 1e3] of the layout "scaled" (log-uniform, fp32)"""
    g = torch.Generator().manual_seed(99)
    return 10.0 ** (torch.rand(Pw, generator=g) * 6.0 - 3.0)


def owned_rows(case, shared):
    """bool (P,): the packed rows that some cloud owns (the others are zeros, or unspecified for a shared cloud)"""
    first, num = case[3], case[4]
    own = torch.zeros(case[2].shape[0], dtype=torch.bool)
    for lo, hi in _ranges(first, num):
        own[lo:hi] = True
    return own


def fixture_case(z):
    """ref_point_grads.npz (np.load) -> (case of fp64 tensors holding fp32-representable numbers, shared = False)"""
    t = lambda k: torch.from_numpy(z[k])
    num = t("num")
    first = torch.cumsum(num, 0) - num
    return (t("points"), t("normals"), t("rgb"), first, num, t("ambient_color").sum(1), t("diffuse_color"),
            t("specular_color"), t("light_vec"), t("cam_center"), t("grad_out")), False


def fixture_expected(z, kind, shininess):
    return tuple(torch.from_numpy(z["%s_s%d_%s" % (kind, int(shininess), k)])
                 for k in ("shaded", "grad_points", "grad_normals", "grad_rgb"))


def run_case(case, shared, kind, shininess, dtype=F64, fn=phong_points):
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    return fn(grad_out, world, normals, rgb, first, num, amb, kd, ks, lvec, kind == "point", cam, shininess, shared,
              dtype=dtype)


def scale_ratios(out_s, gn_s, kind, shininess):
    """`out` / `grad_normals` computed on the layout "scaled" -> (out against the UNSCALED fp64 `out`, factor x grad_normals
    against the unscaled fp64 grad_normals, |m . grad_normals| against sum_i |m_i| A_i), each the largest ratio"""
    base, shared = layout_case("ragged")
    scaled, _ = layout_case("scaled")
    vals, A = run_case(base, shared, kind, shininess)
    _v, A_s = run_case(scaled, shared, kind, shininess)
    f, m = scale_factors(base[0].shape[0]).to(F64)[:, None], scaled[1].to(F64)
    gn_s = gn_s.detach().cpu().to(F64)
    r_out = entry_ratio(out_s, vals[0], A[0])[0]
    r_gn = entry_ratio(gn_s * f, vals[2], A[2])[0]
    den = (m.abs() * A_s[2]).sum(1)
    r_dot = float(((m * gn_s).sum(1).abs()[den > 0] / den[den > 0]).max())
    return r_out, r_gn, r_dot


# the three Phong kernels against each other: name -> (Pw, first, num, shared, L, seed)
IDENTITY_LAYOUTS = {
    "ragged": LAYOUTS["ragged"], "shared3": LAYOUTS["shared3"],
    "big": (20011, [0], [20011], False, 2, 3), "big_shared3": (20011, [0, 20011, 40022], [20011] * 3, True, 2, 3),
}
IDENTITY_CASES = [(n, k, 12) for n in ("ragged", "shared3") for k in KINDS] \
    + [(n, k, 64) for n in ("big", "big_shared3") for k in KINDS]


def identity_case(name):
    LAYOUTS[name + "#identity"] = IDENTITY_LAYOUTS[name]
    try:
        return layout_case(name + "#identity")
    finally:
        del LAYOUTS[name + "#identity"]


def identity_ratio(case, shared, kind, shininess, grad_world, grad_cam, grad_light_vec):
    """|sum_p grad_world + sum_n grad_cam (+ sum_{n,l} grad_light_vec)| per axis against the summed absolute terms of the
    three fp64 closed forms -> the largest of the three ratios (the outputs are summed in fp64)"""
    import light_reference as lref
    from camera_reference import phong_backward_camera
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad_out = case
    _v, A = run_case(case, shared, kind, shininess)
    _g, a_cam = phong_backward_camera(grad_out, world, normals, first, num, ks, lvec, kind == "point", cam, shininess, shared)
    total = grad_world.detach().cpu().to(F64).sum(0) + grad_cam.detach().cpu().to(F64).sum(0)
    scale = A[1].sum(0) + a_cam.sum(0)
    if kind == "point":
        _g, a_l = lref.phong_backward_lights(grad_out, world, normals, rgb, first, num, kd, ks, lvec, True, cam, shininess,
                                             shared)
        total = total + grad_light_vec.detach().cpu().to(F64).sum((0, 1))
        scale = scale + a_l[3].sum((0, 1))
    return float((total.abs() / scale).max())


# ---------------------------------------------------------------------------------------------------------------------
# The bars of tests/test_gpu_shading_points.py: 4 x the largest |err| / A of `phong_points(..., dtype=torch.float32)` (plain
# fp32 torch on the CPU) against fp64, rounded up to one significant digit; tests/test_shading_points_cpu.py re-measures
# the figures and asserts the tie.  (case, light kind, shininess) -> bars of (out, grad_world, grad_normals, grad_rgb).
BARS = {
    ('fixture', 'point', 1): (3e-06, 0.0001, 0.0002, 2e-06),
    ('fixture', 'point', 24): (2e-05, 0.0001, 0.0002, 2e-06),
    ('fixture', 'point', 64): (3e-05, 0.0001, 8e-05, 2e-06),
    ('fixture', 'directional', 1): (3e-06, 3e-05, 6e-05, 2e-06),
    ('fixture', 'directional', 24): (9e-06, 0.0001, 3e-05, 2e-06),
    ('fixture', 'directional', 64): (3e-05, 0.0002, 5e-05, 2e-06),
    ('ragged', 'point', 12): (7e-06, 0.0003, 9e-05, 3e-06),
    ('ragged', 'point', 64): (3e-05, 0.0003, 7e-05, 3e-06),
    ('ragged', 'directional', 12): (1e-05, 0.0002, 0.0002, 2e-06),
    ('ragged', 'directional', 64): (3e-05, 0.0002, 0.0006, 2e-06),
    ('gap', 'point', 12): (1e-05, 0.0005, 0.001, 1e-06),
    ('gap', 'point', 64): (2e-05, 0.0005, 9e-05, 1e-06),
    ('gap', 'directional', 12): (1e-05, 0.0003, 8e-05, 8e-07),
    ('gap', 'directional', 64): (3e-05, 0.0004, 0.0002, 8e-07),
    ('shared3', 'point', 12): (2e-05, 3e-05, 4e-05, 3e-06),
    ('shared3', 'point', 64): (4e-05, 8e-05, 0.0002, 3e-06),
    ('shared3', 'directional', 12): (8e-06, 0.0002, 4e-05, 4e-06),
    ('shared3', 'directional', 64): (2e-05, 0.0001, 9e-05, 4e-06),
    ('shared1', 'point', 12): (7e-06, 4e-05, 7e-05, 2e-06),
    ('shared1', 'point', 64): (2e-05, 4e-05, 7e-05, 2e-06),
    ('shared1', 'directional', 12): (9e-06, 0.0004, 7e-05, 2e-06),
    ('shared1', 'directional', 64): (4e-05, 0.0004, 6e-05, 2e-06),
    ('single', 'point', 12): (2e-05, 7e-05, 9e-05, 6e-07),
    ('single', 'point', 64): (2e-05, 7e-05, 5e-05, 6e-07),
    ('single', 'directional', 12): (3e-06, 0.0002, 7e-05, 6e-07),
    ('single', 'directional', 64): (1e-05, 8e-05, 6e-05, 6e-07),
    ('L0', 'point', 12): (3e-07, 0, 0, 3e-07),
    ('L0', 'point', 64): (3e-07, 0, 0, 3e-07),
    ('L0', 'directional', 12): (3e-07, 0, 0, 3e-07),
    ('L0', 'directional', 64): (3e-07, 0, 0, 3e-07),
    ('L1', 'point', 12): (1e-05, 6e-05, 4e-05, 3e-06),
    ('L1', 'point', 64): (2e-05, 7e-05, 0.004, 3e-06),
    ('L1', 'directional', 12): (8e-06, 0.0001, 0.0002, 2e-06),
    ('L1', 'directional', 64): (4e-05, 0.0001, 6e-05, 2e-06),
    ('L3', 'point', 12): (9e-06, 4e-05, 6e-05, 2e-06),
    ('L3', 'point', 64): (5e-05, 0.0002, 0.0004, 2e-06),
    ('L3', 'directional', 12): (2e-05, 0.0002, 0.0001, 9e-07),
    ('L3', 'directional', 64): (3e-05, 9e-05, 9e-05, 9e-07),
    ('shared_partial', 'point', 12): (2e-05, 4e-05, 4e-05, 3e-06),
    ('shared_partial', 'point', 64): (4e-05, 8e-05, 0.0002, 3e-06),
    ('shared_partial', 'directional', 12): (8e-06, 0.0003, 4e-05, 4e-06),
    ('shared_partial', 'directional', 64): (2e-05, 0.0001, 9e-05, 4e-06),
    ('scaled', 'point', 12): (2e-05, 8e-05, 9e-05, 3e-06),
    ('scaled', 'point', 64): (4e-05, 0.0002, 6e-05, 3e-06),
    ('scaled', 'directional', 12): (2e-05, 9e-05, 0.0006, 2e-06),
    ('scaled', 'directional', 64): (6e-05, 0.0002, 0.0004, 2e-06),
}
# the layout "scaled": (kind, shininess) -> bars of `scale_ratios`
SCALE_BARS = {
    ('point', 12): (2e-05, 9e-05, 2e-05),
    ('point', 64): (4e-05, 6e-05, 2e-05),
    ('directional', 12): (2e-05, 0.0006, 2e-05),
    ('directional', 64): (6e-05, 0.0004, 4e-05),
}
# the three kernels against each other: -> bar of `identity_ratio`
IDENTITY_BARS = {
    ('ragged', 'point', 12): 2e-08,
    ('ragged', 'directional', 12): 2e-07,
    ('shared3', 'point', 12): 6e-09,
    ('shared3', 'directional', 12): 2e-08,
    ('big', 'point', 64): 2e-08,
    ('big', 'directional', 64): 7e-08,
    ('big_shared3', 'point', 64): 3e-09,
    ('big_shared3', 'directional', 64): 2e-08,
}
