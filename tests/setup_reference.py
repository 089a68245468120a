"""fp64 CPU reference of the per-point setup FORWARD (TEST INFRASTRUCTURE; plain torch, no product and no oracle code).

What `setup_point_arith` (`dss_amd/csrc/setup_body.h`; `dss_point_setup` and, fused, `dss_render_forward`) computes for a
packed point, written from the reference method's definition (rasterizer.py:148-254 culling, :293-441 source variance and
det Mk, :443-496 W Jk, :498-565 ellipse, radii and scaler, mathHelper.py:10-21 the two clamps).  For the pair (camera n,
world row wi, packed row p), xh = (x, y, z, 1), n the cloud normal, f the normal of the tangent frame (the cloud normal; in
anisotropic mode the PCA frame's), f^ = f / max(|f|, 1e-12):

    zview = xh . V[n,:,2]      nz = n . V[n,:3,2]      valid = znear <= zview <= zfar  [and nz < 0]
    clip = xh @ M[n]   w = clip_3   screen = (clip_0 / w, clip_1 / w, zview)
    WJ[i][j] = M[n,i,j] (1 / d(w)) + M[n,i,3] (-1 / d(w w) clip_j)                    i < 3, j < 2;  d = eps_denom
    Vr = h (I - f^ f^T)  (0 where |f| <= 1e-12; anisotropic: the given symmetric Vr)     Vk = WJ^T Vr WJ
    G = Vk + sigma px^2 I,  px = 2 / S      detG = G00 G11 - G01 G10
    (a, b, c) = (G11, -G01 - G10, G00) / detG        den = d(4 a c - b b)
    (rx, ry) = sqrt(s(4 (c, a) cutoff / den))                                          s = eps_sqrt
    scaler = |det(Sk WJ)| / d(sqrt(s(4 pi^2 detG))),   |det(Sk WJ)| = |f^ . (WJ[:,0] x WJ[:,1])|   (0 where |f| <= 1e-12)

(Sk = two orthonormal tangents of f^: Binet-Cauchy.  `definition` below evaluates Vr, det(Sk WJ) and G^-1 from an explicit
Sk, `torch.linalg.det` and `torch.linalg.inv` instead; tests/test_setup_reference_cpu.py compares the two.)  h of the pair:
one per cloud (`h_cloud`), per world row (`h_point`) or per PACKED row (`h_packed`: a shared cloud whose cameras cull
differently).  A culled pair and a row that no cloud owns hold screen = (0, 0, -1), ellipse = (1, 0, 1), radii = 0,
scaler = 0, valid = 0; `cutoff` is the constant on every row.

ERROR SCALES.  Next to every real entry stands a scale A >= |entry|, and the error of an entry is always reported as
``|got - ref| / A``.  The rules, applied operation by operation (`Tr`), the inputs being exact:

    a product of inputs          A = |x y|             (so a sum of such products: the sum of the absolute products)
    x + y,  x - y                A = A_x + A_y
    x y                          A = A_x |y| + |x| A_y
    x / y                        A = A_x / |y| + |x| A_y / y^2
    sqrt(x)                      A = A_x / (2 sqrt|x|)
    |x|, -x, a clamp             A = A_x
    and never below |result| itself (the operation's own rounding)

e.g. A_a = |a| (A_G11 / |G11| + A_det / |detG|): where detG cancels, A_det / |detG| is large and the scale of a, b, c, the
radii and the scaler with it -- the cancellation does not hide behind an array maximum, it is what the entry is measured in.

DECISIONS are compared exactly, except on the pairs whose fp64 margin is within rounding of a threshold:
0 < |zview - znear|, |zview - zfar| or |nz| <= NEAR_ULPS 2^-23 A (`near`; a margin of exactly 0 -- the planted boundary
points, whose sums are exact in fp32 as well -- is NOT within rounding: >= and < decide it).  Those pairs are left out of
every comparison; a case may list at most 1 % of its owned pairs (asserted on the CPU).

The same functions take ``dtype=torch.float32``: the formula in plain fp32 torch, what the number format alone costs; the
bars (`BARS`, below) are 4 x that, and ``mut=`` switches on one of the wrong formulas of `MUTANTS`, which the CPU test
shows to lie beyond the bars.
"""
import functools
import math
from collections import namedtuple

import torch

from camera_reference import F64, _ranges
from shading_reference import UNDERFLOW, round_up_1sig  # noqa: F401  (UNDERFLOW: the GPU test's check)

OUTPUTS = ("screen", "ellipse", "radii", "scaler")
DEFAULTS = {"screen": (0.0, 0.0, -1.0), "ellipse": (1.0, 0.0, 1.0), "radii": (0.0, 0.0), "scaler": (0.0,)}
NEAR_ULPS = 4
CUTOFF, SIGMA = 1.0, 1.0
MUTANTS = ("nz_le_0", "zview_gt_znear", "normal_not_normalised", "sigma_px2_dropped", "px_1_over_S", "b_without_two",
           "radii_swapped", "scaler_sqrt_detVk_over_h", "two_pi", "cloud_normal_in_aniso_scaler", "frame_normal_culls",
           "h_by_world_row", "wj_clip_term_dropped", "detMk_without_abs")


class Tr:
    """a value (in the run's dtype) and its error scale A (fp64), by the rules of the header"""
    __slots__ = ("v", "a")

    def __init__(self, v, a=None):
        self.v = v
        self.a = torch.zeros(v.shape, dtype=F64) if a is None else a

    def _o(self, x):
        return x if isinstance(x, Tr) else Tr(torch.full_like(self.v, x))

    @staticmethod
    def _out(v, prop):
        return Tr(v, torch.maximum(prop, v.to(F64).abs()))

    def __add__(self, o):
        o = self._o(o)
        return Tr._out(self.v + o.v, self.a + o.a)

    def __sub__(self, o):
        o = self._o(o)
        return Tr._out(self.v - o.v, self.a + o.a)

    def __neg__(self):
        return Tr(-self.v, self.a)

    def __mul__(self, o):
        o = self._o(o)
        return Tr._out(self.v * o.v, self.a * o.v.to(F64).abs() + self.v.to(F64).abs() * o.a)

    def __truediv__(self, o):
        o = self._o(o)
        y = o.v.to(F64).abs()
        return Tr._out(self.v / o.v, self.a / y + self.v.to(F64).abs() * o.a / (y * y))

    def sqrt(self):
        v = self.v.sqrt()
        return Tr._out(v, self.a / (2.0 * v.to(F64)))

    def abs(self):
        return Tr(self.v.abs(), self.a)

    def where(self, cond, other):
        """self where cond, else `other` (a Tr, or an exact number)"""
        o = self._o(other)
        return Tr(torch.where(cond, self.v, o.v), torch.where(cond, self.a, o.a))


def eps_denom(t, eps=1e-17):
    """mathHelper.py:10-14: sign(d) max(|d|, eps), the sign of 0 being +"""
    sign = t.v.sign() + (t.v == 0).to(t.v.dtype)
    return Tr._out(sign * t.v.abs().clamp_min(eps), t.a)


def eps_sqrt(t, eps=1e-17):
    """mathHelper.py:16-21: max(|d|, eps)"""
    return Tr._out(t.v.abs().clamp_min(eps), t.a)


def _dot(xs, ys):
    s = xs[0] * ys[0]
    for x, y in zip(xs[1:], ys[1:]):
        s = s + x * y
    return s


def _unit(f):
    """f^ = f / max(|f|, 1e-12) -> (f^ (3 Tr), |f| > 1e-12)"""
    nlen = _dot(f, f).sqrt()
    big = nlen.v > 1e-12
    nden = nlen.where(big, 1e-12)
    return [x / nden for x in f], big


Ref = namedtuple("Ref", "valid near owned vals A cutoff")


def pairs_of(c):
    """-> (packed rows p, cameras n, world rows wi) of the owned pairs, in camera order"""
    p, n, wi = [], [], []
    for k, (lo, hi) in enumerate(_ranges(c.first, c.num)):
        p.append(torch.arange(lo, hi))
        n.append(torch.full((hi - lo,), k, dtype=torch.int64))
        wi.append(torch.arange(0, hi - lo) if c.shared else torch.arange(lo, hi))
    cat = lambda ts: torch.cat(ts + [torch.zeros(0, dtype=torch.int64)])
    return cat(p), cat(n), cat(wi)


def packed_rows(c):
    return len(c.num) * c.world.shape[0] if c.shared else c.world.shape[0]


def setup(c, dtype=F64, mut=None):
    """-> Ref of the case: valid, near, owned (P,) bool; vals / A: output name -> (P,k) fp64; cutoff (P,) fp64"""
    assert mut is None or mut in MUTANTS
    rows, cam, wi = pairs_of(c)
    K, P = rows.numel(), packed_rows(c)
    L = lambda a: Tr(a.to(dtype))
    M, V = c.M[cam], c.V[cam]
    xh = [L(c.world[wi, i]) for i in range(3)] + [L(torch.ones(K))]
    ncl = [L(c.normals[wi, i]) for i in range(3)]
    aniso = c.mode == "aniso"
    nfr = [L(c.fn[wi, i]) for i in range(3)] if aniso else ncl
    m = lambda i, j: L(M[:, i, j])

    # culling
    zview = _dot(xh, [L(V[:, i, 2]) for i in range(4)])
    nz = _dot(nfr if mut == "frame_normal_culls" else ncl, [L(V[:, i, 2]) for i in range(3)])
    zn, zf = c.znear[cam].to(dtype), c.zfar[cam].to(dtype)
    ok = ((zview.v > zn) if mut == "zview_gt_znear" else (zview.v >= zn)) & (zview.v <= zf)
    tol = NEAR_ULPS * 2.0 ** -23
    margin = lambda d, a: (d.to(F64).abs() > 0) & (d.to(F64).abs() <= tol * a)
    near = margin(zview.v - zn, zview.a) | margin(zview.v - zf, zview.a)
    if c.backface:
        ok = ok & ((nz.v <= 0) if mut == "nz_le_0" else (nz.v < 0))
        near = near | margin(nz.v, nz.a)

    # projection and its Jacobian
    clip = [_dot(xh, [m(i, j) for i in range(4)]) for j in range(4)]
    w = clip[3]
    sx, sy = clip[0] / w, clip[1] / w
    one = L(torch.ones(K))
    dw, dw2 = eps_denom(w), eps_denom(w * w)
    if mut == "wj_clip_term_dropped":
        WJ = [[m(i, j) * (one / dw) for j in range(2)] for i in range(3)]
    else:
        WJ = [[m(i, j) * (one / dw) + m(i, 3) * ((-one) / dw2 * clip[j]) for j in range(2)] for i in range(3)]

    # source variance
    nn, big = _unit(nfr)
    if aniso:
        q = [L(c.vr6[wi, k]) for k in range(6)]
        Vr = [[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]]
        hh = None
    else:
        if c.mode == "h_cloud":
            hh = L(c.h[cam])
        elif c.mode == "h_point" or mut == "h_by_world_row":
            hh = L(c.h[wi])
        else:
            hh = L(c.h[rows])
        hv = hh.where(big, 0.0)
        nv = nfr if mut == "normal_not_normalised" else nn
        Vr = [[hv * (L(torch.full((K,), 1.0 if i == j else 0.0)) - nv[i] * nv[j]) for j in range(3)] for i in range(3)]
    T = [[Vr[i][0] * WJ[0][j] + Vr[i][1] * WJ[1][j] + Vr[i][2] * WJ[2][j] for j in range(2)] for i in range(3)]
    Vk = [[WJ[0][i] * T[0][j] + WJ[1][i] * T[1][j] + WJ[2][i] * T[2][j] for j in range(2)] for i in range(2)]

    # |det(Sk WJ)|
    cx = [WJ[1][0] * WJ[2][1] - WJ[2][0] * WJ[1][1], WJ[2][0] * WJ[0][1] - WJ[0][0] * WJ[2][1],
          WJ[0][0] * WJ[1][1] - WJ[1][0] * WJ[0][1]]
    ns, bs = _unit(ncl) if (mut == "cloud_normal_in_aniso_scaler" and aniso) else (nn, big)
    det_m = _dot(ns, cx)
    if mut == "scaler_sqrt_detVk_over_h" and not aniso:
        absdet = (Vk[0][0] * Vk[1][1] - Vk[0][1] * Vk[1][0]).sqrt() / hh
    else:
        absdet = (det_m if mut == "detMk_without_abs" else det_m.abs()).where(bs, 0.0)

    # low-pass filter, ellipse, radii, scaler
    px = L(torch.full((K,), (1.0 if mut == "px_1_over_S" else 2.0) / c.S))
    sp = L(torch.full((K,), 0.0 if mut == "sigma_px2_dropped" else SIGMA)) * (px * px)
    G00, G11, G01, G10 = Vk[0][0] + sp, Vk[1][1] + sp, Vk[0][1], Vk[1][0]
    detG = G00 * G11 - G01 * G10
    ea, ec = G11 / detG, G00 / detG
    eb = (-G01) / detG if mut == "b_without_two" else (-G01) / detG + (-G10) / detG
    den = eps_denom(ea * 4.0 * ec - eb * eb)
    rx = eps_sqrt(ec * 4.0 * CUTOFF / den).sqrt()
    ry = eps_sqrt(ea * 4.0 * CUTOFF / den).sqrt()
    if mut == "radii_swapped":
        rx, ry = ry, rx
    s2 = eps_sqrt(detG * ((2.0 if mut == "two_pi" else 4.0 * math.pi) * math.pi)).sqrt()
    sc = absdet / eps_denom(s2)

    outs = {"screen": (sx, sy, zview), "ellipse": (ea, eb, ec), "radii": (rx, ry), "scaler": (sc,)}
    vals, A = {}, {}
    for name, ts in outs.items():
        v = torch.tensor(DEFAULTS[name], dtype=F64).repeat(P, 1)
        a = torch.zeros(P, len(ts), dtype=F64)
        dflt = torch.tensor(DEFAULTS[name], dtype=F64)
        v[rows] = torch.where(ok[:, None], torch.stack([t.v.to(F64) for t in ts], 1), dflt[None])
        a[rows] = torch.where(ok[:, None], torch.stack([t.a for t in ts], 1), torch.zeros(1, dtype=F64))
        vals[name], A[name] = v, a
    full = lambda x: torch.zeros(P, dtype=torch.bool).index_put_((rows,), x)
    return Ref(full(ok), full(near), full(torch.ones(K, dtype=torch.bool)), vals, A, torch.full((P,), CUTOFF, dtype=F64))


def definition(c):
    """The same outputs from independent fp64 arithmetic, for the owned pairs in the order of `pairs_of`: the projection by
    `camera_reference.project`, Vr and det Mk from an explicit tangent basis Sk (Mk = Sk WJ, `torch.linalg.det`), the
    ellipse from `torch.linalg.inv` of G -> dict name -> (K,k) fp64 (no culling: every owned pair)"""
    from camera_reference import project
    rows, cam, wi = pairs_of(c)
    K = rows.numel()
    M, x = c.M.to(F64)[cam], c.world.to(F64)[wi]
    xh = torch.cat([x, torch.ones(K, 1, dtype=F64)], 1)
    clip = torch.einsum("ki,kij->kj", xh, M)
    w = clip[:, 3]
    Jk = torch.zeros(K, 4, 2, dtype=F64)
    Jk[:, 0, 0] = Jk[:, 1, 1] = 1.0 / w
    Jk[:, 3, :] = -clip[:, :2] / (w * w)[:, None]
    WJ = M[:, :3, :] @ Jk
    f = (c.fn if c.mode == "aniso" else c.normals).to(F64)[wi]
    flen = f.norm(dim=1, keepdim=True)
    big = (flen > 1e-12)[:, 0]
    fh = f / flen.clamp_min(1e-12)
    e = torch.eye(3, dtype=F64)[fh.abs().argmin(1)]          # the axis the normal is least aligned with
    u0 = torch.linalg.cross(fh, e)
    u0 = u0 / u0.norm(dim=1, keepdim=True).clamp_min(1e-300)
    u1 = torch.linalg.cross(fh, u0)
    Sk = torch.stack([u0, u1], 1) * big[:, None, None]
    if c.mode == "aniso":
        q = c.vr6.to(F64)[wi]
        Vr = torch.stack([q[:, [0, 1, 2]], q[:, [1, 3, 4]], q[:, [2, 4, 5]]], 1)
    else:
        h = c.h[{"h_cloud": cam, "h_point": wi, "h_packed": rows}[c.mode]].to(F64)
        Vr = h[:, None, None] * Sk.transpose(1, 2) @ Sk
    G = WJ.transpose(1, 2) @ Vr @ WJ + SIGMA * (2.0 / c.S) ** 2 * torch.eye(2, dtype=F64)
    Gi = torch.linalg.inv(G)
    a, b, cc = Gi[:, 0, 0], Gi[:, 0, 1] + Gi[:, 1, 0], Gi[:, 1, 1]
    den = 4 * a * cc - b * b
    scr = project(c.world.to(F64), c.M.to(F64), c.V.to(F64), c.first, c.num, c.shared)
    return {"screen": scr, "ellipse": torch.stack([a, b, cc], 1),
            "radii": torch.stack([(4 * cc * CUTOFF / den).sqrt(), (4 * a * CUTOFF / den).sqrt()], 1),
            "scaler": (torch.linalg.det(Sk @ WJ).abs() / (torch.linalg.det(G) * 4 * math.pi ** 2).sqrt())[:, None]}


def ratios(got, ref):
    """The check of the CPU and the GPU test.  ``got``: output name -> (P,k) tensor, and "valid" (P,) bool.  On the rows that
    `ref.near` does not list -> (largest (|got - ref| - UNDERFLOW) / A per output over the valid rows' entries with A > 0,
    list of what is wrong beyond a ratio: a decision, an entry with A == 0 -- a default of a culled or unowned row among
    them -- that is not the reference's number exactly).  A non-finite entry counts as an infinite ratio."""
    use = ~ref.near
    wrong = []
    gv = got["valid"].detach().cpu().bool()
    if not torch.equal(gv[use], ref.valid[use]):
        wrong.append("valid: %d decisions differ" % int((gv[use] != ref.valid[use]).sum()))
    worst = []
    for name in OUTPUTS:
        g = got[name].detach().cpu().to(F64).reshape(ref.vals[name].shape)[use]
        r, a = ref.vals[name][use], ref.A[name][use]
        exact = a == 0
        if not torch.equal(g[exact], r[exact]):
            wrong.append("%s: %d entries without a scale are not the reference's numbers" % (name, int((g[exact] != r[exact]).sum())))
        err = ((g - r).abs() - UNDERFLOW).clamp_min(0)[~exact] / a[~exact]
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
        worst.append(float(err.max()) if err.numel() else 0.0)
    return tuple(worst), wrong


def violation(got, ref, bars):
    """by what factor `got` misses ``|got - ref| <= bar A + UNDERFLOW`` on its worst entry (inf: anything `ratios` calls
    wrong, or any error at a bar of 0); <= 1 passes"""
    worst, wrong = ratios(got, ref)
    if wrong or any(b == 0 and w > 0 for w, b in zip(worst, bars)):
        return math.inf
    return max([w / b for w, b in zip(worst, bars) if b > 0] + [0.0])


def band_reach(sx, sy, rx, ry, valid, S, rows, slack_x, slack_y):
    """Which splats can reach the image rows [rows[0], rows[1]) of an S x S image (image column c / row r <-> NDC index
    S - 1 - c / S - 1 - r, pixel centre -1 + (2 i + 1) / S): a valid splat reaches when the pixel centre nearest to it lies
    within its radius on both axes, |ndc - s| <= r.  fp64, on the tensors' device -> (reaches for sure, misses for sure)
    (P,) bool, the test passing / failing with the radii widened and narrowed by the slacks; the rest is within rounding of
    the band's edge."""
    sx, sy, rx, ry, slack_x, slack_y = (torch.as_tensor(t, dtype=F64, device=sx.device) for t in (sx, sy, rx, ry, slack_x, slack_y))

    def dist(s, lo, hi):
        i = torch.round((s + 1.0) * S / 2.0 - 0.5).clamp(lo, hi)
        return (-1.0 + (2.0 * i + 1.0) / S - s).abs()
    dx, dy = dist(sx, 0, S - 1), dist(sy, S - rows[1], S - 1 - rows[0])
    hi = valid & (dx <= rx + slack_x) & (dy <= ry + slack_y)
    lo = valid & (dx <= rx - slack_x) & (dy <= ry - slack_y)
    return lo, ~hi


def reference_reach(ref, bars, S, rows):
    """`band_reach` of a case from its fp64 reference, the slacks being what the bars allow the position and the radius
    (+ the fp32 rounding of the pixel centre and of the difference) -> (reaches, misses, within rounding) (P,) bool"""
    scr, rad = ref.vals["screen"], ref.vals["radii"]
    slack = [bars[0] * ref.A["screen"][:, k] + bars[2] * ref.A["radii"][:, k] + 2.0 ** -22 * (1.0 + scr[:, k].abs() + rad[:, k])
             for k in range(2)]
    lo, miss = band_reach(scr[:, 0], scr[:, 1], rad[:, 0], rad[:, 1], ref.valid, S, rows, slack[0], slack[1])
    return lo, miss, ~lo & ~miss


def oracle_outputs(c, valid):
    """`oracle.point_setup` (the fp32 C mirror of the kernel's arithmetic; it does not cull) on every owned pair of the case,
    in the form `ratios` takes: the rows that ``valid`` (P,) bool does not keep, and the rows no cloud owns, hold the defaults"""
    import numpy as np

    import oracle
    rows, cam, wi = pairs_of(c)
    h = torch.zeros(rows.numel()) if c.mode == "aniso" else c.h[{"h_cloud": cam, "h_point": wi, "h_packed": rows}[c.mode]]
    kw = dict(vr6=c.vr6[wi].numpy(), frame_normals=c.fn[wi].numpy()) if c.mode == "aniso" else {}
    res = oracle.point_setup(c.world[wi].numpy(), c.normals[wi].numpy(), h.numpy(), cam.numpy().astype(np.int32), c.M.numpy(),
                             c.V.numpy(), c.S, CUTOFF, SIGMA, **kw)
    valid = valid.detach().cpu().bool()
    got = {"valid": valid}
    for name, arr in zip(OUTPUTS, res):
        full = torch.tensor(DEFAULTS[name], dtype=torch.float32).repeat(valid.shape[0], 1)
        full[rows] = torch.from_numpy(arr).reshape(rows.numel(), -1)
        got[name] = torch.where(valid[:, None], full, torch.tensor(DEFAULTS[name], dtype=torch.float32)[None])
    return got


def as_got(ref):
    """a Ref (of another dtype, or of a mutant) in the form `ratios` takes"""
    return dict(ref.vals, valid=ref.valid)


# ---------------------------------------------------------------------------------------------------------------------
# the cases that tests/test_setup_reference_cpu.py and tests/test_gpu_setup_reference.py share
# name -> (shared, Pw, first, num, cameras).  No cloud size is a multiple of 64 and no boundary lies on one: wavefronts
# straddle them.  `ragged`: rows [0, 37) and [338, 500) belong to no cloud, cloud 1 is a single point, cloud 2 is empty.
# `shared_partial`: packed out of camera order, camera 1 owns 123 of the 500 points, camera 2 none, rows [623, 1500) no owner.
LAYOUTS = {
    "packed": (False, 1907, [0, 1000, 1777], [1000, 777, 130], ("p0", "ortho", "mirror")),
    "shared": (True, 641, [0, 641, 1282], [641, 641, 641], ("p2", "mirror", "p5")),
    "ragged": (False, 500, [37, 337, 338], [300, 1, 0], ("mirror", "p1", "ortho")),
    "shared_partial": (True, 500, [123, 0, 623], [500, 123, 0], ("p1", "p3", "p4")),
}
MODES = ("h_cloud", "h_point", "h_packed", "aniso")
SIZES = (64, 1024)
CASES = [(layout, mode, backface, S) for layout in LAYOUTS for mode in MODES if mode != "h_packed" or LAYOUTS[layout][0]
         for backface in (False, True) for S in SIZES]
H_MIN, H_MAX = 5e-5, 1e-2          # the reference's clamp of the isotropic h (rasterizer.py:388)
PLANTS = ("zero_normal", "normal_1e-13", "normal_1e-11", "edge_on", "edge_on_1e-4", "off_screen", "big_h_edge_on",
          "vr6_zero", "vr6_rank_one", "frame_normal_other_side")
MIRROR_PLANTS = ("nz_zero", "z_at_near", "z_at_far", "edge_on_exact")      # need the camera whose V is the identity
MIRROR_NEAR, MIRROR_FAR = 0.125, 0.375

Case = namedtuple("Case", "layout mode backface S world normals h M V znear zfar first num shared vr6 fn plants cam_names")


def case_id(key):
    return "%s-%s-%s-S%d" % (key[0], key[1], "backface" if key[2] else "nocull", key[3])


@functools.lru_cache(maxsize=1)
def camera_pool():
    """name -> (M (4,4), V (4,4) fp32, znear, zfar).  p0 ... p5: the views and near planes of `projection_reference.cameras`
    (distances 0.55 ... 29.5 from the unit cube of points, w = view z from 0.3 to 30, the near plane 0.25 in front of the
    cube's centre; p0's far plane cuts the cube as well) under the 60 degree perspective of pytorch3d's FoV camera,
    M = V @ P composed here entry by entry (a library matrix product rounds differently from one CPU to the next, and the
    bars are tied to these very numbers).  `ortho`: the view of p1 with M[:,3] = (0,0,0,1) -- w = 1, the second term of WJ
    vanishes.  `mirror`: V = the identity (zview = z, nz = n_z exactly) and the perspective with its x axis negated
    (negative handedness); w = z in [0.125, 0.375]: the nearest camera."""
    import projection_reference as pr
    _M, V, zn = pr.cameras(6)
    s, far = math.sqrt(3.0), 100.0          # 1 / tan(30 degrees)

    def perspective(v, near, sx=s):
        v, m = v.to(F64), torch.zeros(4, 4, dtype=F64)
        m[:, 0], m[:, 1], m[:, 3] = v[:, 0] * sx, v[:, 1] * s, v[:, 2]
        m[:, 2] = v[:, 2] * (far / (far - near)) + v[:, 3] * (-far * near / (far - near))
        return m.float()
    pool = {"p%d" % k: (perspective(V[k], float(zn[k])), V[k].clone(), float(zn[k]), far) for k in range(6)}
    pool["p0"] = pool["p0"][:3] + (0.55 + 0.3,)
    Mo = (V[1].to(F64) * torch.tensor([1.0 / 1.2, 1.0 / 1.2, 1.0, 1.0], dtype=F64)[None]).float()
    Mo[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    pool["ortho"] = (Mo, V[1].clone(), float(zn[1]), far)
    pool["mirror"] = (perspective(torch.eye(4), 0.1, -s), torch.eye(4), MIRROR_NEAR, MIRROR_FAR)
    return pool


# (the helpers of the plants: products and the 3 x 3 solve written out term by term -- a library matrix product or solver rounds
# differently from one CPU to the next)
def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _unit3(a):
    return a / a.norm()


def _cross3(a, b):
    return torch.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _place(M, V, zn, zf, ndc, frac):
    """the world point (fp64 solve, rounded to fp32) that camera (M, V) sees at ``ndc`` and at view depth
    zn + frac (min(zf, zn + 0.5) - zn)"""
    M, V = M.to(F64), V.to(F64)
    zt = zn + frac * (min(zf, zn + 0.5) - zn)
    coef = torch.stack([M[:, 0] - ndc[0] * M[:, 3], M[:, 1] - ndc[1] * M[:, 3], V[:, 2]])      # (3,4) . xh = (0, 0, zt)
    A, b = coef[:, :3], torch.tensor([0.0, 0.0, zt], dtype=F64) - coef[:, 3]
    cols = [A[:, 0], A[:, 1], A[:, 2]]
    det = _dot3(cols[0], _cross3(cols[1], cols[2]))                                              # Cramer's rule
    return torch.stack([_dot3(b, _cross3(cols[1], cols[2])), _dot3(cols[0], _cross3(b, cols[2])),
                        _dot3(cols[0], _cross3(cols[1], b))]).div(det).float()


def _ray(M, x):
    """the unit world direction along which the projection of camera M does not move at x (WJ[:,0] x WJ[:,1]), fp64"""
    M = M.to(F64)
    x = x.to(F64)
    clip = x[0] * M[0] + x[1] * M[1] + x[2] * M[2] + M[3]
    WJ = M[:3, :2] / clip[3] - M[:3, 3:4] * clip[None, :2] / (clip[3] * clip[3])
    return _unit3(_cross3(WJ[:, 0], WJ[:, 1]))


def _perp(r):
    e = torch.eye(3, dtype=F64)[int(r.abs().argmin())]
    return _unit3(_cross3(r, e))


def case(layout, mode, backface, S):
    """-> Case of fp32 / int64 CPU tensors (see `_geometry`) in one mode, culling setting and image size"""
    world, normals, hs, M, V, znear, zfar, first, num, shared, vr6, fn, plants, cams = _geometry(layout)
    aniso = mode == "aniso"
    return Case(layout, mode, backface, S, world, normals, hs[mode], M, V, znear, zfar, first, num, shared,
                vr6 if aniso else None, fn if aniso else None, plants, cams)


@functools.lru_cache(maxsize=None)
def _geometry(layout):
    """The geometry is seeded by the layout alone (every mode, both culling settings and
    both image sizes see the same points): points uniform in the cube [-0.5, 0.5]^3, normals of random direction and length
    m 2^e, m uniform in [1, 2), e in [-10, 9] (1e-3 ... 1e3), h = 5e-5 m 2^e with e in [0, 7], clamped to [5e-5, 1e-2];
    `h_cloud`: (1e-2 on the camera of the plants, then 7e-4, 5e-5).  Anisotropic: frame normals of random direction
    (independent of the cloud normals: half of them face the other way) and Vr = s P B B^T P with P the projector off the
    frame normal, B uniform in [-1, 1]^(3x3), s like h.  Only `rand`, `randint`, elementwise operations and norms of
    three-vectors (no library matrix product or solver, whose rounding depends on the CPU).  The PLANTS overwrite rows spread over the cloud of the plants' camera (`mirror` where
    the layout has it, else camera 0); `plants`: name -> packed row."""
    shared, Pw, first, num, cams = LAYOUTS[layout]
    N = len(num)
    P = N * Pw if shared else Pw
    g = torch.Generator().manual_seed(4000 + list(LAYOUTS).index(layout))
    u = lambda *s: torch.rand(*s, generator=g)
    logu = lambda n, lo, hi: torch.ldexp(1.0 + u(n), torch.randint(lo, hi + 1, (n,), generator=g))
    unit = lambda n: torch.nn.functional.normalize(u(n, 3) * 2.0 - 1.0, dim=1)
    pool = camera_pool()
    M, V = torch.stack([pool[k][0] for k in cams]), torch.stack([pool[k][1] for k in cams])
    znear = torch.tensor([pool[k][2] for k in cams], dtype=torch.float32)
    zfar = torch.tensor([pool[k][3] for k in cams], dtype=torch.float32)
    world = u(Pw, 3) - 0.5
    normals = unit(Pw) * logu(Pw, -10, 9)[:, None]
    h_point = (5e-5 * logu(Pw, 0, 7)).clamp(H_MIN, H_MAX)
    h_packed = (5e-5 * logu(P, 0, 7)).clamp(H_MIN, H_MAX)
    fn = unit(Pw)
    B = (u(Pw, 3, 3) * 2.0 - 1.0).to(F64)
    s_vr = (5e-5 * logu(Pw, 0, 7)).clamp(H_MIN, H_MAX).to(F64)
    first_t, num_t = torch.tensor(first, dtype=torch.int64), torch.tensor(num, dtype=torch.int64)

    star = cams.index("mirror") if "mirror" in cams else 0
    h_cloud = torch.tensor([H_MAX, 7e-4, H_MIN])[[(k - star) % N for k in range(N)]]
    Ms, Vs, zn, zf = M[star], V[star], float(znear[star]), float(zfar[star])
    names = PLANTS + (MIRROR_PLANTS if "mirror" in cams else ())
    count = num[star]
    spots = [int((i + 0.5) * count / len(names)) for i in range(len(names))]          # cloud-local
    plants = {}

    def mm3(a, b):
        return torch.stack([torch.stack([a[..., i, 0] * b[..., 0, j] + a[..., i, 1] * b[..., 1, j] + a[..., i, 2] * b[..., 2, j]
                                         for j in range(3)], -1) for i in range(3)], -2)

    def vr_of(f, Bm, s):
        Pm = torch.eye(3, dtype=F64) - f[..., :, None] * f[..., None, :]
        return s[..., None, None] * mm3(mm3(Pm, mm3(Bm, Bm.transpose(-1, -2))), Pm)

    vr = vr_of(fn.to(F64), B, s_vr)
    for k, name in enumerate(names):
        loc = spots[k]
        wi, p = (loc if shared else first[star] + loc), first[star] + loc
        plants[name] = p
        x = _place(Ms, Vs, zn, zf, (0.3 - 0.05 * k, -0.2 + 0.04 * k), 0.1 if name == "big_h_edge_on" else 0.3 + 0.04 * k)
        facing = lambda t: -t if float(_dot3(t, Vs[:3, 2].to(F64))) > 0 else t          # towards the camera: nz < 0
        nrm, keep_fn = None, False
        if name == "zero_normal":
            nrm = torch.zeros(3)
        elif name in ("normal_1e-13", "normal_1e-11"):
            nrm = facing(unit(1)[0].to(F64)).float() * float(name[7:])
        elif name in ("edge_on", "edge_on_1e-4", "big_h_edge_on"):
            r = _ray(Ms, x)
            t = facing(_perp(r))
            if name == "edge_on_1e-4":
                t = t * math.cos(1e-4) - facing(r) * math.sin(1e-4)
            nrm = t.float()
            if name == "big_h_edge_on":
                h_point[wi], h_packed[p], s_vr[wi] = H_MAX, H_MAX, H_MAX
        elif name == "off_screen":
            x = _place(Ms, Vs, zn, zf, (5.0, -5.0), 0.5)
            nrm = (facing(Vs[:3, 2].to(F64)) * 2.0).float()
        elif name == "vr6_zero":
            vr[wi] = 0.0
            nrm, keep_fn = (facing(Vs[:3, 2].to(F64)) * 0.5).float(), True
        elif name == "vr6_rank_one":
            t = _perp(fn[wi].to(F64))
            vr[wi] = s_vr[wi] * (t[:, None] * t[None, :])
            nrm, keep_fn = (facing(Vs[:3, 2].to(F64)) * 0.25).float(), True
        elif name == "frame_normal_other_side":
            # the cloud normal faces the camera, the frame normal looks away from it, half a radian off the cloud normal's axis
            d = facing(unit(1)[0].to(F64))
            d = d if abs(float(_dot3(d, Vs[:3, 2].to(F64)))) > 0.2 else facing(Vs[:3, 2].to(F64))
            nrm = (d * 3.0).float()
            f = -d * math.cos(0.5) + _perp(d) * math.sin(0.5)
            fn[wi] = _unit3(f).float()
            vr[wi] = vr_of(fn[wi].to(F64), B[wi], s_vr[wi])
            keep_fn = True
        elif name == "nz_zero":
            nrm = torch.tensor([3.0, 0.0, 0.0])
        elif name == "z_at_near":
            x, nrm = torch.tensor([0.03125, -0.0625, MIRROR_NEAR]), torch.tensor([0.0, 0.0, -2.0])
        elif name == "z_at_far":
            x, nrm = torch.tensor([-0.0625, 0.03125, MIRROR_FAR]), torch.tensor([0.0, 0.0, -0.5])
        elif name == "edge_on_exact":
            x, nrm = torch.tensor([0.0625, -0.03125, 0.25]), torch.tensor([0.5, 0.0, -0.125])
        world[wi] = x
        if nrm is not None:
            normals[wi] = nrm
            if not keep_fn:      # in anisotropic mode the frame normal is what the arithmetic sees: it gets the plant as well
                fn[wi] = nrm if float(nrm.norm()) < 1e-6 else torch.nn.functional.normalize(nrm, dim=0)
                vr[wi] = vr_of(fn[wi].to(F64), B[wi], s_vr[wi])
    vr6 = torch.stack([vr[:, 0, 0], vr[:, 0, 1], vr[:, 0, 2], vr[:, 1, 1], vr[:, 1, 2], vr[:, 2, 2]], 1).float()
    hs = {"h_cloud": h_cloud.contiguous(), "h_point": h_point, "h_packed": h_packed, "aniso": torch.zeros(Pw)}
    return world, normals, hs, M, V, znear, zfar, first_t, num_t, shared, vr6, fn, plants, cams


@functools.lru_cache(maxsize=4)
def reference(layout, mode, backface, S):
    return setup(case(layout, mode, backface, S))


def fp32_figures(key):
    """the largest |fp32 torch - fp64| / A of the case per output (what a bar is 4 x of); the fp32 run decides every pair
    that the reference does not list as `near` like fp64 does, and its entries without a scale are fp64's numbers"""
    worst, wrong = ratios(as_got(setup(case(*key), dtype=torch.float32)), reference(*key))
    assert not wrong, (key, wrong)
    return worst


def print_bars():
    """`python -c "import setup_reference as s; s.print_bars()"` in tests/: the table below, measured anew"""
    for key in CASES:
        print("    %r: (%s)," % (key, ", ".join("%.0e" % round_up_1sig(4 * f) if f else "0" for f in fp32_figures(key))))


# ---------------------------------------------------------------------------------------------------------------------
# The bars of tests/test_gpu_setup_reference.py: 4 x the largest |err| / A of `setup(..., dtype=torch.float32)` (plain fp32
# torch on the CPU) against fp64, rounded up to one significant digit; tests/test_setup_reference_cpu.py re-measures the
# figures and asserts the tie.  (layout, mode, backface, S) -> bars of (screen, ellipse, radii, scaler).
BARS = {
    ('packed', 'h_cloud', False, 64): (3e-07, 3e-07, 2e-07, 3e-07),
    ('packed', 'h_cloud', False, 1024): (3e-07, 3e-07, 4e-08, 2e-07),
    ('packed', 'h_cloud', True, 64): (3e-07, 3e-07, 2e-07, 3e-07),
    ('packed', 'h_cloud', True, 1024): (3e-07, 3e-07, 4e-08, 2e-07),
    ('packed', 'h_point', False, 64): (3e-07, 3e-07, 1e-07, 2e-07),
    ('packed', 'h_point', False, 1024): (3e-07, 3e-07, 4e-08, 3e-07),
    ('packed', 'h_point', True, 64): (3e-07, 3e-07, 1e-07, 2e-07),
    ('packed', 'h_point', True, 1024): (3e-07, 3e-07, 4e-08, 3e-07),
    ('packed', 'aniso', False, 64): (3e-07, 2e-07, 2e-07, 3e-07),
    ('packed', 'aniso', False, 1024): (3e-07, 2e-07, 7e-08, 2e-07),
    ('packed', 'aniso', True, 64): (3e-07, 2e-07, 2e-07, 2e-07),
    ('packed', 'aniso', True, 1024): (3e-07, 2e-07, 4e-08, 2e-07),
    ('shared', 'h_cloud', False, 64): (4e-07, 3e-07, 2e-07, 4e-07),
    ('shared', 'h_cloud', False, 1024): (4e-07, 3e-07, 7e-08, 3e-07),
    ('shared', 'h_cloud', True, 64): (4e-07, 3e-07, 2e-07, 4e-07),
    ('shared', 'h_cloud', True, 1024): (4e-07, 3e-07, 7e-08, 3e-07),
    ('shared', 'h_point', False, 64): (4e-07, 3e-07, 2e-07, 4e-07),
    ('shared', 'h_point', False, 1024): (4e-07, 2e-07, 1e-07, 4e-07),
    ('shared', 'h_point', True, 64): (4e-07, 3e-07, 2e-07, 4e-07),
    ('shared', 'h_point', True, 1024): (4e-07, 2e-07, 1e-07, 4e-07),
    ('shared', 'h_packed', False, 64): (4e-07, 3e-07, 2e-07, 4e-07),
    ('shared', 'h_packed', False, 1024): (4e-07, 3e-07, 1e-07, 4e-07),
    ('shared', 'h_packed', True, 64): (4e-07, 3e-07, 2e-07, 4e-07),
    ('shared', 'h_packed', True, 1024): (4e-07, 3e-07, 1e-07, 4e-07),
    ('shared', 'aniso', False, 64): (4e-07, 4e-07, 2e-07, 4e-07),
    ('shared', 'aniso', False, 1024): (4e-07, 4e-07, 2e-07, 3e-07),
    ('shared', 'aniso', True, 64): (4e-07, 4e-07, 2e-07, 4e-07),
    ('shared', 'aniso', True, 1024): (4e-07, 3e-07, 2e-07, 3e-07),
    ('ragged', 'h_cloud', False, 64): (2e-07, 2e-07, 4e-08, 2e-07),
    ('ragged', 'h_cloud', False, 1024): (2e-07, 2e-07, 4e-08, 2e-07),
    ('ragged', 'h_cloud', True, 64): (2e-07, 2e-07, 4e-08, 1e-07),
    ('ragged', 'h_cloud', True, 1024): (2e-07, 2e-07, 4e-08, 2e-07),
    ('ragged', 'h_point', False, 64): (2e-07, 2e-07, 4e-08, 1e-07),
    ('ragged', 'h_point', False, 1024): (2e-07, 2e-07, 4e-08, 2e-07),
    ('ragged', 'h_point', True, 64): (2e-07, 2e-07, 4e-08, 9e-08),
    ('ragged', 'h_point', True, 1024): (2e-07, 2e-07, 4e-08, 2e-07),
    ('ragged', 'aniso', False, 64): (2e-07, 2e-07, 7e-08, 2e-07),
    ('ragged', 'aniso', False, 1024): (2e-07, 1e-07, 3e-08, 2e-07),
    ('ragged', 'aniso', True, 64): (2e-07, 2e-07, 7e-08, 2e-07),
    ('ragged', 'aniso', True, 1024): (2e-07, 1e-07, 3e-08, 2e-07),
    ('shared_partial', 'h_cloud', False, 64): (4e-07, 2e-07, 2e-07, 2e-07),
    ('shared_partial', 'h_cloud', False, 1024): (4e-07, 2e-07, 5e-08, 2e-07),
    ('shared_partial', 'h_cloud', True, 64): (4e-07, 2e-07, 2e-07, 2e-07),
    ('shared_partial', 'h_cloud', True, 1024): (4e-07, 2e-07, 5e-08, 2e-07),
    ('shared_partial', 'h_point', False, 64): (4e-07, 2e-07, 2e-07, 3e-07),
    ('shared_partial', 'h_point', False, 1024): (4e-07, 2e-07, 6e-08, 2e-07),
    ('shared_partial', 'h_point', True, 64): (4e-07, 2e-07, 2e-07, 3e-07),
    ('shared_partial', 'h_point', True, 1024): (4e-07, 2e-07, 5e-08, 2e-07),
    ('shared_partial', 'h_packed', False, 64): (4e-07, 3e-07, 2e-07, 3e-07),
    ('shared_partial', 'h_packed', False, 1024): (4e-07, 2e-07, 5e-08, 2e-07),
    ('shared_partial', 'h_packed', True, 64): (4e-07, 2e-07, 2e-07, 2e-07),
    ('shared_partial', 'h_packed', True, 1024): (4e-07, 2e-07, 5e-08, 2e-07),
    ('shared_partial', 'aniso', False, 64): (4e-07, 3e-07, 2e-07, 3e-07),
    ('shared_partial', 'aniso', False, 1024): (4e-07, 2e-07, 6e-08, 2e-07),
    ('shared_partial', 'aniso', True, 64): (4e-07, 3e-07, 2e-07, 2e-07),
    ('shared_partial', 'aniso', True, 1024): (4e-07, 2e-07, 6e-08, 2e-07),
}
