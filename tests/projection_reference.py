"""fp64 CPU reference of the projection backward (TEST INFRASTRUCTURE; plain torch, no product code in the formulas).

The closed form of ``dss_project_backward`` / ``dss_project_backward_features`` (`dss_amd/csrc/setup.hip`): the gradient of
(ndc_x, ndc_y, view_z) of every valid (camera, point) pair w.r.t. the world points, each ENTRY with the sum of its
ABSOLUTE products next to it (the error of a kernel is measured against ``A`` of that entry, not against a sum that may
cancel).  `tests/test_projection_grad_cpu.py` compares it with `torch.autograd` of `camera_reference.project`, ties the bars
below to what plain fp32 torch loses, and shows that eleven wrong formulas lie beyond them.

For the pair (camera n, world point wi; packed row p) with the clipped screen gradient g (`camera_reference.
clip_screen_grad`), xh = (x, y, z, 1), c = xh @ M[n], w = c_w, ndc = c_xy / w, and for i = 0, 1, 2:

    term_i = ((M[n,i,0] - ndc_x M[n,i,3]) g_x + (M[n,i,1] - ndc_y M[n,i,3]) g_y) / w + V[n,i,2] g_z
    A_i    = ((|M[n,i,0]| + a_x |M[n,i,3]|) |g_x| + (|M[n,i,1]| + a_y |M[n,i,3]|) |g_y|) / |w| + |V[n,i,2] g_z|
    a_x    = (|x M[n,0,0]| + |y M[n,1,0]| + |z M[n,2,0]| + |M[n,3,0]|) / |w|      (a_y: column 1)

    grad_world[wi] = sum of term over the cameras n that own wi and whose pair is valid

A cloud that is not shared: world point wi IS packed row wi and one camera at most owns it.  A shared cloud: world point wi
of camera n is packed row ``first[n] + wi`` for ``wi < num[n]``.  An entry without a term (a point no cloud owns, every
owner culled, beyond every camera's ``num``) is an exact zero.  The feature gradients are summed over the OWNING cameras
whatever ``valid`` says (a culled point still carries its colour's gradient); clouds that are not shared keep theirs, and
rows that no cloud owns are zeros.
"""
import functools
import math
from collections import namedtuple

import torch

from camera_reference import F64, _ranges, clip_screen_grad, project
from shading_reference import UNDERFLOW, entry_ratio, round_up_1sig  # noqa: F401  (the GPU test's check)

OUTPUTS = ("grad_world", "grad_features")


def project_backward(world, M, V, first, num, grad_screen, valid, shared, clip, dtype=F64):
    """closed form -> (grad_world (Pw,3), A (Pw,3)), both fp64
    (`dtype=torch.float32`: the same formula in plain fp32 torch, to see what the number format alone costs)"""
    world, M, V, g = (t.to(dtype) for t in (world, M, V, grad_screen))
    g = clip_screen_grad(g, clip)
    val, A = torch.zeros(world.shape[0], 3, dtype=dtype), torch.zeros(world.shape[0], 3, dtype=F64)
    for n, (lo, hi) in enumerate(_ranges(first, num)):
        if hi == lo:
            continue
        wr = slice(0, hi - lo) if shared else slice(lo, hi)
        x, y, z = world[wr].unbind(1)
        m, v, ok = M[n], V[n], valid[lo:hi].bool()
        gx, gy, gz = g[lo:hi].unbind(1)
        parts = lambda j: (x * m[0, j], y * m[1, j], z * m[2, j], m[3, j].expand_as(x))
        total = lambda s: s[0] + s[1] + s[2] + s[3]
        sx, sy = parts(0), parts(1)
        w = total(parts(3))
        nx, ny = total(sx) / w, total(sy) / w
        ax, ay = total([s.abs() for s in sx]) / w.abs(), total([s.abs() for s in sy]) / w.abs()
        for i in range(3):
            t = ((m[i, 0] - nx * m[i, 3]) * gx + (m[i, 1] - ny * m[i, 3]) * gy) / w + v[i, 2] * gz
            a = ((m[i, 0].abs() + ax * m[i, 3].abs()) * gx.abs() + (m[i, 1].abs() + ay * m[i, 3].abs()) * gy.abs()) / w.abs() \
                + (v[i, 2] * gz).abs()
            val[wr, i] += torch.where(ok, t, torch.zeros_like(t))
            A[wr, i] += torch.where(ok, a, torch.zeros_like(a)).to(F64)
    return val.to(F64), A


def owned_rows(first, num):
    """the packed rows that some cloud owns, in camera order (the row order of `camera_reference.project`)"""
    return torch.cat([torch.arange(lo, hi) for lo, hi in _ranges(first, num)] + [torch.zeros(0, dtype=torch.int64)])


def project_backward_autograd(world, M, V, first, num, grad_screen, valid, shared, clip):
    """the same gradient from torch.autograd of `camera_reference.project` -> grad_world (Pw,3) fp64"""
    x = world.to(F64).clone().requires_grad_(True)
    g = clip_screen_grad(grad_screen.to(F64), clip) * valid.to(F64)[:, None]
    own = owned_rows(first, num)
    if own.numel():
        (project(x, M.to(F64), V.to(F64), first, num, shared) * g[own]).sum().backward()
    return torch.zeros_like(x) if x.grad is None else x.grad


def feature_reduce(grad_feat, first, num, shared, Pw=None, dtype=F64):
    """-> (sum (Pw,C), A (Pw,C)) fp64.  Shared: the rows of a world point summed over the cameras that own it, in camera
    order, and the sum of their absolute values (``Pw`` defaults to P / N).  Not shared: the identity on the rows that a
    cloud owns, zeros elsewhere."""
    f = grad_feat.to(dtype)
    if Pw is None:
        Pw = f.shape[0] // len(num) if shared else f.shape[0]
    s, A = torch.zeros(Pw, f.shape[1], dtype=dtype), torch.zeros(Pw, f.shape[1], dtype=F64)
    for lo, hi in _ranges(first, num):
        wr = slice(0, hi - lo) if shared else slice(lo, hi)
        s[wr] += f[lo:hi]
        A[wr] += f[lo:hi].to(F64).abs()
    return s.to(F64), A


# ---------------------------------------------------------------------------------------------------------------------
# the cases that tests/test_projection_grad_cpu.py and tests/test_gpu_projection_grad.py share
SWITCH = 262144        # `project_backward_impl`: a shared cloud of N >= 2 cameras and Pw <= SWITCH takes eight lanes per point
_LANES = [("lanes%d_%d" % (N, Pw), (True, N, Pw, [n * Pw for n in range(N)], [Pw] * N))
          for N in (2, 3, 8, 9, 11, 17) for Pw in (33, 3001)]
_BIG = [("big%d" % N, (True, N, SWITCH + 1, [n * (SWITCH + 1) for n in range(N)], [SWITCH + 1] * N)) for N in (2, 8, 9, 11)]
# name -> (shared, N, Pw, first, num); a shared cloud's tensors have N Pw packed rows (`ops.project_backward` asks that of
# grad_features), whatever part of them the cameras own
LAYOUTS = dict([
    ("one", (True, 1, 1, [0], [1])),
    ("single_cam", (True, 1, 3001, [0], [3001])),
] + _LANES + [
    # camera 1 owns 123 of the 500 points, camera 2 none; packed out of camera order, so that no row is where n Pw + wi is
    ("shared_partial", (True, 3, 500, [123, 0, 623], [500, 123, 0])),
    ("ragged", (False, 4, 378, [0, 300, 300, 377], [300, 0, 77, 1])),
    ("gap", (False, 2, 300, [10, 200], [64, 64])),
] + _BIG + [
    ("all_culled_shared", (True, 3, 257, [0, 257, 514], [257] * 3)),
    ("all_culled_packed", (False, 3, 257, [0, 100, 157], [100, 57, 100])),
])
CASES = [(name, clipped) for name in LAYOUTS for clipped in (False, True)]
FEATURE_CHANNELS = (1, 3, 5, 8)
PLANTS = ("zero", "norm 1e-25", "norm == clip exactly", "norm == clip to the last bit", "norm 1e6 clip")

Case = namedtuple("Case", "name world M V first num grad valid shared clip feat planted")


def kernel_of(case):
    """which kernel `project_backward_impl` launches for the case (from the dispatch rule, not from the kernel)"""
    return "eight-lane" if case.shared and len(case.num) >= 2 and case.world.shape[0] <= SWITCH else "one-thread"


def cameras(N):
    """N perspective cameras (`scenes.camera_matrices`) around the unit cube of points at distances from 0.55 to 29.5, so
    that w = view z spans 0.3 ... 30; the near plane lies 0.25 in front of the cube's centre and cuts the cloud
    -> M, V (N,4,4) fp32, znear (N,)"""
    import numpy as np

    import scenes
    dist = (0.55, 2.0, 4.5, 9.0, 17.0, 29.5)
    Ms, Vs, zn = [], [], []
    for k in range(N):
        d = dist[k % len(dist)]
        M, V, _cam = scenes.camera_matrices(d, 12.0 + 9.0 * (k % 7), 25.0 + 47.0 * k, znear=d - 0.25)
        Ms.append(M)
        Vs.append(V)
        zn.append(d - 0.25)
    return (torch.from_numpy(np.ascontiguousarray(np.concatenate(Ms))), torch.from_numpy(np.ascontiguousarray(np.concatenate(Vs))),
            torch.tensor(zn, dtype=F64))


@functools.lru_cache(maxsize=2)
def case(name, clipped):
    """-> Case of fp32 / int64 / bool CPU tensors, seeded by the name.  Points uniform in the cube [-0.5, 0.5]^3; screen
    gradients normal x 0.05 x 10^U(-1, 1), so that their norms cover two decades; a pair is valid when it is owned, its view
    depth is behind the camera's near plane and a coin (20 %) did not cull it (`all_culled_*`: none is; `one`: its one pair
    is).  ``clipped``: clip = the median norm of the owned pairs (`one`: half the norm of its one pair -- at the median the
    clip would be the identity there), and the PLANTS overwrite five valid pairs spread over the packing (where there are
    eight or more).  `feat` (P,8): the feature gradients, of which a test takes the first C columns."""
    shared, N, Pw, first, num = LAYOUTS[name]
    P = N * Pw if shared else Pw
    g = torch.Generator().manual_seed(1000 + list(LAYOUTS).index(name))
    first, num = torch.tensor(first, dtype=torch.int64), torch.tensor(num, dtype=torch.int64)
    M, V, znear = cameras(N)
    world = torch.rand(Pw, 3, generator=g) - 0.5
    grad = torch.randn(P, 3, generator=g) * 0.05 * 10.0 ** (torch.rand(P, 1, generator=g) * 2.0 - 1.0)
    coin = torch.rand(P, generator=g) > 0.2
    feat = torch.randn(P, 8, generator=g)
    valid = torch.zeros(P, dtype=torch.bool)
    own = torch.zeros(P, dtype=torch.bool)
    for n, (lo, hi) in enumerate(_ranges(first, num)):
        x = world[:hi - lo] if shared else world[lo:hi]
        w = torch.cat([x, torch.ones_like(x[:, :1])], 1).to(F64) @ M[n].to(F64)[:, 3]
        valid[lo:hi] = (w >= znear[n]) & coin[lo:hi]
        own[lo:hi] = True
    if name == "one":
        valid[:] = True
    if name.startswith("all_culled"):
        valid[:] = False
    clip, planted = -1.0, torch.zeros(0, dtype=torch.int64)
    if clipped:
        norms = grad.to(F64).norm(dim=1)[own]
        clip = float((norms.median() * (0.5 if name == "one" else 1.0)).float())      # an fp32 number
        rows = torch.nonzero(valid)[:, 0]
        if rows.numel() >= 8:
            planted = rows[[0, rows.numel() // 4, rows.numel() // 2, 3 * rows.numel() // 4, rows.numel() - 1]]
            grad[planted[0]] = 0.0
            grad[planted[1]] = torch.tensor([0.6, -0.64, 0.48]) * 1e-25
            grad[planted[2]] = torch.tensor([0.0, 0.0, clip])
            grad[planted[3]] = torch.tensor([2.0, 1.0, 2.0]) / 3.0 * clip
            grad[planted[4]] = torch.tensor([-0.48, 0.6, 0.64]) * (1e6 * clip)
    return Case(name, world, M, V, first, num, grad, valid, shared, clip, feat, planted)


def truncated(c, Pw):
    """the first ``Pw`` points of a shared case whose cameras each own all its points: same numbers, same clip"""
    N, full = len(c.num), c.world.shape[0]
    assert c.shared and c.first.tolist() == [n * full for n in range(N)] and c.num.tolist() == [full] * N and Pw <= full
    rows = (torch.arange(N)[:, None] * full + torch.arange(Pw)[None]).reshape(-1)
    return c._replace(world=c.world[:Pw].contiguous(), first=torch.arange(N) * Pw, num=torch.full((N,), Pw, dtype=torch.int64),
                      grad=c.grad[rows], valid=c.valid[rows], feat=c.feat[rows])


@functools.lru_cache(maxsize=2)
def reference(name, clipped):
    """-> ((grad_world, A), (feature sum, A)) of the case in fp64; the feature sum over all eight columns"""
    c = case(name, clipped)
    return reference_of(c)


def reference_of(c, dtype=F64):
    return (project_backward(c.world, c.M, c.V, c.first, c.num, c.grad, c.valid, c.shared, c.clip, dtype=dtype),
            feature_reduce(c.feat, c.first, c.num, c.shared, c.world.shape[0], dtype=dtype))


def fp32_figures(name, clipped):
    """the largest |fp32 torch - fp64| / A of the case per output (what a bar is 4 x of); entries without a term are zeros
    in fp32 as well"""
    c = case(name, clipped)
    figs = []
    for (v32, _a), (v, a) in zip(reference_of(c, dtype=torch.float32), reference(name, clipped)):
        fig, zeros_ok = entry_ratio(v32, v, a)
        assert zeros_ok
        figs.append(fig)
    return tuple(figs)


def violation(got, ref, A, bar):
    """by what factor the worst entry of ``got`` misses ``|got - ref| <= bar A + UNDERFLOW`` (inf: a non-zero entry where
    no term exists, or any error at a bar of 0); <= 1 passes"""
    worst, zeros_ok = entry_ratio(got, ref, A)
    if not zeros_ok or (bar == 0 and worst > 0):
        return math.inf
    return worst / bar if bar > 0 else 0.0


def print_bars():
    """`python -c "import projection_reference as p; p.print_bars()"` in tests/: the table below, measured anew"""
    for name, clipped in CASES:
        figs = fp32_figures(name, clipped)
        print("    (%r, %r): (%s)," % (name, clipped, ", ".join("%.0e" % round_up_1sig(4 * f) if f else "0" for f in figs)))


# ---------------------------------------------------------------------------------------------------------------------
# The bars of tests/test_gpu_projection_grad.py: 4 x the largest |err| / A of the closed form in plain fp32 torch on the CPU
# against fp64, rounded up to one significant digit; tests/test_projection_grad_cpu.py re-measures the figures and asserts
# the tie.  (case, clipped) -> bars of (grad_world, grad_features).
BARS = {
    ('one', False): (3e-07, 0),
    ('one', True): (2e-07, 0),
    ('single_cam', False): (1e-06, 0),
    ('single_cam', True): (1e-06, 0),
    ('lanes2_33', False): (5e-07, 3e-07),
    ('lanes2_33', True): (5e-07, 3e-07),
    ('lanes2_3001', False): (2e-06, 3e-07),
    ('lanes2_3001', True): (1e-06, 3e-07),
    ('lanes3_33', False): (6e-07, 3e-07),
    ('lanes3_33', True): (7e-07, 3e-07),
    ('lanes3_3001', False): (9e-07, 5e-07),
    ('lanes3_3001', True): (2e-06, 5e-07),
    ('lanes8_33', False): (6e-07, 4e-07),
    ('lanes8_33', True): (6e-07, 4e-07),
    ('lanes8_3001', False): (9e-07, 6e-07),
    ('lanes8_3001', True): (9e-07, 6e-07),
    ('lanes9_33', False): (9e-07, 4e-07),
    ('lanes9_33', True): (7e-07, 4e-07),
    ('lanes9_3001', False): (8e-07, 6e-07),
    ('lanes9_3001', True): (9e-07, 6e-07),
    ('lanes11_33', False): (5e-07, 6e-07),
    ('lanes11_33', True): (5e-07, 6e-07),
    ('lanes11_3001', False): (1e-06, 7e-07),
    ('lanes11_3001', True): (2e-06, 7e-07),
    ('lanes17_33', False): (6e-07, 5e-07),
    ('lanes17_33', True): (5e-07, 5e-07),
    ('lanes17_3001', False): (1e-06, 7e-07),
    ('lanes17_3001', True): (1e-06, 7e-07),
    ('shared_partial', False): (7e-07, 3e-07),
    ('shared_partial', True): (1e-06, 3e-07),
    ('ragged', False): (7e-07, 0),
    ('ragged', True): (9e-07, 0),
    ('gap', False): (7e-07, 0),
    ('gap', True): (7e-07, 0),
    ('big2', False): (2e-06, 3e-07),
    ('big2', True): (2e-06, 3e-07),
    ('big8', False): (2e-06, 9e-07),
    ('big8', True): (2e-06, 9e-07),
    ('big9', False): (2e-06, 9e-07),
    ('big9', True): (2e-06, 9e-07),
    ('big11', False): (2e-06, 9e-07),
    ('big11', True): (2e-06, 9e-07),
    ('all_culled_shared', False): (0, 4e-07),
    ('all_culled_shared', True): (0, 4e-07),
    ('all_culled_packed', False): (0, 0),
    ('all_culled_packed', True): (0, 0),
}
