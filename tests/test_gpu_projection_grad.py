"""GPU: the projection backward -- `ops.project_backward` (`project_backward_kernel`, one thread per point, and
`project_backward_shared_kernel`, eight lanes per point; `csrc/setup.hip::project_backward_impl` chooses) and its restatement
in the gather's epilogue (`render_backward(..., project=)`) against the fp64 closed form of `tests/projection_reference.py`,
entry by entry.

Error bookkeeping: every entry of `grad_world`, and of the reduced feature gradient, is compared with its fp64 value
RELATIVE TO ``A`` = the sum of the absolute products of that entry (`projection_reference`'s header),
``|got - ref| <= bar * A`` (+ `UNDERFLOW` = 1e-30 absolute: the clip squares the components, so a gradient of norm below
about 1e-19 clips to 0 in fp32 while fp64 keeps it); entries without a term must be exact zeros.  No entry is left out.  Each
test prints the largest observed ratio per output.

The bars (`projection_reference.BARS`): for every (case, clip or not) the same formula ran in plain fp32 torch on the CPU
against fp64; a bar is 4 x that figure rounded up to one significant digit (the kernels' operation order, their contracted
multiply-adds and their reciprocal differ from torch's by a few ulp; `tests/test_projection_grad_cpu.py` shows that each of
eleven wrong formulas lies at least 10 x beyond a bar on every case it can affect, and re-measures the figures).  A bar of 0:
nothing is added (one owner per point), the output is the input's bits.

The kernel of a case follows from the dispatch rule (`projection_reference.kernel_of`): 8 = eight lanes per point (a shared
cloud, N >= 2, Pw <= 262,144), 1 = one thread per point (everything else; the `big` cases take its batches of 8 cameras).

fp32 torch on the CPU / bar / kernel on an MI355X, largest |err| / A per output (features: over C = 1, 3, 5, 8):

    case                   clip   k  grad_world                grad_features
    one                    noclip 1  6.7e-08/3e-07/2.5e-08   0.0e+00/0e+00/0.0e+00
    one                    clip   1  4.4e-08/2e-07/2.5e-08   0.0e+00/0e+00/0.0e+00
    single_cam             noclip 1  2.3e-07/1e-06/2.3e-07   0.0e+00/0e+00/0.0e+00
    single_cam             clip   1  2.4e-07/1e-06/2.6e-07   0.0e+00/0e+00/0.0e+00
    lanes2_33              noclip 8  1.0e-07/5e-07/1.7e-07   5.8e-08/3e-07/5.8e-08
    lanes2_33              clip   8  1.2e-07/5e-07/1.7e-07   5.8e-08/3e-07/5.8e-08
    lanes2_3001            noclip 8  2.8e-07/2e-06/2.2e-07   6.0e-08/3e-07/6.0e-08
    lanes2_3001            clip   8  2.3e-07/1e-06/2.5e-07   6.0e-08/3e-07/6.0e-08
    lanes3_33              noclip 8  1.3e-07/6e-07/1.7e-07   7.4e-08/3e-07/7.4e-08
    lanes3_33              clip   8  1.6e-07/7e-07/1.6e-07   7.4e-08/3e-07/7.4e-08
    lanes3_3001            noclip 8  2.2e-07/9e-07/2.7e-07   1.1e-07/5e-07/1.1e-07
    lanes3_3001            clip   8  2.7e-07/2e-06/2.9e-07   1.1e-07/5e-07/1.1e-07
    lanes8_33              noclip 8  1.5e-07/6e-07/1.1e-07   8.0e-08/4e-07/6.4e-08
    lanes8_33              clip   8  1.5e-07/6e-07/1.0e-07   8.0e-08/4e-07/6.4e-08
    lanes8_3001            noclip 8  2.1e-07/9e-07/2.2e-07   1.5e-07/6e-07/1.0e-07
    lanes8_3001            clip   8  2.1e-07/9e-07/2.2e-07   1.5e-07/6e-07/1.0e-07
    lanes9_33              noclip 8  2.1e-07/9e-07/9.5e-08   9.5e-08/4e-07/1.0e-07
    lanes9_33              clip   8  1.7e-07/7e-07/1.1e-07   9.5e-08/4e-07/1.0e-07
    lanes9_3001            noclip 8  1.9e-07/8e-07/2.5e-07   1.5e-07/6e-07/1.3e-07
    lanes9_3001            clip   8  2.2e-07/9e-07/2.9e-07   1.5e-07/6e-07/1.3e-07
    lanes11_33             noclip 8  1.1e-07/5e-07/8.3e-08   1.4e-07/6e-07/6.6e-08
    lanes11_33             clip   8  1.1e-07/5e-07/1.1e-07   1.4e-07/6e-07/6.6e-08
    lanes11_3001           noclip 8  2.3e-07/1e-06/2.2e-07   1.7e-07/7e-07/1.2e-07
    lanes11_3001           clip   8  2.7e-07/2e-06/3.3e-07   1.7e-07/7e-07/1.2e-07
    lanes17_33             noclip 8  1.5e-07/6e-07/1.4e-07   1.0e-07/5e-07/4.9e-08
    lanes17_33             clip   8  1.2e-07/5e-07/1.5e-07   1.0e-07/5e-07/4.9e-08
    lanes17_3001           noclip 8  2.4e-07/1e-06/2.6e-07   1.7e-07/7e-07/1.0e-07
    lanes17_3001           clip   8  2.4e-07/1e-06/2.1e-07   1.7e-07/7e-07/1.0e-07
    shared_partial         noclip 8  1.7e-07/7e-07/2.2e-07   5.9e-08/3e-07/5.9e-08
    shared_partial         clip   8  2.4e-07/1e-06/2.2e-07   5.9e-08/3e-07/5.9e-08
    ragged                 noclip 1  1.6e-07/7e-07/2.1e-07   0.0e+00/0e+00/0.0e+00
    ragged                 clip   1  2.2e-07/9e-07/2.6e-07   0.0e+00/0e+00/0.0e+00
    gap                    noclip 1  1.7e-07/7e-07/1.8e-07   0.0e+00/0e+00/0.0e+00
    gap                    clip   1  1.7e-07/7e-07/1.8e-07   0.0e+00/0e+00/0.0e+00
    big2                   noclip 1  2.8e-07/2e-06/3.5e-07   6.0e-08/3e-07/6.0e-08
    big2                   clip   1  3.7e-07/2e-06/3.5e-07   6.0e-08/3e-07/6.0e-08
    big8                   noclip 1  3.3e-07/2e-06/4.2e-07   2.1e-07/9e-07/2.1e-07
    big8                   clip   1  3.5e-07/2e-06/4.3e-07   2.1e-07/9e-07/2.1e-07
    big9                   noclip 1  3.4e-07/2e-06/4.0e-07   2.0e-07/9e-07/2.0e-07
    big9                   clip   1  3.2e-07/2e-06/3.5e-07   2.0e-07/9e-07/2.0e-07
    big11                  noclip 1  3.3e-07/2e-06/3.1e-07   2.1e-07/9e-07/2.1e-07
    big11                  clip   1  3.6e-07/2e-06/4.1e-07   2.1e-07/9e-07/2.1e-07
    all_culled_shared      noclip 8  0.0e+00/0e+00/0.0e+00   8.7e-08/4e-07/8.7e-08
    all_culled_shared      clip   8  0.0e+00/0e+00/0.0e+00   8.7e-08/4e-07/8.7e-08
    all_culled_packed      noclip 1  0.0e+00/0e+00/0.0e+00   0.0e+00/0e+00/0.0e+00
    all_culled_packed      clip   1  0.0e+00/0e+00/0.0e+00   0.0e+00/0e+00/0.0e+00

    the first 262,144 points of big8 / big11 (test_both_sides_of_the_dispatch; figure and bar of the whole case)
    big8 @262144           noclip 8  3.3e-07/2e-06/4.2e-07   2.1e-07/9e-07/1.3e-07
    big8 @262144           clip   8  3.5e-07/2e-06/4.3e-07   2.1e-07/9e-07/1.3e-07
    big11 @262144          noclip 8  3.3e-07/2e-06/3.1e-07   2.1e-07/9e-07/1.4e-07
    big11 @262144          clip   8  3.6e-07/2e-06/3.5e-07   2.1e-07/9e-07/1.4e-07

    the gather's epilogue (test_fused_epilogue_against_the_closed_form; bar derived at run time): bar/kernel
    tasks per wavefront option 0   9e-07/2.1e-07
    tasks per wavefront option 1   9e-07/2.1e-07
    tasks per wavefront option 2   9e-07/2.5e-07
    tasks per wavefront option 4   9e-07/2.5e-07

No kernel figure exceeds 1.7 x the fp32-torch figure of its case (lanes2_33: 1.7e-07 against 1.0e-07); where the feature
sum has two addends (N = 2, shared_partial) the kernel's figure IS torch's, one correctly rounded addition.
"""
import numpy as np
import pytest
import torch

import projection_reference as pr
import scenes
from dss_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ids = ["%s-%s" % (n, "clip" if c else "noclip") for n, c in pr.CASES]


def _args(c, grad=None):
    return [t.to(DEV) for t in (c.world, c.M, c.V, c.first, c.num, c.grad if grad is None else grad, c.valid)]


def _run(c, C=None, grad=None, out=None):
    """-> grad_world, or (grad_world, grad_features_world) with the first C feature columns"""
    feat = None if C is None else c.feat[:, :C].contiguous().to(DEV)
    return ops.project_backward(*_args(c, grad), c.shared, clip=c.clip, grad_features=feat, out=out)


def _ratio(tag, out_name, got, ref, A, bar):
    """the per-entry check of every comparison here -> the largest (|got - ref| - UNDERFLOW) / A"""
    worst, zeros_ok = pr.entry_ratio(got, ref, A)
    assert zeros_ok, "%s %s: entries without a term must be exact zeros" % (tag, out_name)
    assert worst <= bar, (tag, out_name, worst, bar)
    return worst


def _check_case(c, ref, tag=None):
    """`c` through the operator without and with C = 1, 3, 5, 8 feature columns, every entry against fp64"""
    (gw_ref, A), (fs_ref, fA) = ref
    bars = pr.BARS[(c.name, c.clip > 0)]
    tag = tag or "%s %s (%s)" % (c.name, "clip %.3g" % c.clip if c.clip > 0 else "no clip", pr.kernel_of(c))
    gw = _run(c)
    assert tuple(gw.shape) == tuple(gw_ref.shape)
    worst = [_ratio(tag, "grad_world", gw, gw_ref, A, bars[0]), 0.0]
    for C in pr.FEATURE_CHANNELS:
        gw2, gfw = _run(c, C)
        assert tuple(gfw.shape) == (c.world.shape[0], C)
        worst[0] = max(worst[0], _ratio(tag, "grad_world (C = %d)" % C, gw2, gw_ref, A, bars[0]))
        worst[1] = max(worst[1], _ratio(tag, "grad_features (C = %d)" % C, gfw, fs_ref[:, :C], fA[:, :C], bars[1]))
    print("project_backward %-44s max |err| / A: %s" % (tag, "  ".join("%s %.1e (bar %.0e)" % (n, w, b)
                                                                      for n, w, b in zip(pr.OUTPUTS, worst, bars))))
    return gw


@pytest.mark.parametrize("name,clipped", pr.CASES, ids=_ids)
def test_cases_against_the_closed_form(name, clipped):
    c = pr.case(name, clipped)
    gw = _check_case(c, pr.reference(name, clipped))
    if name.startswith("all_culled"):
        assert bool((gw == 0).all())
    if name == "gap":
        own = torch.zeros(300, dtype=torch.bool)
        own[pr.owned_rows(c.first, c.num)] = True
        gw2, gfw = _run(c, 5)
        assert bool((gw2[~own.to(DEV)] == 0).all()) and bool((gfw[~own.to(DEV)] == 0).all())
        assert torch.equal(gfw[own.to(DEV)], c.feat[own][:, :5].to(DEV))


@pytest.mark.parametrize("clipped", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("name", ["big8", "big11"])
def test_both_sides_of_the_dispatch(name, clipped):
    """The same inputs at Pw = 262,144 (eight lanes per point) and at 262,145 (one thread per point, whose cameras beyond
    the eighth take a second batch of loads with parked addresses): both pinned to fp64, and the first 262,144 points of
    the two agree within the sum of their bars -- not bit for bit, the order of the additions differs."""
    c = pr.case(name, clipped)
    t = pr.truncated(c, pr.SWITCH)
    assert pr.kernel_of(c) == "one-thread" and pr.kernel_of(t) == "eight-lane"
    (gw_ref, A), (fs_ref, fA) = pr.reference(name, clipped)
    cut = ((gw_ref[:pr.SWITCH], A[:pr.SWITCH]), (fs_ref[:pr.SWITCH], fA[:pr.SWITCH]))      # an entry depends on its point alone
    _check_case(t, cut, "%s %s at Pw = 262144 (eight-lane)" % (name, "clip" if clipped else "no clip"))
    bars = pr.BARS[(name, clipped)]
    one, eight = _run(c, 8), _run(t, 8)
    for out_name, a, b, scale, bar in zip(pr.OUTPUTS, one, eight, (A, fA), bars):
        _ratio("%s one-thread" % name, out_name, a, (gw_ref, fs_ref)[out_name == "grad_features"], scale, bar)
        diff = (a[:pr.SWITCH].cpu().double() - b.cpu().double()).abs()
        assert bool((diff <= 2 * bar * scale[:pr.SWITCH] + 2 * pr.UNDERFLOW).all()), out_name
    assert not torch.equal(one[0][:pr.SWITCH], eight[0])      # (two orders of adding: were they equal, one kernel ran twice)


@pytest.mark.parametrize("name", ["lanes11_3001", "shared_partial", "single_cam", "ragged", "gap", "big11"])
def test_culled_slots_do_not_leak(name):
    """NaN and +-inf in `grad_screen` wherever valid == 0 (culled pairs, rows no cloud owns, the parked addresses of the
    one-thread kernel's masked loads among them): the output is finite and has the bits of the run with zeros there."""
    c = pr.case(name, True)
    bad = torch.nonzero(~c.valid)[:, 0]
    assert bad.numel() > 0
    poison, zeros = c.grad.clone(), c.grad.clone()
    poison[bad] = torch.tensor([float("nan"), float("inf"), -float("inf")])[torch.arange(bad.numel()) % 3][:, None]
    zeros[bad] = 0.0
    for C in (None, 3):
        got, want = _run(c, C, grad=poison), _run(c, C, grad=zeros)
        got, want = (got, want) if C else ((got,), (want,))
        for g, w in zip(got, want):
            assert bool(torch.isfinite(g).all()) and torch.equal(g, w)
    assert float(want[0].abs().max()) > 0


def _fused_scene(P, S, N):
    """the smallest shape of test_render_backward_with_fused_projection_equals_project_backward: the bunny cut to P points,
    N distinct clouds, one camera each"""
    pts, nrm = scenes.load_cloud("bunny")
    pts = scenes.normalize_unit_sphere(pts)[:P]
    nrm = nrm[:P]
    h = scenes.global_h(pts)
    az = [30.0, 150.0, 260.0][:N]
    M = np.concatenate([scenes.camera_matrices(2.0, 20.0, a)[0] for a in az])
    V = np.concatenate([scenes.camera_matrices(2.0, 20.0, a)[1] for a in az])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    world = t(np.tile(pts, (N, 1)) + np.repeat(np.arange(N, dtype=np.float32)[:, None] * 0.01, P, 0))
    first = torch.arange(N, device=DEV, dtype=torch.int64) * P
    num = torch.full((N,), P, dtype=torch.int64, device=DEV)
    f = ops.render_forward(world, t(np.tile(nrm, (N, 1))), torch.full((N,), float(h), device=DEV), t(M), t(V),
                           torch.full((N,), 0.1, device=DEV), torch.full((N,), 100.0, device=DEV), first, num,
                           torch.rand((N * P, 3), device=DEV), S, 5, 1.0, 0.05, 1.0, False, False)
    return world, t(M), t(V), first, num, f


def test_fused_epilogue_against_the_closed_form():
    """`render_backward(..., project=(world, M))` against fp64, not only against the separate launch: the reference is fed
    the (clipped) screen gradients of the unfused call of the same variant, whose z component is 0.  The bar is derived as
    everywhere, 4 x what fp32 torch loses on these very inputs, rounded up (at run time: the inputs come from the render)."""
    P, S, N = 3000, 96, 3
    world, M, V, first, num, f = _fused_scene(P, S, N)
    go = torch.randn((N, S, S, 4), device=DEV)
    a = (go, f["idx"], f["qvalue"], f["wsum"], f["scaler"], f["pts_screen"], f["radii"], f["visible"], first, num, 4.0, 0.05)
    cpu = lambda *ts: [t.cpu() for t in ts]
    for tpw in (0, 1, 2, 4):
        _lib.set_option(_lib.OPT_BACKWARD_TPW, tpw)
        try:
            _gf, gs = ops.render_backward(*a)
            _gf2, gw = ops.render_backward(*a, project=(world, M))
        finally:
            _lib.set_option(_lib.OPT_BACKWARD_TPW, 0)
        assert bool((gs[:, 2] == 0).all()) and int((gs[:, 0] != 0).sum()) > 500
        ins = cpu(world, M, V, first, num, gs, f["valid"])
        ref, A = pr.project_backward(*ins, False, -1.0)
        v32, _a = pr.project_backward(*ins, False, -1.0, dtype=torch.float32)
        bar = pr.round_up_1sig(4 * pr.entry_ratio(v32, ref, A)[0])
        worst = _ratio("fused epilogue tpw %d" % tpw, "grad_world", gw, ref, A, bar)
        print("project_backward fused epilogue, tasks per wavefront option %d: max |err| / A = %.1e (bar %.0e)" % (tpw, worst, bar))


@pytest.mark.parametrize("name", ["lanes3_3001", "big2", "ragged"])
def test_out_views_of_one_buffer(name):
    """`out=`: grad_world and grad_features_world as two views of one buffer with sentinels between and after them -- both
    fully written (the bits of the call that allocates), the sentinels untouched"""
    c = pr.case(name, True)
    Pw, C, pad, mark = c.world.shape[0], 5, 64, 7.25
    want = _run(c, C)
    buf = torch.full((Pw * 3 + pad + Pw * C + pad,), mark, device=DEV)
    gw, gfw = buf[:Pw * 3].view(Pw, 3), buf[Pw * 3 + pad:Pw * 3 + pad + Pw * C].view(Pw, C)
    got = _run(c, C, out=(gw, gfw))
    assert got[0].data_ptr() == gw.data_ptr() and got[1].data_ptr() == gfw.data_ptr()
    assert torch.equal(gw, want[0]) and torch.equal(gfw, want[1]) and not bool((gw == mark).any()) and not bool((gfw == mark).any())
    assert bool((buf[Pw * 3:Pw * 3 + pad] == mark).all()) and bool((buf[Pw * 3 + pad + Pw * C:] == mark).all())
    # without features only the first view is written
    buf.fill_(mark)
    assert _run(c, out=(gw, None)).data_ptr() == gw.data_ptr()
    assert torch.equal(gw, want[0]) and bool((buf[Pw * 3:] == mark).all())


@pytest.mark.parametrize("name", ["lanes11_3001", "shared_partial", "big9", "ragged"])
def test_reproducible(name):
    c = pr.case(name, True)
    a = _run(c, 8)
    b = _run(c, 8)
    _run(pr.case("lanes3_33", False), 3)      # an unrelated launch in between
    torch.randn(1 << 20, device=DEV).sum()
    d = _run(c, 8)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, d))


def test_refusals():
    c = pr.case("lanes3_33", False)
    nine = torch.zeros(c.grad.shape[0], 9, device=DEV)
    with pytest.raises(RuntimeError, match=r"dss_project_backward_features failed \(-1\): dss_project_backward_features: the "
                                           r"feature-gradient reduction needs an output and 1 <= C <= 8 \(C = 9\)"):
        ops.project_backward(*_args(c), True, grad_features=nine)
    with pytest.raises(RuntimeError, match=r"grad_features must be packed \(P,C\) with P=99, got \(98, 3\)"):
        ops.project_backward(*_args(c), True, grad_features=nine[:98, :3].contiguous())
    with pytest.raises(RuntimeError, match=r"grad_features must be packed \(P,C\) with P=33, got \(99, 3\)"):
        ops.project_backward(*_args(c)[:3], c.first[:1].to(DEV), c.num[:1].to(DEV), *_args(c)[5:], False,
                             grad_features=nine[:, :3].contiguous())
