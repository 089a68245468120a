"""GPU: the four kernels of dss_amd/csrc/regularizers.hip against the float64 yardstick of tests/regularizer_reference.py,
entry by entry.

Error of an entry = |got - want| / magnitude (1e-30 floor), magnitude = the sum of the absolute values of every product
added to form it.  An entry of magnitude 0 (a kept normal, a row no cloud owns) must hold its value exactly; NaN must
appear exactly where the yardstick has it.  The neighbour lists are built on the CPU (float64 brute force, cloud-local
ids, squared distances rounded to float32), so the kernels and the yardstick see the same inputs; the loss kernels take
the yardstick's mollified normals rounded to float32.

BARS: per case and output (figure, bar).  The figure is the largest per-entry error of the float32 restatement
(`regularizer_reference.restate_*`, numpy, not the code under test) against the yardstick, measured on the CPU; the bar
is 4x the figure -- room for another summation order and the GPU's expf.  tests/test_regularizers_cpu.py re-measures
every figure and fails if a bar is below 2x or above 8x of it.
"""
import os
import types

import numpy as np
import pytest
import torch

import regularizer_cases as rc
import regularizer_reference as rr
from dss_amd import _lib, ops
from dss_amd.cloud import PointClouds3D
from dss_amd.losses import ProjectionLoss, RepulsionLoss, SurfaceLoss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

BARS = {
    # case: {output: (the restatement's figure, bar = 4 x figure)}   # the kernels' figures on an MI355X, same order of outputs
    "P255": {"mollified": (2.59e-07, 1.04e-06), "proj_loss": (1.21e-07, 4.84e-07), "proj_grad": (1.31e-07, 5.24e-07), "rep_loss": (9.82e-08, 3.93e-07), "rep_grad": (2.44e-07, 9.76e-07)},   # kernel: 3.07e-07 4.83e-08 1.23e-07 6.78e-08 2.26e-07
    "P256": {"mollified": (2.75e-07, 1.10e-06), "proj_loss": (8.99e-08, 3.60e-07), "proj_grad": (1.46e-07, 5.84e-07), "rep_loss": (8.84e-08, 3.54e-07), "rep_grad": (3.14e-07, 1.26e-06)},   # kernel: 2.89e-07 6.32e-08 1.50e-07 7.00e-08 3.17e-07
    "P257": {"mollified": (3.53e-07, 1.41e-06), "proj_loss": (9.51e-08, 3.80e-07), "proj_grad": (1.48e-07, 5.92e-07), "rep_loss": (1.43e-07, 5.72e-07), "rep_grad": (2.66e-07, 1.06e-06)},   # kernel: 2.67e-07 5.73e-08 1.34e-07 7.19e-08 2.29e-07
    "K2": {"mollified": (7.51e-08, 3.00e-07), "proj_loss": (2.16e-07, 8.64e-07), "proj_grad": (1.80e-07, 7.20e-07), "rep_loss": (1.03e-07, 4.12e-07), "rep_grad": (2.18e-07, 8.72e-07)},   # kernel: 7.51e-08 2.16e-07 1.80e-07 4.87e-08 2.08e-07
    "K13": {"mollified": (2.52e-07, 1.01e-06), "proj_loss": (7.96e-08, 3.18e-07), "proj_grad": (1.62e-07, 6.48e-07), "rep_loss": (1.30e-07, 5.20e-07), "rep_grad": (2.26e-07, 9.04e-07)},   # kernel: 2.88e-07 6.47e-08 1.45e-07 7.81e-08 2.77e-07
    "K40": {"mollified": (4.17e-07, 1.67e-06), "proj_loss": (4.92e-08, 1.97e-07), "proj_grad": (1.35e-07, 5.40e-07), "rep_loss": (1.81e-07, 7.24e-07), "rep_grad": (2.96e-07, 1.18e-06)},   # kernel: 5.81e-07 7.95e-08 1.72e-07 1.37e-07 3.30e-07
    "ragged": {"mollified": (3.39e-07, 1.36e-06), "proj_loss": (2.95e-07, 1.18e-06), "proj_grad": (1.75e-07, 7.00e-07), "rep_loss": (1.23e-07, 4.92e-07), "rep_grad": (3.09e-07, 1.24e-06)},   # kernel: 3.39e-07 1.75e-07 1.75e-07 1.84e-07 5.04e-07
    "gap": {"mollified": (2.62e-07, 1.05e-06), "proj_loss": (1.30e-07, 5.20e-07), "proj_grad": (1.68e-07, 6.72e-07), "rep_loss": (1.12e-07, 4.48e-07), "rep_grad": (2.70e-07, 1.08e-06)},   # kernel: 3.42e-07 1.30e-07 1.92e-07 6.98e-08 2.19e-07
    "constructed": {"mollified": (2.39e-07, 9.56e-07), "proj_loss": (3.21e-07, 1.28e-06), "proj_grad": (3.91e-07, 1.56e-06), "rep_loss": (1.24e-07, 4.96e-07), "rep_grad": (2.62e-07, 1.05e-06)},   # kernel: 2.38e-07 1.78e-07 2.98e-07 1.14e-07 2.82e-07
    "constructed_sharp": {"mollified": (2.39e-07, 9.56e-07), "proj_loss": (1.62e-06, 6.48e-06), "proj_grad": (3.59e-06, 1.44e-05), "rep_loss": (6.89e-07, 2.76e-06), "rep_grad": (9.87e-06, 3.95e-05)},   # kernel: 2.38e-07 3.17e-06 4.85e-06 8.18e-07 9.76e-06
    "collinear": {"mollified": (2.29e-07, 9.16e-07), "proj_loss": (1.14e-07, 4.56e-07), "proj_grad": (1.75e-07, 7.00e-07), "rep_loss": (1.24e-07, 4.96e-07), "rep_grad": (1.66e-07, 6.64e-07)},   # kernel: 2.29e-07 1.40e-07 2.04e-07 5.38e-08 1.79e-07
    "offset": {"mollified": (2.59e-07, 1.04e-06), "proj_loss": (1.27e-07, 5.08e-07), "proj_grad": (1.39e-07, 5.56e-07), "rep_loss": (1.06e-07, 4.24e-07), "rep_grad": (3.15e-07, 1.26e-06)},   # kernel: 3.09e-07 1.27e-07 1.39e-07 3.78e-08 3.15e-07
    "no_masks": {"mollified": (3.53e-07, 1.41e-06), "proj_loss": (5.92e-08, 2.37e-07), "proj_grad": (1.11e-07, 4.44e-07), "rep_loss": (1.30e-07, 5.20e-07), "rep_grad": (2.76e-07, 1.10e-06)},   # kernel: 3.24e-07 1.36e-07 1.81e-07 7.20e-08 2.54e-07
    "no_grad_loss": {"mollified": (3.53e-07, 1.41e-06), "proj_loss": (9.51e-08, 3.80e-07), "proj_grad": (1.42e-07, 5.68e-07), "rep_loss": (1.43e-07, 5.72e-07), "rep_grad": (2.43e-07, 9.72e-07)},   # kernel: 2.67e-07 5.73e-08 1.40e-07 7.19e-08 2.11e-07
}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(c, moll32):
    g = {k: _t(c[k]) for k in ("points", "normals", "first", "num", "knn_d2", "knn_idx", "visible", "gl1", "gl3")}
    g["keep"], g["moll"] = _t(rc.keep_of(c)), _t(moll32)
    return g


def _kernels(c, g):
    """The three launches of a case -> {output: numpy}"""
    moll = ops.mollify_normals(g["normals"], g["knn_d2"], g["knn_idx"], g["keep"], g["first"], g["num"])
    pl, pg = ops.projection_loss(g["points"], g["moll"], g["knn_d2"], g["knn_idx"], g["visible"], g["first"], g["num"],
                                 c["sigma"], grad_loss=g["gl1"], want_grad=True)
    rl, rg = ops.repulsion_loss(g["points"], g["moll"], g["knn_idx"], g["first"], g["num"], c["sigma"], c["filter_scale"],
                                grad_loss=g["gl3"], want_grad=True)
    return {"mollified": _np(moll), "proj_loss": _np(pl), "proj_grad": _np(pg), "rep_loss": _np(rl), "rep_grad": _np(rg)}


def _check(name, got, want, outputs=rc.OUTPUTS, tag=""):
    """Every finite entry within its bar, NaN exactly where the yardstick has it; prints each figure first."""
    figs = {o: rr.rel_err(got[o], *want[o]) for o in outputs}
    for o in outputs:
        print("%s%s %-9s restatement %.3g  bar %.3g  kernel %.3g" % (name, tag, o, BARS[name][o][0], BARS[name][o][1], figs[o].max()))
    for o in outputs:
        assert np.array_equal(np.isnan(got[o]), np.isnan(want[o][0])), (name, o, "NaN pattern")
        worst = int(np.argmax(figs[o]))
        assert figs[o].max() <= BARS[name][o][1], (name, o, float(figs[o].max()), "entry", np.unravel_index(worst, figs[o].shape))


@pytest.mark.parametrize("name", list(rc.CASES))
def test_kernels_entry_by_entry(name):
    c = rc.case(name)
    want, moll32 = rc.yardstick(name)
    _check(name, _kernels(c, _inputs(c, moll32)), want)


def test_rows_no_cloud_owns_are_written():
    """Three rows between the two clouds belong to no cloud.  Every launch writes them -- the outputs are pre-filled
    with NaN here -- with: the row's own normal, projection loss 0, both gradients exactly 0, and repulsion loss 1 (its
    sums are empty, r = 0, exp(-0); pinned as it is, DESIGN 'Regularisers, entry by entry')."""
    c = rc.case("gap")
    want, moll32 = rc.yardstick("gap")
    g = _inputs(c, moll32)
    P, N, K = len(c["points"]), len(c["num"]), c["K"]
    dev = g["points"].device
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)   # noqa: E731
    moll, pl, pg, rl, rg = nan(P, 3), nan(P), nan(P, 3), nan(P, 3), nan(P, 3)
    keep, vis = g["keep"].view(torch.uint8), g["visible"].view(torch.uint8)
    _lib.call("dss_mollify_normals", dev, g["normals"], g["knn_d2"], g["knn_idx"], keep, g["first"], g["num"], N, P, K, moll)
    _lib.call("dss_projection_loss", dev, g["points"], g["moll"], g["knn_d2"], g["knn_idx"], vis, g["first"], g["num"], N, P, K,
              c["sigma"], g["gl1"], pl, pg)
    ws = _lib.workspace(dev, 24 * N)
    _lib.call("dss_repulsion_loss", dev, g["points"], g["moll"], g["knn_idx"], g["first"], g["num"], N, P, K, c["sigma"],
              c["filter_scale"], g["gl3"], rl, rg, ws, ws.numel())
    got = {"mollified": _np(moll), "proj_loss": _np(pl), "proj_grad": _np(pg), "rep_loss": _np(rl), "rep_grad": _np(rg)}
    gap = np.arange(130, 133)
    assert (rr.cloud_of(P, c["first"], c["num"])[gap] == -1).all()
    assert np.array_equal(got["mollified"][gap], c["normals"][gap])
    assert (got["proj_loss"][gap] == 0).all() and (got["proj_grad"][gap] == 0).all()
    assert (got["rep_loss"][gap] == 1).all() and (got["rep_grad"][gap] == 0).all()
    _check("gap", got, want)                                   # no NaN left anywhere: every row was written


def test_the_three_call_forms_are_bit_equal():
    c = rc.case("ragged")
    g = _inputs(c, rc.yardstick("ragged")[1])
    pa = (g["points"], g["moll"], g["knn_d2"], g["knn_idx"], g["visible"], g["first"], g["num"], c["sigma"])
    ra = (g["points"], g["moll"], g["knn_idx"], g["first"], g["num"], c["sigma"], c["filter_scale"])
    for fn, args, gl in ((ops.projection_loss, pa, g["gl1"]), (ops.repulsion_loss, ra, g["gl3"])):
        both_l, both_g = fn(*args, grad_loss=gl, want_loss=True, want_grad=True)
        only_l, none_g = fn(*args, grad_loss=gl, want_loss=True, want_grad=False)
        none_l, only_g = fn(*args, grad_loss=gl, want_loss=False, want_grad=True)
        assert none_g is None and none_l is None
        for a, b in ((both_l, only_l), (both_g, only_g)):       # bit-equal, NaN rows (the one-point cloud) included
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_masks_of_another_dtype_are_true_where_nonzero():
    """0.5 and 256.0 are true, as for the reference's .bool(); a cast to uint8 made both false."""
    c = rc.case("P257")
    g = _inputs(c, rc.yardstick("P257")[1])
    as_float = lambda m: torch.where(m, torch.tensor([0.5, 256.0], device=DEV).repeat(len(m))[: len(m)], torch.zeros((), device=DEV))  # noqa: E731
    moll = ops.mollify_normals(g["normals"], g["knn_d2"], g["knn_idx"], as_float(g["keep"]), g["first"], g["num"])
    assert torch.equal(moll, ops.mollify_normals(g["normals"], g["knn_d2"], g["knn_idx"], g["keep"], g["first"], g["num"]))
    args = (g["points"], g["moll"], g["knn_d2"], g["knn_idx"])
    assert torch.equal(ops.projection_loss(*args, as_float(g["visible"]), g["first"], g["num"], c["sigma"])[0],
                       ops.projection_loss(*args, g["visible"], g["first"], g["num"], c["sigma"])[0])


def test_end_to_end_through_the_gpu_neighbour_search():
    """ops.knn_points -> the three kernels.  The search finds the brute-force neighbours; its squared distances are the
    GPU's own float32 arithmetic, so the yardstick is evaluated on the lists the kernels were given.  The bars of the
    same cloud with CPU lists hold: the inputs differ by an ulp of d2, the shapes and the arithmetic do not."""
    c = dict(rc.case("P257"))
    g = _inputs(c, None)
    d2, idx = ops.knn_points(g["points"], g["first"], g["num"], c["K"])
    c["knn_d2"], c["knn_idx"] = _found(c, d2, idx)
    lists = (c["knn_d2"], c["knn_idx"])
    moll, moll_mag = rr.mollify_normals(c["normals"], *lists, rc.keep_of(c), c["first"], c["num"])
    moll32 = moll.astype(np.float32)
    want = {"mollified": (moll, moll_mag)}
    want["proj_loss"], want["proj_grad"] = _pairs(rr.projection_loss(c["points"], moll32, *lists, c["visible"], c["first"],
                                                                     c["num"], c["sigma"], c["gl1"]))
    want["rep_loss"], want["rep_grad"] = _pairs(rr.repulsion_loss(c["points"], moll32, c["knn_idx"], c["first"], c["num"],
                                                                  c["sigma"], c["filter_scale"], c["gl3"]))
    _check("P257", _kernels(c, _inputs(c, moll32)), want, tag=" (GPU lists)")


def _found(c, d2, idx):
    """The GPU search's lists on the host, after checking them: self first, the brute-force distances rank by rank, and
    ids that lie at those distances (two neighbours an ulp apart may swap ranks)."""
    d2, idx = _np(d2), _np(idx)
    own = rr.cloud_of(len(d2), c["first"], c["num"])
    rows = np.nonzero(c["num"][own] >= c["K"])[0]              # rows of full lists; shorter clouds are zero-padded
    assert np.array_equal(idx[rows, 0], rows - c["first"][own[rows]])
    assert np.allclose(d2, c["knn_d2"], rtol=1e-5, atol=0)
    x = c["points"].astype(np.float64)
    at = ((x[rows, None] - x[c["first"][own[rows], None] + idx[rows]]) ** 2).sum(-1)
    assert np.allclose(at, d2[rows], rtol=1e-5, atol=0)
    return d2, idx


def _pairs(four):
    return (four[0], four[1]), (four[2], four[3])


def test_loss_modules_through_autograd_on_the_ragged_batch():
    """ProjectionLoss / RepulsionLoss (reduction 'none') on clouds of 257, 0, 5, 1 and 700 points: the value, and the
    gradient autograd delivers to every cloud's points for a random upstream gradient.  The yardstick takes the lists and
    the mollified normals the modules used (both checked on their own above and here)."""
    c = rc.case("ragged")
    first, num = c["first"], c["num"]
    cut = lambda a: [_t(a[f: f + n]) for f, n in zip(first, num)]   # noqa: E731
    params = [torch.nn.Parameter(p) for p in cut(c["points"])]
    pc = PointClouds3D(params, cut(c["normals"]))
    flt = types.SimpleNamespace(visibility=_t(c["visible"]), inmask=_t(c["inmask"]))
    proj = ProjectionLoss(reduction="none", knn_k=c["K"], sharpness_sigma=c["sigma"])
    loss = proj(pc, rebuild_knn=True, points_filter=flt)
    nb = proj.knn_tree
    d2, idx = _found(c, nb.dists, nb.idx)
    moll32 = _np(SurfaceLoss._mollified(pc, nb, flt))
    want = {"mollified": rr.mollify_normals(c["normals"], d2, idx, rc.keep_of(c), first, num)}
    _check("ragged", {"mollified": moll32}, want, outputs=("mollified",), tag=" (modules)")
    (loss * _t(c["gl1"])).sum().backward()
    got = {"proj_loss": _np(loss), "proj_grad": _np(torch.cat([p.grad for p in params]))}
    want["proj_loss"], want["proj_grad"] = _pairs(rr.projection_loss(c["points"], moll32, d2, idx, c["visible"], first, num,
                                                                     c["sigma"], c["gl1"]))
    for p in params:
        p.grad = None
    rep = RepulsionLoss(reduction="none", knn_k=c["K"], sharpness_sigma=c["sigma"], filter_scale=c["filter_scale"])
    lossr = rep(pc, rebuild_knn=True, points_filter=flt)
    assert tuple(lossr.shape) == (len(c["points"]), 3)
    (lossr * _t(c["gl3"])).sum().backward()
    got["rep_loss"], got["rep_grad"] = _np(lossr), _np(torch.cat([p.grad for p in params]))
    want["rep_loss"], want["rep_grad"] = _pairs(rr.repulsion_loss(c["points"], moll32, idx, first, num, c["sigma"],
                                                                  c["filter_scale"], c["gl3"]))
    _check("ragged", got, want, outputs=rc.OUTPUTS[1:], tag=" (modules)")


# ---------------------------------------------------------------------------------------------------------------------
# In-mask filter
# ---------------------------------------------------------------------------------------------------------------------
SCENARIOS = rc.inmask_scenarios()


@pytest.mark.parametrize("scenario", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_inmask_at_constructed_positions(scenario):
    """Positions that are exact in float32: the flags are exact.  A NaN position (NaN coordinate, 0/0) is never in mask."""
    name, pts, M, mask, vis, hand = scenario
    want, _ = rr.points_inmask(pts, M, mask, vis)
    if hand is not None:
        assert np.array_equal(want, hand)
    got = _np(ops.points_inmask(_t(pts), _t(M), _t(mask), _t(vis)))
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0])
    if vis is None:                                             # all-true flags change nothing
        again = _np(ops.points_inmask(_t(pts), _t(M), _t(mask)[:, None], torch.ones(len(pts), dtype=torch.bool, device=DEV)))
        assert np.array_equal(again, want)


def test_inmask_with_perspective_cameras():
    """Random points, three perspective cameras: equal to the yardstick except where the float64 sample lies within
    1e-4 px of a decision boundary (float32 projection error at these sizes is ~1e-5 px); at most 1 % are left out."""
    pts, M, mask = rc.inmask_perspective(GOLDEN)
    want, margin = rr.points_inmask(pts, M, mask)
    sure = margin >= 1e-4
    assert (~sure).mean() <= 0.01 and 0.2 < want.mean() < 0.8
    got = _np(ops.points_inmask(_t(pts), _t(M), _t(mask)))
    assert np.array_equal(got[sure], want[sure]), np.nonzero((got != want) & sure)[0]
