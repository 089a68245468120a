"""GPU: the four kernels and eight entries of dss_amd/csrc/image_loss.hip against the fp64 reference of
tests/image_loss_reference.py, entry by entry, on every path: forward + backward, band sums + losses from sums + band backward,
the fused band form (block partials, all-reduced here in fp64, then gradient + losses + sums in one launch) in its layouts, and
the two autograd wrappers.

Error of an entry = |got - want| / A (floor 1e-30), A = the sum of the absolute values of the terms added to form it.  Where
A == 0 the entry is expected exactly: rgb gradients outside `inside`, at colour ties and with no pixel inside, an all-empty
image's terms; the inside counts are exact.  No entry is left out: every decision is a comparison of fp32 inputs.  The gradient
is compared with the reference evaluated on the sums that the kernel was given (its own forward's), as the backward takes them.

BARS: per case and output (figure, bar).  The figure is the largest per-entry error of the fp32 restatement
(`image_loss_reference.reference_of(dtype=np.float32)`, numpy, not the code under test) against the reference, measured on the
CPU over both lambda pairs, both `grad_total` and three orders of a wavefront's additions; the bar is 4x the figure -- room for
the kernel's own order of additions (the band forms partition the pixels differently) and for fused multiply-adds.
tests/test_image_loss_reference_cpu.py re-measures every figure and fails if a bar is below 2x or above 8x of it.
"""
import numpy as np
import pytest
import torch

import image_loss_reference as ir
from dss_amd import ops
from dss_amd.distributed import RowPartition, band_image_loss
from dss_amd.losses import calc_dr_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BARS = {
    # case: {output: (the restatement's figure, bar = 4 x figure)}   # the kernels' worst figure on an MI355X, all paths, same order
    "soft_1x1x1": {"sums": (3.15e-08, 1.26e-07), "losses": (5.71e-08, 2.28e-07), "grad": (6.94e-08, 2.78e-07)},   # kernel: 3.15e-08 5.71e-08 6.89e-08
    "bin_1x1x1": {"sums": (1.52e-08, 6.08e-08), "losses": (5.36e-08, 2.14e-07), "grad": (2.24e-08, 8.96e-08)},   # kernel: 1.52e-08 5.36e-08 2.24e-08
    "soft_1x1x5": {"sums": (3.34e-08, 1.34e-07), "losses": (2.02e-08, 8.08e-08), "grad": (4.52e-08, 1.81e-07)},   # kernel: 3.34e-08 2.02e-08 4.52e-08
    "bin_1x1x5": {"sums": (1.71e-08, 6.84e-08), "losses": (3.27e-08, 1.31e-07), "grad": (3.98e-08, 1.59e-07)},   # kernel: 1.71e-08 3.27e-08 3.98e-08
    "soft_2x3x1021": {"sums": (5.54e-08, 2.22e-07), "losses": (5.31e-08, 2.12e-07), "grad": (1.05e-07, 4.20e-07)},   # kernel: 1.98e-08 1.47e-08 1.05e-07
    "bin_2x3x1021": {"sums": (3.87e-08, 1.55e-07), "losses": (4.29e-08, 1.72e-07), "grad": (5.54e-08, 2.22e-07)},   # kernel: 1.48e-08 4.29e-08 5.54e-08
    "soft_1x64x64": {"sums": (2.84e-08, 1.14e-07), "losses": (5.02e-08, 2.01e-07), "grad": (9.79e-08, 3.92e-07)},   # kernel: 1.17e-08 4.34e-08 9.78e-08
    "bin_1x64x64": {"sums": (1.34e-08, 5.36e-08), "losses": (5.38e-08, 2.15e-07), "grad": (5.49e-08, 2.20e-07)},   # kernel: 5.49e-09 3.38e-08 5.49e-08
    "soft_1x17x241": {"sums": (2.86e-08, 1.14e-07), "losses": (3.15e-08, 1.26e-07), "grad": (9.65e-08, 3.86e-07)},   # kernel: 7.59e-09 3.15e-08 9.65e-08
    "bin_1x17x241": {"sums": (2.38e-08, 9.52e-08), "losses": (4.77e-08, 1.91e-07), "grad": (7.73e-08, 3.09e-07)},   # kernel: 7.36e-09 2.84e-08 7.73e-08
    "soft_3x37x53": {"sums": (5.04e-08, 2.02e-07), "losses": (6.05e-08, 2.42e-07), "grad": (1.09e-07, 4.36e-07)},   # kernel: 1.12e-08 4.94e-08 1.09e-07
    "bin_3x37x53": {"sums": (2.57e-08, 1.03e-07), "losses": (3.85e-08, 1.54e-07), "grad": (7.17e-08, 2.87e-07)},   # kernel: 2.57e-08 4.86e-08 7.17e-08
    "soft_5x8x8": {"sums": (2.20e-07, 8.80e-07), "losses": (1.41e-07, 5.64e-07), "grad": (8.63e-08, 3.45e-07)},   # kernel: 9.05e-08 2.42e-08 8.59e-08
    "bin_5x8x8": {"sums": (1.49e-07, 5.96e-07), "losses": (7.40e-08, 2.96e-07), "grad": (9.18e-08, 3.67e-07)},   # kernel: 1.22e-07 3.57e-08 9.18e-08
    "soft_65x3x5": {"sums": (1.68e-07, 6.72e-07), "losses": (4.66e-08, 1.86e-07), "grad": (1.28e-07, 5.12e-07)},   # kernel: 1.03e-07 4.38e-08 1.29e-07
    "bin_65x3x5": {"sums": (1.03e-07, 4.12e-07), "losses": (5.99e-08, 2.40e-07), "grad": (1.30e-07, 5.20e-07)},   # kernel: 1.03e-07 5.99e-08 1.30e-07
    "soft_1x512x512": {"sums": (5.26e-09, 2.10e-08), "losses": (2.72e-08, 1.09e-07), "grad": (9.81e-08, 3.92e-07)},   # kernel: 1.90e-09 2.72e-08 9.81e-08
    "bin_1x512x512": {"sums": (2.46e-09, 9.84e-09), "losses": (3.30e-08, 1.32e-07), "grad": (3.39e-08, 1.36e-07)},   # kernel: 2.46e-09 3.30e-08 3.39e-08
    "soft_1x513x512": {"sums": (1.26e-08, 5.04e-08), "losses": (2.58e-08, 1.03e-07), "grad": (1.05e-07, 4.20e-07)},   # kernel: 2.70e-09 2.58e-08 1.05e-07
    "bin_1x513x512": {"sums": (2.89e-09, 1.16e-08), "losses": (2.96e-08, 1.18e-07), "grad": (4.73e-08, 1.89e-07)},   # kernel: 2.29e-09 2.96e-08 4.73e-08
    "soft_1x641x512": {"sums": (4.23e-09, 1.69e-08), "losses": (4.24e-08, 1.70e-07), "grad": (9.77e-08, 3.91e-07)},   # kernel: 1.12e-09 4.24e-08 9.88e-08
    "bin_1x641x512": {"sums": (5.51e-09, 2.20e-08), "losses": (2.41e-08, 9.64e-08), "grad": (4.70e-08, 1.88e-07)},   # kernel: 2.44e-09 2.41e-08 4.70e-08
    "soft_3x128x20": {"sums": (4.76e-08, 1.90e-07), "losses": (7.12e-08, 2.85e-07), "grad": (1.41e-07, 5.64e-07)},   # kernel: 1.92e-08 5.14e-08 1.41e-07
    "soft_2x72x20": {"sums": (3.25e-08, 1.30e-07), "losses": (3.26e-08, 1.30e-07), "grad": (1.17e-07, 4.68e-07)},   # kernel: 1.79e-08 3.26e-08 1.17e-07
    "soft_64x2x3": {"sums": (1.12e-07, 4.48e-07), "losses": (4.02e-08, 1.61e-07), "grad": (1.12e-07, 4.48e-07)},   # kernel: 9.47e-08 3.72e-08 1.11e-07
}


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a C-ordered copy: the cases are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def _up(gt):
    return None if gt is None else torch.tensor([gt], dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def gpu():
    """case -> layout -> (rgba, img, mask) on the device, uploaded once.  Layout 0: dense (N,H,W,3) target, (N,H,W) mask;
    layout 1: the permuted view of an NCHW target (trainer.py:306), (N,1,H,W) mask."""
    cache = {}

    def get(name, layout=0):
        if name not in cache:
            c = ir.case(name)
            rgba, mask = _t(c.rgba), _t(c.mask)
            cache[name] = ((rgba, _t(c.img), mask), (rgba, _t(c.img.transpose(0, 3, 1, 2)).permute(0, 2, 3, 1), mask[:, None]))
            assert not cache[name][1][1].is_contiguous() or c.H * c.W == 1
        return cache[name][layout]
    return get


WORST = {}


def _check(name, out, got, want, A, tag=""):
    """every entry within the case's bar, exact where A == 0; records the ratio for the report"""
    v = ir.violation(got, want, A, BARS[name][out][1])
    WORST[(name, out)] = max(WORST.get((name, out), 0.0), v)
    if not v <= 1:
        e = ir.rel_err(got, want, A)
        i = np.unravel_index(int(np.argmax(e)), e.shape)
        raise AssertionError("%s %s%s: %.3g x the bar at entry %s: got %r want %r A %r" % (name, out, tag, v, i, np.asarray(got)[i],
                                                                                         np.asarray(want)[i], np.asarray(A)[i]))
    return v


def _report(name):
    for o in ir.OUTPUTS:
        if (name, o) in WORST:
            f, b = BARS[name][o]
            print("%s %-6s restatement %.3g  bar %.3g  kernel %.3g (%.2f of the bar)" % (name, o, f, b, WORST[(name, o)] * b, WORST[(name, o)]))


def _check_all(name, lam, gt, losses, sums, grad, rows=None, tag=""):
    """losses (4,), sums (N+1,5), grad (N,r,W,4) of one path (device tensors) against the reference"""
    c, r = ir.case(name), ir.ref(name, lam, gt)
    s = _np(sums)
    _check(name, "sums", s, r.sums, r.sums_A, tag)
    _check(name, "losses", _np(losses), r.losses, r.losses_A, tag)
    want, A = ir.grad_of(c, s, lam, gt, rows)
    _check(name, "grad", _np(grad), want, A, tag)


# ------------------------------------------------------------------------------------------------------------------------
# 1. forward + backward on every shape
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ir.CASES)
def test_forward_backward_entry_by_entry(name, gpu):
    for lam in ir.LAMBDAS:
        for gt in ir.GRAD_TOTALS:
            first = None
            for layout in (0, 1):
                rgba, img, mask = gpu(name, layout)
                losses, sums = ops.image_loss_forward(rgba, img, mask, *lam)
                grad = ops.image_loss_backward(rgba, img, mask, *lam, sums, grad_total=_up(gt))
                if first is None:
                    _check_all(name, lam, gt, losses, sums, grad)
                    first = (losses, sums, grad)
                    again = ops.image_loss_forward(rgba, img, mask, *lam)
                    assert torch.equal(again[0], losses) and torch.equal(again[1], sums)          # a repeated call: the same bits
                else:                                                                              # a strided target: the same bits
                    assert torch.equal(losses, first[0]) and torch.equal(sums, first[1]) and torch.equal(grad, first[2])
    _report(name)


# ------------------------------------------------------------------------------------------------------------------------
# 2. + 3. row bands
# ------------------------------------------------------------------------------------------------------------------------
def _partition(H, kind, arg):
    """-> [(rows argument of ops, image rows)] of every rank"""
    if kind == "contiguous":
        return [((arg[g], arg[g + 1]), np.arange(arg[g], arg[g + 1])) for g in range(len(arg) - 1)]
    parts = [RowPartition(H, arg, g, cyclic=True) for g in range(arg)]
    assert [p.row_indices() for p in parts] == [list(r) for r in ir.cyclic(H, arg)]
    return [(p.rows, np.array(p.row_indices(), np.int64)) for p in parts]


BAND_VARIANTS = [("soft_3x128x20", "contiguous", (0, 64, 128)), ("soft_3x128x20", "contiguous", (0, 40, 41, 128)),
                 ("soft_3x128x20", "contiguous", (0, 0, 128)), ("soft_3x128x20", "cyclic", 2), ("soft_3x128x20", "cyclic", 4),
                 ("soft_2x72x20", "cyclic", 2), ("soft_2x72x20", "cyclic", 4), ("soft_64x2x3", "contiguous", (0, 1, 2)),
                 ("soft_65x3x5", "contiguous", (0, 2, 3))]
_IDS = ["%s-%s-%s" % (n, k, "+".join(str(v) for v in np.diff(a)) if k == "contiguous" else "G%d" % a) for n, k, a in BAND_VARIANTS]


@pytest.mark.parametrize("name,kind,arg", BAND_VARIANTS, ids=_IDS)
def test_band_sums_then_losses_then_band_backward(name, kind, arg, gpu):
    """`image_loss_band_sums` per band, added in fp64 as the all-reduce adds them, `image_loss_from_sums`,
    `image_loss_band_backward`: N = 65 included (the unfused path has no limit on N)"""
    c = ir.case(name)
    parts = _partition(c.H, kind, arg)
    for layout in (0, 1):
        rgba, img, mask = gpu(name, layout)
        bands = [rgba[:, _t(rows)].contiguous() for _a, rows in parts]
        reduced = torch.stack([ops.image_loss_band_sums(b, img, mask, a) for b, (a, _r) in zip(bands, parts)]).sum(0)
        for lam in ir.LAMBDAS:
            losses = ops.image_loss_from_sums(reduced, (c.H, c.W), *lam)                          # fills the totals row
            for gt in ir.GRAD_TOTALS:
                full = ops.image_loss_backward(rgba, img, mask, *lam, ops.image_loss_forward(rgba, img, mask, *lam)[1], grad_total=_up(gt))
                for b, (a, rows) in zip(bands, parts):
                    gb = ops.image_loss_band_backward(b, img, mask, a, *lam, reduced, grad_total=_up(gt))
                    assert tuple(gb.shape) == (c.N, len(rows), c.W, 4)
                    if len(rows):
                        _check_all(name, lam, gt, losses, reduced, gb, rows, " band %s" % (a,))
                        assert torch.equal(gb[..., :3], full[:, _t(rows)][..., :3])               # rgb: the same bits on every path
                        bt = ops.band_targets(img, mask, a)
                        assert torch.equal(ops.image_loss_band_backward(b, img, mask, a, *lam, reduced, grad_total=_up(gt), band_targets=bt), gb)
    _report(name)


@pytest.mark.parametrize("name,kind,arg", BAND_VARIANTS[:-1], ids=_IDS[:-1])
def test_fused_band_form_in_every_layout(name, kind, arg, gpu):
    """`image_loss_band_partials` + `image_loss_band_backward_partials`: the partials of the bands added in fp64 as the
    all-reduce adds them; dense band, (row, camera, col, 4) send-buffer view, column-cropped view of a wider buffer (row stride
    > 4 W); with and without `band_targets`; `alpha_out` into a strided buffer; `want_sums`; N = 64."""
    c = ir.case(name)
    N, W = c.N, c.W
    parts = _partition(c.H, kind, arg)
    for layout in (0, 1):
        rgba, img, mask = gpu(name, layout)
        bands, views, crops, targets = [], [], [], []
        for a, rows in parts:
            b = rgba[:, _t(rows)].contiguous()
            send = torch.zeros((len(rows) + 3, N, W, 4), device=DEV)
            view = send[:len(rows)].permute(1, 0, 2, 3)
            view.copy_(b)
            wide = torch.full((N, len(rows), W + 5, 4), float("nan"), device=DEV)
            crop = wide[:, :, 2:2 + W]
            crop.copy_(b)
            bt = tuple(x.contiguous() for x in ops.band_targets(img, mask, a)) if len(a) > 2 else ops.band_targets(img, mask, a)
            assert len(rows) < 2 or N == 1 or not (view.is_contiguous() or crop.is_contiguous())
            bands.append(b), views.append(view), crops.append(crop), targets.append(bt)
        ps = [ops.image_loss_band_partials(b, img, mask, a) for b, (a, _r) in zip(bands, parts)]
        for p, b, v, cr, bt, (a, _r) in zip(ps, bands, views, crops, targets, parts):              # every layout: the dense call's bits
            assert tuple(p.shape) == (N, 64, 5)
            for band, kw in ((b, dict(band_targets=bt)), (v, {}), (v, dict(band_targets=bt)), (cr, {}), (b, {})):
                assert torch.equal(ops.image_loss_band_partials(band, img, mask, a, **kw), p)
        red = torch.stack(ps).sum(0)                                                               # the all-reduce
        seq = np.zeros((N, 5))
        for blk in range(64):                                                                      # sequentially, in block order
            seq = seq + _np(red)[:, blk]
        tot = np.zeros(5)
        for n in range(N):
            tot = tot + seq[n]
        for lam in ir.LAMBDAS:
            for gt in ir.GRAD_TOTALS:
                up = _up(gt)
                full = ops.image_loss_backward(rgba, img, mask, *lam, ops.image_loss_forward(rgba, img, mask, *lam)[1], grad_total=up)
                for b, v, cr, bt, (a, rows) in zip(bands, views, crops, targets, parts):
                    gb, lb, sb = ops.image_loss_band_backward_partials(b, img, mask, a, *lam, red, grad_total=up, want_sums=True)
                    assert np.array_equal(_np(sb), np.concatenate([seq, tot[None]]))               # the fp64 sum in block order, bit for bit
                    assert tuple(gb.shape) == (N, len(rows), W, 4) and gb.is_contiguous()
                    _check_all(name, lam, gt, lb, sb, gb, rows, " fused %s" % (a,))
                    assert torch.equal(gb[..., :3], full[:, _t(rows)][..., :3])                   # rgb: the same bits on every path
                    asend = torch.full((len(rows) + 3, N, W), 7.0, device=DEV)
                    aview = asend[:len(rows)].permute(1, 0, 2)
                    for band, kw in ((b, dict(band_targets=bt)), (v, {}), (v, dict(band_targets=bt, alpha_out=aview)), (cr, dict(band_targets=bt)),
                                     (cr, {}), (b, {})):
                        g2, l2 = ops.image_loss_band_backward_partials(band, img, mask, a, *lam, red, grad_total=up, **kw)
                        assert torch.equal(g2, gb) and torch.equal(l2, lb) and g2.is_contiguous()
                    assert torch.equal(aview, gb[..., 3]) and bool((asend[len(rows):] == 7.0).all())   # alpha_out == grad[..., 3]; the rest keeps its fill
                    assert np.array_equal(_np(asend), ir.alpha_plane(_np(gb[..., 3]).astype(np.float64)))
    _report(name)


def test_fused_band_form_refuses_more_than_64_images(gpu):
    rgba, img, mask = gpu("soft_65x3x5")
    with pytest.raises(RuntimeError, match=r"dss_image_loss_band_partials: bad arguments \(1 <= N <= 64"):
        ops.image_loss_band_partials(rgba, img, mask, (0, 3))
    part = torch.zeros((65, 64, 5), dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match=r"dss_image_loss_band_backward_partials: bad arguments \(1 <= N <= 64"):
        ops.image_loss_band_backward_partials(rgba, img, mask, (0, 3), 1.0, 1.0, part)


@pytest.mark.parametrize("rows", [(0, 0), (5, 5), (40, 41), (127, 128)])
def test_partials_that_no_pixel_feeds_are_written_as_zeros(rows, gpu):
    """An `out=` buffer prefilled with NaN: every one of the N 64 5 entries is written, those of blocks without pixels are
    exact zeros -- a rank without rows adds nothing to the all-reduce -- and block 0 of a one-row band holds the row's sums."""
    name = "soft_3x128x20"
    c = ir.case(name)
    rgba, img, mask = gpu(name, 1)
    out = torch.full((c.N, 64, 5), float("nan"), dtype=torch.float64, device=DEV)
    band = rgba[:, rows[0]:rows[1]].contiguous()
    got = ops.image_loss_band_partials(band, img, mask, rows, out=out)
    assert got.data_ptr() == out.data_ptr()
    p = _np(out)
    assert not np.isnan(p).any()
    assert (p[:, 1:] == 0).all() and (rows[1] > rows[0] or (p == 0).all())
    if rows[1] > rows[0]:
        want, A = ir.band_sums(c, np.arange(rows[0], rows[1]), nb=64)
        assert ir.violation(p[:, 0], want, A, BARS[name]["sums"][1]) <= 1 and p[0, 0, 2] > 0


# ------------------------------------------------------------------------------------------------------------------------
# 4. the autograd wrappers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soft_3x37x53", "bin_3x37x53", "soft_5x8x8", "soft_1x1x1", "soft_1x513x512"])
def test_autograd_wrappers_entry_by_entry(name, gpu):
    """`losses.calc_dr_loss` and `distributed.band_image_loss` on a single rank; `grad_total` arrives through autograd"""
    c = ir.case(name)
    for lam in ir.LAMBDAS:
        for gt in ir.GRAD_TOTALS:
            rgba, img, mask = gpu(name, 1)
            losses, sums = ops.image_loss_forward(rgba, img, mask, *lam)
            grad = ops.image_loss_backward(rgba, img, mask, *lam, sums, grad_total=_up(gt))
            leaf = rgba.clone().requires_grad_(True)
            out = calc_dr_loss(leaf, img, mask, *lam)
            (out["loss"] if gt is None else out["loss"] * gt).backward()
            got = torch.stack([out["loss"], out["loss_dr_rgb"], out["loss_dr_silhouette"], out["loss_iou"]]).detach()
            assert torch.equal(got, losses) and torch.equal(leaf.grad, grad)                       # the same two launches
            _check_all(name, lam, gt, got, sums, leaf.grad, tag=" calc_dr_loss")
            leaf = rgba.clone().requires_grad_(True)
            out = band_image_loss(leaf, img, mask, RowPartition(c.H, 1, 0), *lam)
            (out["loss"] if gt is None else out["loss"] * gt).backward()
            got = torch.stack([out["loss"], out["loss_dr_rgb"], out["loss_dr_silhouette"], out["loss_iou"]]).detach()
            part = ops.image_loss_band_partials(rgba, img, mask, (0, c.H))
            _g, _l, sb = ops.image_loss_band_backward_partials(rgba, img, mask, (0, c.H), *lam, part, want_sums=True)
            _check_all(name, lam, gt, got, sb, leaf.grad, tag=" band_image_loss")
            assert torch.equal(leaf.grad[..., :3], grad[..., :3])                                  # rgb: the same bits on every path
    _report(name)


# ------------------------------------------------------------------------------------------------------------------------
# lambda gates
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soft_1x1x5", "soft_64x2x3", "bin_3x37x53"])
def test_a_zero_lambda_gives_exact_zeros_on_finite_inputs(name, gpu):
    c = ir.case(name)
    assert np.isfinite(c.rgba).all() and np.isfinite(c.img).all()
    rgba, img, mask = gpu(name)
    part = ops.image_loss_band_partials(rgba, img, mask, (0, c.H))
    for lam, zero_loss, zero_ch in (((0.0, 2.0), 1, slice(0, 3)), ((ir.LAMBDAS[1][0], 0.0), 2, slice(3, 4))):
        losses, sums = ops.image_loss_forward(rgba, img, mask, *lam)
        grad = ops.image_loss_backward(rgba, img, mask, *lam, sums, grad_total=_up(ir.GRAD_TOTALS[1]))
        gb, lb = ops.image_loss_band_backward_partials(rgba, img, mask, (0, c.H), *lam, part, grad_total=_up(ir.GRAD_TOTALS[1]))
        for l, g in ((losses, grad), (lb, gb)):
            assert float(l[zero_loss]) == 0 and bool((g[..., zero_ch] == 0).all())
            assert float(l[0]) == float(l[3 - zero_loss]) > 0 and bool((g != 0).any())
        _check_all(name, lam, ir.GRAD_TOTALS[1], losses, sums, grad, tag=" lambda %s" % (lam,))      # the reference drops the term: the same values


def test_a_negative_lambda_multiplies(gpu):
    """The reference drops a term whose lambda is not positive; the kernels multiply.  Pinned as the kernels have
    it: the reference with its gates taken out (`gate=False`), same bars."""
    name, lam, gt = "soft_3x37x53", (-0.5, -1.5), ir.GRAD_TOTALS[1]
    c = ir.case(name)
    rgba, img, mask = gpu(name)
    losses, sums = ops.image_loss_forward(rgba, img, mask, *lam)
    grad = ops.image_loss_backward(rgba, img, mask, *lam, sums, grad_total=_up(gt))
    r = ir.reference_of(c, lam, gt, gate=False)
    assert r.losses[1] < 0 and r.losses[2] < 0 and (ir.reference_of(c, lam, gt).losses[:3] == 0).all()
    _check(name, "losses", _np(losses), r.losses, r.losses_A, " negative lambda")
    want, A = ir.grad_of(c, _np(sums), lam, gt, gate=False)
    _check(name, "grad", _np(grad), want, A, " negative lambda")
    assert (want[..., :3] < 0).any() and (want[..., :3] > 0).any() and (want[..., 3] != 0).any()


def test_a_zero_lambda_next_to_a_nan_colour_inside_the_masks(gpu):
    """lambda_rgb = 0 with a NaN colour INSIDE both masks: the reference never evaluates the rgb term, the kernels form
    0 * NaN.  Pinned as the kernels have it: the rgb term and the total are NaN, the silhouette and IoU terms and the whole
    gradient are the reference's (the sign of a NaN difference is 0)."""
    name, lam = "soft_1x1x5", (0.0, 2.0)
    c = ir.case(name)
    rgba_np = c.rgba.copy()
    inside = np.argwhere(ir.inside_of(c.rgba[..., 3], c.mask))
    assert len(inside)
    rgba_np[tuple(inside[0])][1] = np.nan
    rgba, (_r, img, mask) = _t(rgba_np), gpu(name)
    losses, sums = ops.image_loss_forward(rgba, img, mask, *lam)
    grad = ops.image_loss_backward(rgba, img, mask, *lam, sums)
    l, r = _np(losses), ir.ref(name, lam)
    assert np.isnan(l[0]) and np.isnan(l[1])
    _check(name, "losses", l[2:], r.losses[2:], r.losses_A[2:], " NaN inside")
    s = _np(sums)
    assert np.isnan(s[:, 1]).all() and np.array_equal(s[:, [0, 2, 3, 4]], _np(ops.image_loss_forward(gpu(name)[0], img, mask, *lam)[1])[:, [0, 2, 3, 4]])
    want, A = ir.grad_of(c, np.nan_to_num(s), lam)
    _check(name, "grad", _np(grad), want, A, " NaN inside")
