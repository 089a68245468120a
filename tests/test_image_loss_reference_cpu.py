"""CPU: what the entry-by-entry GPU tests of the image loss stand on (tests/test_gpu_image_loss_reference.py).

  - the fp64 reference (tests/image_loss_reference.py) against the reference project's own `Trainer.calc_dr_loss` run in float64
    with autograd on soft data (tests/golden/ref_image_loss_f64.npz): 1e-12 of each entry's magnitude A;
  - against the fp32 recording of the same method on binary data (tests/golden/ref_image_loss.npz) and against
    `oracle.image_loss` on every case, soft ones included: the float32 rounding of their outputs;
  - every bar written in the GPU module against the re-measured fp32 restatement: between 2x and 8x of it, 4x as written;
  - every wrong formula of `image_loss_reference.MUTATIONS` at least 10x beyond the bar on every case listed for it;
  - the binary-only scenes that were all the suite had do not separate the first five of them: the reason for this module.
"""
import os
import types

import numpy as np
import pytest

import image_loss_reference as ir
import oracle
import test_gpu_image_loss_reference as gpu_tests

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32_EPS = 2.0 ** -24


def _old_golden(tag):
    z = np.load(os.path.join(GOLDEN, "ref_image_loss.npz"))
    rgba = np.concatenate([z[tag + "_pred"], z[tag + "_mask_pred"][..., None]], -1)
    N, H, W = z[tag + "_mask"].shape
    c = types.SimpleNamespace(name=tag, N=N, H=H, W=W, rgba=rgba, img=z[tag + "_img"], mask=z[tag + "_mask"])
    lam = tuple(float(v) for v in z[tag + "_lambdas"].astype(np.float64))
    return z, c, lam


def test_cases_hold_what_they_claim():
    assert len(ir.CASES) == len(set(ir.CASES)) and set(gpu_tests.BARS) == set(ir.CASES)
    for name in ir.CASES:
        c = ir.case(name)
        a, t = c.rgba[..., 3], c.mask
        if name.startswith("bin_"):
            assert np.isin(a, (0, 1)).all() and np.isin(t, (0, 1)).all()
        else:
            soft = lambda v: ((v > 0) & (v < 1)).any()   # noqa: E731
            assert soft(a) and soft(t)
        assert np.isfinite(ir.ref(name).sums).all() and np.isfinite(ir.ref(name).grad).all()
    for name, n in ir.TINY_U.items():
        s = ir.ref(name).sums[n]
        assert 0 < s[4] < ir.EPS and s[0] >= 1 and ir.case(name).mask[n].max() > 0
        assert (ir.ref(name).grad[n, ..., 3] != 0).any()              # the clamped branch has a non-zero gradient
    for name, n in ir.EMPTY.items():
        assert ir.ref(name).sums[n, 4] == 0 and ir.ref(name).sums[n, 0] == 0
    for name, n in ir.NO_TARGET.items():
        assert not ir.case(name).mask[n].any() and ir.case(name).rgba[n, ..., 3].any()
    c = ir.case("soft_1x64x64")
    a, t, p, g = c.rgba[0, ..., 3].reshape(-1), c.mask[0].reshape(-1), c.rgba[0, ..., :3].reshape(-1, 3), c.img[0].reshape(-1, 3)
    with np.errstate(under="ignore"):
        assert a[0] != t[0] and 0 < abs(np.float64(a[0]) - np.float64(t[0])) < 1.2e-38      # a subnormal difference
        assert all(a[i] != 0 and t[i] != 0 and a[i] * t[i] == 0 for i in (2, 3))          # the fp32 product underflows
    assert not np.isfinite(p[5:8]).all() and not np.isfinite(g[5:8]).all() and not ir.inside_of(a, t)[5:8].any()
    r = ir.ref("soft_1x64x64")
    ga = r.grad[0].reshape(-1, 4)
    assert ga[0, 3] != 0 and ga[0, 0] == r.grad_A[0].reshape(-1, 4)[0, 0] > 0             # signs -1 / +1, not 0
    assert (ga[8, :3] == 0).all() and (r.grad_A[0].reshape(-1, 4)[8, :3] == 0).all()      # colour ties: exact zeros
    assert (ga[5:8, :3] == 0).all()
    # the reduce loop's forks: one block, two blocks, 64 blocks in one trip, a second trip, a last trip with slot 1 cut
    assert [ir.image_blocks(h, w) for _n, h, w in ir.SHAPES[3:5] + ir.SHAPES[8:]] == [1, 2, 64, 64, 64]
    assert 512 * 512 == 4 * 64 * ir.THREADS and 641 * 512 - 5 * 64 * ir.THREADS == 512


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_matches_the_reference_trainer_in_float64(tag):
    z = np.load(os.path.join(GOLDEN, "ref_image_loss_f64.npz"))
    c = ir.golden_case()
    for k in ("rgba", "img", "mask"):
        assert np.array_equal(z[k], getattr(c, k)) and z[k].dtype == np.float32, k      # generated from these inputs
    lam = tuple(z[tag + "_lambdas"])
    assert lam == ir.LAMBDAS["ab".index(tag)]
    r = ir.reference_of(c, lam)
    assert 0 < r.sums[3, 4] < ir.EPS and r.sums[2, 4] == 0 and r.sums[1, 0] == 0 and r.sums[4, 0] > 100
    err = ir.rel_err(z[tag + "_losses"], r.losses[:3], r.losses_A[:3])
    print("golden %s losses %.3g" % (tag, err.max()))
    assert err.max() <= 1e-12
    err = ir.rel_err(z[tag + "_grad"], r.grad, r.grad_A)
    print("golden %s grad %.3g" % (tag, err.max()))
    assert err.max() <= 1e-12
    assert (z[tag + "_grad"][3, ..., 3] != 0).any()


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_reference_matches_the_fp32_recording_on_binary_data(tag):
    """The recording is torch's fp32 arithmetic end to end, its lambdas Python floats.  The gradient entries are one product
    of fp32-rounded factors (two for alpha): two roundings; the losses are fp32 means over up to 5760 pixels, pairwise:
    8 roundings allowed."""
    z, c, lam = _old_golden(tag)
    lam64 = {"a": (1.0, 1.0), "b": (0.7, 2.0), "c": (1.0, 1.0)}[tag]
    assert np.allclose(lam, lam64, rtol=1e-7)
    r = ir.reference_of(c, lam64)
    got = np.array([z[tag + "_loss"], z[tag + "_loss_rgb"], z[tag + "_loss_sil"]], np.float64)
    err = ir.rel_err(got, r.losses[:3], r.losses_A[:3])
    print("recording %s losses %.3g" % (tag, err.max()))
    assert err.max() <= 8 * F32_EPS
    g = np.concatenate([z[tag + "_grad_pred"], z[tag + "_grad_mask_pred"][..., None]], -1)
    err = ir.rel_err(g, r.grad, r.grad_A)
    print("recording %s grad %.3g" % (tag, err.max()))
    assert err.max() <= 4 * F32_EPS


@pytest.mark.parametrize("name", ir.CASES)
def test_oracle_matches_the_reference_to_float32_rounding(name):
    """The oracle computes in double and stores float: every entry within one fp32 rounding of the reference's value (plus
    1e-12 of its magnitude for the two double evaluations, 1e-9 where the IoU gradient's two terms cancel)."""
    c = ir.case(name)
    for lam in ir.LAMBDAS:
        r = ir.ref(name, lam)
        with np.errstate(all="ignore"):
            losses, grad = oracle.image_loss(c.rgba, c.img, c.mask, *lam)
        for got, want, A in ((losses, r.losses, r.losses_A), (grad, r.grad, r.grad_A)):
            got = got.astype(np.float64)
            assert np.isfinite(got).all()
            exact = A == 0
            assert np.array_equal(got[exact], want[exact])
            assert (np.abs(got - want) <= F32_EPS * np.abs(want) + 1e-9 * A + 1e-45).all(), name


def test_restatement_in_float64_is_the_reference():
    for name in ir.CASES[:12]:
        c, r = ir.case(name), ir.ref(name, ir.LAMBDAS[1], ir.GRAD_TOTALS[1])
        f = ir.reference_of(c, ir.LAMBDAS[1], ir.GRAD_TOTALS[1], dtype=np.float64, order="tree")
        for o in ir.OUTPUTS:
            assert np.array_equal(getattr(f, o), getattr(r, o))


def test_bands_add_up_to_the_image():
    """per-band sums added in fp64 are the image's sums (to the rounding of another order), the band gradients its gradient"""
    c = ir.case("soft_3x128x20")
    r = ir.ref("soft_3x128x20", ir.LAMBDAS[1], ir.GRAD_TOTALS[1])
    for bands in (ir.contiguous((0, 64, 128)), ir.contiguous(ir.BANDS_3x128), ir.contiguous((0, 0, 128)), ir.cyclic(128, 2), ir.cyclic(128, 4)):
        assert sorted(np.concatenate(bands)) == list(range(128))
        b = ir.reference_of(c, ir.LAMBDAS[1], ir.GRAD_TOTALS[1], bands=bands)
        assert np.array_equal(b.sums[:, 0], r.sums[:, 0])
        assert ir.rel_err(b.sums, r.sums, np.where(r.sums_A == 0, 1.0, r.sums_A)).max() <= 1e-14
        assert ir.rel_err(b.grad, r.grad, r.grad_A).max() <= 1e-11
    assert [len(b) for b in ir.cyclic(72, 4)] == [24, 16, 16, 16]


@pytest.mark.parametrize("name", ir.CASES)
def test_bars_are_four_times_the_restatement(name):
    """Re-measure the fp32 restatement: the written figure is this machine's to 2 %, the bar 2x to 8x of the measurement."""
    now = ir.case_figures(name)
    assert set(gpu_tests.BARS[name]) == set(ir.OUTPUTS)
    for out in ir.OUTPUTS:
        figure, bar = gpu_tests.BARS[name][out]
        print("%s %-6s measured %.3g  written %.3g  bar %.3g" % (name, out, now[out], figure, bar))
        assert 0 < now[out] < 1e-6
        assert 2 * now[out] <= bar <= 8 * now[out], (name, out, now[out], bar)
        assert abs(bar - 4 * figure) <= 0.02 * bar, (name, out)


def _mutated(mut, name):
    """-> the violation of the mutation's output on the case, worst over lambda and grad_total"""
    out, _names, bounds = ir.MUTATIONS[mut]
    c = ir.case(name) if name in ir.CASES else None
    if out == "alpha_out":                          # the second copy of the alpha gradient in the exchange's send buffer
        g = ir.ref(name).grad[..., 3]
        rows = ir.cyclic(c.H, 4)[0]
        good, bad = ir.alpha_plane(g[:, rows]), ir.alpha_plane(g[:, rows], mut)
        return ir.violation(bad, good, np.zeros_like(good), 0.0)
    bands = None if bounds is None else ir.contiguous(bounds)
    worst = 0.0
    for lam, gt in ir.variants():
        r, bad = ir.ref(name, lam, gt), ir.reference_of(c, lam, gt, mut=mut, bands=bands)
        worst = max(worst, ir.violation(getattr(bad, out), getattr(r, out), getattr(r, out + "_A"), gpu_tests.BARS[name][out][1]))
    return worst


@pytest.mark.parametrize("mut,name", [(m, n) for m, (_o, names, _b) in ir.MUTATIONS.items() for n in names])
def test_wrong_formulas_lie_ten_times_beyond_the_bar(mut, name):
    v = _mutated(mut, name)
    print("%s on %s: %.3g x the bar" % (mut, name, v))
    assert v >= 10, (mut, name, v)


def test_every_mutation_lists_a_case():
    asked = ["inside_half", "inside_product", "union_max", "inter_min", "iou_no_one_minus_t", "iou_no_over_n", "no_001",
             "l1_mean_over_band", "rgb_mean_over_3cnt", "sign_flipped", "grad_total_ignored", "mask_stride_band",
             "target_strides_swapped", "second_trip_dropped", "tail_slot_dropped", "last_block_dropped", "images_from_4_dropped",
             "clamp_branch_full_formula", "alpha_out_dense_strides"]
    assert list(ir.MUTATIONS) == asked and ir.BINARY_BLIND == asked[:5]
    assert all(len(names) >= 1 for _o, names, _b in ir.MUTATIONS.values())


@pytest.mark.parametrize("mut", ir.BINARY_BLIND)
def test_binary_data_cannot_see_the_first_five(mut):
    """On the scenes that were all the suite had -- the three of ref_image_loss.npz and binary images at the GPU test's
    sizes -- these wrong formulas give the reference's sums, losses and gradient bit for bit."""
    scenes = [_old_golden(tag)[1] for tag in "abc"] + [ir.case(n) for n in ("bin_3x37x53", "bin_1x512x512", "bin_5x8x8")]
    for c in scenes:
        for lam, gt in ir.variants():
            r, bad = ir.reference_of(c, lam, gt), ir.reference_of(c, lam, gt, mut=mut)
            for o in ir.OUTPUTS:
                assert np.array_equal(getattr(bad, o), getattr(r, o)), (mut, c.name, o)
