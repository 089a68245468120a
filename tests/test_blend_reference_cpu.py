"""CPU: the fp64 reference of the forward blend (`tests/blend_reference.py`) against the C oracle, the reference project's
recorded images and the backward's weight sum; the tie of its bars to what plain fp32 loses; and the wrong formulas that the
bars must catch.

1. The reference against `oracle.blend_forward` on every case (the oracle has no limit on K): the oracle evaluates
   ``expf(-0.5 q)`` and ``f w / cum`` in fp32 with sequential sums, so it is held to the bars of the kernels, entry by entry;
   against ``<name>_norm_image`` of tests/golden/ref_blend.npz (the reference project's renderer and weighted-sum kernels,
   executed) on its three scenes; and the fp32 restatement's `wsum` against `gather_reference._weight_sum`.
2. `blend_reference.BARS` is 4 x the re-measured figure of the fp32 restatement, rounded up to one significant digit, and no
   bar exceeds 1e-5.
3. Every floor-bearing case has at least 10 occupied pixels below the floor and 10 above, `floor` at least 10 in each of
   its planted classes, `holes` at least 100 pixels with a live slot behind a dead one, and every splat case pixels whose
   list is full.
4. Every wrong formula of `blend_reference.MUTATIONS` lies at least 10 x beyond the bar on at least one entry of every case
   listed next to it there:

       no_scaler / exp_const             weight without scaler; -0.7213 for -0.72134752      fragments, splats, teapot (wsum)
       q_neighbour / unnormalised        q of the slot before; no division by cum              fragments, splats, teapot
       no_clamp / clamp_1e5              the floor missing; 1e-5 for 1e-4                      floor, grazing
       stop_at_hole / alpha_any_slot     stops at the first -1; alpha from any live slot       holes
       tail_dropped                      only k < 4 (K // 4)                                   every K % 4 != 0 fragment and splat case
       feat_stride8 / feat_stride3       feat rows 8 (3) floats apart                          the C cases other than C = 8 (C = 3)
       wsum_unclamped                    the wsum output without the floor                     floor, splats, grazing
"""
import os

import numpy as np
import pytest

import blend_reference as br
import gather_reference as gr
import oracle


def _below_above(c):
    s = br.weight_sum64(c)[c.occ > 0]
    return int((s < 1e-4).sum()), int((s > 1e-4).sum())


@pytest.mark.parametrize("name", br.CASES)
def test_case_reaches_its_fork(name):
    c = br.case(name)
    live = c.idx >= 0
    if name in br.FRAGMENT_CASES:
        assert (c.N, c.S, c.P) == (2, 40, 500) and (c.N * c.S * c.S) % 256 != 0
    if name.startswith("frag_"):
        n = live.sum(-1)
        assert n.min() == 0 and n.max() == c.K and (c.occ == (n > 0)).all()
        assert float(c.qv[live].max()) > 15.0 and float(c.scaler.min()) < 1e-5 and float(c.scaler.max()) > 10.0
    if name in br.FLOOR_CASES:
        below, above = _below_above(c)
        assert below >= 10 and above >= 10, (name, below, above)
    if name in br.SPLAT_CASES:
        n = live.sum(-1)
        assert int((n == c.K).sum()) >= 100 and (c.K == 1 or int(((n > 0) & (n < c.K)).sum()) >= 100), name
    if name.startswith("grazing_"):
        assert float(c.qv[live].max()) > 15.0
    if name == "floor":
        s, f = br.weight_sum64(c), float(br.FLOOR)
        rel = s / f - 1.0
        classes = dict(far_below=(s > 0) & (s < 0.1 * f), near_below=(rel < 0) & (rel > -1e-6), near_above=(rel > 0) & (rel < 1e-6),
                       far_above=s > 10 * f, empty=~live.any(-1))
        assert all(int(m.sum()) >= 10 for m in classes.values()), {k: int(m.sum()) for k, m in classes.items()}
        assert int((classes["empty"] & (c.occ == 0)).sum()) >= br.FLOOR_PLANTED
    if name == "holes":
        behind = (live & (np.cumsum(~live, -1) > 0)).any(-1)
        assert int(behind.sum()) >= 100 and int((behind & ~live[..., 0]).sum()) >= 100 and (c.occ == live[..., 0]).all()


@pytest.mark.parametrize("name", br.CASES)
def test_reference_against_the_oracle(name):
    c, r, bars = br.case(name), br.ref(name), br.BARS[name]
    img = oracle.blend_forward(c.idx, c.qv, c.occ, c.scaler, c.feat)
    assert np.array_equal(img[..., c.C], c.occ)
    v = br.violation(img, r.img, r.img_A, bars["img"])
    print("oracle on %s: %.3g of the bar" % (name, v))
    assert v <= 1, (name, v)


@pytest.mark.parametrize("name", br.GOLDEN_CASES)
def test_reference_against_the_recorded_reference_images(name, golden_dir):
    r = br.ref(name)
    g = np.load(os.path.join(golden_dir, "ref_blend.npz"))[name + "_norm_image"]
    v = br.violation(g, r.img, r.img_A, br.BARS[name]["img"])
    print("recorded image of %s: %.3g of the bar" % (name, v))
    assert v <= 1, (name, v)


@pytest.mark.parametrize("name", br.CASES)
def test_fp32_weight_sum_against_the_backward_reference(name):
    """`gather_reference._weight_sum` (the fp32 weight sum that the backward's cases take as their input: ``exp(-0.5 q)``,
    sequential) and the restatement's `wsum` are two fp32 evaluations of one sum: both within the bar of the fp64 value"""
    c, r = br.case(name), br.ref(name)
    w = gr._weight_sum(c.idx, c.qv, c.scaler)
    assert w.dtype == np.float32
    assert br.violation(w, r.wsum, r.wsum_A, br.BARS[name]["wsum"]) <= 1
    assert br.violation(br.reference_of(c, np.float32).wsum, r.wsum, r.wsum_A, br.BARS[name]["wsum"]) <= 1


def test_the_case_lists_are_the_ones_asked_for():
    assert set(br.BARS) == set(br.CASES) and len(br.CASES) == len(set(br.CASES))
    ks = lambda names, c: sorted(int(n.split("_")[1][1:]) for n in names if n.endswith("_c%d" % c))
    frag = [n for n in br.FRAGMENT_CASES if n.startswith("frag_")]
    assert ks(frag, 3) == ks(frag, 5) == [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 33, 150]
    for K in (5, 13):
        assert all("frag_k%d_c%d" % (K, C) in br.CASES for C in (1, 2, 3, 4, 5, 8))
    assert ks(br.SPLAT_CASES, 3) == list(range(1, 10)) + [12, 13, 16, 17, 24, 25, 32] and len(br.SPLAT_CASES) == 32
    assert {int(n.rsplit("_c", 1)[1]) for n in br.SPLAT_CASES} == {1, 2, 3, 4, 5, 8}
    signed = [bool((br.case(n).feat < 0).any()) for n in frag]
    assert sum(signed) == len(frag) // 2


@pytest.mark.parametrize("name", br.CASES)
def test_bars_are_four_times_the_fp32_figures(name):
    figs = br.case_figures(name)
    assert br.bars_of(figs) == br.BARS[name], (name, figs)
    assert all(0 < b <= br.BAR_CAP for b in br.BARS[name].values()), name


@pytest.mark.parametrize("mut,name", [(m, n) for m, (_out, names) in br.MUTATIONS.items() for n in names])
def test_wrong_formulas_lie_ten_times_beyond_the_bar(mut, name):
    out = br.MUTATIONS[mut][0]
    r, bad = br.ref(name), br.reference_of(br.case(name), mut=mut)
    v = br.violation(getattr(bad, out), getattr(r, out), getattr(r, out + "_A"), br.BARS[name][out])
    print("%s on %s: %.3g x the bar" % (mut, name, v))
    assert v >= 10, (mut, name, v)
