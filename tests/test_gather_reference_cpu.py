"""CPU: the fp64 reference of the render backward's gather (`tests/gather_reference.py`) against the oracle, the tie of its
bars to what plain fp32 loses, and the wrong formulas that the bars must catch.

1. The reference against `oracle.backward_radius` (bit for bit), `oracle.occ_backward_fast`, `oracle.zbuf_backward` +
   `oracle.clip_grad` and `oracle.blend_backward` on every case the oracle fits (all but `long`, whose 260,000 filler
   points are invisible): the oracle rounds every term to fp32 and sums in double, so it is held to the bars of the kernels,
   entry by entry, and its non-zero entries must be exactly the entries that have a term.
2. `gather_reference.BARS` is 4 x the re-measured figure of the fp32 restatement, rounded up to one significant digit.
3. Every wrong formula of `gather_reference.MUTATIONS` lies at least 10 x beyond the bar on at least one entry of every case
   listed next to it there:

       window_xlo / _xhi / _ylo / _yhi   the window one pixel short on one side            pow2, odd100, wide, tiny
       radius_ge                         >= for > at the radius                            tie (pixels at d2 == rs^2 exactly)
       box_and / box_neg / rxry_swap     AND for OR; the box rule for g < 0 too; rx <-> ry  pow2, wide, odd100
       no_mirror                         column xi instead of S - 1 - xi                   pow2, odd37
       centre_map_pow2                   (2 i + 1) fl(1 / S) at an S that is no 2^k         odd37, odd100 (points 1e-5 from a centre)
       no_floor                          the 1e-10 floor missing                           pow2, odd100 (points 5e-6 from a centre)
       upper_median / median_all_points  rs from the upper median; over all points          pow2, ragged
       no_scaler / q_neighbour           weight without scaler; Q of the slot before         pow2, depth_*
       no_clamp                          the 1e-4 clamp missing with wsum = None            nowsum
       exp_const                         -0.7213 for -0.72134752                            pow2, depth_k12c3
       clip_one_component                the clip on x only                                 clip_all, clip_median
       last_row_small_g                  the window's last row dropped where |g| is small    pow2_loss
"""
import numpy as np
import pytest

import gather_reference as gr
import oracle


@pytest.mark.parametrize("name", gr.CASES)
def test_case_reaches_its_fork(name):
    """the shapes the cases are there for (the per-case summary of the reference)"""
    c, info = gr.case(name), gr.reference(name).info
    assert info["candidates"] > 0 and int(c.vis.sum()) > info["candidates"] - 1
    want = dict(pow2=(10, 11), tie=(11, 11), odd37_whole=(37, 37), wide=(44, 128), tiny=(1, 2)).get(name)
    if want:
        assert want[0] <= info["window"] <= want[1], info
    if name in ("odd37", "odd100"):
        assert min(info["cut"]) > 0      # windows cut by each of the four image borders
    if name.startswith("ragged"):
        assert int(c.vis.sum()) % 2 == 1 and c.num.tolist() == [0, 1, 777, 1501] and c.P > int(c.first[-1] + c.num[-1])
    if name == "wide":
        assert info["box"] > 64          # beyond one sweep of 4 x 4 patches at any tasks-per-wavefront value
    if name == "tiny":
        assert info["without_pair"] > 100 and info["box"] <= 2
    if name.startswith("clip"):
        p = int(c.planted[0])
        assert c.vis[p] and gr.reference(name).pairs[p] == 0 and not gr.reference(name).pts[p].any()
    if name == "ragged_flags":
        r = gr.reference(name)
        assert r.rs[0] == 0 and r.rs[3] == 0 and r.rs[1] > 0 and r.rs[2] > 0
        byhand = 40 + 5 + 13 * np.arange(20)
        assert c.vis[byhand].all() and not r.pts_A[byhand].any()
    if name == "long":
        assert c.P > 262144 and int(c.vis.sum()) < 5000
    if name == "nowsum":
        cum = gr._weight_sum(c.idx, c.qv, c.scaler)[c.idx[..., 0] >= 0]
        assert (cum <= 1e-4).mean() > 0.05 and (cum > 1e-2).mean() > 0.05
    if name == "tie":
        on = c.planted[c.vis[c.planted]]
        d = gr.reference_of(c, mut="radius_ge").pairs[on] - gr.reference(name).pairs[on]
        assert (d <= 0).all() and (d < 0).mean() > 0.9      # points on a pixel centre have pixels at d2 == rs^2 exactly


@pytest.mark.parametrize("name", gr.ORACLE_CASES)
def test_reference_against_the_oracle(name):
    c, bars = gr.case(name), gr.BARS[name]
    ref = gr.reference(name, clip=-1.0)
    rs = oracle.backward_radius(c.radii, c.vis, c.first, c.num, c.radii_s)
    assert np.array_equal(rs, ref.rs) and rs.dtype == ref.rs.dtype
    galpha = np.ascontiguousarray(c.grad_out[..., c.C])
    gxy = oracle.occ_backward_fast(c.pts, c.radii, c.vis, rs, galpha, c.first, c.num)
    assert np.array_equal(gxy != 0, ref.pts_A[:, :2] > 0)
    worst, zeros_ok = gr.ratio(gxy, ref.pts[:, :2], ref.pts_A[:, :2])
    assert zeros_ok and worst <= bars["pts"], (name, worst)
    if np.array_equal(oracle.visibility(c.idx, c.P), c.vis):      # no flag set by hand: the oracle's one call is these pieces
        for gz_in in (None, c.grad_zbuf):
            g, o_vis, o_rs = oracle.splat_backward(c.pts, c.radii, c.idx, galpha, gz_in, c.first, c.num, c.radii_s, c.clip)
            r = gr.reference(name, with_z=gz_in is not None)
            worst, zeros_ok = gr.ratio(g, r.pts, r.pts_A)
            assert np.array_equal(o_rs, ref.rs) and zeros_ok and worst <= max(bars["pts"], bars["pts3_clip"], bars["z"]), (name, worst)
    # z column and the clip on the 3-vector
    gz = oracle.zbuf_backward(c.idx, c.grad_zbuf, c.P)
    for clip in (-1.0, gr.CLIP3) + ((c.clip,) if c.clip > 0 else ()):
        g3 = np.concatenate([gxy, gz[:, None]], 1).astype(np.float32)
        r3 = gr.reference(name, with_z=True, clip=clip)
        worst, zeros_ok = gr.ratio(oracle.clip_grad(g3, clip) if clip > 0 else g3, r3.pts, r3.pts_A)
        assert zeros_ok and worst <= max(bars["pts3_clip"], bars["z"], bars["pts"]), (name, clip, worst)
    if c.clip > 0:
        g2 = oracle.clip_grad(np.concatenate([gxy, 0 * gz[:, None]], 1).astype(np.float32), c.clip)
        r2 = gr.reference(name)
        worst, zeros_ok = gr.ratio(g2, r2.pts, r2.pts_A)
        assert zeros_ok and worst <= bars["pts"], (name, worst)
    gf, gocc = oracle.blend_backward(c.grad_out, c.idx, c.qv, c.scaler, c.P)
    assert np.array_equal(gocc, galpha) and np.array_equal(gf != 0, ref.feat_A > 0)
    for key, use_wsum in (("feat", True), ("feat_nowsum", False)):
        r = gr.reference(name, use_wsum=use_wsum)
        worst, zeros_ok = gr.ratio(gf, r.feat, r.feat_A)
        assert zeros_ok and worst <= bars[key], (name, key, worst)


@pytest.mark.parametrize("name", gr.CASES)
def test_bars_are_four_times_the_fp32_figures(name):
    figs = gr.case_figures(name)
    assert gr.bars_of(figs) == gr.BARS[name], (name, figs)


def test_band_references_add_up_to_the_whole_image():
    for name in ("band96", "band100"):
        whole = gr.reference(name)
        bands = gr.band_rows(name)
        for group in (bands[:2], bands[2:14], bands[14:]):
            assert sorted(r for _l, _a, rows in group for r in rows) == list(range(gr.case(name).S))
            parts = [gr.reference(name, tuple(rows)) for _l, _a, rows in group]
            for out, scale in (("pts", whole.pts_A), ("pts_A", whole.pts_A), ("feat", whole.feat_A), ("feat_A", whole.feat_A)):
                total = sum(getattr(p, out) for p in parts)
                assert (np.abs(total - getattr(whole, out)) <= 1e-13 * scale).all(), (name, out)      # (the sums cancel)
            assert np.array_equal(sum(p.pairs for p in parts), whole.pairs)


def test_long_bands_add_up_and_every_band_drops_and_keeps_visible_points():
    """`long` in two contiguous bands (0, 104, 256) and the tile-row-cyclic partition of 4: the band references add up to the
    whole image, and the band filter of the long-list path has something to do on every band -- visible points that no filter
    may drop (the centre of an owned row lies within max(rs, ry) of them) and visible points that every conservative filter
    of the kind drops (no owned row within max(rs, ry) + 3 pixels: the filter's slack is a pixel or two)."""
    c, whole = gr.case("long"), gr.reference("long")
    bands = gr.band_rows("long")
    assert c.P > 262144 and int(c.vis.sum()) < 5000 and len(bands) == 6
    vis = c.vis.astype(bool)
    cloud = np.searchsorted(c.first, np.arange(c.P), side="right") - 1
    reach = np.maximum(whole.rs[cloud], c.radii[:, 1])[vis].astype(np.float64)
    py = c.pts[vis, 1].astype(np.float64)
    for group in (bands[:2], bands[2:]):
        assert sorted(r for _l, _a, rows in group for r in rows) == list(range(c.S))
        parts = [gr.reference("long", tuple(rows)) for _l, _a, rows in group]
        for out, scale in (("pts", whole.pts_A), ("pts_A", whole.pts_A), ("feat", whole.feat_A), ("feat_A", whole.feat_A)):
            total = sum(getattr(p, out) for p in parts)
            assert (np.abs(total - getattr(whole, out)) <= 1e-13 * scale).all(), out
        assert np.array_equal(sum(p.pairs for p in parts), whole.pairs)
        for label, _arg, rows in group:
            centres = gr.pix_to_ndc(c.S - 1 - np.asarray(rows), c.S).astype(np.float64)
            nearest = np.abs(py[:, None] - centres[None]).min(1)
            must_keep, must_drop = int((nearest <= reach).sum()), int((nearest > reach + 6.0 / c.S).sum())
            print("long %-16s of %d visible points: %d must be kept, %d are dropped by any such filter" % (label, py.size, must_keep, must_drop))
            assert must_keep > 0 and must_drop > 0, label


@pytest.mark.parametrize("mut,name", [(m, n) for m, (_out, names) in gr.MUTATIONS.items() for n in names])
def test_wrong_formulas_lie_ten_times_beyond_the_bar(mut, name):
    out = gr.MUTATIONS[mut][0]
    c = gr.case(name)
    use_wsum = out != "feat_nowsum"
    ref, bad = gr.reference(name, use_wsum=use_wsum), gr.reference_of(c, mut=mut, use_wsum=use_wsum)
    got, want, A = (bad.pts, ref.pts, ref.pts_A) if out == "pts" else (bad.feat, ref.feat, ref.feat_A)
    v = gr.violation(got, want, A, gr.BARS[name][out])
    print("%s on %s: %.3g x the bar" % (mut, name, v))
    assert v >= 10, (mut, name, v)
