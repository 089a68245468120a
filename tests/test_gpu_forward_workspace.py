"""GPU: what `dss_render_forward` keeps in its workspace from one call to the next, on every spill path.

Under DSS_WS_CLEAN the call skips the counter memset and trusts that every counter, flag and queue slot of the zero region is
reset by its one owning workgroup after its last read (include/dss_hip.h).  A word left dirty does not show in the call that
leaves it; it corrupts the next one.  This module is the gate for that state.  Everything is compared bit for bit: there is no
tolerance in this file.

References.  Fragments (idx, zbuf, qvalue, occupancy): `oracle.splat_forward` on the CPU, fed the per-point arrays of
`ops.point_setup` -- which every call under test must return bit for bit (under DSS_WS_BAND_OUTPUTS: position, radii, validity
everywhere, ellipse / scaler / cutoff where the prover's rectangle reaches the band), so the oracle sees what the call
returned.  Bands are compared with the oracle's rows of the whole image, `visible` with the ids present in the compared
fragments, `image` / `wsum` with the bits of `ops.blend_forward` on the returned fragments.  The cell-ordered case uses
`ops.splat_points(bin_size=0)`, the whole-cloud scan without any workspace, on the per-point arrays of a workspace_state = 0 call.

Matrix (classes of tests/forward_workspace.py; scenes proven on the CPU by tests/test_forward_workspace_cpu.py and again here
from the call's own outputs):
  1 zero region after each of three DSS_WS_CLEAN calls   a b c d e1 e2 e3  x  S128-N1, S128-N16 (4,096 tiles: prio), S128-N17
                                                         (4,352 tiles: not prio), S100-N4 (fill_tile_rows); N > 2: ragged
                                                         clouds, one empty, one all culled, points of no cloud
  2 sequences on one clean buffer, S128-N1               A -> X -> A for every X != A (all ordered pairs of a..e2); per class:
                                                         whole image, band, cyclic band, band outputs only, no zbuf,
                                                         K = 12, C = 5 (no records), lean on -> off -> on (e3)
  3 arbitrary contents, a c d e2                         DSS_WS_UNKNOWN on 0xFF / random bytes; DSS_WS_CLEAN with such bytes
                                                         behind the zero region
  4 the path taken, a..e3                                after DSS_WS_UNKNOWN: counts == the prover's, cursor / offset on exactly
                                                         the over-full sub-lists (b c d), fail[0] == fail[1] iff e2 / e3, tails
  5 DSS_WS_BINNED after state 0                          a c e1
  6 ops.render_forward and the fused renderer            every class; renderer: a, d, a on its cached clean buffer
  7 cell-ordered binning, 2,000,101 points, N = 3        small splats / a few hundred wide ones; save, reuse, reuse with the
                                                         cluster moved, plain call on one clean buffer

What the scenes reached (S128-N1, cap 64, pool 65,536, 1,024 giant records per segment): b 24 over-full sub-lists of small
splats; c 113 of 5 x 5-tile splats; d 486 of 9 x 9-tile splats, 80..416 records per segment; e1 pool demand 80,948; e2 between
1,144 and 1,400 records in segment 0; e3 150 over-full sub-lists at cap 32.

Observed on the MI355X: all 83 cases pass on the library as it is -- no word of the zero region was found dirty on any path,
no output bit differed; the module takes ~5 s, the slowest case (the first, which compiles the prover) 0.7 s, the 2M-point
cases 0.7 s and 0.1 s.  At 2,000,101 points cap is 8,192; the two loaded tiles hold ~103,000 splats each, more than
8 cap, so sub-lists of both end above cap whatever the order dealt them.  The cell-ordered reference was `ops.splat_points(bin_size=0)` (well under a second).

Side builds (development copies of the library loaded through DSS_HIP_LIBRARY, one reset removed each; none is kept):
  (i)   fine_tile does not reset cursor / offset: test 1 fails for b c d e1 e2 at every shape ("cursor[32] = 286" after the
        first call) and passes for a and e3, where the words are never written (lean mode has no mask for the wide splats, so
        the pool pass moves nothing); tests 2, 3 (clean state), 6 and 7 fail, 4 and 5 (DSS_WS_UNKNOWN) pass.
  (ii)  the pool pass's last workgroup resets ctrl[0] only: test 1 fails for b c d e1 e2 ("ctrl[1] = 1264"), passes for a;
        tests 2, 3 (clean state), 4 ("ctrl [0 1264 0 ...]"), 6 (d, renderer) and 7 fail.
  (iii) the fill workgroups do not reset queue.flag: every class fails test 1, a included (every occupied tile raises its
        flag: "flag[38] = 1"), and so do tests 2, 3 (clean state), 6 and 7.
  (iv)  spill_begin does not copy fail[2] to fail[3]: the first spilling call on a buffer is fine, the second one's last
        pool workgroup no longer recognises itself: test 1 fails for b..e3 at call 1 ("ctrl[0] = 1", "cursor[200] = 32"),
        passes for a; tests 2 and 6 (renderer) fail.  Tests 3 and 7 were not run with it: its tiles read the pool before the
        pool pass wrote it, which on a buffer of arbitrary bytes means arbitrary point ids.
  test_render_forward_leaves_its_workspace_clean[40.0] (tests/test_gpu_setup.py) fails with all four as well, [1.0] only with
  (iii): that test already guards the resets on ITS scene; what it cannot say is which word, on which path, and it has no
  case for the pool running out, the giant records, lean mode, bands, N above 4,096 tiles, arbitrary bytes or 2M points.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref_loop"))
import forward_workspace as fw  # noqa: E402
import oracle  # noqa: E402
from dss_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FRAGS = ("idx", "zbuf", "qvalue", "occupancy")
SIX = ("pts_screen", "radii", "valid", "ellipse_params", "scaler", "cutoff_threshold")
UNKNOWN, CLEAN, BINNED = 0, 1, 2
A_TO_E2 = fw.CLASSES[:6]

_tensors, _refs, _feat5 = {}, {}, {}


def _t(s):
    if id(s) not in _tensors:
        _tensors[id(s)] = s.tensors(DEV)
    return _tensors[id(s)]


def _ref(s, K=5):
    """per-point bits of ops.point_setup (stateless, pinned by test_gpu_setup_reference.py) and the oracle's fragments for them;
    computed once per (scene, K) and never modified"""
    key = (id(s), K)
    if key not in _refs:
        t = _t(s)
        ps = ops.point_setup(t["world"], t["normals"], t["h"], t["M"], t["V"], t["znear"], t["zfar"], t["first"], t["num"], s.S,
                             fw.CUTOFF, fw.SIGMA, False, False)
        c = lambda k: ps[k].cpu().numpy()
        idx, zbuf, qv, occ = oracle.splat_forward(c("pts_screen"), c("ellipse_params"), c("cutoff_threshold"), c("radii"), s.first,
                                                  s.num, s.S, K, fw.THR)
        g = lambda a: torch.from_numpy(a).to(DEV)
        _refs[key] = dict(ps=ps, idx=g(idx), zbuf=g(zbuf), qvalue=g(qv), occupancy=g(occ))
    return _refs[key]


def _prove(s, o, rows=None, lean=False):
    c = lambda k: o[k].cpu().numpy()
    return fw.prove(c("pts_screen"), c("radii"), c("valid"), s.first, s.num, s.S, rows=rows, lean=lean)


class lean_mode:
    def __init__(self, on):
        self.on = int(bool(on))

    def __enter__(self):
        self.old = _lib.set_option(_lib.OPT_LEAN_WORKSPACE, self.on)

    def __exit__(self, *a):
        _lib.set_option(_lib.OPT_LEAN_WORKSPACE, self.old)
        return False


def _new_ws(s, fill=None, seed=0):
    n = fw.workspace_bytes(s.N, s.P, s.S)        # (the non-lean size: the lean layout is shorter)
    if fill is None:
        return torch.zeros(n, dtype=torch.uint8, device=DEV)
    if fill == "ff":
        return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def _check(s, o, what, K=5, rows=None, feat=None, band_only=False, want_zbuf=True):
    """the outputs of one call against the references"""
    ref, t = _ref(s, K), _t(s)
    feat = t["feat"] if feat is None else feat
    _, ri = fw.band(rows, s.S)
    ri = torch.tensor(ri, device=DEV)
    ps = ref["ps"]
    for k in SIX[:3]:
        assert torch.equal(o[k], ps[k]), (what, k)
    if band_only:
        reach = torch.from_numpy(_prove(s, ps, rows).rect[:, 0] >= 0).to(DEV)
        assert bool(reach.any()) and not bool(reach.all()), what
        for k in SIX[3:]:
            assert torch.equal(o[k][reach], ps[k][reach]), (what, k)
    else:
        for k in SIX[3:]:
            assert torch.equal(o[k], ps[k]), (what, k)
    for k in FRAGS:
        if k == "zbuf" and not want_zbuf:
            assert o[k] is None
            continue
        want = ref[k].index_select(1, ri)
        if not torch.equal(o[k], want):
            bad = (o[k] != want).nonzero()
            raise AssertionError("%s: %s differs from the oracle at %d entries, first %s" % (what, k, bad.shape[0], bad[0].tolist()))
    vis = torch.zeros(s.P, dtype=torch.bool, device=DEV)
    ids = o["idx"][o["idx"] >= 0].long()
    vis[ids] = True
    assert torch.equal(o["visible"], vis), (what, "visible")
    image, wsum = ops.blend_forward(o["idx"], o["qvalue"], o["occupancy"], o["scaler"], feat, return_wsum=True)
    assert torch.equal(o["image"], image) and torch.equal(o["wsum"], wsum), (what, "image / wsum")


def _zeros(lay, ws, what):
    torch.cuda.synchronize()
    dirty = lay.first_dirty(ws)
    assert dirty is None, "%s: zero region dirty at %s" % (what, dirty)


def _call(s, ws, state, what, lay=None, lean=False, **kw):
    """one call + its references (+ the zero region when `lay` is given)"""
    with lean_mode(lean):
        o = fw.render(_t(s), s.S, ws, state, **kw)
    _check(s, o, what, **{k: v for k, v in kw.items() if k in ("K", "rows", "feat", "want_zbuf")},
           band_only=kw.get("band_outputs_only", False))
    if lay is not None:
        _zeros(lay, ws, what)
    return o


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(fw.SHAPES))
@pytest.mark.parametrize("cls", fw.CLASSES)
def test_zero_region_is_zero_after_every_clean_call(cls, shape):
    s, lean = fw.scene(cls, shape), cls == "e3"
    lay = fw.layout(s.N, s.P, s.S, lean, with_records=True)
    assert lay.clean_bytes == _lib.load().dss_splat_forward_clean_bytes(s.N, s.P, s.S)
    assert (s.N * lay.tiles_x * lay.tiles_y <= 4096) == (shape != "S128-N17")           # `prio` of attach_workspace
    ws = _new_ws(s)
    for rep in range(3):
        o = _call(s, ws, CLEAN, "%s %s call %d" % (cls, shape, rep), lay, lean)
    print(fw.check_minimum(_prove(s, o, lean=lean), cls, shape))        # the class, from the call's own outputs


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", A_TO_E2)
def test_sequences_of_classes_on_one_clean_buffer(first):
    """A -> X -> A -> Y -> A ...: with the six parametrised cases every ordered pair of different classes a..e2"""
    sa = fw.scene(first)
    lay, ws = fw.layout(sa.N, sa.P, sa.S, with_records=True), _new_ws(sa)
    _call(sa, ws, CLEAN, first, lay)
    for other in A_TO_E2:
        if other == first:
            continue
        so = fw.scene(other)
        assert (so.N, so.P, so.S) == (sa.N, sa.P, sa.S)
        _call(so, ws, CLEAN, "%s -> %s" % (first, other), lay)
        _call(sa, ws, CLEAN, "%s -> %s" % (other, first), lay)


def _variants(s):
    from dss_amd.distributed import RowPartition
    if id(s) not in _feat5:
        _feat5[id(s)] = torch.rand((s.P, 5), device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    cyc = RowPartition(s.S, 4, 1, cyclic=True).rows
    return [("whole", {}), ("band", dict(rows=(24, 104))), ("cyclic band", dict(rows=cyc)),
            ("band, band outputs only", dict(rows=(24, 104), band_outputs_only=True)), ("whole", {}),
            ("cyclic band, band outputs only", dict(rows=cyc, band_outputs_only=True)), ("no zbuf", dict(want_zbuf=False)),
            ("K = 12", dict(K=12)), ("K = 5, C = 3", {}), ("K = 5, C = 5", dict(feat=_feat5[id(s)])), ("band", dict(rows=(40, 128))),
            ("whole", {}), ("lean", dict(lean=True)), ("not lean", {}), ("lean band", dict(lean=True, rows=(24, 104))),
            ("lean", dict(lean=True)), ("not lean", {})]


@pytest.mark.parametrize("cls", A_TO_E2)
def test_bands_options_and_lean_interleaved_on_one_clean_buffer(cls):
    """what ops.render_forward does on one cached buffer (its tag is (N, P, S) alone): whole image, contiguous and
    tile-row-cyclic bands, DSS_WS_BAND_OUTPUTS, no depth plane, K = 12, C = 5 (no packed records) and
    DSS_OPT_LEAN_WORKSPACE on -> off -> on (scene c under lean is class e3) in one sequence of DSS_WS_CLEAN calls"""
    s = fw.scene(cls)
    lay, ws = fw.layout(s.N, s.P, s.S, with_records=True), _new_ws(s)
    for i, (name, kw) in enumerate(_variants(s)):
        kw = dict(kw)
        _call(s, ws, CLEAN, "%s, call %d: %s" % (cls, i, name), lay, kw.pop("lean", False), **kw)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["ff", "random"])
@pytest.mark.parametrize("cls", ["a", "c", "d", "e2"])
def test_unknown_state_on_arbitrary_bytes(cls, fill):
    """DSS_WS_UNKNOWN, "contents arbitrary": lists, pool, big and giant are read only where this call wrote them, and
    fail[0..3] work from any initial value"""
    s = fw.scene(cls)
    ws = _new_ws(s, fill, seed=11)
    _call(s, ws, UNKNOWN, "%s on %s bytes" % (cls, fill))
    _call(fw.scene("c" if cls != "c" else "d"), ws, UNKNOWN, "other class after %s on %s bytes" % (cls, fill))
    _call(s, ws, UNKNOWN, "%s on %s bytes, again" % (cls, fill))


@pytest.mark.parametrize("fill", ["ff", "random"])
@pytest.mark.parametrize("cls", ["a", "c", "d", "e2"])
def test_clean_state_with_arbitrary_bytes_behind_the_zero_region(cls, fill):
    s = fw.scene(cls)
    lay = fw.layout(s.N, s.P, s.S, with_records=True)
    ws = _new_ws(s, fill, seed=12)
    ws[: lay.clean_bytes] = 0
    for rep in range(2):
        _call(s, ws, CLEAN, "%s, %s bytes behind the zero region, call %d" % (cls, fill, rep), lay)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["S128-N1", "S100-N4"])
@pytest.mark.parametrize("cls", fw.CLASSES)
def test_unknown_state_leaves_the_evidence_of_its_path(cls, shape):
    """after DSS_WS_UNKNOWN nothing of the zero region is reset but ctrl and mask (the pool pass inside the fine launch)"""
    s, lean = fw.scene(cls, shape), cls == "e3"
    lay, ws = fw.layout(s.N, s.P, s.S, lean, with_records=True), _new_ws(s)
    o = _call(s, ws, UNKNOWN, "%s %s" % (cls, shape), lean=lean)
    torch.cuda.synchronize()
    pr = _prove(s, o, lean=lean)
    counts = lay.words(ws, "counts")
    want = pr.counts.reshape(-1).astype(np.int64)
    assert counts.shape == want.shape and np.array_equal(counts, want), "counts: %d sub-lists differ" % int((counts != want).sum())
    over = want > lay.cap
    assert int(over.sum()) == pr.n_over and (pr.n_over > 0) == (cls != "a")
    cursor, offset = lay.words(ws, "cursor"), lay.words(ws, "offset")
    assert not cursor[~over].any() and not offset[~over].any()
    if cls in ("b", "c", "d"):
        assert np.array_equal(cursor[over], want[over] - lay.cap) and offset[over].all()
        # the pool ranges of the over-full sub-lists are disjoint and fill [0, demand)
        lo = np.sort(offset[over] - 1)
        assert lo[0] == 0 and int((want[over] - lay.cap).sum()) == pr.pool_demand
        assert len(np.unique(lo)) == len(lo) and lo[-1] < pr.pool_demand
    fail = lay.words(ws, "fail", 4)
    assert (fail[0] == fail[1]) == (cls in ("e2", "e3")), fail
    tc = lay.words(ws, "tail+ctrl", 42)
    assert int(tc[:32].sum()) == pr.occupied_tiles and int(tc[:32].max()) <= lay.capq
    assert not tc[32:].any(), "ctrl %s" % tc[32:]
    flag = lay.words(ws, "flag")
    assert int(flag.sum()) == pr.occupied_tiles and set(np.unique(flag)) <= {0, 1}
    off, n = lay.regions["mask"]
    assert int(ws[off: off + n].count_nonzero()) == 0


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["a", "c", "e1"])
def test_binned_state_repeats_the_fine_pass(cls):
    s = fw.scene(cls)
    ws = _new_ws(s)
    first = _call(s, ws, UNKNOWN, cls)
    for rep in range(2):
        again = fw.render(_t(s), s.S, ws, BINNED, per_point=first)
        for k in FRAGS + ("image", "wsum", "visible"):
            assert torch.equal(again[k], first[k]), (cls, rep, k)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", fw.CLASSES)
def test_ops_render_forward_gives_the_wrapper_bits(cls):
    s, lean, t = fw.scene(cls), cls == "e3", _t(fw.scene(cls))
    mine = _call(s, _new_ws(s), CLEAN, cls, lean=lean)
    with lean_mode(lean):
        for rep in range(2):
            o = ops.render_forward(t["world"], t["normals"], t["h"], t["M"], t["V"], t["znear"], t["zfar"], t["first"], t["num"], t["feat"],
                                   s.S, 5, fw.CUTOFF, fw.THR, fw.SIGMA, False, False)
            for k in SIX + FRAGS + ("image", "wsum", "visible"):
                assert torch.equal(o[k], mine[k]), (cls, rep, k)


def _renderer():
    from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
    from dss_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting
    from dss_amd.renderer import NormWeightedCompositor, SurfaceSplattingRenderer
    R, T = look_at_view_transform(2.0, 0.0, 0.0)
    cams = FoVPerspectiveCameras(znear=fw.ZNEAR, zfar=fw.ZFAR, R=R, T=T, device=DEV)
    settings = PointsRasterizationSettings(backface_culling=False, cutoff_threshold=fw.CUTOFF, Vrk_invariant=True, radii_backward_scaler=5,
                                           image_size=128, points_per_pixel=5, bin_size=None, clip_pts_grad=0.05)
    return SurfaceSplattingRenderer(SurfaceSplatting(cameras=cams, raster_settings=settings), NormWeightedCompositor(), fused=True)


def test_fused_renderer_through_classes_a_d_a():
    """one renderer, three clouds of the same size (class a, class d, class a): the images of three fresh renderers, and the
    zero region of the renderer's cached clean workspace is zero after each"""
    from dss_amd.cloud import PointClouds3D
    seq = [fw.scene("a"), fw.scene("d"), fw.scene("a")]
    lay = fw.layout(1, seq[0].P, 128, with_records=True)
    tag = ("render_forward", 1, seq[0].P, 128)

    def draw(renderer, s):
        t = _t(s)
        cloud = PointClouds3D([t["world"]], [t["normals"]], [t["feat"]])
        with torch.no_grad():
            return renderer(cloud, Vrk_h=t["h"]).clone()
    fresh = [draw(_renderer(), s) for s in seq]
    assert not torch.equal(fresh[0], fresh[1]) and torch.equal(fresh[0], fresh[2])
    for s, want in zip(seq, fresh):      # the renderer's image is the wrapper's (same M, V: the scene's camera)
        o = _call(s, _new_ws(s), CLEAN, "renderer scene " + s.cls)
        assert torch.equal(want, o["image"]), s.cls
    one = _renderer()
    for i, (s, want) in enumerate(zip(seq, fresh)):
        got = draw(one, s)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (i, s.cls)
        bufs = [b for k, b in _lib._clean_cache.items() if k[2] == tag]
        assert len(bufs) == 1
        _zeros(lay, bufs[0], "renderer call %d (%s)" % (i, s.cls))


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def _big_case(wide):
    """the 2,000,101-point, three-cloud input of test_gpu_setup_reference._big_inputs with 200,000 points of cloud 0 moved next
    to two of its own visible points (two tiles), per-point h; wide: 400 of the moved points get a pixel radius of ~12 / ~40"""
    import test_gpu_setup_reference as big
    import setup_reference as sr
    (world, normals, h, M, V, zn, zf, first, num), feat, backface = big._big_inputs()
    P, S = world.shape[0], big.BIG_S
    hp = h[torch.repeat_interleave(torch.arange(3, device=DEV), num)].contiguous()
    base = ops.point_setup(world, normals, hp, M, V, zn, zf, first, num, S, sr.CUTOFF, sr.SIGMA, backface, False)
    f1, n1 = int(first[0]), int(num[0])      # cloud 0: ~10 x 10 tiles on screen
    ps, ok = base["pts_screen"][f1:f1 + n1], base["valid"][f1:f1 + n1]
    col, row = (1.0 - ps[:, 0]) * 0.5 * S, (1.0 - ps[:, 1]) * 0.5 * S
    # four anchors: visible points of that cloud near the centre of four tiles that lie at least three tiles apart
    inner = lambda v: ((v % 8) > 3.0) & ((v % 8) < 5.0) & (v > 8) & (v < S - 8)
    cand = (ok & inner(col) & inner(row)).nonzero()[:20000, 0].cpu().numpy()
    tcol, trow = (col[cand] / 8).long().cpu().numpy(), (row[cand] / 8).long().cpu().numpy()
    picked = []
    for i in range(len(cand)):
        if all(max(abs(int(tcol[i]) - int(tcol[j])), abs(int(trow[i]) - int(trow[j]))) >= 3 for j in picked):
            picked.append(i)
            if len(picked) == 4:
                break
    assert len(picked) == 4
    anchors = {name: f1 + int(cand[i]) for name, i in zip("abcd", picked)}
    moved = torch.arange(f1 + 1000, f1 + 201_000, device=DEV)
    r_px = float(base["radii"][anchors["a"], 0]) * S / 2
    assert r_px > 1.0
    grow = lambda target: float(hp[anchors["a"]]) * (target * target - 1.0) / max(r_px * r_px - 1.0, 1e-6)

    def place(pair):
        w, nr, hh = world.clone(), normals.clone(), hp.clone()
        half = moved.shape[0] // 2
        for part, key in ((moved[:half], pair[0]), (moved[half:], pair[1])):
            jit = (torch.rand((part.shape[0], 3), device=DEV, generator=torch.Generator(DEV).manual_seed(9)) - 0.5) * 2e-4
            w[part], nr[part], hh[part] = w[anchors[key]].clone() + jit, nr[anchors[key]].clone(), float(hh[anchors[key]])
        if wide:
            hh[moved[:200]], hh[moved[200:400]] = grow(12.0), grow(40.0)
        return [w, nr, hh, M, V, zn, zf, first, num]
    return place(("a", "b")), place(("c", "d")), feat, backface, S, sr


@pytest.mark.parametrize("wide", [False, True], ids=["small splats", "wide splats"])
def test_cell_ordered_binning_keeps_the_workspace_clean(wide):
    """above 2,000,000 points the binning runs in cell order (bin_sorted_kernel: sub-lists by position, spills recorded "the same
    way", spill_sorted = 1): save the order, reuse it, reuse it with the cluster moved to other tiles, plain call -- on one
    clean buffer.  Reference: the whole-cloud scan (ops.splat_points, bin_size = 0) on the per-point arrays of a state-0 call."""
    here, there, feat, backface, S, sr = _big_case(wide)
    N, P, K = 3, here[0].shape[0], 5
    lay = fw.layout(N, P, S, with_records=True)
    assert "sort_id" in lay.regions and lay.total == fw.workspace_bytes(N, P, S)
    first, num = here[7].cpu().numpy(), here[8].cpu().numpy()

    def run(args, ws, state):
        t = dict(zip(("world", "normals", "h", "M", "V", "znear", "zfar", "first", "num"), args), feat=feat)
        return fw.render(t, S, ws, state, K=K, backface=backface)
    refs = {}
    scratch = torch.zeros(lay.total, dtype=torch.uint8, device=DEV)
    for name, args in (("here", here), ("there", there)):
        o = run(args, scratch, UNKNOWN)
        torch.cuda.synchronize()
        pr = _prove(type("S", (), dict(first=first, num=num, S=S)), o)
        counts = lay.words(scratch, "counts").reshape(-1, 8)
        assert np.array_equal(counts.sum(1), pr.counts.reshape(-1, 8).sum(1).astype(np.int64))        # per tile: the sub-list is by position
        assert int((pr.counts.reshape(-1, 8).sum(1) > 8 * lay.cap).sum()) >= 2                         # two tiles above 8 cap for certain
        n_over = int((counts > lay.cap).sum())
        assert n_over >= 2, n_over
        if wide:
            over_tile = (counts > lay.cap).any(1)
            by = pr.by_width.reshape(3, -1, 8).sum(2)
            assert int(by[1][over_tile].sum()) >= 100 and int(by[2][over_tile].sum()) >= 100           # up to 8 x 8 tiles / wider
        idx, zbuf, qv, occ, vis = ops.splat_points(o["pts_screen"], o["ellipse_params"], o["cutoff_threshold"], o["radii"], args[7],
                                                   args[8], fw.THR, S, K, 0, None, return_visible=True)
        for k, want in zip(FRAGS + ("visible",), (idx, zbuf, qv, occ, vis)):
            assert torch.equal(o[k], want), (name, "state 0", k)
        refs[name] = o
        print(name, "cap", lay.cap, "over-full sub-lists", n_over, "tiles", int((counts > lay.cap).any(1).sum()))
    del scratch
    ws = torch.zeros(lay.total, dtype=torch.uint8, device=DEV)
    for what, name, args, state in (("save", "here", here, CLEAN | _lib.WS_ORDER_SAVE), ("reuse", "here", here, CLEAN | _lib.WS_ORDER_REUSE),
                                    ("reuse, cluster moved", "there", there, CLEAN | _lib.WS_ORDER_REUSE), ("plain", "here", here, CLEAN)):
        o = run(args, ws, state)
        for k in SIX + FRAGS + ("image", "wsum", "visible"):
            assert torch.equal(o[k], refs[name][k]), (what, k)
        _zeros(lay, ws, what)
