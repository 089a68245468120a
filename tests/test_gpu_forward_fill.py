"""GPU: the constants `dss_render_forward` writes for the tiles that no splat reaches, in every form of DSS_OPT_FORWARD_FILL.

The fine launch's first workgroups ("fill workgroups", 32 tiles each) write idx = -1, zbuf = -1, qvalue = -1, occupancy = 0,
wsum = 1e-4 and RGBA = 0 for every tile whose flag binning did not raise: in aligned 16-byte pieces (`fill_tiles`, plain stores
with the option at 0, write-through stores at 1) or, where a piece would not be aligned (S % 8 != 0, C != 3, a pointer or an image
stride off a 16-byte boundary), row by row with 4-byte stores (`fill_tile_rows`, always plain).  The option changes the cache
policy of stores, never a value or an address, so every case runs once per form and everything is compared bit for bit: there is no
tolerance in this file.

Every output tensor of every call is 0xFF bytes before the call (idx = -1 is 0xFFFFFFFF too, which is why the float planes, whose
constants have other bits, are all checked): a tile that nobody wrote, or that kept an earlier call's contents, shows.

References, per call: fragments (idx, zbuf, qvalue, occupancy) = `oracle.splat_forward` on the per-point arrays the scene's first
call returned (every later call of the scene must return the same bits), the band's rows taken from the whole image; image / wsum
= `ops.blend_forward` on the returned fragments; and, stated on its own, every pixel of a tile that no splat's tile rectangle
(tile_rect.h through `forward_workspace.prove`) meets holds exactly the six constants.

Cases (the smallest shapes at which the fill can go wrong; each well under a second):
  S = 64, N = 1          64 tiles = two groups of 32; the grid is rounded up to 8 fill workgroups, six of them past the last tile.
                         "empty group": tile rows 0-3 hold nothing; "full group": every tile of rows 0-3 is occupied and rows 4-7
                         hold nothing; "mixed": both groups hold both kinds
  S = 72, N = 3          81 tiles per camera: groups straddle the cameras, the last group has 19 tiles; cloud 1 is empty
  bands                  rows 8..45 (five tile rows, the last with five valid rows); tile-row-cyclic band (every second tile row)
  strided image          (row, camera, column, channel) buffer handed over with its camera / row strides, N = 3
  K = 1, 8 / K = 12      2 K pieces per tile row / the kernel without packed records; no zbuf: the depth plane is not written
  fallbacks              S = 100, C = 5, qvalue 4 bytes past a 16-byte boundary: fill_tile_rows, plain in every form
  workspace states       one buffer: DSS_WS_UNKNOWN, then (zero region zeroed: DSS_WS_UNKNOWN does not restore it, and DSS_WS_CLEAN
                         is only defined on a zero region) DSS_WS_CLEAN with the splats moved to the other half of the image,
                         DSS_WS_CLEAN with them moved back -- the zero region is zero after each, by the check of
                         test_gpu_forward_workspace --, then DSS_WS_UNKNOWN and DSS_WS_BINNED (defined only behind a
                         DSS_WS_UNKNOWN call with the same inputs) into fresh 0xFF outputs: the re-run fills the empty tiles itself

Observed on the MI355X: all 35 cases pass, the module takes under 3 s (the first case compiles the prover: 0.6 s).
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
from test_gpu_forward_workspace import _zeros  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FORMS = (0, 1)      # DSS_OPT_FORWARD_FILL: plain / write-through
UNKNOWN, CLEAN, BINNED = 0, 1, 2
PER_POINT = ("pts_screen", "ellipse_params", "radii", "scaler", "cutoff_threshold")
FRAGS = ("idx", "zbuf", "qvalue", "occupancy")
WSUM_BITS = int(np.float32(1e-4).view(np.int32))
MINUS_ONE_BITS = int(np.float32(-1.0).view(np.int32))


class fill_form:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = _lib.set_option(_lib.OPT_FORWARD_FILL, self.form)

    def __exit__(self, *a):
        _lib.set_option(_lib.OPT_FORWARD_FILL, self.old)
        return False


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def _build(S, clouds, seed=0, C=3):
    """one cloud per entry of `clouds`: a list of pixel boxes (points, col0, col1, row0, row1) of 1-pixel splats that face the
    scene camera of forward_workspace (an empty list: an empty cloud)"""
    rng = np.random.default_rng(seed)
    M, V = fw._camera()
    J, a = fw._plane_map(M)
    Jinv = np.linalg.inv(J)
    world, normals, h, sizes = [], [], [], []
    for boxes in clouds:
        col = np.concatenate([rng.uniform(c0, c1, n) for n, c0, c1, r0, r1 in boxes] + [np.zeros(0)])
        row = np.concatenate([rng.uniform(r0, r1, n) for n, c0, c1, r0, r1 in boxes] + [np.zeros(0)])
        size = col.shape[0]
        ndc = np.stack([1.0 - 2.0 * col / S, 1.0 - 2.0 * row / S], 1)
        xy = ndc @ Jinv
        z = -0.05 * (xy ** 2).sum(1) + rng.uniform(-0.02, 0.02, size)
        world.append(np.concatenate([xy, z[:, None]], 1))
        nr = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.05, 0.05, (size, 3))
        normals.append(nr / np.linalg.norm(nr, axis=1, keepdims=True))
        h.append(fw.h_for_radius(rng.uniform(0.8, 1.6, size), S, a))
        sizes.append(size)
    s = fw.Scene()
    s.N, s.S = len(clouds), S
    s.world = np.concatenate(world).astype(np.float32)
    s.normals = np.concatenate(normals).astype(np.float32)
    s.h = np.concatenate(h).astype(np.float32)
    s.P = s.world.shape[0]
    s.num = np.asarray(sizes, np.int64)
    s.first = np.cumsum(s.num) - s.num
    s.M, s.V = np.tile(M, (s.N, 1, 1)).astype(np.float32), np.tile(V, (s.N, 1, 1)).astype(np.float32)
    s.znear, s.zfar = np.full(s.N, fw.ZNEAR, np.float32), np.full(s.N, fw.ZFAR, np.float32)
    s.feat = rng.uniform(0, 1, (s.P, C)).astype(np.float32)
    return s


_RECIPES = {
    # S = 64: tile rows 0-3 are fill group 0, tile rows 4-7 group 1
    "empty group": lambda: _build(64, [[(500, 10, 44, 42, 60)]]),
    "full group": lambda: _build(64, [[(3000, 0.5, 63.5, 0.5, 29.0)]]),
    "mixed": lambda: _build(64, [[(60, 3, 12, 3, 12), (60, 41, 52, 17, 22), (80, 20, 30, 34, 45), (40, 58, 62, 58, 62)]]),
    "moved": lambda: _build(64, [[(60, 35, 44, 35, 44), (60, 9, 20, 49, 54), (80, 36, 46, 2, 13), (40, 2, 6, 26, 30)]]),
    "three clouds": lambda: _build(72, [[(300, 5, 40, 5, 30), (100, 50, 70, 60, 70)], [], [(250, 30, 70, 20, 50)]]),
    "S100": lambda: _build(100, [[(300, 10, 60, 10, 50), (50, 90, 98, 90, 98)]]),
    "C5": lambda: _build(64, [[(60, 3, 12, 3, 12), (80, 20, 30, 34, 45)]], C=5),
}
_scenes, _tensors, _refs = {}, {}, {}


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _RECIPES[name]()
        _tensors[name] = _scenes[name].tensors(DEV)
    return _scenes[name], _tensors[name]


# ---- the call, into 0xFF outputs ---------------------------------------------------------------------------------------------
def _poison(*shape, dtype=torch.float32, skew=0):
    """a tensor of 0xFF bytes; skew: its first element lies that many elements past the allocation's 256-byte aligned start"""
    n = int(np.prod(shape)) + skew
    flat = torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=DEV).view(dtype)
    return flat[skew:].view(*shape)


def _render(name, ws, state, K=5, rows=None, want_zbuf=True, strided=False, skew=0, per_point=None):
    s, t = _scene(name)
    S, N, P, C = s.S, s.N, s.P, s.feat.shape[1]
    (row0, row1, cyc), ri = fw.band(rows, S)
    nr = len(ri)
    o = dict(pts_screen=_poison(P, 3), ellipse_params=_poison(P, 3), radii=_poison(P, 2), scaler=_poison(P), cutoff_threshold=_poison(P),
             idx=_poison(N, nr, S, K, dtype=torch.int32), zbuf=_poison(N, nr, S, K) if want_zbuf else None,
             qvalue=_poison(N, nr, S, K, skew=skew), occupancy=_poison(N, nr, S), wsum=_poison(N, nr, S))
    if strided:     # the multi-GPU send buffer: (row, camera, column, channel); the call sees its (camera, row, ...) view
        o["image"] = _poison(nr, N, S, C + 1).permute(1, 0, 2, 3)
        sn, sr = int(o["image"].stride(0)), int(o["image"].stride(1))
        assert (sn, sr) == (S * (C + 1), N * S * (C + 1))
    else:
        o["image"], sn, sr = _poison(N, nr, S, C + 1), 0, 0
    valid, vis = _poison(P, dtype=torch.uint8), _poison(P, dtype=torch.uint8)
    if per_point is not None:
        for k in PER_POINT:
            o[k] = per_point[k]
        valid, vis = per_point["valid"].view(torch.uint8), per_point["visible"].view(torch.uint8).clone()
    assert o["qvalue"].data_ptr() % 16 == (4 * skew) % 16
    _lib.call("dss_render_forward", DEV, t["world"], t["normals"], t["h"], None, None, None, t["M"], t["V"], t["znear"], t["zfar"],
              t["first"], t["num"], N, P, 0, 0, S, K, fw.CUTOFF, fw.SIGMA, fw.THR, row0, row1, cyc, t["feat"], C,
              o["pts_screen"], o["ellipse_params"], o["radii"], o["scaler"], o["cutoff_threshold"], valid, o["idx"], o["zbuf"],
              o["qvalue"], o["occupancy"], vis, o["image"], sn, sr, o["wsum"], ws, ws.numel(), int(state))
    o["valid"], o["visible"] = valid.view(torch.bool), vis.view(torch.bool)
    return o


def _ref(name, o, K, rows):
    """(oracle fragments of the whole image, pixel mask of the band's tiles that no splat rectangle meets, tile mask), from
    the per-point arrays of the scene's first call; computed once per (scene, K, band) and never modified"""
    s, _ = _scene(name)
    if name not in _refs:
        _refs[name] = dict(per_point={k: o[k].clone() for k in PER_POINT + ("valid",)})
    r = _refs[name]
    c = lambda k: r["per_point"][k].cpu().numpy()
    if ("frag", K) not in r:
        idx, zbuf, qv, occ = oracle.splat_forward(c("pts_screen"), c("ellipse_params"), c("cutoff_threshold"), c("radii"), s.first,
                                                  s.num, s.S, K, fw.THR)
        r[("frag", K)] = {k: torch.from_numpy(a).to(DEV) for k, a in zip(FRAGS, (idx, zbuf, qv, occ))}
    bkey = ("band", None if rows is None else tuple(int(x) for x in rows))
    if bkey not in r:
        pr = fw.prove(c("pts_screen"), c("radii"), c("valid"), s.first, s.num, s.S, rows=rows)
        _, ri = fw.band(rows, s.S)
        occupied = (pr.counts > 0).any(-1)                                              # (N, tiles_y, tiles_x)
        pix = np.repeat(np.repeat(~occupied, fw.TILE, 1), fw.TILE, 2)[:, :len(ri), :s.S]
        r[bkey] = (torch.from_numpy(np.ascontiguousarray(pix)).to(DEV), occupied)
    return r["per_point"], r[("frag", K)], r[bkey][0], r[bkey][1]


def _check(name, o, what, K=5, rows=None, want_zbuf=True, **_):
    s, t = _scene(name)
    per_point, frag, empty, occupied = _ref(name, o, K, rows)
    for k in PER_POINT + ("valid",):
        assert torch.equal(o[k], per_point[k]), (what, k)
    ri = torch.tensor(fw.band(rows, s.S)[1], device=DEV)
    for k in FRAGS:
        if k == "zbuf" and not want_zbuf:
            assert o[k] is None
            continue
        want = frag[k].index_select(1, ri)
        if not torch.equal(o[k], want):
            bad = (o[k] != want).nonzero()
            raise AssertionError("%s: %s differs from the oracle at %d entries, first %s" % (what, k, bad.shape[0], bad[0].tolist()))
    vis = torch.zeros(s.P, dtype=torch.bool, device=DEV)
    vis[o["idx"][o["idx"] >= 0].long()] = True
    assert torch.equal(o["visible"], vis), (what, "visible")
    image, wsum = ops.blend_forward(o["idx"], o["qvalue"], o["occupancy"], o["scaler"], t["feat"], return_wsum=True)
    assert torch.equal(o["image"], image) and torch.equal(o["wsum"], wsum), (what, "image / wsum")
    # the six constants, bit for bit, in every pixel of a tile that no splat rectangle meets
    assert bool(empty.any()), (what, "no empty tile")
    bits = lambda a: a[empty].contiguous().view(torch.int32)
    assert bool((o["idx"][empty] == -1).all()), (what, "idx of empty tiles")
    assert bool((bits(o["qvalue"]) == MINUS_ONE_BITS).all()), (what, "qvalue of empty tiles")
    if want_zbuf:
        assert bool((bits(o["zbuf"]) == MINUS_ONE_BITS).all()), (what, "zbuf of empty tiles")
    assert bool((bits(o["occupancy"]) == 0).all()), (what, "occupancy of empty tiles")
    assert bool((bits(o["wsum"]) == WSUM_BITS).all()), (what, "wsum of empty tiles")
    assert bool((bits(o["image"]) == 0).all()), (what, "image of empty tiles")
    return occupied


def _new_ws(name):
    s, _ = _scene(name)
    return torch.zeros(fw.workspace_bytes(s.N, s.P, s.S), dtype=torch.uint8, device=DEV)


# ---- cases -----------------------------------------------------------------------------------------------------------------
def _cyclic(S):
    from dss_amd.distributed import RowPartition
    return RowPartition(S, 2, 1, cyclic=True).rows


CASES = [
    ("empty group", {}), ("full group", {}), ("mixed", {}), ("three clouds", {}),
    ("mixed", dict(rows=(8, 45))), ("mixed", dict(rows="cyclic")), ("three clouds", dict(rows=(16, 61), strided=True)),
    ("three clouds", dict(strided=True)), ("mixed", dict(K=1)), ("mixed", dict(K=8)), ("mixed", dict(K=12)),
    ("mixed", dict(want_zbuf=False)), ("three clouds", dict(want_zbuf=False, K=8)),
    ("S100", {}), ("C5", {}), ("mixed", dict(skew=1)),
]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s %s" % (n, " ".join("%s=%s" % kv for kv in kw.items())) for n, kw in CASES])
def test_empty_tiles_hold_the_constants(case, form):
    name, kw = CASES[case]
    kw = dict(kw)
    s, _ = _scene(name)
    if kw.get("rows") == "cyclic":
        kw["rows"] = _cyclic(s.S)
    ws = _new_ws(name)
    what = "%s %s form %d" % (name, kw, form)
    with fill_form(form):
        assert _lib.load().dss_get_option(_lib.OPT_FORWARD_FILL) == form
        for state in (UNKNOWN, CLEAN):      # (a fresh buffer is clean as well; the second call runs without the memset)
            ws.zero_()
            o = _render(name, ws, state, **kw)
            occupied = _check(name, o, "%s state %d" % (what, state), **kw)
    # the scene is what the case says it is, from the call's own outputs
    tiles = occupied.reshape(-1)
    groups = [tiles[i:i + 32] for i in range(0, len(tiles), 32)]
    assert tiles.any() and not tiles.all(), what
    if name == "empty group":
        assert not groups[0].any() and groups[1].any() and not groups[1].all(), what
    if name == "full group":
        assert groups[0].all() and not groups[1].any(), what
    if name == "mixed" and "rows" not in kw:
        assert all(g.any() and not g.all() for g in groups) and len(groups) == 2, what
    if name == "three clouds" and "rows" not in kw:
        assert len(groups) == 8 and len(groups[-1]) == 19 and not occupied[1].any() and occupied[0].any() and occupied[2].any(), what
    if kw.get("rows") == (8, 45):
        assert occupied.shape[1] == 5 and occupied[:, -1].any() and not occupied[:, -1].all(), what   # the short tile row holds both kinds


@pytest.mark.parametrize("form", FORMS)
def test_workspace_states_on_one_buffer(form):
    a, b = "mixed", "moved"
    sa, sb = _scene(a)[0], _scene(b)[0]
    assert (sa.N, sa.P, sa.S) == (sb.N, sb.P, sb.S)
    lay, ws = fw.layout(sa.N, sa.P, sa.S, with_records=True), _new_ws(a)
    with fill_form(form):
        oa = _check(a, _render(a, ws, UNKNOWN), "unknown, form %d" % form)
        ws[: lay.clean_bytes] = 0
        for i, name in enumerate((b, a, b)):
            occ = _check(name, _render(name, ws, CLEAN), "clean call %d (%s), form %d" % (i, name, form))
            _zeros(lay, ws, "clean call %d (%s), form %d" % (i, name, form))
        ob = occ
        # tiles occupied in one call are empty in the next and the reverse
        assert (oa & ~ob).sum() >= 4 and (ob & ~oa).sum() >= 4
        first = _render(a, ws, UNKNOWN)
        _check(a, first, "unknown again, form %d" % form)
        again = _render(a, ws, BINNED, per_point=first)
        _check(a, again, "binned re-run into fresh outputs, form %d" % form)
        for k in FRAGS + ("image", "wsum", "visible"):
            assert torch.equal(again[k], first[k]), (form, k)


def test_option_values():
    lib = _lib.load()
    assert lib.dss_get_option(_lib.OPT_FORWARD_FILL) == 1       # the default: write-through
    assert lib.dss_set_option(_lib.OPT_FORWARD_FILL, 2) == -1 and b"DSS_OPT_FORWARD_FILL" in lib.dss_last_error()
    assert lib.dss_set_option(_lib.OPT_FORWARD_FILL, -1) == -1
    assert lib.dss_get_option(_lib.OPT_FORWARD_FILL) == 1
