"""TEST INFRASTRUCTURE: what `dss_render_forward` keeps in its workspace, seen from outside the library.

Four parts, used by tests/test_forward_workspace_cpu.py (no GPU) and tests/test_gpu_forward_workspace.py:

* `layout`      a plain-Python mirror of `carve_fwd` (dss_amd/csrc/raster_forward.hip): byte offset and length of every region,
                the zero region (DSS_WS_CLEAN) first and in the library's order, for both values of DSS_OPT_LEAN_WORKSPACE and
                with / without the fused forward's records.  The CPU test pins it to the library's three size queries.
* `render`      `dss_render_forward` through `_lib.call` on a caller-owned workspace with a caller-chosen workspace_state.
* `build_scene` world-space scenes for the fused entry (it does the setup itself): a gently curved patch that faces the
                camera, a per-point h that sets every splat's pixel radius, and a share of the points clustered on a few tiles.
* `prove`       from the per-point screen arrays of a call (or of the CPU oracle): every splat's tile rectangle by the rule of
                tile_rect.h (the header itself, compiled with the host compiler), the per-sub-list counts of the direct binning
                (sub-list = p & 7), and which classes of binning outcome the scene reaches for certain.

Classes (widest last): a no sub-list above cap | b overflow by splats of at most 2 x 2 tiles | c ... of up to 8 x 8 tiles
(`big`) | d ... wider than 8 x 8 tiles (`giant` records, sufficing) | e1 pool demand above the pool | e2 giant records of one
segment above giant_cap | e3 lean mode: a splat wider than 2 x 2 tiles meets a full sub-list.
WHICH splats of an over-full sub-list arrive late is decided by the order of the atomics, so a width is "certain" only by
pigeonhole: more than `cap` splats of that width in one sub-list.  The scenes are built so that certain == possible."""
import ctypes
import os
import subprocess
import tempfile
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, SUB, QUEUES, SB_SHIFT = 8, 8, 32, 2
SORT_MIN_P, SORT_SEG, CELL_SORT_THREADS, CELL_SORT_MAX, SORT_PER_THREAD = 2_000_000, 8, 1024, 16384, 16
CLASSES = ("a", "b", "c", "d", "e1", "e2", "e3")


# ---------------------------------------------------------------------------------------------------------------------
# layout mirror
# ---------------------------------------------------------------------------------------------------------------------
def bin_capacity(N, P, S, lean=False):
    t = (S + TILE - 1) // TILE
    mean_sub = 2.0 * (float(P) / max(N, 1)) / (float(t * t) * SUB)
    cap = 32 if lean else 64
    while cap < 16384 and float(cap) < (2.0 if lean else 8.0) * mean_sub:
        cap <<= 1
    return cap


def spill_capacity(P, lean=False):
    c = max((2 if lean else 8) * P, 65536)
    return min(c, 0x7fffff00)


def giant_cap(P):
    return max(P // 16, 1024)


def queue_capacity(N, tiles_x, tiles_y):
    sb = lambda t: (t + (1 << SB_SHIFT) - 1) >> SB_SHIFT
    return ((sb(tiles_x) + 7) // 8) * sb(tiles_y) * N * ((1 << SB_SHIFT) * (1 << SB_SHIFT) // 4)


def _cell_total(N, S, extra):
    shift = 5
    while True:
        cx = ((S - 1) >> shift) + 1
        total = N * cx * cx + extra
        if total <= CELL_SORT_MAX or shift >= 14:
            return total
        shift += 1


def _sort_blocks(P):
    per = min(max(P // (CELL_SORT_THREADS * 512), 1), SORT_PER_THREAD)
    chunk = CELL_SORT_THREADS * per
    return (P + chunk - 1) // chunk


class Layout:
    """regions: name -> (byte offset, byte length as requested); every region starts on a 256-byte boundary (`Bump`)"""

    def __init__(self, N, P, S, lean=False, with_records=False):
        self.N, self.P, self.S, self.lean = N, P, S, bool(lean)
        self.tiles_x = self.tiles_y = (S + TILE - 1) // TILE
        self.tiles = N * self.tiles_x * self.tiles_y
        self.cap, self.spill_cap = bin_capacity(N, P, S, lean), spill_capacity(P, lean)
        self.giant_cap = 0 if lean else giant_cap(P)
        self.capq = queue_capacity(N, self.tiles_x, self.tiles_y)
        self.regions, used = OrderedDict(), 0

        def take(name, nbytes):
            nonlocal used
            self.regions[name] = (used, nbytes)
            used += (nbytes + 255) // 256 * 256
        t = self.tiles
        take("counts", 4 * t * SUB)
        take("cursor", 4 * t * SUB)
        take("offset", 4 * t * SUB)
        take("flag", 4 * t)
        take("tail+ctrl", 4 * 64)                 # 32 queue tails, then the ten spill control words
        take("queue.list", 4 * QUEUES * self.capq)
        take("mask", P)
        self.clean_bytes = used
        take("lists", 4 * t * SUB * self.cap)
        take("pool", 4 * self.spill_cap)
        if not lean:
            take("big", 8 * P)
            take("giant", 16 * 8 * self.giant_cap)
        take("fail", 4 * 64)
        if with_records and not lean:
            take("rec", 64 * P)
            if P > SORT_MIN_P:
                total, blocks = _cell_total(N, S, 1), _sort_blocks(P)
                take("sort_cell_of", 4 * P)
                take("sort_block_hist", 4 * blocks * total)
                take("sort_seg_tot", 4 * ((blocks + SORT_SEG - 1) // SORT_SEG) * total)
                take("sort_cell_total", 4 * total)
                take("sort_cell_start", 4 * total)
                take("sort_count", 4)
                take("sort_crec", 32 * P)
                take("sort_id", 4 * P)
                take("sort_inv", 4 * P)
                take("sort_live", P)
        self.total = used

    def words(self, ws, name, count=None, first=0):
        """int64 numpy copy of `count` uint32 words of region `name` of the workspace tensor `ws`"""
        off, nbytes = self.regions[name]
        count = nbytes // 4 - first if count is None else count
        raw = ws[off + 4 * first: off + 4 * (first + count)].cpu().numpy()
        return raw.view(np.uint32).astype(np.int64)

    def first_dirty(self, ws):
        """None when the zero region of `ws` is zero, else '<region>[word i] = value' of its first non-zero word"""
        import torch
        head = ws[: self.clean_bytes]
        if int(torch.count_nonzero(head)) == 0:
            return None
        at = int(torch.nonzero(head)[0, 0])
        for name, (off, nbytes) in self.regions.items():
            if off <= at < off + (nbytes + 255) // 256 * 256:
                if name == "mask":
                    return "mask[%d] = %d" % (at - off, int(head[at]))
                w = (at - off) // 4
                v = int(np.frombuffer(head[off + 4 * w: off + 4 * w + 4].cpu().numpy().tobytes(), np.uint32)[0])
                if name == "tail+ctrl":
                    return ("tail[%d] = %d" % (w, v)) if w < QUEUES else ("ctrl[%d] = %d" % (w - QUEUES, v))
                return "%s[%d] = %d" % (name, w, v)
        return "byte %d" % at


def layout(N, P, S, lean=False, with_records=False):
    return Layout(N, P, S, lean, with_records)


# ---------------------------------------------------------------------------------------------------------------------
# scenes (world space)
# ---------------------------------------------------------------------------------------------------------------------
CUTOFF, SIGMA, THR, ZNEAR, ZFAR = 1.0, 1.0, 0.05, 0.1, 100.0


def _camera():
    import scenes
    M, V, _ = scenes.camera_matrices(2.0, 0.0, 0.0, znear=ZNEAR, zfar=ZFAR)
    return M[0], V[0]


def _plane_map(M):
    """2 x 2 matrix J with ndc = (X, Y) @ J for points (X, Y, 0) of the plane through the origin that faces the camera, and
    a = |d ndc / d world| there"""
    def ndc(p):
        c = np.array([p[0], p[1], p[2], 1.0]) @ M.astype(np.float64)
        return c[:2] / c[3]
    o = ndc((0, 0, 0))
    J = np.stack([ndc((1e-3, 0, 0)) - o, ndc((0, 1e-3, 0)) - o]) / 1e-3
    return J, float(np.sqrt(abs(np.linalg.det(J))))


def h_for_radius(r_px, S, a):
    """h of a splat that faces the camera whose bounding radius is r_px pixels: radius_ndc^2 = cutoff (h a^2 + sigma pixel^2)"""
    pix = 2.0 / S
    r = np.asarray(r_px, np.float64) * pix
    return np.maximum((r * r / CUTOFF - SIGMA * pix * pix) / (a * a), 1e-9).astype(np.float32)


class Scene:
    """numpy inputs of one fused call: packed clouds (not shared), one camera per cloud, h per point"""

    def tensors(self, dev):
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return dict(world=t(self.world), normals=t(self.normals), h=t(self.h), M=t(self.M), V=t(self.V), znear=t(self.znear),
                    zfar=t(self.zfar), first=t(self.first), num=t(self.num), feat=t(self.feat))

    @property
    def cloud_of(self):
        c = np.full((self.P,), -1, np.int32)
        for n, (f, k) in enumerate(zip(self.first.tolist(), self.num.tolist())):
            c[f:f + k] = n
        return c


# per class: number and pixel radius of the clustered points, the residues p & 7 that carry the cluster (two more points of
# every other residue join it: sub-lists that stay below cap in the same tiles), and where in its centre tile the cluster sits
_RECIPE = {
    "a": dict(n=0, r=0.0, res=range(8), at=(4.0, 4.0)),
    "b": dict(n=700, r=2.5, res=range(6), at=(0.0, 0.0)),        # a tile corner: four tiles
    "c": dict(n=620, r=13.0, res=range(6), at=(4.0, 4.0)),       # 5 x 5 tiles
    "d": dict(n=620, r=33.0, res=range(6), at=(4.0, 4.0)),       # 9 x 9 tiles: 2 x 2 blocks of 8 x 8
    "e1": dict(n=2100, r=25.0, res=range(7), at=(4.0, 4.0)),     # 7 x 7 tiles x 7 sub-lists x (300 - 64) entries > 65,536
    "e2": dict(n=350, r=33.0, res=(0,), at=(4.0, 4.0)),          # one segment: 4 blocks x (350 - 64) records > 1,024
}
_RECIPE["e3"] = _RECIPE["c"]     # the same splats under DSS_OPT_LEAN_WORKSPACE
CLUSTER_TILE_ROW = 4             # the cluster's centre tile: row 4 (a 9 x 9 rectangle starts at tile row 0), middle column


def build_scene(cls, N=1, S=128, Pc=3000, seed=0, move=0):
    """Cloud 0 carries the class's cluster (upper part of the image) on top of a background patch of 1-pixel splats (lower
    part); clouds 1.. are small background patches of ragged sizes over the whole image, cloud 1 (N > 2) is empty, the last
    cloud (N > 1) lies behind its camera: all culled.  A few packed points behind the last cloud belong to no cloud.
    `move` shifts the cluster by that many tiles along the image row."""
    rc = _RECIPE[cls]
    rng = np.random.default_rng(seed + 17 * CLASSES.index(cls))
    M, V = _camera()
    J, a = _plane_map(M)
    Jinv = np.linalg.inv(J)
    sizes = [Pc] + [0 if (n == 1 and N > 2) else 150 + 37 * (n % 5) for n in range(1, N)]
    tc, tr = ((S + TILE - 1) // TILE) // 2 + int(move), CLUSTER_TILE_ROW
    world, normals, h = [], [], []
    for n, size in enumerate(sizes):
        col = rng.uniform(0.03 * S, 0.97 * S, size)
        row = rng.uniform(TILE * (tr + 6) + 1 if n == 0 else 0.03 * S, S - 3.0, size)
        rad = rng.uniform(0.8, 1.6, size)
        if n == 0 and rc["n"]:
            res = set(rc["res"])
            ids = [i for i in range(size) if (i & 7) in res][: rc["n"]]
            assert len(ids) == rc["n"], "cloud too small for the cluster"
            for r in sorted(set(range(8)) - res):
                ids += [r + 8, r + 16]
            ids = np.asarray(ids)
            jit = 0.35 if rc["r"] < 4 else 1.0
            col[ids] = TILE * tc + rc["at"][0] + rng.uniform(-jit, jit, len(ids))
            row[ids] = TILE * tr + rc["at"][1] + rng.uniform(-jit, jit, len(ids))
            rad[ids] = rc["r"] * rng.uniform(0.98, 1.02, len(ids))
        # image column c <-> NDC index S - 1 - c (tile_rect.h): the centre of pixel c has ndc = 1 - (2 c + 1) / S
        ndc = np.stack([1.0 - 2.0 * col / S, 1.0 - 2.0 * row / S], 1)
        xy = ndc @ Jinv
        z = -0.05 * (xy ** 2).sum(1) + rng.uniform(-0.02, 0.02, size)      # gently curved, a little depth noise
        if N > 1 and n == N - 1:
            z = z + 5.0                                                   # behind the camera: culled by depth
        world.append(np.concatenate([xy, z[:, None]], 1))
        nr = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.05, 0.05, (size, 3))
        normals.append(nr / np.linalg.norm(nr, axis=1, keepdims=True))
        h.append(h_for_radius(rad, S, a))
    orphans = 5 if N > 1 else 0
    world.append(np.zeros((orphans, 3))); normals.append(np.tile([0.0, 0.0, 1.0], (orphans, 1))); h.append(np.full(orphans, 1e-4))
    s = Scene()
    s.cls, s.N, s.S = cls, N, S
    s.world = np.concatenate(world).astype(np.float32)
    s.normals = np.concatenate(normals).astype(np.float32)
    s.h = np.concatenate(h).astype(np.float32)
    s.P = s.world.shape[0]
    s.num = np.asarray(sizes, np.int64)
    s.first = np.cumsum(s.num) - s.num
    s.M, s.V = np.tile(M, (N, 1, 1)).astype(np.float32), np.tile(V, (N, 1, 1)).astype(np.float32)
    s.znear, s.zfar = np.full(N, ZNEAR, np.float32), np.full(N, ZFAR, np.float32)
    s.feat = rng.uniform(0, 1, (s.P, 3)).astype(np.float32)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------------------------------------------------
def band(rows, S):
    """(row0, row1, cycle) of `rows` = None | (row0, row1) | (row0, row1, cycle), and the image rows it holds in band order"""
    if rows is None:
        return (0, S, 1), list(range(S))
    r0, r1, c = int(rows[0]), int(rows[1]), (int(rows[2]) if len(rows) > 2 else 1)
    if c > 1:
        return (r0, r1, c), [r + i for r in range(r0, r1, 8 * c) for i in range(8) if r + i < r1]
    return (r0, r1, c), list(range(r0, r1))


def workspace_bytes(N, P, S, K=5):
    from dss_amd import _lib
    return int(_lib.load().dss_render_forward_workspace(N, P, S, K))


def render(t, S, ws, state, K=5, rows=None, feat=None, want_zbuf=True, band_outputs_only=False, backface=False, per_point=None):
    """dss_render_forward on the caller's workspace `ws` (uint8 tensor) with workspace_state `state`; `t` = Scene.tensors().
    `per_point`: the outputs of an earlier call whose per-point tensors this call is handed (DSS_WS_BINNED does not rewrite
    them, and its fine pass reads them); `visible` is handed over as a copy."""
    import torch
    from dss_amd import _lib
    dev = t["world"].device
    feat = t["feat"] if feat is None else feat
    N, P, C = t["first"].shape[0], t["world"].shape[0], feat.shape[1]
    (row0, row1, cyc), ri = band(rows, S)
    nr = len(ri)
    e = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    bo = band_outputs_only and (state & 0xf) != 2
    o = dict(pts_screen=e(P, 3), ellipse_params=z(P, 3) if bo else e(P, 3), radii=e(P, 2), scaler=z(P) if bo else e(P),
             cutoff_threshold=z(P) if bo else e(P), idx=e(N, nr, S, K, dtype=torch.int32),
             zbuf=e(N, nr, S, K) if want_zbuf else None, qvalue=e(N, nr, S, K), occupancy=e(N, nr, S), image=e(N, nr, S, C + 1),
             wsum=e(N, nr, S))
    valid, vis = e(P, dtype=torch.uint8), e(P, dtype=torch.uint8)
    if per_point is not None:
        for k in ("pts_screen", "ellipse_params", "radii", "scaler", "cutoff_threshold"):
            o[k] = per_point[k]
        valid, vis = per_point["valid"].view(torch.uint8), per_point["visible"].view(torch.uint8).clone()
    if bo:
        state |= _lib.WS_BAND_OUTPUTS
    _lib.call("dss_render_forward", dev, t["world"], t["normals"], t["h"], None, None, None, t["M"], t["V"], t["znear"], t["zfar"],
              t["first"], t["num"], N, P, 0, int(backface), S, K, CUTOFF, SIGMA, THR, row0, row1, cyc, feat, C,
              o["pts_screen"], o["ellipse_params"], o["radii"], o["scaler"], o["cutoff_threshold"], valid, o["idx"], o["zbuf"],
              o["qvalue"], o["occupancy"], vis, o["image"], 0, 0, o["wsum"], ws, ws.numel(), int(state))
    o["valid"], o["visible"] = valid.view(torch.bool), vis.view(torch.bool)
    return o


# ---------------------------------------------------------------------------------------------------------------------
# class prover
# ---------------------------------------------------------------------------------------------------------------------
_PROVER_SRC = r"""
#include "tile_rect.h"
using namespace dss;
// counts: (3, N * tiles * 8) int32 -- splats of at most 2 x 2 tiles | of up to 8 x 8 tiles | wider -- per sub-list p & 7;
// rect: (P, 4) tx0 tx1 ty0 ty1, -1 where the splat reaches no tile of the band
extern "C" void fw_count(long long P, const float *pts, const float *radii, const int *cloud_of, int N, int S, int row0,
                         int rows, int tiles_y, int tshift, int *counts, int *rect)
{
    TileGrid g;
    g.S = S; g.row0 = row0; g.rows = rows; g.tiles_x = (S + DSS_TILE - 1) / DSS_TILE; g.tiles_y = tiles_y; g.tshift = tshift;
    const long long per = (long long)N * g.tiles_x * g.tiles_y * 8;
    for (long long p = 0; p < P; ++p) {
        int tx0, tx1, ty0, ty1;
        rect[4 * p] = rect[4 * p + 1] = rect[4 * p + 2] = rect[4 * p + 3] = -1;
        const int n = cloud_of[p];
        if (n < 0 || !splat_tile_rect(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], radii[2 * p], radii[2 * p + 1], g, tx0, tx1, ty0, ty1))
            continue;
        rect[4 * p] = tx0; rect[4 * p + 1] = tx1; rect[4 * p + 2] = ty0; rect[4 * p + 3] = ty1;
        const int w = (tx1 - tx0 <= 1 && ty1 - ty0 <= 1) ? 0 : (tx1 - tx0 < 8 && ty1 - ty0 < 8) ? 1 : 2;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx)
                ++counts[w * per + (((long long)n * g.tiles_y + ty) * g.tiles_x + tx) * 8 + (p & 7)];
    }
}
// upper bound of the giant records per segment p & 7: one per 8 x 8 block of a wide splat's rectangle that holds a tile whose
// sub-list (p & 7) ends above cap
extern "C" void fw_giant_upper(long long P, const int *rect, const int *cloud_of, const int *total, int tiles_x, int tiles_y,
                               int cap, long long *upper)
{
    for (long long p = 0; p < P; ++p) {
        const int tx0 = rect[4 * p], tx1 = rect[4 * p + 1], ty0 = rect[4 * p + 2], ty1 = rect[4 * p + 3];
        if (tx0 < 0 || (tx1 - tx0 < 8 && ty1 - ty0 < 8)) continue;
        for (int by = ty0; by <= ty1; by += 8)
            for (int bx = tx0; bx <= tx1; bx += 8) {
                bool any = false;
                for (int ty = by; ty <= ty1 && ty < by + 8; ++ty)
                    for (int tx = bx; tx <= tx1 && tx < bx + 8; ++tx)
                        any = any || total[(((long long)cloud_of[p] * tiles_y + ty) * tiles_x + tx) * 8 + (p & 7)] > cap;
                upper[p & 7] += any;
            }
    }
}
"""
_prover = None


def _prover_lib():
    global _prover
    if _prover is None:
        d = tempfile.mkdtemp(prefix="fw_prover_")
        src, so = os.path.join(d, "prover.cpp"), os.path.join(d, "prover.so")
        with open(src, "w") as f:
            f.write(_PROVER_SRC)
        subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "dss_amd", "csrc"), src, "-o", so], check=True)
        _prover = ctypes.CDLL(so)
    return _prover


def _grid(S, rows):
    (row0, row1, cyc), ri = band(rows, S)
    tshift = 3 + (cyc.bit_length() - 1)
    return row0, len(ri), (len(ri) + TILE - 1) // TILE, tshift


class Proof:
    pass


def prove(pts_screen, radii, valid, first, num, S, rows=None, lean=False):
    """`valid` only restates pts_screen z < 0 (a culled splat has z = -1 and reaches nothing); it is checked, not used"""
    ps, ra = np.ascontiguousarray(pts_screen, np.float32), np.ascontiguousarray(radii, np.float32)
    P, N = ps.shape[0], len(first)
    cloud_of = np.full((P,), -1, np.int32)
    for n, (f, k) in enumerate(zip(np.asarray(first).tolist(), np.asarray(num).tolist())):
        cloud_of[f:f + k] = n
    assert not bool((np.asarray(valid).astype(bool) & (ps[:, 2] < 0)).any())
    row0, nrows, tiles_y, tshift = _grid(S, rows)
    tiles_x = (S + TILE - 1) // TILE
    L = _prover_lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cnt = np.zeros((3, N, tiles_y, tiles_x, SUB), np.int32)
    rect = np.empty((P, 4), np.int32)
    L.fw_count(ctypes.c_longlong(P), vp(ps), vp(ra), vp(cloud_of), N, S, row0, nrows, tiles_y, tshift, vp(cnt), vp(rect))
    lay = Layout(N, P, S, lean)
    cap = lay.cap
    pr = Proof()
    pr.cap, pr.layout, pr.rect = cap, lay, rect
    pr.by_width = cnt
    pr.counts = total = np.ascontiguousarray(cnt.sum(0))                     # (N, tiles_y, tiles_x, 8)
    over = total > cap
    pr.over = over
    pr.n_over = int(over.sum())
    tile_over, tile_occ = over.any(-1), (total > 0).any(-1)
    pr.mixed_tiles = int((tile_over & ((total < cap) & (total > 0)).any(-1)).sum())  # a full and a partly filled sub-list in one tile
    pr.empty_tiles = int((~tile_occ).sum())
    pr.plain_tiles = int((tile_occ & ~tile_over).sum())
    pr.occupied_tiles = int(tile_occ.sum())
    pr.pool_demand = int(np.maximum(total - cap, 0).sum())
    # per width: sub-lists in which a splat of that width meets a full sub-list for certain / possibly
    pr.certain = [int((over & (cnt[w] > cap)).sum()) for w in range(3)]
    pr.possible = [int((over & (cnt[w] > 0)).sum()) for w in range(3)]
    # giant records per segment: at least (count - cap) per tile, summed over tiles that no 8 x 8 block can share
    # (a lattice of stride 8: a block is 8 tiles wide; the best of its 64 offsets); at most one per (splat, block)
    lower = np.zeros(8, np.int64)
    g = cnt[2]
    for s in range(8):
        for n in range(N):
            m = np.maximum(g[n, :, :, s] - cap, 0)
            if m.any():
                lower[s] += max(int(m[oy::8, ox::8].sum()) for oy in range(8) for ox in range(8))
    upper = np.zeros(8, np.int64)
    L.fw_giant_upper(ctypes.c_longlong(P), vp(rect), vp(cloud_of), vp(total), tiles_x, tiles_y, cap, vp(upper))
    pr.giant_lower, pr.giant_upper = lower, upper
    reached = {"a"} if pr.n_over == 0 else set()
    if pr.n_over:
        if pr.certain[0]:
            reached.add("b")
        if pr.certain[1]:
            reached.add("e3" if lean else "c")
        if pr.certain[2]:
            reached.add("e3" if lean else "d")
        if pr.pool_demand > lay.spill_cap:
            reached.add("e1")
        if not lean and int(lower.max()) > lay.giant_cap:
            reached.add("e2")
    pr.reached = reached
    # what the scene can NOT reach: no splat of that width in an over-full sub-list, records / pool certainly sufficient
    pr.excluded = set(CLASSES[1:]) if pr.n_over == 0 else set()
    if not pr.possible[1] and not pr.possible[2]:
        pr.excluded |= {"c", "d", "e2", "e3"}
    if not pr.possible[2]:
        pr.excluded |= {"d", "e2"}
    if lean or int(upper.max()) <= lay.giant_cap:
        pr.excluded.add("e2")
    if pr.pool_demand <= lay.spill_cap:
        pr.excluded.add("e1")
    if not lean:
        pr.excluded.add("e3")
    pr.widest = max(reached, key=CLASSES.index)
    return pr


def check_minimum(pr, cls, where=""):
    """the minimum counts every scene of a class must show (asserted on the CPU, and again from a GPU call's own outputs)"""
    w = {"b": 0, "c": 1, "d": 2, "e1": 1, "e2": 2, "e3": 1}.get(cls)
    msg = "%s class %s: reached %s, %d over-full sub-lists, certain %s, mixed %d, empty %d, plain %d, pool %d / %d, giant %s..%s / %d" % (
        where, cls, sorted(pr.reached), pr.n_over, pr.certain, pr.mixed_tiles, pr.empty_tiles, pr.plain_tiles, pr.pool_demand,
        pr.layout.spill_cap, pr.giant_lower.max(), pr.giant_upper.max(), pr.layout.giant_cap)
    assert cls in pr.reached and pr.widest == cls, msg
    for c in CLASSES[CLASSES.index(cls) + 1:]:
        assert c in pr.excluded, "%s: class %s not excluded" % (msg, c)
    assert pr.empty_tiles >= 64 and pr.plain_tiles >= 64, msg
    if cls != "a":
        assert pr.certain[w] >= 8 and pr.mixed_tiles >= 1, msg
    return msg


# ---------------------------------------------------------------------------------------------------------------------
# the cases both test modules use
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = OrderedDict([("S128-N1", (1, 128)), ("S128-N16", (16, 128)), ("S128-N17", (17, 128)), ("S100-N4", (4, 100))])
_scenes = {}


def scene(cls, shape="S128-N1", move=0):
    """the scene of class `cls` at shape `shape` (built once; every class of one shape has the same N, P, S)"""
    key = (cls, shape, move)
    if key not in _scenes:
        N, S = SHAPES[shape]
        _scenes[key] = build_scene(cls, N, S, move=move)
    return _scenes[key]
