"""fp64 CPU reference of the render backward's gather (TEST INFRASTRUCTURE; plain numpy, no product code in the formulas).

What `dss_render_backward` (`dss_amd/csrc/raster_backward.hip`) and its unfused entries (`ops.splat_backward`,
`ops.occ_backward`, `ops.blend_backward`) compute, each ENTRY with the sum of its ABSOLUTE terms next to it: the position
gradient of the occupancy surrogate cancels (|sum| / sum |term| has a median of 0.1-0.2 and goes down to 3e-5), so the error
of a kernel is measured against ``A = sum |term|`` of that entry, neither against the entry nor against the whole vector.
Everything the reference method DECIDES in fp32 is decided in fp32 here; everything after a decision is fp64.  The rules are
those of `oracle_occ_backward_fast`, `oracle_blend_backward` and `oracle_backward_radius` (`oracle/dss_oracle.c`).

    rs[n]  = fp32: lower median of the flattened radii of the VISIBLE points of cloud n, times radii_s; 0 without one
    a point is a candidate when it is visible, owned by a cloud and not (pz < 0 or |px| > 1 or |py| > 1)
    pair (p, pixel (xi, yi)) of p's camera, g = alpha channel of grad_out at image element (S-1-yi, S-1-xi):
        fp32: dx = ndc(xi) - px, dy = ndc(yi) - py, ndc(i) = -1 + (2 i + 1) / S, d2 = dx dx + dy dy (every operation rounded)
        skipped when g == 0, d2 > rs rs, (g > 0 and (|dx| > rx or |dy| > ry)), or d2 == 0
        fp64: term = (dx, dy) g / max(dx^2 + dy^2, 1e-10)
    grad_pts[p, :2] = sum term,  A[p, :2] = sum |term|,  the z column is 0
    clip > 0: k = min(|v|, clip) / max(|v|, 1e-12); the value is k v, the scale of EVERY component k sum_i A_i (the norm
              couples them: |d(k v_i)| <= k sum_j |dv_j|)
    grad_features[p] = sum over the pixels and slots k with idx == p of grad_out[ch] exp(-q_k / 2) scaler[p] / cum
              cum = the given `wsum` of the pixel (its fp32 value is an input), or with wsum = None
              max(sum_k exp(-q_k / 2) scaler[idx_k], 1e-4) recomputed in fp64

``rows`` (a list of image rows) restricts both pixel sets to a band: the partial sums that a band entry returns.

``dtype=np.float32`` evaluates the same formulas in plain fp32, every operation rounded and the sums sequential: what the
number format alone costs, and what a bar is 4 x of (`BARS`).  ``mut`` names one of `MUTATIONS`, a wrong formula that
`tests/test_gather_reference_cpu.py` shows to lie at least 10 x beyond the bars.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from shading_reference import UNDERFLOW, entry_ratio, round_up_1sig  # noqa: F401  (the tests' check)

F32, F64 = np.float32, np.float64
OUTPUTS = ("pts", "feat", "feat_nowsum", "z", "pts3_clip")
CLIP3 = 0.05          # the clip of the `pts3_clip` output (`ops.splat_backward` with grad_zbuf and a clip)


def pix_to_ndc(i, S, mut=None):
    """fp32 pixel centre, as the reference evaluates it"""
    odd = (2 * np.asarray(i) + 1).astype(F32)
    if mut == "centre_map_pow2":
        return F32(-1) + odd * (F32(1) / F32(S))
    return F32(-1) + odd / F32(S)


def _ranges(first, num):
    return [(int(a), int(a) + int(b)) for a, b in zip(first, num)]


def search_radius(radii, vis, first, num, radii_s, mut=None):
    """-> rs (N,) fp32"""
    rs = np.zeros(len(num), F32)
    for n, (lo, hi) in enumerate(_ranges(first, num)):
        r = radii[lo:hi]
        flat = np.sort((r if mut == "median_all_points" else r[vis[lo:hi].astype(bool)]).reshape(-1))
        if flat.size:
            rs[n] = flat[flat.size // 2 if mut == "upper_median" else (flat.size - 1) // 2] * F32(radii_s)
    return rs


def _seq_sum(t):
    """fp32 sum of the last axis, one addition after the other"""
    return np.cumsum(t, axis=-1, dtype=F32)[..., -1]


def position(pts, radii, vis, first, num, galpha, rs, rows=None, dtype=F64, mut=None):
    """the occupancy surrogate -> (val (P,2) fp64, A (P,2) fp64, pairs (P,) int64, info); ``galpha`` (N,S,S) fp32 is the
    alpha plane of the WHOLE image gradient, ``rows`` the image rows whose pixels take part"""
    N, S = galpha.shape[:2]
    P = pts.shape[0]
    val, A, pairs = np.zeros((P, 2), F64), np.zeros((P, 2), F64), np.zeros(P, np.int64)
    rowmask = np.ones(S, bool)
    if rows is not None:
        rowmask[:] = False
        rowmask[np.asarray(rows, np.int64)] = True
    info = dict(candidates=0, window=0, without_pair=0, cut=[0, 0, 0, 0])       # cut: windows that reach past a border
    vis = vis.astype(bool)
    for n, (lo, hi) in enumerate(_ranges(first, num)):
        p_all = np.arange(lo, hi)
        x, y, z = pts[lo:hi, 0], pts[lo:hi, 1], pts[lo:hi, 2]
        p_all = p_all[vis[lo:hi] & ~((z < 0) | (np.abs(x) > 1) | (np.abs(y) > 1))]
        info["candidates"] += p_all.size
        if not p_all.size:
            continue
        for k, past in enumerate((pts[p_all, 0] - rs[n] < -1, pts[p_all, 0] + rs[n] > 1, pts[p_all, 1] - rs[n] < -1,
                                  pts[p_all, 1] + rs[n] > 1)):
            info["cut"][k] += int(past.sum())
        W = min(int(math.ceil(float(rs[n]) * S / 2)) + 2, S)
        off = np.arange(-W, W + 1)
        w = off.size
        rs2 = rs[n] * rs[n]
        small_g = 0.1 * float(np.abs(galpha[n]).max())
        step = max(1, 1500000 // (w * w))
        for c0 in range(0, p_all.size, step):
            c = p_all[c0:c0 + step]
            px, py, rx, ry = pts[c, 0], pts[c, 1], radii[c, 0], radii[c, 1]
            if mut == "rxry_swap":
                rx, ry = ry, rx
            xi = np.floor((px.astype(F64) + 1) * S / 2).astype(np.int64)[:, None] + off[None]
            yi = np.floor((py.astype(F64) + 1) * S / 2).astype(np.int64)[:, None] + off[None]
            okx, oky = (xi >= 0) & (xi < S), (yi >= 0) & (yi < S)
            xi, yi = np.clip(xi, 0, S - 1), np.clip(yi, 0, S - 1)
            dx = pix_to_ndc(xi, S, mut) - px[:, None]          # (m, w) fp32
            dy = pix_to_ndc(yi, S, mut) - py[:, None]
            d2 = (dx * dx)[:, None, :] + (dy * dy)[:, :, None]   # (m, y, x) fp32
            r_img = S - 1 - yi
            c_img = xi if mut == "no_mirror" else S - 1 - xi
            g = galpha[n][r_img[:, :, None], c_img[:, None, :]]
            inr = (oky[:, :, None] & okx[:, None, :]) & ~((d2 >= rs2) if mut == "radius_ge" else (d2 > rs2))
            ox, oy = (np.abs(dx) > rx[:, None])[:, None, :], (np.abs(dy) > ry[:, None])[:, :, None]
            outside = (ox & oy) if mut == "box_and" else (ox | oy)
            boxed = (g != 0) if mut == "box_neg" else (g > 0)
            keep = inr & rowmask[r_img][:, :, None] & (g != 0) & ~(boxed & outside) & (d2 != 0)
            cols, rws = inr.any(axis=1), inr.any(axis=2)       # (m, w): the columns / rows of the point's window
            info["window"] = max(info["window"], int(cols.sum(1).max()), int(rws.sum(1).max()))
            ar = np.arange(w)[None]
            if mut == "window_xlo":
                keep &= ~(ar == np.argmax(cols, 1)[:, None])[:, None, :]
            elif mut == "window_xhi":
                keep &= ~(ar == w - 1 - np.argmax(cols[:, ::-1], 1)[:, None])[:, None, :]
            elif mut == "window_ylo":
                keep &= ~(ar == np.argmax(rws, 1)[:, None])[:, :, None]
            elif mut == "window_yhi":
                keep &= ~(ar == w - 1 - np.argmax(rws[:, ::-1], 1)[:, None])[:, :, None]
            elif mut == "last_row_small_g":
                keep &= ~((ar == w - 1 - np.argmax(rws[:, ::-1], 1)[:, None])[:, :, None] & (np.abs(g) <= small_g))
            m = c.size
            dx64, dy64 = dx.astype(F64)[:, None, :], dy.astype(F64)[:, :, None]
            den = dx64 * dx64 + dy64 * dy64
            if mut != "no_floor":
                den = np.maximum(den, 1e-10)
            s = np.where(keep, g.astype(F64) / np.where(keep, den, 1.0), 0.0)
            tx, ty = (dx64 * s).reshape(m, -1), (dy64 * s).reshape(m, -1)
            A[c, 0], A[c, 1] = np.abs(tx).sum(1), np.abs(ty).sum(1)
            pairs[c] = keep.reshape(m, -1).sum(1)
            if dtype is F64:
                val[c, 0], val[c, 1] = tx.sum(1), ty.sum(1)
            else:
                den32 = np.maximum(d2, F32(1e-10))
                val[c, 0] = _seq_sum(np.where(keep, dx[:, None, :] / den32 * g, F32(0)).reshape(m, -1))
                val[c, 1] = _seq_sum(np.where(keep, dy[:, :, None] / den32 * g, F32(0)).reshape(m, -1))
        info["without_pair"] += int((pairs[p_all] == 0).sum())
    return val, A, pairs, info


def clip_rows(v, A, clip, dtype=F64, mut=None):
    """the per-point clip hook on (P,d) rows -> (k v, k sum_i A_i in every column)"""
    if not clip > 0:
        return v, A
    if dtype is F64:
        nrm = np.sqrt((v * v).sum(1))
        k = np.minimum(nrm, clip) / np.maximum(nrm, 1e-12)
        out = v * k[:, None]
    else:
        v32 = v.astype(F32)
        sq = v32 * v32
        nrm = np.sqrt(_seq_sum(sq))
        out = (v32 / np.maximum(nrm, F32(1e-12))[:, None] * np.minimum(nrm, F32(clip))[:, None]).astype(F64)
        k = (np.minimum(nrm, F32(clip)) / np.maximum(nrm, F32(1e-12))).astype(F64)
    if mut == "clip_one_component":
        out[:, 1:] = v[:, 1:]
    return out, np.repeat((k * A.sum(1))[:, None], v.shape[1], 1)


def features(grad_out, idx, qv, wsum, scaler, P, rows=None, dtype=F64, mut=None):
    """the blend backward -> (val (P,C) fp64, A (P,C) fp64); tensors of the WHOLE image, ``rows`` the image rows taking part"""
    if rows is not None:
        rows = np.asarray(rows, np.int64)
        grad_out, idx, qv = grad_out[:, rows], idx[:, rows], qv[:, rows]
        wsum = None if wsum is None else wsum[:, rows]
    C = grad_out.shape[-1] - 1
    ok = idx >= 0
    pc = np.where(ok, idx, 0)
    q = qv.astype(dtype)
    if mut == "q_neighbour":
        q = np.roll(q, 1, axis=-1)
    sc = np.ones(pc.shape, dtype) if mut == "no_scaler" else scaler[pc].astype(dtype)
    if mut == "exp_const":
        wgt = np.exp2(-0.7213 * q) * sc
    else:
        wgt = np.exp(dtype(-0.5) * q) * sc
    wgt = np.where(ok, wgt, dtype(0))
    if wsum is None:
        cum = wgt.sum(-1) if dtype is F64 else _seq_sum(wgt)
        cum = np.where(ok.any(-1), cum, dtype(1)) if mut == "no_clamp" else np.maximum(cum, dtype(F32(1e-4)))
    else:
        cum = wsum.astype(dtype)
    term = (grad_out[..., None, :C].astype(dtype) * wgt[..., None] / cum[..., None, None])[ok]     # (M, C)
    assert term.dtype == dtype
    val, A = np.zeros((P, C), dtype), np.zeros((P, C), F64)
    np.add.at(val, pc[ok], term)            # unbuffered: one addition after the other, in pixel order
    np.add.at(A, pc[ok], np.abs(term).astype(F64))
    return val.astype(F64), A


def depth_sum(idx, grad_zbuf, P, dtype=F64):
    """the z-buffer backward -> (val (P,), A (P,)): grad_zbuf summed over the fragments of a point"""
    ok = idx >= 0
    val, A = np.zeros(P, dtype), np.zeros(P, F64)
    np.add.at(val, idx[ok], grad_zbuf[ok].astype(dtype))
    np.add.at(A, idx[ok], np.abs(grad_zbuf[ok]).astype(F64))
    return val.astype(F64), A


# ---------------------------------------------------------------------------------------------------------------------
# the cases that tests/test_gather_reference_cpu.py and tests/test_gpu_gather_grad.py share
Case = namedtuple("Case", "name S N K C P pts radii vis first num idx qv wsum scaler grad_out grad_zbuf radii_s clip planted")
Ref = namedtuple("Ref", "pts pts_A feat feat_A pairs rs info")


def position_of(c, rows=None, dtype=F64, mut=None):
    """-> (rs, val, A, pairs, info) of a case: the part of `reference_of` that the clip, the z column and the weight sums
    leave alone"""
    rs = search_radius(c.radii, c.vis, c.first, c.num, c.radii_s, mut)
    return (rs,) + position(c.pts, c.radii, c.vis, c.first, c.num, c.grad_out[..., c.C], rs, rows, dtype, mut)


def reference_of(c, rows=None, dtype=F64, mut=None, use_wsum=True, clip=None, with_z=False, pos=None):
    """-> Ref of a case (fp64, or the fp32 restatement); ``rows``: the band's partial sums (no clip then); ``with_z``: the
    3-vector of `ops.splat_backward` with grad_zbuf, the clip on all three components; ``pos``: `position_of` of the same
    case, rows, dtype and mut, computed before"""
    clip = c.clip if clip is None else clip
    rs, v, A, pairs, info = position_of(c, rows, dtype, mut) if pos is None else pos
    if with_z:
        z, zA = depth_sum(c.idx, c.grad_zbuf, c.P, dtype)
    else:
        z, zA = np.zeros(c.P), np.zeros(c.P)
    if clip > 0 and with_z:
        v, A = clip_rows(np.concatenate([v, z[:, None]], 1), np.concatenate([A, zA[:, None]], 1), clip, dtype, mut)
    else:
        v, A = clip_rows(v, A, clip, dtype, mut)
        v, A = np.concatenate([v, z[:, None]], 1), np.concatenate([A, zA[:, None]], 1)
    f, fA = features(c.grad_out, c.idx, c.qv, c.wsum if use_wsum else None, c.scaler, c.P, rows, dtype, mut)
    r = c.radii[c.vis.astype(bool)]
    info = dict(info, box=int(math.ceil(float(r.max()) * c.S)) if r.size else 0, rs_px=[float(x) * c.S / 2 for x in rs])
    return Ref(v, A, f, fA, pairs, rs, info)


def _forward(sc, S, K, thr=0.3):
    import oracle
    idx, zbuf, qv, _occ = oracle.splat_forward(sc["points"], sc["ellipse"], sc["cutoff"], sc["radii"], sc["first_idx"],
                                               sc["num_pts"], S, K, thr)
    return idx, qv, oracle.visibility(idx, sc["points"].shape[0])


def _weight_sum(idx, qv, scaler):
    """the forward's per-pixel weight sum in fp32: an INPUT of the backward"""
    ok = idx >= 0
    w = np.where(ok, np.exp(F32(-0.5) * qv) * scaler[np.where(ok, idx, 0)], F32(0)).astype(F32)
    return np.maximum(_seq_sum(w), F32(1e-4))


def _grad_out(rng, N, S, C, loss_shaped=False):
    """the image gradient: normal colours; the alpha channel mixes signs with about 10 % exact zeros, or has the shape of the
    image loss's gradient (+-w on a ring around a disc's edge, plus a small per-camera term everywhere)"""
    go = rng.standard_normal((N, S, S, C + 1)).astype(F32)
    if loss_shaped:
        yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        r = np.hypot(xx - S / 2 + 0.5, yy - S / 2 + 0.5) / (S / 2)
        w = 1.0 / (S * S)
        ring = np.where(np.abs(r - 0.5) < 0.15, np.where(r < 0.5, w, -w), 0.0)
        go[..., C] = (ring[None] + (0.01 * w * (1 + np.arange(N)))[:, None, None]).astype(F32)
    else:
        go[..., C][rng.random((N, S, S)) < 0.1] = 0.0
    return go


def _near_centres(sc, S, rows, rng):
    """moves the points ``rows`` next to pixel centres: by (3e-6, 4e-6) (d2 = 2.5e-11, below the 1e-10 floor) and by a few
    1e-5 (where one ulp of a pixel centre is 1e-3 of the distance)"""
    for j, p in enumerate(rows):
        i = rng.integers(S // 4, 3 * S // 4, 2)
        d = (3e-6, 4e-6) if j % 2 == 0 else tuple(rng.uniform(1e-5, 4e-5, 2))
        sc["points"][p, 0] = pix_to_ndc(i[0], S) + F32(d[0])
        sc["points"][p, 1] = pix_to_ndc(i[1], S) + F32(d[1])
        sc["points"][p, 2] = 0.4            # in front of everything: visible


def _splats(name, seed, P, S, N, K=5, C=3, rmin=1.5, rmax=6.0, rs_px=5.0, clip=-1.0, loss_shaped=False, near=0, radii_s=None,
            scaler_decades=0.0, first=None, num=None, edit=None):
    """a case from `scenes.random_splats`: ``rs_px`` chooses radii_s so that the first cloud's search radius is that many
    pixels; ``near`` points per cloud are moved next to pixel centres; ``edit(sc, rng)`` changes the scene before the forward
    and returns the rows whose visible flag is set by hand"""
    import scenes
    rng = np.random.default_rng(seed)
    sc = scenes.random_splats(P, S, N, seed=seed, rmin=rmin, rmax=rmax)
    if first is not None:
        sc["first_idx"], sc["num_pts"] = np.asarray(first, np.int64), np.asarray(num, np.int64)
        N = len(first)
    planted = np.concatenate([lo + 7 + 11 * np.arange(near) for lo, hi in _ranges(sc["first_idx"], sc["num_pts"]) if hi - lo > 7 + 11 * near]
                             + [np.zeros(0, np.int64)]).astype(np.int64)
    _near_centres(sc, S, planted, rng)
    by_hand = np.zeros(0, np.int64) if edit is None else np.asarray(edit(sc, rng), np.int64)
    if scaler_decades:
        sc["scaler"] = (sc["scaler"] * 10.0 ** rng.uniform(-scaler_decades, 0.0, sc["scaler"].shape)).astype(F32)
    idx, qv, vis = _forward(sc, S, K)
    vis[by_hand] = True
    if radii_s is None:
        probe = search_radius(sc["radii"], vis, sc["first_idx"], sc["num_pts"], 1.0)
        radii_s = float(F32(rs_px * 2.0 / S / float(probe[probe > 0][0])))
    go = _grad_out(rng, N, S, C, loss_shaped)
    gz = rng.standard_normal(idx.shape).astype(F32)
    return Case(name, S, N, K, C, sc["points"].shape[0], sc["points"], sc["radii"], vis, sc["first_idx"], sc["num_pts"], idx, qv,
                _weight_sum(idx, qv, sc["scaler"]), sc["scaler"], go, gz, radii_s, clip, planted)


def _tie_case(name, seed=5):
    """circular splats of ONE radius, 5 / S exactly, half of them exactly on pixel centres, radii_s = 2: rs = 10 / S, and
    the pixels 3 and 4, or 5 and 0, columns and rows away lie at d2 == rs^2 to the last bit; the pair at d2 == 0 exists"""
    S, N, Pc, K, C = 64, 2, 300, 5, 3
    rng = np.random.default_rng(seed)
    P = N * Pc
    pts = rng.uniform(-0.95, 0.95, (P, 3)).astype(F32)
    pts[:, 2] = rng.uniform(0.5, 3, P).astype(F32)
    on = np.arange(0, P, 2)
    pts[on, 0], pts[on, 1] = pix_to_ndc(rng.integers(0, S, on.size), S), pix_to_ndc(rng.integers(0, S, on.size), S)
    r0 = F32(5) / F32(S)
    sc = dict(points=pts, radii=np.full((P, 2), r0, F32), cutoff=np.ones(P, F32),
              ellipse=np.stack([np.full(P, 1 / float(r0) ** 2), np.zeros(P), np.full(P, 1 / float(r0) ** 2)], 1).astype(F32),
              scaler=rng.uniform(0.5, 2.0, P).astype(F32), first_idx=(np.arange(N) * Pc).astype(np.int64), num_pts=np.full(N, Pc, np.int64))
    idx, qv, vis = _forward(sc, S, K)
    vis[on] = True
    go = _grad_out(rng, N, S, C)
    return Case(name, S, N, K, C, P, pts, sc["radii"], vis, sc["first_idx"], sc["num_pts"], idx, qv, _weight_sum(idx, qv, sc["scaler"]),
                sc["scaler"], go, rng.standard_normal(idx.shape).astype(F32), 2.0, -1.0, on)


def _ragged_flags(sc, rng):
    """cloud 3 (1501 points) moves off the screen: nothing of it is visible, rs = 0.  In cloud 2 (777 points) twenty points
    go off-screen or behind the camera and get a visible flag by hand: no candidates."""
    lo = int(sc["first_idx"][3])
    sc["points"][lo:lo + 1501, 0] += 3.0
    rows = int(sc["first_idx"][2]) + 5 + 13 * np.arange(20)
    sc["points"][rows[:7], 0] = 1.02
    sc["points"][rows[7:14], 1] = -1.04
    sc["points"][rows[14:], 2] = -0.2
    return rows


_RAGGED = dict(first=[0, 0, 40, 900], num=[0, 1, 777, 1501])      # rows 1 .. 39 and 817 .. 899 are owned by no cloud; P = 2500


def _zero_patch(c, p, half):
    """grad_out's alpha zeroed around point p: a candidate without a pair, whose gradient is exactly zero"""
    xi, yi = (int(math.floor((float(c.pts[p, k]) + 1) * c.S / 2)) for k in (0, 1))
    n = [k for k, (lo, hi) in enumerate(_ranges(c.first, c.num)) if lo <= p < hi][0]
    r, col = c.S - 1 - yi, c.S - 1 - xi
    c.grad_out[n, max(r - half, 0):r + half + 1, max(col - half, 0):col + half + 1, c.C] = 0.0


def _clip_case(name, clip):
    c = _splats(name, 41, 800, 96, 2)
    p = int(np.nonzero(c.vis & (np.abs(c.pts[:, :2]) < 0.5).all(1) & (c.pts[:, 2] > 0))[0][3])
    _zero_patch(c, p, 9)
    if clip is None:      # the median norm of the unclipped gradient: about half the points are clipped
        r = reference_of(c, clip=-1.0)
        nrm = np.sqrt((r.pts ** 2).sum(1))
        clip = float(F32(np.median(nrm[nrm > 0])))
    return c._replace(clip=clip, planted=np.array([p]))


def _long_case(name):
    """P above 262,144: each cloud's visible points are followed by off-screen filler, which no forward needs to see"""
    c = _splats(name, 61, 2000, 256, 2, rmin=1.5, rmax=4.0, rs_px=4.0)
    fill, Pc = 130000, 2000
    P = 2 * (Pc + fill)
    rng = np.random.default_rng(62)
    grow = lambda a, v: np.concatenate([a[:Pc], v, a[Pc:], v]).astype(a.dtype)
    off = np.concatenate([rng.uniform(1.5, 3.0, (fill, 2)), rng.uniform(0.5, 3, (fill, 1))], 1).astype(F32)
    idx = np.where((c.idx >= Pc), c.idx + fill, c.idx).astype(np.int32)
    return c._replace(P=P, pts=grow(c.pts, off), radii=grow(c.radii, rng.uniform(0.01, 0.05, (fill, 2)).astype(F32)),
                      vis=grow(c.vis, np.zeros(fill, c.vis.dtype)), scaler=grow(c.scaler, np.ones(fill, F32)), idx=idx,
                      first=np.array([0, Pc + fill], np.int64), num=np.array([Pc + fill] * 2, np.int64),
                      planted=np.where(c.planted >= Pc, c.planted + fill, c.planted))


def _bench_case(name):
    """the benchmark's shape (`test_cfg2_bunny_512_forward_backward_vs_oracle`): the bunny x 4 = 32,684 points through the
    oracle's per-point setup, one camera, 512^2, K 5, radii_s 5, clip 0.05 -- the one case above 128^2 besides `long`"""
    import scenes
    S, K = 512, 5
    pts, nrm = scenes.load_cloud("bunny")
    pts, nrm = scenes.upsample_jitter(scenes.normalize_unit_sphere(pts), nrm, 4, seed=0)
    M, V, _ = scenes.camera_matrices(2.0, 30.0, 45.0)
    rng = np.random.default_rng(0)
    sc = scenes.setup_scene(pts, nrm, M, V, S, colors=rng.uniform(0, 1, (pts.shape[0], 3)).astype(F32))
    idx, qv, vis = _forward(sc, S, K, 0.05)
    rng = np.random.default_rng(1)
    go, gz = rng.standard_normal((1, S, S, 4)).astype(F32), rng.standard_normal((1, S, S, K)).astype(F32)
    return Case(name, S, 1, K, 3, sc["points"].shape[0], sc["points"], sc["radii"], vis, sc["first_idx"], sc["num_pts"], idx, qv,
                _weight_sum(idx, qv, sc["scaler"]), sc["scaler"], go, gz, 5.0, 0.05, np.zeros(0, np.int64))


_BUILDERS = {
    "pow2": lambda n: _splats(n, 11, 1500, 128, 2, near=6),
    "pow2_loss": lambda n: _splats(n, 11, 1500, 128, 2, near=6, loss_shaped=True),
    "tie": _tie_case,
    "odd37": lambda n: _splats(n, 12, 300, 37, 2, rs_px=5.0, near=4),
    "odd37_whole": lambda n: _splats(n, 12, 300, 37, 2, rs_px=53.0, near=4),      # 53 px > the diagonal: every window is the image
    "odd100": lambda n: _splats(n, 13, 1000, 100, 2, near=6),
    "wide": lambda n: _splats(n, 14, 1000, 128, 2, rmin=2.0, rmax=40.0, rs_px=22.0),
    "tiny": lambda n: _splats(n, 15, 3000, 128, 2, rmin=0.3, rmax=1.0, radii_s=0.4),
    "depth_k1c1": lambda n: _splats(n, 16, 1500, 128, 2, K=1, C=1, rmin=3.0, rmax=8.0),
    "depth_k8c5": lambda n: _splats(n, 17, 1500, 128, 2, K=8, C=5, rmin=3.0, rmax=8.0),
    "depth_k9c8": lambda n: _splats(n, 18, 1500, 128, 2, K=9, C=8, rmin=3.0, rmax=8.0),
    "depth_k12c3": lambda n: _splats(n, 19, 1500, 128, 2, K=12, C=3, rmin=3.0, rmax=8.0),
    "nowsum": lambda n: _splats(n, 20, 1000, 96, 2, scaler_decades=7.0),
    "ragged": lambda n: _splats(n, 21, 2500, 64, 1, **_RAGGED),
    "ragged_flags": lambda n: _splats(n, 21, 2500, 64, 1, edit=_ragged_flags, **_RAGGED),
    "clip_all": lambda n: _clip_case(n, 0.05),
    "clip_none": lambda n: _clip_case(n, 1e6),
    "clip_median": lambda n: _clip_case(n, None),
    "band96": lambda n: _splats(n, 31, 1500, 96, 2),
    "band100": lambda n: _splats(n, 32, 1500, 100, 2),
    "long": _long_case,
    "bench512": _bench_case,
}
CASES = tuple(_BUILDERS)
ORACLE_CASES = tuple(n for n in CASES if n != "long")       # (the oracle's window loop over 260,000 filler points adds nothing)


def band_rows(name):
    """the row sets of the band cases: the contiguous bands (0, 40, S), twelve bands of 8 rows (the last one shorter or
    longer at S = 100), and the tile-row-cyclic partition of 4 -> [(label, `rows` argument of the entry, image rows)].
    `long` (S = 256): the two contiguous bands (0, 104, S) and the cyclic partition of 4 only"""
    from dss_amd.distributed import RowPartition
    S = case(name).S
    cut = 104 if name == "long" else 40
    out = [("rows %d-%d" % (a, b), (a, b), list(range(a, b))) for a, b in ((0, cut), (cut, S))]
    if name != "long":
        cuts = list(range(0, 88 + 1, 8)) + [S]
        out += [("rows %d-%d" % (a, b), (a, b), list(range(a, b))) for a, b in zip(cuts[:-1], cuts[1:])]
    for g in range(4):
        part = RowPartition(S, 4, g, cyclic=True)
        out.append(("cyclic %d of 4" % g, part.rows, list(part.row_indices())))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name](name)
    owned = np.zeros(c.P, bool)
    for lo, hi in _ranges(c.first, c.num):
        owned[lo:hi] = True
    assert bool(c.vis[c.idx[c.idx >= 0]].all()) and not bool(c.vis[~owned].any())      # what a forward guarantees
    for a in c:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _position(name, rows):
    return position_of(case(name), None if rows is None else list(rows))


@functools.lru_cache(maxsize=None)
def reference(name, rows=None, use_wsum=True, with_z=False, clip=None):
    """the fp64 reference of a case, cached for the module (``rows``: a tuple of image rows)"""
    return reference_of(case(name), rows=None if rows is None else list(rows), use_wsum=use_wsum, with_z=with_z, clip=clip,
                        pos=_position(name, rows))


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def ratio(got, ref, A):
    """`entry_ratio` on numpy arrays or tensors -> (largest (|got - ref| - UNDERFLOW) / A, zeros exact where A == 0)"""
    return entry_ratio(_t(got), _t(ref).double(), _t(A).double())


def fp32_figures(name, rows=None):
    """the largest |fp32 restatement - fp64| / A of the case per output of `OUTPUTS` (what a bar is 4 x of)"""
    c = case(name)
    rows_t = None if rows is None else tuple(rows)
    figs = {}

    def put(key, v32, v, A):
        fig, zeros_ok = ratio(v32, v, A)
        assert zeros_ok, (name, key)
        figs[key] = fig
    pos32 = position_of(c, rows, F32)
    ref, r32 = reference(name, rows_t), reference_of(c, rows=rows, dtype=F32, pos=pos32)
    put("pts", r32.pts, ref.pts, ref.pts_A)
    put("feat", r32.feat, ref.feat, ref.feat_A)
    ref, r32 = reference(name, rows_t, use_wsum=False), reference_of(c, rows=rows, dtype=F32, use_wsum=False, pos=pos32)
    put("feat_nowsum", r32.feat, ref.feat, ref.feat_A)
    if rows is None:
        ref, r32 = reference(name, with_z=True, clip=-1.0), reference_of(c, dtype=F32, with_z=True, clip=-1.0, pos=pos32)
        put("z", r32.pts[:, 2], ref.pts[:, 2], ref.pts_A[:, 2])
        ref, r32 = reference(name, with_z=True, clip=CLIP3), reference_of(c, dtype=F32, with_z=True, clip=CLIP3, pos=pos32)
        put("pts3_clip", r32.pts, ref.pts, ref.pts_A)
    return figs


def case_figures(name):
    """the figures a case's bars come from: the whole image, and for a band case every band as well (the largest counts)"""
    figs = fp32_figures(name)
    if name.startswith("band"):
        for _label, _arg, rows in band_rows(name):
            for k, v in fp32_figures(name, rows).items():
                figs[k] = max(figs[k], v)
    return figs


def bars_of(figs):
    return {k: round_up_1sig(4 * v) for k, v in figs.items()}


def violation(got, ref, A, bar):
    """by what factor the worst entry of ``got`` misses ``|got - ref| <= bar A + UNDERFLOW`` (inf: a non-zero entry where no
    term exists); <= 1 passes"""
    worst, zeros_ok = ratio(got, ref, A)
    if not zeros_ok or (bar == 0 and worst > 0):
        return math.inf
    return worst / bar if bar > 0 else 0.0


def print_bars():
    """`python -c "import gather_reference as g; g.print_bars()"` in tests/: the table below, measured anew"""
    for name in CASES:
        b = bars_of(case_figures(name))
        print("    %r: dict(%s)," % (name, ", ".join("%s=%s" % (k, "%.0e" % b[k] if b[k] else "0") for k in OUTPUTS)))


# which cases each wrong formula must show on (at least 10 x beyond the bar on at least one entry of EVERY listed case), and
# the output it shows in
_WINDOW = ("pow2", "odd100", "wide", "tiny")
MUTATIONS = {
    "window_xlo": ("pts", _WINDOW), "window_xhi": ("pts", _WINDOW), "window_ylo": ("pts", _WINDOW), "window_yhi": ("pts", _WINDOW),
    "radius_ge": ("pts", ("tie",)),
    "box_and": ("pts", ("pow2", "wide", "odd100")),
    "box_neg": ("pts", ("pow2", "wide", "odd100")),
    "rxry_swap": ("pts", ("pow2", "wide", "odd100")),
    "no_mirror": ("pts", ("pow2", "odd37")),
    "centre_map_pow2": ("pts", ("odd37", "odd100")),
    "no_floor": ("pts", ("pow2", "odd100")),
    "upper_median": ("pts", ("pow2", "ragged")),
    "median_all_points": ("pts", ("pow2", "ragged")),
    "no_scaler": ("feat", ("pow2", "depth_k1c1", "depth_k9c8")),
    "q_neighbour": ("feat", ("pow2", "depth_k8c5")),
    "no_clamp": ("feat_nowsum", ("nowsum",)),
    "exp_const": ("feat", ("pow2", "depth_k12c3")),
    "clip_one_component": ("pts", ("clip_all", "clip_median")),
    "last_row_small_g": ("pts", ("pow2_loss",)),
}

# ---------------------------------------------------------------------------------------------------------------------
# The bars of tests/test_gpu_gather_grad.py: 4 x the largest |err| / A of the fp32 restatement against fp64, rounded up to one
# significant digit; tests/test_gather_reference_cpu.py re-measures the figures and asserts the tie.
BARS = {
    'pow2': dict(pts=2e-06, feat=9e-07, feat_nowsum=9e-07, z=7e-07, pts3_clip=4e-07),
    'pow2_loss': dict(pts=2e-06, feat=9e-07, feat_nowsum=9e-07, z=7e-07, pts3_clip=5e-07),
    'tie': dict(pts=7e-07, feat=7e-07, feat_nowsum=7e-07, z=5e-07, pts3_clip=3e-07),
    'odd37': dict(pts=1e-06, feat=8e-07, feat_nowsum=8e-07, z=5e-07, pts3_clip=4e-07),
    'odd37_whole': dict(pts=3e-06, feat=8e-07, feat_nowsum=8e-07, z=5e-07, pts3_clip=1e-06),
    'odd100': dict(pts=2e-06, feat=8e-07, feat_nowsum=8e-07, z=5e-07, pts3_clip=4e-07),
    'wide': dict(pts=2e-06, feat=5e-07, feat_nowsum=5e-07, z=4e-07, pts3_clip=4e-07),
    'tiny': dict(pts=7e-07, feat=1e-06, feat_nowsum=8e-07, z=5e-07, pts3_clip=6e-07),
    'depth_k1c1': dict(pts=7e-07, feat=6e-07, feat_nowsum=5e-07, z=4e-07, pts3_clip=4e-07),
    'depth_k8c5': dict(pts=9e-07, feat=9e-07, feat_nowsum=1e-06, z=5e-07, pts3_clip=4e-07),
    'depth_k9c8': dict(pts=8e-07, feat=1e-06, feat_nowsum=1e-06, z=5e-07, pts3_clip=3e-07),
    'depth_k12c3': dict(pts=1e-06, feat=1e-06, feat_nowsum=1e-06, z=6e-07, pts3_clip=3e-07),
    'nowsum': dict(pts=2e-06, feat=2e-06, feat_nowsum=2e-06, z=5e-07, pts3_clip=3e-07),
    'ragged': dict(pts=2e-06, feat=9e-07, feat_nowsum=8e-07, z=5e-07, pts3_clip=6e-07),
    'ragged_flags': dict(pts=2e-06, feat=9e-07, feat_nowsum=8e-07, z=5e-07, pts3_clip=5e-07),
    'clip_all': dict(pts=3e-07, feat=9e-07, feat_nowsum=1e-06, z=6e-07, pts3_clip=3e-07),
    'clip_none': dict(pts=5e-07, feat=9e-07, feat_nowsum=1e-06, z=6e-07, pts3_clip=3e-07),
    'clip_median': dict(pts=5e-07, feat=9e-07, feat_nowsum=1e-06, z=6e-07, pts3_clip=3e-07),
    'band96': dict(pts=2e-06, feat=2e-06, feat_nowsum=2e-06, z=6e-07, pts3_clip=4e-07),
    'band100': dict(pts=2e-06, feat=1e-06, feat_nowsum=1e-06, z=6e-07, pts3_clip=4e-07),
    'long': dict(pts=2e-06, feat=9e-07, feat_nowsum=8e-07, z=7e-07, pts3_clip=3e-07),
    'bench512': dict(pts=9e-07, feat=1e-06, feat_nowsum=2e-06, z=6e-07, pts3_clip=9e-07),
}
