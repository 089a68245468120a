"""GPU: dss_local_frames (local_frames_kernel, setup.hip) off the well-conditioned path, against frames_reference.py.

What test_gpu_setup.py's one cloud, one K and `gap > 1e-2` mask do not reach: packed layouts of several clouds (the `f0` that
turns cloud-local list entries into packed ids, boundaries that are no multiples of 64), clouds shorter than K (kk = min(K,
num) entries, divided by kk), slots that no cloud owns, zero and denormal traces, and spectra chosen by construction: axis-
aligned covariances that no Jacobi rotation touches (the `m0 / m1` selection alone, all orderings and ties), exactly planar,
collinear and isotropic neighbourhoods, tiny and huge extents, neighbourhoods far from the origin, K = 2 and 3.

Most cases hand the kernel a CONSTRUCTED list: every shape is a group of K points whose lists name the K points of the group.

Every point of every case is asserted, without a mask, on what holds whatever basis a degenerate eigenspace gets (see
`_check`); the values are compared with the fp64 reference where they are determined: `vr6` where (lam1 - lam0) / lam2 > 1e-2
(within B tr / gap) or lam0 <= 1e-6 tr (then vr6 = C - lam0 e0 e0^T is C up to lam0 whatever e0 is: |C_k - C| <= B tr and
lam0_k <= lam0 + B tr give 2 B tr + 2 lam0; where both hold, the smaller bound), the normal where the gap holds.  What that
comparison may skip is capped: nothing in the constructed families beyond the shapes that are undetermined by construction
(octahedra with a = b <= c: e0 is any direction of a plane or of space), at most 1 % of the points of a measured cloud.

The bound B.  Not the 1e-4 of test_gpu_setup.py and not taken from the kernel: the yardstick is `frames_reference.
local_frames_fp32`, the whole pipeline in float32 with LAPACK's single-precision solver, and its largest error against the
fp64 reference over all cases of this file, max(|C32 - C|, |lam32 - lam|) / tr per point (lists from a KD-tree where the GPU
tests take them from dss_knn_points):

    yardstick = 1.8683e-07, set by the teapot at K = 3 (an eigenvalue; its covariances show 1.67e-07)
    B = 8 * yardstick = 1.4947e-06

(the factor 8: Jacobi instead of QR, another summation order).  Per family the yardstick shows 2.0e-08 on the axis-aligned
octahedra, 1.4e-07 on the rotated ones, 1.9e-07 on the planes, 1.3e-07 on the lines, 0.9e-07 .. 1.6e-07 over the extents and
translations, 1.3e-07 on the four clouds, 1.6e-07 / 1.9e-07 / 1.0e-07 / 1.2e-07 on the teapot at K = 2 / 3 / 8 / 20.

Share of the points whose vr6 the comparison skips, by the reference alone: 4 of 13 octahedra by construction (a = b <= c), none
of the flats, of the four clouds and of the teapot at K = 2, 3 and 20, 0.013 % (one point) of the teapot at K = 8.

Two findings of these tests, both fixed in local_frames_kernel: a trace below FLT_MIN (the extent of 1e-21) gave NaN in all
three outputs, and the middle curvature, the sum minus the two others, came out a rounding error below the smallest one where
two eigenvalues are equal or zero (lines, K = 2 and 3, octahedra with a tie)."""
import itertools
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest
import torch

import frames_reference as fr
import scenes
from dss_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

YARDSTICK = 1.8683e-07
B = 8 * YARDSTICK
GAP, RANK = 1e-2, 1e-6
FLT_MIN = float(np.finfo(np.float32).tiny)
EXTENTS = (1e-12, 1e-4, 1.0, 1e3)
SHIFTS = ((0.0, 0.0, 0.0), (1e3, -2e3, 3e3))
SIZES = (517, 5, 300, 1)

# name; pts (P,3) float32; idx (P,K) cloud-local ids; first, num; determined: None = measured cloud (skip cap 1 %), else (P,)
# bool, whether vr6 is determined by construction
Case = namedtuple("Case", "name pts idx first num determined")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# constructed neighbourhoods
# ----------------------------------------------------------------------------------------------------------------------
def _rotations(n, seed):
    """n proper rotations, Haar-distributed (QR of a normal matrix, signs fixed), from a seeded generator"""
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    assert np.allclose(np.linalg.det(q), 1.0) and np.allclose(q @ q.transpose(0, 2, 1), np.eye(3))
    return q


def _octa_axes():
    """the semi-axes (a, b, c) of the octahedra: the six orderings of three distinct values, then every tie pattern at every
    position; -> (list of (a, b, c), vr6 determined by construction: the two smallest differ)"""
    sets = list(itertools.permutations((1.0, 2.0, 3.0)))
    for tie in ((1.0, 1.0, 2.0), (1.0, 2.0, 2.0), (1.0, 1.0, 1.0)):
        sets += sorted(set(itertools.permutations(tie)))
    assert len(sets) == 13
    return sets, np.array([sorted(s)[0] < sorted(s)[1] for s in sets])


def _octahedra(rotations=None):
    """+-a e1, +-b e2, +-c e3 (K = 6, mean exactly zero, covariance exactly diag(a^2, b^2, c^2) / 3), optionally every set under
    every rotation -> (shapes (S,6,3) float64, determined (S,), axes (S,3))"""
    sets, det = _octa_axes()
    base = np.zeros((len(sets), 6, 3))
    for s, abc in enumerate(sets):
        for a in range(3):
            base[s, 2 * a, a], base[s, 2 * a + 1, a] = abc[a], -abc[a]
    axes = np.array(sets)
    if rotations is None:
        return base, det, axes
    rot = np.einsum("rij,skj->rski", rotations, base).reshape(-1, 6, 3)
    return rot, np.tile(det, len(rotations)), np.tile(axes, (len(rotations), 1))


def _flats(kind, n, K=8, seed=11):
    """n groups of K points in a plane through the origin (coordinates in a random 2-D basis), on a line, or K copies of one
    point -> shapes (n,K,3) float64"""
    rng = np.random.default_rng(seed)
    R = _rotations(n, seed + 1)
    x, y = rng.uniform(-1, 1, (n, K, 1)), rng.uniform(-1, 1, (n, K, 1))
    if kind == "plane":
        return x * R[:, None, :, 0] + y * R[:, None, :, 1]
    if kind == "line":
        return x * R[:, None, :, 0]
    return np.repeat(rng.uniform(-1, 1, (n, 1, 3)), K, 1)


def _shape_case(name, shapes, determined, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """one cloud of S groups of K points; the list of a point names its group, itself first, the others in cyclic order"""
    S, K, _ = shapes.shape
    pts = (scale * shapes + np.asarray(shift)).reshape(-1, 3).astype(np.float32)
    cyc = (np.arange(K)[:, None] + np.arange(K)[None, :]) % K
    idx = (K * np.arange(S)[:, None, None] + cyc[None]).reshape(S * K, K).astype(np.int64)
    det = np.repeat(np.broadcast_to(determined, (S,)), K)
    return Case(name, pts, idx, np.array([0], np.int64), np.array([S * K], np.int64), det)


def _grid_cases(family):
    """the family under every extent x translation -> list of (extent, shift, Case)"""
    if family == "octahedra":
        shapes, det, _ = _octahedra(_rotations(4, 5))
    else:
        shapes, det = _flats("plane", 40, seed=23), True
    return [(e, s, _shape_case("%s x %g + %s" % (family, e, s), shapes, det, e, s)) for e in EXTENTS for s in SHIFTS]


def _collapsed(case, base_ref):
    """whether fp32 rounding of the scaled, translated points has collapsed the shapes: decided on the fp32 points in the fp64
    reference -- a trace of zero, or a trace-normalised spectrum more than 1e-2 from the one of the shapes at extent 1 around
    the origin"""
    ref = _reference(case)
    tr = ref.lam.sum(1)
    if (tr <= 0).any():
        return True
    return bool(np.abs(ref.lam / tr[:, None] - base_ref.lam / base_ref.lam.sum(1)[:, None]).max() > 1e-2)


# ----------------------------------------------------------------------------------------------------------------------
# measured clouds (lists from a kNN search: `knn(pts, first, num, K)` -> (P,K) cloud-local ids)
# ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _teapot():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_setup_teapot.npz"))
    pts = np.ascontiguousarray(z["points"], np.float32)
    assert pts.shape == (7991, 3)
    return pts


@lru_cache(maxsize=None)
def _four_clouds():
    """four clouds of SIZES points -- a noisy sphere, five points, a slab, one point -- at different places, so that a
    neighbour looked up in the wrong cloud is a far point"""
    rng = np.random.default_rng(31)
    v = rng.normal(size=(SIZES[0], 3))
    sphere = 0.5 * v / np.linalg.norm(v, axis=1, keepdims=True) * (1 + 0.02 * rng.normal(size=(SIZES[0], 1)))
    five = rng.uniform(-0.1, 0.1, (SIZES[1], 3)) + [2.0, 0.0, -1.0]
    slab = rng.uniform(-0.4, 0.4, (SIZES[2], 3)) * [1.0, 1.0, 0.05] + [-1.5, 1.0, 0.5]
    one = np.array([[0.3, -0.7, 1.1]])
    clouds = tuple(c.astype(np.float32) for c in (sphere, five, slab, one))
    assert tuple(c.shape[0] for c in clouds) == SIZES and all(s % 64 for s in np.cumsum(SIZES))
    return clouds


def _pack(clouds, gaps=None):
    """packed layout with gaps[n] unused slots before cloud n and gaps[-1] behind the last one, holding NaN positions (nothing
    may read them) -> pts, first, num"""
    gaps = gaps or (0,) * (len(clouds) + 1)
    parts, first, at = [], [], 0
    for c, g in zip(clouds, gaps):
        parts.append(np.full((g, 3), np.nan, np.float32))
        first.append(at + g)
        parts.append(c)
        at += g + c.shape[0]
    parts.append(np.full((gaps[-1], 3), np.nan, np.float32))
    return np.concatenate(parts, 0), np.array(first, np.int64), np.array([c.shape[0] for c in clouds], np.int64)


def _knn_case(name, pts, first, num, K, knn):
    return Case(name, pts, knn(pts, first, num, K), first, num, None)


def all_cases(knn):
    """every case of this file (the yardstick behind B runs over them on the CPU, with a KD-tree as `knn`)"""
    out = [_shape_case("octahedra, axis-aligned", *_octahedra()[:2]),
           _shape_case("octahedra, rotated", *_octahedra(_rotations(16, 3))[:2])]
    out += [_shape_case(kind, _flats(kind, 40), True) for kind in ("plane", "line", "copies")]
    out += [c for fam in ("octahedra", "planes") for _, _, c in _grid_cases(fam)]
    out.append(_shape_case("octahedra x 1e-21", *_octahedra(_rotations(4, 5))[:2], scale=1e-21))
    out.append(_knn_case("four clouds", *_pack(_four_clouds()), 8, knn))
    out += [_knn_case("teapot K = %d" % K, _teapot(), np.array([0], np.int64), np.array([7991], np.int64), K, knn)
            for K in (2, 3, 8, 20)]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the kernel, the reference, the assertions
# ----------------------------------------------------------------------------------------------------------------------
def _gpu_knn(pts, first, num, K):
    return ops.knn_points(t(pts), t(first), t(num), K)[1].cpu().numpy()


def _run(case):
    out = ops.local_frames(t(case.pts), t(case.idx), t(case.first), t(case.num), return_curvature=True)
    return tuple(o.cpu().numpy() for o in out)


def _run_raw(case):
    """dss_local_frames through the C ABI like ops.local_frames, into outputs pre-filled with NaN"""
    lib = _lib.load()
    P_, I_, F_, N_ = t(case.pts), t(case.idx), t(case.first), t(case.num)
    dev = P_.device
    P, K = case.idx.shape
    with torch.cuda.device(dev):
        outs = [torch.full((P, w), float("nan"), dtype=torch.float32, device=dev) for w in (6, 3, 3)]
        rc = lib.dss_local_frames(_lib.ptr(P_), _lib.ptr(I_), _lib.ptr(F_), _lib.ptr(N_), len(case.first), P, int(K),
                                  _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.stream_ptr(dev))
    _lib.check(rc, "dss_local_frames")
    return tuple(o.cpu().numpy() for o in outs)


def _reference(case):
    return fr.local_frames_reference(case.pts, case.idx, case.first, case.num)


def _check(case, got, ref=None, bound=None):
    """Every assertion of the file on one case -> share of the live points whose vr6 the reference comparison skipped.
    `got` = (vr6, frame_n, curv) of the kernel."""
    bound = B if bound is None else bound
    ref = _reference(case) if ref is None else ref
    vr6, n, cv = (np.asarray(g, np.float64) for g in got)
    what = case.name
    for name, a in (("vr6", vr6), ("frame_n", n), ("curv", cv)):
        assert np.isfinite(a).all(), (what, name, "not finite at", np.flatnonzero(~np.isfinite(a).all(1))[:8])
    tr_all = np.trace(ref.C, axis1=1, axis2=2)
    live = ref.owned & (tr_all >= FLT_MIN)
    # slots that no cloud owns, traces of zero or below the normal range: the documented constants, exactly
    dead = ~live
    assert (vr6[dead] == fr.CONST_VR6).all() and (n[dead] == fr.CONST_NORMAL).all() and (cv[dead] == fr.CONST_CURV).all(), \
        (what, "constants", np.flatnonzero(dead)[:8])
    if not live.any():
        return 0.0
    vr6, n, cv, tr = vr6[live], n[live], cv[live], tr_all[live]
    C, lam, rvr6, e0 = ref.C[live], ref.lam[live], ref.vr6[live], ref.vec[live][:, :, 0]
    bt = bound * tr

    def below(x, lim, name):
        assert (x <= lim).all(), (what, name, "worst excess / tr %.3g" % float(((x - lim) / tr).max()),
                                  "at", int(np.argmax((x - lim) / tr)), "bound %.3g" % bound)
    # -- what holds whatever basis a degenerate eigenspace gets
    below(np.abs(np.linalg.norm(n, axis=1) - 1), bound, "|frame_n| = 1")
    assert (cv[:, 0] <= cv[:, 1]).all() and (cv[:, 1] <= cv[:, 2]).all(), (what, "curvatures ascend")
    below(-cv[:, 0], bt, "curvatures >= 0")
    below(np.abs(cv.sum(1) - tr), bt, "sum of the curvatures = trace")
    Vr = fr.mat33(vr6)
    below(np.linalg.norm(np.einsum("pab,pb->pa", Vr, n), axis=1), bt, "Vr e0 = 0")
    below(np.abs(np.trace(Vr, axis1=1, axis2=2) - (lam[:, 1] + lam[:, 2])), bt, "trace(Vr) = lam1 + lam2")
    below(-np.linalg.eigvalsh(Vr)[:, 0], bt, "Vr >= 0")
    below(np.einsum("pa,pab,pb->p", n, C, n) - lam[:, 0], bt, "e0 in the minimum eigenspace")
    # -- against the reference's values
    below(np.abs(cv - lam).max(1), bt, "curvatures")
    gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    by_gap, by_rank = gap > GAP, lam[:, 0] <= RANK * tr
    with np.errstate(divide="ignore"):
        tol = np.minimum(np.where(by_gap, bt / np.maximum(gap, 1e-300), np.inf),
                         np.where(by_rank, 2 * bt + 2 * np.abs(lam[:, 0]), np.inf))
    det = by_gap | by_rank
    below(np.abs(vr6 - rvr6).max(1)[det], tol[det], "vr6")
    g = gap[by_gap]
    assert (1 - np.abs((n * e0).sum(1))[by_gap] <= np.maximum((bound / g) ** 2, bound)).all(), (what, "frame_n")
    if case.determined is None:
        assert (~det).mean() <= 0.01, (what, "skipped share", float((~det).mean()))
    else:   # constructed: the comparison covers exactly the shapes it covers by construction
        assert np.array_equal(det, case.determined[live]), (what, "determined", int((det != case.determined[live]).sum()))
    return float((~det).mean())


# ----------------------------------------------------------------------------------------------------------------------
# degenerate spectra
# ----------------------------------------------------------------------------------------------------------------------
def test_axis_aligned_octahedra_pin_the_selection_in_every_ordering_and_tie():
    """Off-diagonal entries exactly zero: no rotation runs, V stays the identity, the result is the `m0 / m1` selection alone.
    The normal is exactly a coordinate axis, one of those with the smallest semi-axis; with a = b < c and a = b = c nothing
    else is determined, and everything `_check` asserts without a mask still holds."""
    shapes, det, axes = _octahedra()
    case = _shape_case("octahedra, axis-aligned", shapes, det)
    ref = _reference(case)
    assert np.abs(ref.C - np.repeat(np.stack([np.diag(a ** 2 / 3) for a in axes]), 6, 0)).max() <= 1e-15
    got = _run(case)
    skipped = _check(case, got, ref)
    assert skipped == float((~det).mean())
    n, ax = got[1], np.repeat(axes, 6, 0)
    assert ((np.abs(n) == 1).sum(1) == 1).all() and ((n == 0).sum(1) == 2).all()
    picked = np.abs(n).argmax(1)
    assert (ax[np.arange(len(ax)), picked] == ax.min(1)).all()
    assert set(picked[np.repeat(det, 6)]) == {0, 1, 2}    # every column is selected somewhere


def test_rotated_octahedra():
    """the same thirteen sets under sixteen random rotations: the Jacobi sweeps run, the spectra are known"""
    case = _shape_case("octahedra, rotated", *_octahedra(_rotations(16, 3))[:2])
    ref = _reference(case)
    want = np.sort(np.tile(np.array(_octa_axes()[0]) ** 2 / 3, (16, 1)), 1)
    assert np.abs(ref.lam - np.repeat(want, 6, 0)).max() <= 1e-6
    _check(case, _run(case), ref)


@pytest.mark.parametrize("kind", ["plane", "line", "copies"])
def test_flat_neighbourhoods(kind):
    """K = 8 points exactly (to fp32 rounding of the coordinates) in a plane, on a line, in one place: lam0 = 0, lam0 = lam1 = 0,
    trace = 0.  vr6 = C in the first two, the constants in the third."""
    case = _shape_case(kind, _flats(kind, 40), True)
    ref = _reference(case)
    tr = ref.lam.sum(1)
    if kind == "copies":
        assert (tr == 0).all()
    else:
        assert (ref.lam[:, 0] <= 1e-12 * tr).all() and ((ref.lam[:, 1] <= 1e-12 * tr) == (kind == "line")).all()
    if kind == "plane":   # the normal of every plane is compared
        assert ((ref.lam[:, 1] - ref.lam[:, 0]) / ref.lam[:, 2] > GAP).all()
    assert _check(case, _run(case), ref) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# scale and offset
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["octahedra", "planes"])
def test_extents_and_translations(family):
    """extents 1e-12 .. 1e3 around the origin and around 1e3 (1, -2, 3): the kernel subtracts the query point first, so a
    neighbourhood far from the origin costs nothing beyond the rounding of its coordinates.  Around the far point the two small
    extents are below the spacing of fp32 there (6e-5 .. 2.4e-4) and collapse; everything else is kept."""
    cases = _grid_cases(family)
    base_ref = _reference(next(c for e, s, c in cases if e == 1.0 and s == SHIFTS[0]))
    kept = []
    for e, s, case in cases:
        if _collapsed(case, base_ref):
            continue
        kept.append((e, s))
        _check(case, _run(case))
    assert kept == [(e, s) for e in EXTENTS for s in SHIFTS if s == SHIFTS[0] or e >= 1.0]


def test_trace_below_the_normal_range_gives_the_constants():
    """extent 1e-21 at the origin: the squares are denormal, the trace is (4.7e-42 .. 0), 1 / trace is not finite.  The entry
    point treats a trace below FLT_MIN as zero."""
    case = _shape_case("octahedra x 1e-21", *_octahedra(_rotations(4, 5))[:2], scale=1e-21)
    ref = _reference(case)
    tr = np.trace(ref.C, axis1=1, axis2=2)
    assert (tr > 0).all() and (tr < FLT_MIN).all() and (np.abs(case.pts).max(1) > 0).all()
    vr6, n, cv = _run(case)
    assert np.isfinite(vr6).all() and np.isfinite(n).all() and np.isfinite(cv).all()
    assert (vr6 == 0).all() and (n == [0, 0, 1]).all() and (cv == 0).all()
    _check(case, (vr6, n, cv), ref)


# ----------------------------------------------------------------------------------------------------------------------
# packed layouts
# ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _four_clouds_run():
    """the four clouds packed back to back, lists from dss_knn_points -> (case, reference, kernel outputs)"""
    case = _knn_case("four clouds", *_pack(_four_clouds()), 8, _gpu_knn)
    return case, _reference(case), _run(case)


def test_four_clouds_of_which_one_is_shorter_than_k_and_one_a_single_point():
    """(517, 5, 300, 1) points, K = 8: boundaries at 517, 522, 822 (no multiples of 64); the five-point cloud uses the first
    five entries of its zero-padded lists and divides by five; the single point has no extent and gets the constants"""
    case, ref, got = _four_clouds_run()
    first, num = case.first, case.num
    assert (case.idx[first[1]:first[1] + 5, 5:] == 0).all() and (np.sort(case.idx[first[1]:first[1] + 5, :5], 1) == np.arange(5)).all()
    _check(case, got, ref)
    # the five-point cloud: every point sees the whole cloud, so all five share one covariance (up to rounding)
    five = slice(int(first[1]), int(first[1] + 5))
    assert np.abs(ref.C[five] - ref.C[five][:1]).max() <= 1e-12
    c5 = _four_clouds()[1].astype(np.float64)
    assert np.allclose(ref.C[five][0], np.cov(c5.T, bias=True), rtol=1e-12, atol=1e-18)
    assert (got[0][-1] == 0).all() and (got[1][-1] == [0, 0, 1]).all() and (got[2][-1] == 0).all()


def test_unused_slots_around_the_clouds_hold_the_constants():
    """the same clouds with unused slots before, between and behind them (NaN positions), through the C ABI into outputs
    pre-filled with NaN: the slots of the clouds hold the bits of the dense layout, every other slot the constants"""
    dense, _, want = _four_clouds_run()
    gaps = (5, 70, 1, 130, 9)
    pts, first, num = _pack(_four_clouds(), gaps)
    covered = np.zeros(pts.shape[0], bool)
    idx = np.zeros((pts.shape[0], 8), np.int64)
    for f, n, f0 in zip(first, num, dense.first):
        covered[f:f + n] = True
        idx[f:f + n] = dense.idx[f0:f0 + n]
    assert (~covered).sum() == sum(gaps) and np.isnan(pts[~covered]).all() and not np.isnan(pts[covered]).any()
    assert np.array_equal(_gpu_knn(pts, first, num, 8)[covered], dense.idx)    # dss_knn_points gives the same lists here
    case = Case("four clouds with unused slots", pts, idx, first, num, None)
    got = _run_raw(case)
    _check(case, got)
    for g, w in zip(got, want):
        assert np.array_equal(g[covered], w)
    assert (got[0][~covered] == 0).all() and (got[1][~covered] == [0, 0, 1]).all() and (got[2][~covered] == 0).all()


def test_permuting_the_clouds_permutes_the_outputs_bit_for_bit():
    dense, _, want = _four_clouds_run()
    order = (2, 3, 1, 0)
    clouds = _four_clouds()
    pts, first, num = _pack([clouds[o] for o in order])
    rows = np.concatenate([np.arange(dense.first[o], dense.first[o] + dense.num[o]) for o in order])
    assert np.array_equal(pts, dense.pts[rows])
    case = Case("four clouds, permuted", pts, dense.idx[rows], first, num, None)
    got = _run(case)
    for g, w in zip(got, want):
        assert np.array_equal(g, w[rows])
    _check(case, got)


# ----------------------------------------------------------------------------------------------------------------------
# K
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 8, 20])
def test_teapot_at_every_k(K):
    """K = 2: rank 1 (lam0 = lam1 = 0), K = 3: rank <= 2 (lam0 = 0): vr6 = C there; 8 is what the rasterizer asks for, 20 a long
    sum.  No mask: the comparison with the reference skips at most 1 % of the points (asserted in `_check`)."""
    case = _knn_case("teapot K = %d" % K, _teapot(), np.array([0], np.int64), np.array([7991], np.int64), K, _gpu_knn)
    ref = _reference(case)
    tr = ref.lam.sum(1)
    if K <= 3:
        assert (ref.lam[:, 0] <= 1e-12 * tr).all()
    _check(case, _run(case), ref)


# ----------------------------------------------------------------------------------------------------------------------
# through the class
# ----------------------------------------------------------------------------------------------------------------------
def test_batch_of_two_different_clouds_equals_each_cloud_alone():
    """SurfaceSplatting in the anisotropic mode: 3,001 teapot points under one camera and 2,050 bunny points under another in
    one batch give, point for point, the bits of each cloud rendered alone -- the second cloud's lists are cloud-local and its
    points start at 3,001"""
    from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
    from dss_amd.cloud import PointClouds3D
    from dss_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting
    sizes = (3001, 2050)
    clouds = []
    for name, n in zip(("teapot", "bunny"), sizes):
        p, nr = scenes.load_cloud(name)
        clouds.append((t(scenes.normalize_unit_sphere(p)[:n]), t(nr[:n]), torch.ones(n, 3, device=DEV)))
    R, T = look_at_view_transform(2.0, [30.0, -10.0], [45.0, 200.0])
    st = PointsRasterizationSettings(cutoff_threshold=1.0, image_size=64, antialiasing_sigma=1.0, Vrk_invariant=False,
                                     Vrk_isotropic=False, points_per_pixel=5, backface_culling=False)

    def render(which):
        cams = FoVPerspectiveCameras(znear=0.1, R=R[which], T=T[which], device=DEV)
        cloud = PointClouds3D(*[[clouds[w][k] for w in which] for k in range(3)])
        frags, _, info = SurfaceSplatting(cameras=cams, raster_settings=st)(cloud, verbose=True)
        assert frags.occupancy.mean().item() > 0.02
        return {k: info[k] for k in ("radii", "ellipse_params", "scaler")}
    both, alone = render([0, 1]), [render([0]), render([1])]
    for k, v in both.items():
        assert v.shape[0] == sum(sizes) and bool(torch.isfinite(v).all()), k
        assert torch.equal(v[:sizes[0]], alone[0][k]), (k, "first cloud")
        assert torch.equal(v[sizes[0]:], alone[1][k]), (k, "second cloud")
