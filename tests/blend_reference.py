"""fp64 CPU reference of the forward blend (TEST INFRASTRUCTURE; plain numpy, no product code in the formulas).

What `ops.blend_forward` (`blend_forward_kernel`, `dss_amd/csrc/blend.hip`) and the fused epilogues of the fine pass
(`dss_amd/csrc/raster_forward.hip`: `epilogue_packed`, the packed-record one of `dss_render_forward` at K <= 8 and C = 3, and
the per-point-array one inside `fine_tile`, everywhere else and in `dss_splat_fine_blend`) compute, each ENTRY with the sum of its ABSOLUTE terms
next to it.  Per pixel with the fragment slots k < K, a slot live when idx_k >= 0:

    w_k    = exp(-q_k / 2) scaler[idx_k]                 (live slots; 0 otherwise)
    cum    = max(sum_k w_k, float32(1e-4))
    img_ch = sum_k feat[idx_k, ch] w_k / cum             A_ch = sum_k |feat[idx_k, ch] w_k / cum|
    alpha  = the occupancy of the pixel, copied (channel C of `img`)       A = |occupancy|
    wsum   = cum                                          A_wsum = cum

Nothing here is a decision: the floor is a `max` and continuous, every slot is tested on its own, so no entry is left out of
any comparison.  Signed features (shaded colours, normals) cancel, which is why the error of a kernel is measured
against ``A`` of the entry and not against the entry or the whole image.

``dtype=np.float32`` evaluates the kernels' documented arithmetic in plain fp32, every operation rounded and the sums
sequential: ``w = exp2(float32(-0.72134752) q) scaler`` (`ewa_weight`, `csrc/common.h`), ONE reciprocal of cum, and
``feat (w rcp)``.  (Not ``exp(-q / 2)``: at q = 16 the rounding of the exponent's argument, 11.5 with an ulp of 9.5e-7, is
the largest single term of the error, 3e-7 of w.)  A bar is 4 x the largest |fp32 - fp64| / A of the case, rounded up to
one significant digit (`BARS`).  ``mut`` names one of `MUTATIONS`, a wrong formula that `tests/test_blend_reference_cpu.py`
shows to lie at least 10 x beyond the bars.
"""
import functools
import math
import os
import sys
from collections import namedtuple

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:          # `oracle` and `dss_amd` for `print_bars` run from tests/ (under pytest the conftest did it)
    sys.path.insert(0, _ROOT)

from shading_reference import UNDERFLOW, entry_ratio, round_up_1sig  # noqa: F401  (the tests' check)

F32, F64 = np.float32, np.float64
OUTPUTS = ("img", "wsum")
FLOOR = F32(1e-4)
BAR_CAP = 1e-5          # no bar may exceed it: a larger one means that a case or the restatement is wrong
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Ref = namedtuple("Ref", "img img_A wsum wsum_A")


def _seq_sum(t, axis=-1):
    """fp32 sum along an axis, one addition after the other"""
    return np.take(np.cumsum(t, axis=axis, dtype=F32), -1, axis=axis)


def reference(idx, qv, occ, scaler, feat, dtype=F64, mut=None):
    """idx int32 (..., K), qv fp32 (..., K), occ fp32 (...), scaler fp32 (P,), feat fp32 (P, C) ->
    Ref(img (..., C + 1), its A, wsum (...), its A), all fp64 arrays (holding fp32 values with ``dtype=np.float32``)"""
    K, C = idx.shape[-1], feat.shape[1]
    ok = idx >= 0
    if mut == "stop_at_hole":
        ok = np.cumprod(ok, axis=-1).astype(bool)
    elif mut == "tail_dropped":
        ok = ok & (np.arange(K) < 4 * (K // 4))
    pc = np.where(ok, idx, 0)
    q = qv.astype(dtype)
    if mut == "q_neighbour":
        q = np.roll(q, 1, axis=-1)
    sc = np.ones(pc.shape, dtype) if mut == "no_scaler" else scaler[pc].astype(dtype)
    if mut == "exp_const":
        e = np.exp2(dtype(-0.7213) * q)
    elif dtype is F64:
        e = np.exp(-0.5 * q)
    else:
        e = np.exp2(F32(-0.72134752) * q)
    w = np.where(ok, e * sc, dtype(0))
    raw = w.sum(-1) if dtype is F64 else _seq_sum(w)
    if mut == "no_clamp":
        cum = np.where(raw > 0, raw, dtype(1))
    else:
        cum = np.maximum(raw, dtype(F32(1e-5)) if mut == "clamp_1e5" else dtype(FLOOR))
    if mut in ("feat_stride8", "feat_stride3"):
        flat, stride = feat.reshape(-1), int(mut[-1])
        f = flat[(pc[..., None] * stride + np.arange(C)) % flat.size].astype(dtype)
    else:
        f = feat[pc].astype(dtype)                                   # (..., K, C)
    if mut == "unnormalised":
        wn = w
    elif dtype is F64:
        wn = w / cum[..., None]
    else:
        wn = w * (F32(1) / cum)[..., None]
    term = f * wn[..., None]
    assert term.dtype == dtype and cum.dtype == dtype
    rgb = term.sum(-2) if dtype is F64 else _seq_sum(term, axis=-2)
    alpha = ok.any(-1).astype(dtype) if mut == "alpha_any_slot" else occ.astype(dtype)
    img = np.concatenate([rgb, alpha[..., None]], -1).astype(F64)
    img_A = np.concatenate([np.abs(term.astype(F64)).sum(-2), np.abs(occ.astype(F64))[..., None]], -1)
    wsum = (raw if mut == "wsum_unclamped" else cum).astype(F64)
    return Ref(img, img_A, wsum, cum.astype(F64))


# ---------------------------------------------------------------------------------------------------------------------
# the cases that tests/test_blend_reference_cpu.py and tests/test_gpu_blend_forward.py share; every case is built from seeds.
# kind "frag": the fragments themselves are drawn; "splat": `scenes.random_splats` through the oracle's splat (scene = its
# inputs and the merge threshold); "camera": a cloud through the oracle's setup and splat (scene = what `ops.render_forward`
# takes); "golden": the reference project's recorded fragments (tests/golden/ref_*.npz)
Case = namedtuple("Case", "name kind N S K C P idx qv occ scaler feat scene")

FRAG_N, FRAG_S, FRAG_P = 2, 40, 500      # 3200 pixels = 12.5 blocks of 256: the last block is ragged
FRAG_KS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 33, 150)
FRAG_CS = (1, 2, 3, 4, 5, 8)
SPLAT_KS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 24, 25, 32)
SPLAT_THR = 1.0
CAMERA_KC = tuple((k, 3) for k in range(1, 9)) + ((5, 5), (8, 1), (9, 3), (12, 3), (16, 8), (17, 3), (32, 3))
GOLDEN_CASES = ("ref_random64x2", "ref_teapot256", "ref_ties32")


def _log_uniform(rng, n):
    return (10.0 ** rng.uniform(-6.0, 2.0, n)).astype(F32)


def _features(rng, P, C, signed):
    return (rng.standard_normal((P, C)) if signed else rng.uniform(0.0, 1.0, (P, C))).astype(F32)


def _fragments(rng, K):
    """lists of a random length 0 .. K of random points, q uniform in [0, 16] -> idx, qv, occ"""
    shape = (FRAG_N, FRAG_S, FRAG_S)
    length = rng.integers(0, K + 1, shape)
    live = np.arange(K) < length[..., None]
    idx = np.where(live, rng.integers(0, FRAG_P, shape + (K,)), -1).astype(np.int32)
    qv = np.where(live, rng.uniform(0.0, 16.0, shape + (K,)), -1.0).astype(F32)
    return idx, qv, (length > 0).astype(F32)


def _frag_case(name, seed, K, C, signed):
    rng = np.random.default_rng(seed)
    idx, qv, occ = _fragments(rng, K)
    return Case(name, "frag", FRAG_N, FRAG_S, K, C, FRAG_P, idx, qv, occ, _log_uniform(rng, FRAG_P), _features(rng, FRAG_P, C, signed), None)


def _holes_case(name):
    """-1 slots in the MIDDLE of the lists (the foreign compositor convention hands such lists over); the occupancy is that
    of slot 0, so a pixel whose first slot is dead has alpha 0 and colours"""
    c = _frag_case(name, 700, 8, 3, True)
    rng = np.random.default_rng(701)
    dead = rng.random(c.idx.shape) < 0.3
    idx, qv = np.where(dead, -1, c.idx).astype(np.int32), np.where(dead, F32(-1), c.qv)
    return c._replace(idx=idx, qv=qv, occ=(idx[..., 0] >= 0).astype(F32))


def _ulps(x, n):
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf if n > 0 else -np.inf), dtype=F32)
    return x


FLOOR_PLANTED = 40      # pixels per planted class of the `floor` case


def _floor_case(name):
    """K = 5, C = 3 fragments with planted pixels (q = 0 in the planted slots: the weight is the scaler, exactly) whose fp64
    weight sum is well below the floor (points 16 .. 23, scaler about 1e-6, one to three slots), within 1e-6 of it below
    and above (ONE slot of the points 0 .. 7 / 8 .. 15, the floor -+ 1 .. 8 ulp; TWO slots of the points 24 .. 31, half the
    floor -+ 0 .. 3 ulp), well above it (the drawn pixels) and absent (emptied pixels)"""
    c = _frag_case(name, 710, 5, 3, True)
    rng = np.random.default_rng(711)
    scaler, idx, qv, occ = c.scaler.copy(), c.idx.copy().reshape(-1, 5), c.qv.copy().reshape(-1, 5), c.occ.copy().reshape(-1)
    for j in range(8):
        scaler[j], scaler[8 + j] = _ulps(FLOOR, -(j + 1)), _ulps(FLOOR, j + 1)
        scaler[16 + j] = F32(1e-6 * (1 + j))
        scaler[24 + j] = _ulps(0.5 * float(FLOOR), j - 4)
    pix = rng.permutation(idx.shape[0])[:6 * FLOOR_PLANTED].reshape(6, FLOOR_PLANTED)

    def plant(rows, lists):
        for i, pts in zip(rows, lists):
            idx[i], qv[i], occ[i] = -1, F32(-1), F32(len(pts) > 0)
            idx[i, :len(pts)], qv[i, :len(pts)] = pts, F32(0)
    plant(pix[0], [16 + rng.integers(0, 8, 1 + j % 3) for j in range(FLOOR_PLANTED)])
    plant(pix[1], [[j % 8] for j in range(FLOOR_PLANTED)])
    plant(pix[2], [[8 + j % 8] for j in range(FLOOR_PLANTED)])
    plant(pix[3], [24 + rng.integers(0, 8, 2) for _ in range(FLOOR_PLANTED)])
    plant(pix[4], [[] for _ in range(FLOOR_PLANTED)])
    return c._replace(idx=idx.reshape(c.idx.shape), qv=qv.reshape(c.qv.shape), occ=occ.reshape(c.occ.shape), scaler=scaler)


@functools.lru_cache(maxsize=None)
def _splat_scene(K):
    """`scenes.random_splats(600, 40, 2)` with x and y cubed towards the image centre -- the lists are then one or two
    fragments long near the borders (sums below the floor) and full in the middle at every K up to 32 -- through the
    oracle's splat; the scaler is the log-uniform draw"""
    import oracle
    import scenes
    sc = scenes.random_splats(600, FRAG_S, 2, seed=K)
    xy = sc["points"][:, :2].astype(F64) / 1.05
    sc["points"][:, :2] = (1.05 * np.sign(xy) * np.abs(xy) ** 3).astype(F32)
    sc["scaler"] = _log_uniform(np.random.default_rng(100 + K), sc["points"].shape[0])
    idx, _z, qv, occ = oracle.splat_forward(sc["points"], sc["ellipse"], sc["cutoff"], sc["radii"], sc["first_idx"], sc["num_pts"],
                                            FRAG_S, K, SPLAT_THR)
    sc["thr"] = SPLAT_THR
    return sc, idx, qv, occ


def _splat_case(name, K, C, signed):
    sc, idx, qv, occ = _splat_scene(K)
    P = sc["points"].shape[0]
    return Case(name, "splat", 2, FRAG_S, K, C, P, idx, qv, occ, sc["scaler"], _features(np.random.default_rng(200 + 10 * K + C), P, C, signed), sc)


@functools.lru_cache(maxsize=None)
def _camera_world(which):
    """-> what `ops.render_forward` takes: world points, normals, M, V, h, cutoff threshold, merge threshold, S"""
    import scenes
    if which == "teapot":
        pts, nrm = scenes.load_cloud("teapot")
        pts = scenes.normalize_unit_sphere(pts)
        M, V, _ = scenes.camera_matrices(2.0, 30.0, [45.0, 145.0])
        cutoff = 1.0
    else:
        # a disc in the plane y = 0 seen from one degree above it: the splats are slivers, cut off at q = 16, and their
        # weights reach the floor through the real setup
        u = np.random.default_rng(0).random((300, 2))
        r, th = np.sqrt(u[:, 0]), 2 * np.pi * u[:, 1]
        pts = np.stack([r * np.cos(th), np.zeros(300), r * np.sin(th)], 1).astype(F32)
        nrm = np.tile(np.array([[0.0, 1.0, 0.0]], F32), (300, 1))
        M, V, _ = scenes.camera_matrices(12.0, 1.0, 30.0)
        cutoff = 16.0
    return dict(world=pts, normals=nrm, M=M, V=V, h=scenes.global_h(pts), cutoff=cutoff, thr=0.05, S=64, znear=0.1, zfar=100.0)


@functools.lru_cache(maxsize=None)
def _camera_setup(which):
    import scenes
    w = _camera_world(which)
    sc = scenes.setup_scene(w["world"], w["normals"], w["M"], w["V"], w["S"], cutoff=w["cutoff"], h=w["h"])
    assert (sc["num_pts"] == w["world"].shape[0]).all()          # nothing is culled: packed point n Pw + i is world point i
    return sc


@functools.lru_cache(maxsize=None)
def _camera_fragments(which, K):
    import oracle
    w, sc = _camera_world(which), _camera_setup(which)
    idx, _z, qv, occ = oracle.splat_forward(sc["points"], sc["ellipse"], sc["cutoff"], sc["radii"], sc["first_idx"], sc["num_pts"],
                                            w["S"], K, w["thr"])
    return idx, qv, occ


def camera_features(which, K, C):
    """the packed (P, C) features of a camera case: per world point, repeated per camera; signed where K + C is odd"""
    w = _camera_world(which)
    f = _features(np.random.default_rng(300 + 10 * K + C), w["world"].shape[0], C, (K + C) % 2 == 1)
    return np.tile(f, (w["M"].shape[0], 1))


def _camera_case(name, which, K, C):
    w, sc = _camera_world(which), _camera_setup(which)
    idx, qv, occ = _camera_fragments(which, K)
    return Case(name, "camera", w["M"].shape[0], w["S"], K, C, sc["points"].shape[0], idx, qv, occ, sc["scaler"],
                camera_features(which, K, C), dict(w, which=which))


def _golden_case(name):
    z = np.load(os.path.join(_GOLDEN, name + ".npz"))
    idx, feat = z["ref_idx"], z["colors"].astype(F32)
    return Case(name, "golden", idx.shape[0], idx.shape[1], idx.shape[3], feat.shape[1], feat.shape[0], idx, z["ref_qvalue"],
                z["ref_occ"], z["scaler"].astype(F32), feat, None)


def _builders():
    b, n = {}, 0
    for K, C in [(K, C) for C in (3, 5) for K in FRAG_KS] + [(K, C) for K in (5, 13) for C in FRAG_CS if C not in (3, 5)]:
        b["frag_k%d_c%d" % (K, C)] = functools.partial(_frag_case, seed=500 + n, K=K, C=C, signed=n % 2 == 1)
        n += 1
    b["holes"], b["floor"] = _holes_case, _floor_case
    for j, K in enumerate(SPLAT_KS):
        for C in (3, (1, 2, 4, 5, 8)[j % 5]):
            b["splat_k%d_c%d" % (K, C)] = functools.partial(_splat_case, K=K, C=C, signed=(j + (C != 3)) % 2 == 1)
    for which in ("teapot", "grazing"):
        for K, C in CAMERA_KC:
            b["%s_k%d_c%d" % (which, K, C)] = functools.partial(_camera_case, which=which, K=K, C=C)
    for name in GOLDEN_CASES:
        b[name] = _golden_case
    return b


_BUILDERS = _builders()
CASES = tuple(_BUILDERS)
FRAGMENT_CASES = tuple(n for n in CASES if n.startswith("frag_") or n in ("holes", "floor"))
SPLAT_CASES = tuple(n for n in CASES if n.startswith("splat_"))
CAMERA_CASES = tuple(n for n in CASES if n.startswith(("teapot_", "grazing_")))
FLOOR_CASES = ("floor",) + SPLAT_CASES + tuple(n for n in CAMERA_CASES if n.startswith("grazing_"))


def camera_name(which, K, C):
    return "%s_k%d_c%d" % (which, K, C)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name](name)
    assert c.idx.dtype == np.int32 and c.qv.dtype == F32 and c.occ.dtype == F32 and c.scaler.dtype == F32 and c.feat.dtype == F32
    assert c.idx.shape == (c.N, c.S, c.S, c.K) and c.feat.shape == (c.P, c.C) and int(c.idx.max()) < c.P
    for a in c:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def reference_of(c, dtype=F64, mut=None):
    return reference(c.idx, c.qv, c.occ, c.scaler, c.feat, dtype, mut)


@functools.lru_cache(maxsize=None)
def ref(name):
    """the fp64 reference of a case, cached for the module"""
    return reference_of(case(name))


def weight_sum64(c):
    """the fp64 weight sum of every pixel BEFORE the floor (what the per-case counts are taken from)"""
    ok = c.idx >= 0
    return np.where(ok, np.exp(-0.5 * c.qv.astype(F64)) * c.scaler[np.where(ok, c.idx, 0)].astype(F64), 0.0).sum(-1)


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def ratio(got, want, A):
    """`entry_ratio` on numpy arrays or tensors -> (largest (|got - want| - UNDERFLOW) / A, zeros exact where A == 0)"""
    return entry_ratio(_t(got), _t(want).double(), _t(A).double())


def figures_of(r64, r32):
    """the largest |fp32 restatement - fp64| / A per output of `OUTPUTS` (what a bar is 4 x of)"""
    figs = {}
    for key in OUTPUTS:
        fig, zeros_ok = ratio(getattr(r32, key), getattr(r64, key), getattr(r64, key + "_A"))
        assert zeros_ok, key
        figs[key] = fig
    return figs


def case_figures(name):
    return figures_of(ref(name), reference_of(case(name), F32))


def bars_of(figs):
    return {k: round_up_1sig(4 * v) for k, v in figs.items()}


def violation(got, want, A, bar):
    """by what factor the worst entry of ``got`` misses ``|got - want| <= bar A + UNDERFLOW`` (inf: a non-zero entry where no
    term exists); <= 1 passes"""
    worst, zeros_ok = ratio(got, want, A)
    if not zeros_ok or (bar == 0 and worst > 0):
        return math.inf
    return worst / bar if bar > 0 else 0.0


def print_bars():
    """`python -c "import blend_reference as b; b.print_bars()"` in tests/: the table below, measured anew"""
    for name in CASES:
        b = bars_of(case_figures(name))
        print("    %r: dict(%s)," % (name, ", ".join("%s=%s" % (k, "%.0e" % b[k] if b[k] else "0") for k in OUTPUTS)))


# which cases each wrong formula must show on (at least 10 x beyond the bar on at least one entry of EVERY listed case), and
# the output it shows in
_KC = ("frag_k5_c3", "frag_k13_c5", "frag_k150_c3", "splat_k8_c3", "splat_k32_c3", "teapot_k5_c3", "teapot_k12_c3")
_GRAZING = tuple(n for n in CAMERA_CASES if n.startswith("grazing_"))
_C_CASES = tuple("frag_k%d_c%d" % (K, C) for K in (5, 13) for C in FRAG_CS)
MUTATIONS = {
    "no_scaler": ("wsum", _KC),
    "exp_const": ("wsum", _KC),
    "q_neighbour": ("img", _KC),
    "no_clamp": ("img", ("floor",) + _GRAZING),
    "clamp_1e5": ("img", ("floor",) + _GRAZING),
    "unnormalised": ("img", _KC),
    "stop_at_hole": ("img", ("holes",)),
    "tail_dropped": ("img", tuple(n for n in CASES if n.startswith(("frag_", "splat_")) and int(n.split("_")[1][1:]) % 4)),
    "feat_stride8": ("img", tuple(n for n in _C_CASES if not n.endswith("_c8"))),
    "feat_stride3": ("img", tuple(n for n in _C_CASES if not n.endswith("_c3"))),
    "alpha_any_slot": ("img", ("holes",)),
    "wsum_unclamped": ("wsum", ("floor", "splat_k1_c3", "splat_k32_c3") + _GRAZING),
}

# ---------------------------------------------------------------------------------------------------------------------
# The bars of tests/test_gpu_blend_forward.py: 4 x the largest |err| / A of the fp32 restatement against fp64, rounded up to one
# significant digit; tests/test_blend_reference_cpu.py re-measures the figures and asserts the tie.
BARS = {
    'frag_k1_c3': dict(img=3e-06, wsum=2e-06),
    'frag_k2_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k3_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k4_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k5_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k7_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k8_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k9_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k12_c3': dict(img=2e-06, wsum=3e-06),
    'frag_k13_c3': dict(img=2e-06, wsum=3e-06),
    'frag_k16_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k33_c3': dict(img=2e-06, wsum=2e-06),
    'frag_k150_c3': dict(img=4e-06, wsum=3e-06),
    'frag_k1_c5': dict(img=3e-06, wsum=2e-06),
    'frag_k2_c5': dict(img=2e-06, wsum=3e-06),
    'frag_k3_c5': dict(img=2e-06, wsum=2e-06),
    'frag_k4_c5': dict(img=2e-06, wsum=3e-06),
    'frag_k5_c5': dict(img=2e-06, wsum=2e-06),
    'frag_k7_c5': dict(img=3e-06, wsum=2e-06),
    'frag_k8_c5': dict(img=2e-06, wsum=2e-06),
    'frag_k9_c5': dict(img=2e-06, wsum=2e-06),
    'frag_k12_c5': dict(img=2e-06, wsum=3e-06),
    'frag_k13_c5': dict(img=2e-06, wsum=3e-06),
    'frag_k16_c5': dict(img=3e-06, wsum=2e-06),
    'frag_k33_c5': dict(img=3e-06, wsum=2e-06),
    'frag_k150_c5': dict(img=4e-06, wsum=3e-06),
    'frag_k5_c1': dict(img=2e-06, wsum=3e-06),
    'frag_k5_c2': dict(img=2e-06, wsum=2e-06),
    'frag_k5_c4': dict(img=3e-06, wsum=2e-06),
    'frag_k5_c8': dict(img=2e-06, wsum=3e-06),
    'frag_k13_c1': dict(img=2e-06, wsum=2e-06),
    'frag_k13_c2': dict(img=2e-06, wsum=2e-06),
    'frag_k13_c4': dict(img=2e-06, wsum=2e-06),
    'frag_k13_c8': dict(img=2e-06, wsum=2e-06),
    'holes': dict(img=2e-06, wsum=2e-06),
    'floor': dict(img=2e-06, wsum=2e-06),
    'splat_k1_c3': dict(img=9e-07, wsum=6e-07),
    'splat_k1_c1': dict(img=8e-07, wsum=6e-07),
    'splat_k2_c3': dict(img=8e-07, wsum=7e-07),
    'splat_k2_c2': dict(img=2e-06, wsum=7e-07),
    'splat_k3_c3': dict(img=9e-07, wsum=7e-07),
    'splat_k3_c4': dict(img=9e-07, wsum=7e-07),
    'splat_k4_c3': dict(img=1e-06, wsum=8e-07),
    'splat_k4_c5': dict(img=2e-06, wsum=8e-07),
    'splat_k5_c3': dict(img=2e-06, wsum=8e-07),
    'splat_k5_c8': dict(img=2e-06, wsum=8e-07),
    'splat_k6_c3': dict(img=2e-06, wsum=9e-07),
    'splat_k6_c1': dict(img=2e-06, wsum=9e-07),
    'splat_k7_c3': dict(img=2e-06, wsum=9e-07),
    'splat_k7_c2': dict(img=2e-06, wsum=9e-07),
    'splat_k8_c3': dict(img=2e-06, wsum=9e-07),
    'splat_k8_c4': dict(img=2e-06, wsum=9e-07),
    'splat_k9_c3': dict(img=2e-06, wsum=2e-06),
    'splat_k9_c5': dict(img=2e-06, wsum=2e-06),
    'splat_k12_c3': dict(img=2e-06, wsum=2e-06),
    'splat_k12_c8': dict(img=2e-06, wsum=2e-06),
    'splat_k13_c3': dict(img=2e-06, wsum=2e-06),
    'splat_k13_c1': dict(img=2e-06, wsum=2e-06),
    'splat_k16_c3': dict(img=2e-06, wsum=1e-06),
    'splat_k16_c2': dict(img=2e-06, wsum=1e-06),
    'splat_k17_c3': dict(img=2e-06, wsum=2e-06),
    'splat_k17_c4': dict(img=2e-06, wsum=2e-06),
    'splat_k24_c3': dict(img=2e-06, wsum=2e-06),
    'splat_k24_c5': dict(img=2e-06, wsum=2e-06),
    'splat_k25_c3': dict(img=3e-06, wsum=2e-06),
    'splat_k25_c8': dict(img=3e-06, wsum=2e-06),
    'splat_k32_c3': dict(img=2e-06, wsum=2e-06),
    'splat_k32_c1': dict(img=2e-06, wsum=2e-06),
    'teapot_k1_c3': dict(img=5e-07, wsum=6e-07),
    'teapot_k2_c3': dict(img=8e-07, wsum=6e-07),
    'teapot_k3_c3': dict(img=1e-06, wsum=6e-07),
    'teapot_k4_c3': dict(img=9e-07, wsum=6e-07),
    'teapot_k5_c3': dict(img=9e-07, wsum=6e-07),
    'teapot_k6_c3': dict(img=9e-07, wsum=7e-07),
    'teapot_k7_c3': dict(img=1e-06, wsum=6e-07),
    'teapot_k8_c3': dict(img=9e-07, wsum=7e-07),
    'teapot_k5_c5': dict(img=1e-06, wsum=6e-07),
    'teapot_k8_c1': dict(img=2e-06, wsum=7e-07),
    'teapot_k9_c3': dict(img=2e-06, wsum=7e-07),
    'teapot_k12_c3': dict(img=1e-06, wsum=7e-07),
    'teapot_k16_c8': dict(img=2e-06, wsum=7e-07),
    'teapot_k17_c3': dict(img=2e-06, wsum=7e-07),
    'teapot_k32_c3': dict(img=9e-07, wsum=7e-07),
    'grazing_k1_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k2_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k3_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k4_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k5_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k6_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k7_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k8_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k5_c5': dict(img=2e-06, wsum=2e-06),
    'grazing_k8_c1': dict(img=2e-06, wsum=2e-06),
    'grazing_k9_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k12_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k16_c8': dict(img=2e-06, wsum=2e-06),
    'grazing_k17_c3': dict(img=2e-06, wsum=2e-06),
    'grazing_k32_c3': dict(img=2e-06, wsum=2e-06),
    'ref_random64x2': dict(img=9e-07, wsum=6e-07),
    'ref_teapot256': dict(img=1e-06, wsum=7e-07),
    'ref_ties32': dict(img=1e-06, wsum=5e-07),
}
