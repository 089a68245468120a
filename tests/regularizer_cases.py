"""Inputs of the regulariser tests: packed batches with CPU-built neighbour lists, shared by the float64 fixture
(tests/golden/make_golden_losses_f64.py), the CPU tests (bars, mutations) and the GPU tests.

Every case is a dict: points, normals (P,3) float32; first, num (N,) int64; K; sigma; filter_scale; visible, inmask (P,)
bool or None (keep = visible & inmask); sigma and filter_scale are float32 values too (0.05 is not 0.05f); gl1 (P,), gl3 (P,3) float32 upstream gradients or None; knn_d2 float32 (P,K)
and knn_idx int64 (P,K) from `regularizer_reference.brute_knn`.  Rows no cloud owns carry arbitrary finite values.
"""
import functools

import numpy as np

import regularizer_reference as rr


def sphere(rng, n, centre=(0.0, 0.0, 0.0), radius=1.0, noise=0.01):
    """A noisy sphere with noisy normals of length 0.5 to 1.5 (the optimiser does not keep them unit length)."""
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.asarray(centre) + radius * (d * (1 + rng.normal(0, noise, (n, 1))))
    nrm = d * rng.uniform(0.5, 1.5, (n, 1)) + rng.normal(0, 0.15, (n, 3))
    return pts.astype(np.float32), nrm.astype(np.float32)


def pack(rng, clouds, K, sigma=0.75, filter_scale=2.0, gaps=None, masks=True, grads=True):
    """clouds: list of (points, normals); gaps: {cloud index: unowned rows inserted before it}"""
    gaps = gaps or {}
    pts, nrm, first, num, at = [], [], [], [], 0
    for b, (p, n) in enumerate(clouds):
        g = gaps.get(b, 0)
        if g:
            pts.append(rng.normal(0, 1, (g, 3)).astype(np.float32)); nrm.append(rng.normal(0, 1, (g, 3)).astype(np.float32))
            at += g
        first.append(at); num.append(len(p)); at += len(p)
        pts.append(np.asarray(p, np.float32).reshape(-1, 3)); nrm.append(np.asarray(n, np.float32).reshape(-1, 3))
    case = {"points": np.concatenate(pts), "normals": np.concatenate(nrm), "first": np.array(first, np.int64),
            "num": np.array(num, np.int64), "K": K, "sigma": float(np.float32(sigma)), "filter_scale": float(np.float32(filter_scale))}
    P = at
    case["visible"] = rng.random(P) < 0.6 if masks else None
    case["inmask"] = rng.random(P) < 0.8 if masks else None
    case["gl1"] = rng.normal(0, 1, P).astype(np.float32) if grads else None
    case["gl3"] = rng.normal(0, 1, (P, 3)).astype(np.float32) if grads else None
    return finish(case)


def finish(case):
    case["knn_d2"], case["knn_idx"] = rr.brute_knn(case["points"], case["first"], case["num"], case["K"])
    return case


def keep_of(case):
    return None if case["visible"] is None else case["visible"] & case["inmask"]


def constructed_clouds(rng):
    """Small clouds that put single rows off the well-conditioned path (every normal here is kept: see constructed())"""
    z = np.array([0, 0, 1.0])
    ring = np.stack([np.cos(np.arange(12) * 0.5), np.sin(np.arange(12) * 0.5), 0.1 * np.arange(12)], 1)
    opposite = (np.concatenate([[[0, 0, 0.05]], ring]), np.concatenate([[z], np.tile(-z, (12, 1))]))     # row 0: every weight underflows at sigma 0.05
    zero_n = sphere(rng, 13, radius=0.3)
    zero_n[1][4] = 0                                                                                     # a zero normal
    tight = rng.normal(0, 0.01, (11, 3))
    outlier = (np.concatenate([tight, [[0.2, 0.1, 0.0]]]), sphere(rng, 12)[1])                           # phi == 0 for the far neighbour
    coincident = (np.tile([[0.25, -0.5, 0.125]], (12, 1)), sphere(rng, 12)[1])                           # h == 0
    return [opposite, zero_n, outlier, coincident]


def constructed(sigma):
    rng = np.random.default_rng(31)
    case = pack(rng, [sphere(rng, 150)] + constructed_clouds(rng), 12, sigma=sigma)
    own = case["first"][1]
    case["visible"][own:] = True      # the constructed clouds keep their normals, so the rows are what they were built as
    case["inmask"][own:] = True
    case["visible"][own + 3] = False  # one invisible neighbour among them
    case["visible"][-6:] = False      # half of the coincident cloud is mollified: NaN normals (h == 0)
    return case


def collinear():
    """K = 3: a generic cloud and an evenly spaced collinear triple with one normal; the middle point has r == 0."""
    rng = np.random.default_rng(32)
    triple = (np.array([[-0.25, 0, 0], [0, 0, 0], [0.25, 0, 0]]), np.tile([[0, 0, 0.5]], (3, 1)))
    case = pack(rng, [sphere(rng, 100), triple], 3)
    case["visible"][100:] = True
    case["inmask"][100:] = True
    return case


def _single(P, K, seed, sigma=0.75, filter_scale=2.0, **kw):
    rng = np.random.default_rng(seed)
    return pack(rng, [sphere(rng, P, **kw)], K, sigma, filter_scale)


def _ragged():
    rng = np.random.default_rng(21)
    sizes = (257, 0, 5, 1, 700)
    return pack(rng, [sphere(rng, n, centre=(0.3 * b, 0, 0), radius=1.0 + 0.2 * b) for b, n in enumerate(sizes)], 12)


def _gap():
    rng = np.random.default_rng(22)
    return pack(rng, [sphere(rng, 130), sphere(rng, 90, centre=(0.5, 0.2, 0), radius=0.6)], 12, gaps={1: 3})


def _without(name, *keys):
    case = dict(CASES[name]())
    for k in keys:
        case[k] = None
    return case


def _fixture_a(K, sigma, filter_scale):
    rng = np.random.default_rng(40)
    return pack(rng, [sphere(rng, 300), sphere(rng, 129, centre=(0.2, 0, -0.1), radius=0.8)], K, sigma, filter_scale)


def _fixture_b():
    rng = np.random.default_rng(41)
    return pack(rng, [sphere(rng, 5), sphere(rng, 1)], 12)


CASES = {   # the cases of tests/test_gpu_regularizers.py
    "P255": lambda: _single(255, 12, 1),
    "P256": lambda: _single(256, 12, 2),
    "P257": lambda: _single(257, 12, 3),
    "K2": lambda: _single(300, 2, 4),
    "K13": lambda: _single(300, 13, 5),
    "K40": lambda: _single(300, 40, 6, sigma=0.5, filter_scale=1.0),
    "ragged": _ragged,
    "gap": _gap,
    "constructed": lambda: constructed(0.75),
    "constructed_sharp": lambda: constructed(0.05),
    "collinear": collinear,
    "offset": lambda: _single(300, 12, 7, centre=(50.0, -30.0, 20.0), radius=1e-3 * np.sqrt(300 / (4 * np.pi))),
    "no_masks": lambda: _without("P257", "visible", "inmask"),
    "no_grad_loss": lambda: _without("P257", "gl1", "gl3"),
}
FIXTURE_CASES = {   # the cases of tests/golden/ref_losses_f64.npz
    "a_k12": lambda: _fixture_a(12, 0.75, 2.0),
    "a_k40": lambda: _fixture_a(40, 0.5, 1.0),
    "b": _fixture_b,
    "constructed": CASES["constructed"],
    "constructed_sharp": CASES["constructed_sharp"],
    "collinear": CASES["collinear"],
}
OUTPUTS = ("mollified", "proj_loss", "proj_grad", "rep_loss", "rep_grad")


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or FIXTURE_CASES[name])()


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """The float64 expectation of a case -> {output: (value, magnitude)} and the float32 mollified normals that the loss
    kernels, the yardstick and the restatement all take as their input."""
    c = case(name)
    lists = (c["knn_d2"], c["knn_idx"])
    moll, moll_mag = rr.mollify_normals(c["normals"], *lists, keep_of(c), c["first"], c["num"])
    moll32 = moll.astype(np.float32)
    pl, pl_mag, pg, pg_mag = rr.projection_loss(c["points"], moll32, *lists, c["visible"], c["first"], c["num"], c["sigma"], c["gl1"])
    rl, rl_mag, rg, rg_mag = rr.repulsion_loss(c["points"], moll32, c["knn_idx"], c["first"], c["num"], c["sigma"],
                                               c["filter_scale"], c["gl3"])
    return {"mollified": (moll, moll_mag), "proj_loss": (pl, pl_mag), "proj_grad": (pg, pg_mag), "rep_loss": (rl, rl_mag),
            "rep_grad": (rg, rg_mag)}, moll32


def restate(name, dtype=np.float32, mut=None):
    """The restatement's outputs of a case -> {output: value}"""
    c = case(name)
    _, moll32 = yardstick(name)
    lists = (c["knn_d2"], c["knn_idx"])
    moll = rr.restate_mollify(c["normals"], *lists, keep_of(c), c["first"], c["num"], dtype, mut)
    pl, pg = rr.restate_projection(c["points"], moll32, *lists, c["visible"], c["first"], c["num"], c["sigma"], c["gl1"], dtype, mut)
    rl, rg = rr.restate_repulsion(c["points"], moll32, c["knn_idx"], c["first"], c["num"], c["sigma"], c["filter_scale"],
                                  c["gl3"], dtype, mut)
    return {"mollified": moll, "proj_loss": pl, "proj_grad": pg, "rep_loss": rl, "rep_grad": rg}


def figures(name, got):
    """Largest per-entry error of every output of `got` against the yardstick -> {output: float}"""
    want, _ = yardstick(name)
    return {o: float(rr.rel_err(got[o], *want[o]).max()) for o in OUTPUTS}


# ---------------------------------------------------------------------------------------------------------------------
# In-mask filter: constructed positions that are exact in float32 (orthographic M, power-of-two sizes)
# ---------------------------------------------------------------------------------------------------------------------
def _coord(i, size):
    """world x (or y) whose sample position is pixel coordinate i under the identity M: g = -x = (2 i + 1) / size - 1"""
    return -((2.0 * np.asarray(i, np.float64) + 1.0) / size - 1.0)


def _at(ix, iy, H, W, z=0.0):
    ix, iy = np.broadcast_arrays(np.asarray(ix, np.float64), np.asarray(iy, np.float64))
    return np.stack([_coord(ix.ravel(), W), _coord(iy.ravel(), H), np.full(ix.size, z)], 1).astype(np.float32)


def _one_pixel(H, W, r, c, v=1.0):
    m = np.zeros((1, H, W), np.float32)
    m[0, r, c] = v
    return m


EYE = np.eye(4, dtype=np.float32)[None]
W_IS_Z = EYE.copy()          # Wc = z instead of 1
W_IS_Z[0, 2, 3], W_IS_Z[0, 3, 3] = 1.0, 0.0


def inmask_scenarios():
    """-> [(name, points (P,3) f32, M (N,4,4) f32, mask (N,H,W) f32, visible or None, hand-stated flags or None)]"""
    out = []
    yy, xx = np.mgrid[0:8, 0:8]
    centres = _at(xx, yy, 8, 8)
    out.append(("pixel centres, one lit pixel", centres, EYE, _one_pixel(8, 8, 3, 5), None, ((yy == 3) & (xx == 5)).ravel()))
    # around the lit pixel (3,5): on a tap boundary the lit pixel is the tap whose weight is 0
    ix = np.array([4.0, 4.0 + 2.0 ** -10, 4.5, 5.0, 5.5, 6.0 - 2.0 ** -10, 6.0, 5.0, 5.0, 5.0, 5.0])
    iy = np.array([3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 2.0, 2.0 + 2.0 ** -10, 4.0 - 2.0 ** -10, 4.0])
    out.append(("tap boundaries", _at(ix, iy, 8, 8), EYE, _one_pixel(8, 8, 3, 5), None,
                np.array([0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0], bool)))
    # at and beyond +-1: the position is clamped, the coordinate clipped to the border pixel with weight 1
    edge = np.array([[1.0, 0.0625, 0], [1.5, 0.0625, 0], [-1.0, 0.0625, 0], [-3.0, 0.0625, 0], [0.0625, 1.0, 0], [0.0625, -2.0, 0],
                     [0.8125, 0.0625, 0]], np.float32)                                   # the last one: ix = 0.25
    col0 = np.zeros((1, 8, 8), np.float32); col0[0, :, 0] = 1
    col1 = np.zeros((1, 8, 8), np.float32); col1[0, :, 1] = 1
    out.append(("border, column 0 lit", edge, EYE, col0, None, np.array([1, 1, 0, 0, 0, 0, 1], bool)))     # x = 1 -> g = -1 -> column 0
    out.append(("border, column 1 lit", edge, EYE, col1, None, np.array([0, 0, 0, 0, 0, 0, 1], bool)))     # only ix = 0.25 reaches column 1: the clip leaves the border pixel weight 1
    row = _at(np.arange(-1, 9) + 0.5, np.zeros(10), 1, 8)
    out.append(("H = 1", row, EYE, _one_pixel(1, 8, 0, 2), None, None))
    out.append(("W = 1", row[:, [1, 0, 2]].copy(), EYE, _one_pixel(8, 1, 2, 0), None, None))
    out.append(("1 x 1", edge, EYE, np.ones((1, 1, 1), np.float32), None, np.ones(len(edge), bool)))
    g = np.array([-1.5, -1.0, -0.8, -0.2, 0.0, 0.2, 0.6, 1.0, 2.0])       # 3 x 5: interior positions well away from the taps' edges
    gx, gy = np.meshgrid(g, g)
    m35 = np.zeros((1, 3, 5), np.float32); m35[0, 0, 4] = 1; m35[0, 2, 1] = 0.5
    out.append(("3 x 5", np.stack([-gx.ravel(), -gy.ravel(), np.zeros(gx.size)], 1).astype(np.float32), EYE, m35, None, None))
    soft = np.zeros((1, 8, 8), np.float32); soft[0, 3, 5] = 0.25; soft[0, 6, 1] = 2.0 ** -20
    out.append(("soft mask", centres, EYE, soft, None, (((yy == 3) & (xx == 5)) | ((yy == 6) & (xx == 1))).ravel()))
    cancel = np.zeros((1, 8, 8), np.float32); cancel[0, 0, 0], cancel[0, 0, 1] = 1.0, -1.0
    out.append(("taps cancel", _at([0.5, 0.25, 0.0, 1.0], [0, 0, 0, 0], 8, 8), EYE, cancel, None, np.array([0, 1, 1, 1], bool)))
    nan = np.float32(np.nan)
    # Wc = z: Wc < 0 mirrors the position; Wc == 0 with X != 0 is +-inf, clamped to the border; 0/0 and NaN: never
    wz = np.array([[0.5, 0.5, 1.0], [0.5, 0.5, -1.0], [0.5, 0.25, 0.0], [-0.5, 0.25, 0.0], [0.0, 0.25, 0.0], [0.25, 0.0, 0.0],
                   [0.0, 0.0, 0.0], [nan, 0.0, 1.0], [0.0, nan, 1.0], [0.0, 0.0, nan]], np.float32)
    out.append(("Wc cases, all lit", wz, W_IS_Z, np.ones((1, 8, 8), np.float32), None, np.array([1, 1, 1, 1, 0, 0, 0, 0, 0, 0], bool)))
    quad = np.zeros((1, 8, 8), np.float32); quad[0, :4, :4] = 1                                # lit: g < 0 in both axes
    out.append(("Wc cases, one quadrant lit", wz, W_IS_Z, quad, None, np.array([1, 0, 1, 0, 0, 0, 0, 0, 0, 0], bool)))
    three = np.concatenate([np.zeros((2, 8, 8), np.float32), _one_pixel(8, 8, 3, 5)])
    out.append(("only the third camera sees", centres, np.repeat(EYE, 3, 0), three, None, ((yy == 3) & (xx == 5)).ravel()))
    vis = np.ones(64, bool); vis[3 * 8 + 5] = False
    out.append(("visible given", centres, EYE, np.ones((1, 8, 8), np.float32), vis, vis))
    out.append(("P = 257", np.tile(centres, (5, 1))[:257], EYE, _one_pixel(8, 8, 3, 5), None, None))
    return out


def inmask_perspective(golden_dir):
    """Random points through the three perspective cameras of ref_inmask.npz and a blocky random mask"""
    import os
    M = np.load(os.path.join(golden_dir, "ref_inmask.npz"))["M"].astype(np.float32)
    rng = np.random.default_rng(9)
    pts = rng.normal(0, 0.8, (3000, 3)).astype(np.float32)
    mask = np.kron(rng.random((len(M), 8, 8)) < 0.3, np.ones((8, 8))).astype(np.float32)
    return pts, M, mask
