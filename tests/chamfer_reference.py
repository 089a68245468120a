"""TEST INFRASTRUCTURE: the float64 yardstick of the chamfer tests (test_chamfer_cpu.py, test_gpu_chamfer.py) and their
seeded scenes.

`nearest_ref` is the exact nearest-point query (brute force while the distance matrix is small, `scipy.spatial.cKDTree`
beyond), `chamfer_ref` the chamfer distance of `pytorch3d.loss.chamfer_distance` (restated by
compat/pytorch3d/loss/chamfer.py, against which test_chamfer_cpu.py checks it) on lists of ragged clouds.  Both take the
float32 inputs as they are and compute in float64, independent of the product's code.
"""
import os

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

NEAR_TIE = 1e-5          # relative gap of the two smallest squared distances below which the index is not compared
NEAR_TIE_CAP = 0.01      # share of such queries a scene may have
_BRUTE_MAX = 1 << 23     # distance-matrix entries up to which the reference is brute force


class Nearest:
    """d2 (Px,) float64 smallest squared distance, idx (Px,) int64 (ties: smaller id, where the search is brute force),
    near_tie (Px,) bool: the second-smallest squared distance is within NEAR_TIE (relative) of the smallest."""

    def __init__(self, d2, idx, second):
        self.d2, self.idx = d2, idx
        with np.errstate(invalid="ignore"):
            self.near_tie = (second - d2) < NEAR_TIE * second


def _sqdist(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_ref(x, y):
    """one cloud x (Px,3) in one cloud y (Py,3), Py >= 1"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    Px, Py = x.shape[0], y.shape[0]
    if Px * Py <= _BRUTE_MAX:
        d = _sqdist(x[:, None, :], y[None, :, :])
        idx = d.argmin(1)            # the first minimum: the smaller id
        d2 = d[np.arange(Px), idx]
        if Py > 1:
            d[np.arange(Px), idx] = np.inf
            second = d.min(1)
        else:
            second = np.full(Px, np.inf)
        return Nearest(d2, idx.astype(np.int64), second)
    from scipy.spatial import cKDTree
    _, ii = cKDTree(y).query(x, k=2)
    d_a, d_b = _sqdist(x, y[ii[:, 0]]), _sqdist(x, y[ii[:, 1]])     # the tree ranks, the distances are recomputed
    swap = (d_b < d_a) | ((d_b == d_a) & (ii[:, 1] < ii[:, 0]))
    return Nearest(np.where(swap, d_b, d_a), np.where(swap, ii[:, 1], ii[:, 0]).astype(np.int64), np.where(swap, d_a, d_b))


def _normal_term(a, b, eps=1e-6):
    """1 - |cos| as torch.nn.functional.cosine_similarity(a, b, eps) computes it: each norm clamped from below by eps"""
    na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    return 1.0 - np.abs((a * b).sum(1) / (np.maximum(na, eps) * np.maximum(nb, eps)))


def chamfer_ref(x, y, x_normals=None, y_normals=None, weights=None, batch_reduction="mean", point_reduction="mean",
                idx_xy=None, idx_yx=None):
    """x, y: lists of N clouds (P_n,3); normals likewise or None -> (cham_dist, cham_normals or None) in float64, scalars or
    (N,) arrays (batch_reduction None).  idx_xy / idx_yx: lists of index arrays to use instead of searching."""
    N = len(x)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    normals = x_normals is not None and y_normals is not None
    cham, cham_n = np.zeros(N), np.zeros(N)
    for n in range(N):
        a, b = np.asarray(x[n], np.float64), np.asarray(y[n], np.float64)
        i_ab = nearest_ref(a, b).idx if idx_xy is None else np.asarray(idx_xy[n])
        i_ba = nearest_ref(b, a).idx if idx_yx is None else np.asarray(idx_yx[n])
        ca, cb = _sqdist(a, b[i_ab]).sum(), _sqdist(b, a[i_ba]).sum()
        if normals:
            na, nb = np.asarray(x_normals[n], np.float64), np.asarray(y_normals[n], np.float64)
            cna, cnb = _normal_term(na, nb[i_ab]).sum(), _normal_term(nb, na[i_ba]).sum()
        else:
            cna = cnb = 0.0
        if point_reduction == "mean":
            ca, cb, cna, cnb = ca / a.shape[0], cb / b.shape[0], cna / a.shape[0], cnb / b.shape[0]
        cham[n], cham_n[n] = w[n] * (ca + cb), w[n] * (cna + cnb)
    if batch_reduction is not None:
        cham, cham_n = cham.sum(), cham_n.sum()
        if batch_reduction == "mean":
            div = w.sum() if weights is not None else N
            cham, cham_n = cham / div, cham_n / div
    return cham, (cham_n if normals else None)


# ---------------------------------------------------------------------------------------------------------------
# scenes: {"x": [clouds], "y": [clouds], "xn": [normals], "yn": [normals]} float32, seeded
# ---------------------------------------------------------------------------------------------------------------
def _normals(rng, clouds):
    return [rng.standard_normal(c.shape).astype(np.float32) for c in clouds]


def _scene(rng, x, y, one_normal=False):
    """one_normal: every point of a cloud carries the same normal (scenes with exact ties: the normal term must not depend on
    which of the tied neighbours a search reports)"""
    x, y = [np.ascontiguousarray(c, np.float32) for c in x], [np.ascontiguousarray(c, np.float32) for c in y]
    xn, yn = _normals(rng, x), _normals(rng, y)
    if one_normal:
        xn, yn = [np.tile(n[:1], (n.shape[0], 1)) for n in xn], [np.tile(n[:1], (n.shape[0], 1)) for n in yn]
    return {"x": x, "y": y, "xn": xn, "yn": yn}


def scene_lattice():
    """exact ties: x a 3x3x3 lattice, y a 2x2x2 lattice, coordinates multiples of 1/4 -- every fp32 operation is exact"""
    g3, g2 = np.arange(3) * 0.5, np.arange(2) * 0.5 + 0.25
    x = np.stack(np.meshgrid(g3, g3, g3, indexing="ij"), -1).reshape(-1, 3)
    y = np.stack(np.meshgrid(g2, g2, g2, indexing="ij"), -1).reshape(-1, 3)
    return _scene(np.random.default_rng(10), [x], [y], one_normal=True)


def scene_ragged():
    """N = 3, no size a multiple of 64, a one-point query cloud and a one-point target"""
    rng = np.random.default_rng(11)
    x = [rng.uniform(-1, 1, (s, 3)) for s in (1, 130, 1000)]
    y = [rng.uniform(-1, 1, (s, 3)) for s in (257, 1, 2049)]
    return _scene(rng, x, y)


def scene_outside():
    """y uniform in the unit cube; x the same law scaled 3x about the centre, plus six points 50 cell widths beyond each face
    (cell width of the target's grid: extent / ceil(sqrt(Py / 24)))"""
    rng = np.random.default_rng(12)
    Py = 3000
    y = rng.uniform(0, 1, (Py, 3))
    x = (rng.uniform(0, 1, (1500, 3)) - 0.5) * 3.0 + 0.5
    cell = 1.0 / np.ceil(np.sqrt(Py / 24.0))
    far = np.full((6, 3), 0.5)
    for a in range(3):
        far[2 * a, a] = -50 * cell
        far[2 * a + 1, a] = 1 + 50 * cell
    far[:, :] += rng.uniform(-0.2, 0.2, (6, 3)) * (far == 0.5)
    return _scene(rng, [np.concatenate([x, far])], [y])


def scene_empty_rings():
    """y: two clusters of 500 points 1.0 apart, each 0.02 wide; x: 256 points on the segment between them"""
    rng = np.random.default_rng(13)
    c0, c1 = np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
    y = np.concatenate([c0 + rng.uniform(-0.01, 0.01, (500, 3)), c1 + rng.uniform(-0.01, 0.01, (500, 3))])
    t = rng.uniform(0.02, 0.98, (256, 1))
    x = c0 + t * (c1 - c0) + rng.uniform(-1e-3, 1e-3, (256, 3))
    return _scene(rng, [x], [y])


def scene_degenerate(kind):
    """y with a degenerate extent -- "coincident" (exact ties: every point is the same), "planar" (constant z), "collinear" --
    x uniform around it (collinear: along it)"""
    rng = np.random.default_rng({"coincident": 14, "planar": 15, "collinear": 16}[kind])
    x = rng.uniform(-1, 1, (500, 3))
    if kind == "coincident":
        y = np.tile(np.array([[0.25, -0.5, 0.125]]), (300, 1))
    elif kind == "planar":
        y = np.concatenate([rng.uniform(-1, 1, (700, 2)), np.full((700, 1), 0.3)], 1)
    else:
        # (queries close to the line and past its ends: from far away neighbouring points of the line are all near-ties)
        y = np.array([[0.1, -0.2, 0.3]]) + rng.uniform(-1, 1, (700, 1)) * np.array([[1.0, 0.0, 0.0]])
        x = np.array([[0.1, -0.2, 0.3]]) + rng.uniform(-1.3, 1.3, (500, 1)) * np.array([[1.0, 0.0, 0.0]]) + rng.uniform(-5e-3, 5e-3, (500, 3))
    return _scene(rng, [x], [y], one_normal=kind == "coincident")


def scene_large():
    """the large grid-build route: Py = 131,073 = KNN_SMALL_P + 1 uniform points, Px = 4,096"""
    rng = np.random.default_rng(17)
    return _scene(rng, [rng.uniform(0, 1, (4096, 3))], [rng.uniform(0, 1, (131073, 3))])


def read_ply_points(path):
    """(P,3) float32 positions of a binary little-endian PLY whose vertices are float properties starting with x, y, z"""
    with open(path, "rb") as f:
        raw = f.read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    count = [int(ln.split()[2]) for ln in lines if ln.startswith("element vertex")][0]
    props, inside = 0, False
    for ln in lines:
        if ln.startswith("element"):
            inside = ln.startswith("element vertex")
        elif inside and ln.startswith("property float"):
            props += 1
    return np.frombuffer(body, "<f4", count * props).reshape(count, props)[:, :3].copy()


def scene_clustered():
    """y: the trained cloud of configs[2] (tests/golden/trained_cloud_cfg3.npz: outliers stretch its box, most points sit in a
    few cells); x: tests/golden/bunny-8000.ply brought to the unit sphere the model is trained in"""
    y = np.load(os.path.join(_GOLDEN, "trained_cloud_cfg3.npz"))["points"]
    x = read_ply_points(os.path.join(_GOLDEN, "bunny-8000.ply"))
    c = (x.max(0) + x.min(0)) / 2
    x = (x - c) / np.linalg.norm(x - c, axis=1).max()
    return _scene(np.random.default_rng(18), [x], [y])


SMALL_SCENES = {
    "lattice": scene_lattice,
    "ragged": scene_ragged,
    "outside": scene_outside,
    "empty_rings": scene_empty_rings,
    "coincident": lambda: scene_degenerate("coincident"),
    "planar": lambda: scene_degenerate("planar"),
    "collinear": lambda: scene_degenerate("collinear"),
}
LARGE_SCENES = {"large": scene_large, "clustered": scene_clustered}
EXACT_TIE_SCENES = ("lattice", "coincident")   # ties that are exact in fp32 as well: the index is compared in full (smaller id)
