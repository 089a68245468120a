"""Yardstick of farthest point sampling (include/dss_hip.h `dss_farthest_points`): a numpy FLOAT32 restatement of
the contract, operation by operation -- every step is a separately rounded fp32 operation that the GPU performs identically, so
the GPU tests demand the same ids and the same `sel_sqdist` bits -- and, independent of the fp32 ordering, a float64
"teacher-forced" check of a given id sequence.  The scenes that the CPU and the GPU tests share are built here, from seeds."""
import numpy as np

REL = 1e-6   # teacher_forced: see there


def farthest(points, k, start=0):
    """The contract for ONE cloud -> (idx (k',) int64, sel_sqdist (k',) float32), k' = min(k, P)."""
    x = np.ascontiguousarray(points, np.float32)
    P = x.shape[0]
    k = max(min(int(k), P), 0)
    idx, rad = np.full(k, -1, np.int64), np.zeros(k, np.float32)
    if k == 0:
        return idx, rad
    d = np.full(P, np.inf, np.float32)
    c, r = int(start), np.float32(np.inf)
    assert 0 <= c < P
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(k):
            idx[t], rad[t] = c, r
            diff = x - x[c]
            dx, dy, dz = diff[:, 0], diff[:, 1], diff[:, 2]
            dist = (dx * dx + dy * dy) + dz * dz          # float32 arrays: every operation rounds on its own
            assert dist.dtype == np.float32
            d = np.where(dist < d, dist, d)               # a NaN distance never changes d
            d[c] = np.float32(-1.0)                       # after the update: never selected again
            c = int(np.argmax(d))                         # the first maximum = the smallest id
            r = d[c]
    return idx, rad


def rows(clouds, counts, K_max, starts=None):
    """`farthest` for every cloud of a batch, padded like the entry's outputs -> idx (N, K_max) with -1, sel_sqdist with 0."""
    N = len(clouds)
    idx, rad = np.full((N, K_max), -1, np.int64), np.zeros((N, K_max), np.float32)
    for n, x in enumerate(clouds):
        k = min(int(counts[n]), K_max)
        if x.shape[0] and k:
            i, r = farthest(x, k, 0 if starts is None else starts[n])
            idx[n, :len(i)], rad[n, :len(r)] = i, r
    return idx, rad


def teacher_forced(points, idx, rel=REL):
    """Float64 check of an id sequence, independent of how fp32 ordered near-equal candidates: follow the GIVEN sequence,
    recompute d in float64 along it, and require of every pick ``d64[pick] >= (1 - rel) * max d64`` -> the smallest ratio
    d64[pick] / max d64 seen (1.0 when every pick was a float64 maximum).  Raises AssertionError otherwise.

    rel = 1e-6 is derived, not measured: an fp32 distance carries one rounding per difference of exactly representable
    inputs, and the three squares and two sums of non-negative terms add at most four more, in all at most
    5 * 2^-24 ~ 3e-7 relative; a pick that fp32 preferred can therefore lie below the float64 maximum by twice that at
    the most."""
    x = np.asarray(points, np.float64)
    d = np.full(x.shape[0], np.inf)
    worst = 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        for t, c in enumerate(np.asarray(idx).tolist()):
            assert 0 <= c < x.shape[0], "id %d at step %d leaves the cloud" % (c, t)
            if t > 0:
                m = d.max()
                assert d[c] >= 0.0, "step %d selects id %d again" % (t, c)
                assert d[c] >= (1.0 - rel) * m, "step %d: d64[%d] = %.17g, max d64 = %.17g" % (t, c, d[c], m)
                if np.isfinite(m) and m > 0:
                    worst = min(worst, d[c] / m)
            dist = ((x - x[c]) ** 2).sum(-1)
            d = np.where(dist < d, dist, d)
            d[c] = -1.0
    return worst


def exact_integer_fps(points, k, start=0):
    """Farthest point sampling of INTEGER coordinates in int64 with the tie rule spelled out -> ids.  Nothing rounds, so this
    is the contract without any floating point."""
    x = np.asarray(points, np.int64)
    d = np.full(x.shape[0], np.iinfo(np.int64).max, np.int64)
    c, out = int(start), []
    for _ in range(k):
        out.append(c)
        d = np.minimum(d, ((x - x[c]) ** 2).sum(-1))
        d[c] = -1
        c = min(np.flatnonzero(d == d.max()).tolist())
    return np.array(out, np.int64)


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def random_cloud(P, seed):
    return np.random.default_rng(seed).standard_normal((P, 3)).astype(np.float32)


def lattice():
    """5 x 5 x 5 integer lattice, id = 25 ix + 5 iy + iz: ties at almost every step"""
    g = np.arange(5)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def duplicates():
    """40 points, each five times (copy j of point i has id 40 j + i)"""
    return np.tile(random_cloud(40, 11), (5, 1))


def collinear():
    return np.stack([np.arange(64) * 0.25, np.zeros(64), np.zeros(64)], -1).astype(np.float32)


def with_nan():
    x = random_cloud(50, 13)
    x[13] = (np.nan, 0.0, 0.0)
    return x


def boundary_cloud(P, seed):
    """P uniform points in the unit cube, the LAST one moved far away: step 1 must select id P - 1"""
    x = np.random.default_rng(seed).uniform(0, 1, (P, 3)).astype(np.float32)
    x[-1] = (100.0, 100.0, 100.0)
    return x


def single_cloud_cases():
    """name -> (points, n_samples, start): the cases that the CPU tests check the yardstick on and the GPU tests run"""
    return {
        "random_257_all": (random_cloud(257, 0), 257, 0),
        "lattice": (lattice(), 125, 0),
        "duplicates": (duplicates(), 200, 0),
        "collinear": (collinear(), 64, 0),
        "one_point": (np.array([[0.25, -0.5, 2.0]], np.float32), 1, 0),
        "more_samples_than_points": (random_cloud(10, 3), 16, 0),
        "nonzero_start": (random_cloud(100, 4), 30, 37),
    }
