"""GPU: the sign of estimated normals (`dss_disambiguate_normals`, `dss_orient_normals`, `ops.disambiguate_normals`,
`ops.orient_normals`, `cloud_ops.estimate_normals`, `cloud_ops.orient_normals`) against the float32 yardstick of
tests/normals_reference.py (checked on itself by test_normals_cpu.py).  Every step of both contracts is an exactly defined
fp32 operation or an integer rule, so normals, stamps and parents are compared bit for bit; the only tolerance in this file
is the unit length of the PCA directions.  The raw entries are called on outputs pre-filled with NaN / -7, so a slot that a
call leaves unwritten shows."""
import numpy as np
import pytest
import torch

import normals_reference as yard

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _i64(values):
    return torch.tensor(list(values), dtype=torch.int64, device=_dev())


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _raw_orient(normals, points, idx, firsts, sizes, KP):
    """dss_orient_normals through the C ABI on pre-filled outputs -> (normals, stamp, parent) as numpy"""
    from dss_amd import _lib
    dev, N, P, K = _dev(), len(sizes), normals.shape[0], idx.shape[1]
    out = torch.full((P, 3), float("nan"), dtype=torch.float32, device=dev)
    stamp = torch.full((P,), -7, dtype=torch.int32, device=dev)
    parent = torch.full((P,), -7, dtype=torch.int64, device=dev)
    nbytes = _lib.load().dss_orient_normals_workspace(N, P)
    ws = _lib.workspace(dev, nbytes) if nbytes else None
    _lib.call("dss_orient_normals", dev, _gpu(normals.astype(np.float32)), _gpu(points.astype(np.float32)),
              _gpu(idx.astype(np.int64)), _i64(firsts), _i64(sizes), N, P, K, KP, out, stamp, parent, ws,
              ws.numel() if ws is not None else 0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), stamp.cpu().numpy(), parent.cpu().numpy()


def _assert_equal(got, want):
    (o, s, p), (wo, ws, wp) = got, want[:3]
    assert np.array_equal(s, ws), "stamps differ first at row %d" % int(np.flatnonzero(s != ws)[0])
    assert np.array_equal(p, wp), "parents differ first at row %d" % int(np.flatnonzero(p != wp)[0])
    assert _same_bits(o, wo)


def _check(normals, points, idx, firsts, sizes, KP):
    """a packed batch against the yardstick, bit for bit -> (normals, stamp, parent, iterations per cloud)"""
    want = yard.orient(normals, points, idx, firsts, sizes, KP)
    _assert_equal(_raw_orient(normals, points, idx, firsts, sizes, KP), want)
    return want


def _alone(points, normals, K, KP, lists=yard.knn_lists):
    idx = lists(points, K)
    return _check(normals, points, idx, [0], [points.shape[0]], KP)


@pytest.mark.parametrize("K,KP", [(8, 8), (12, 12), (16, 9), (5, 3)])   # lists of up to 8 entries and longer ones: two code paths
def test_a_sphere_of_257_points_with_random_signs(K, KP):
    p, outward = yard.fibonacci_sphere(257)
    o, stamp, parent, its = _alone(p, yard.random_signs(outward, 9), K, KP)
    if KP >= 8:    # (two neighbours do not connect the sphere: more seeds, each turned upwards)
        assert yard.outward_share(o, outward) == 1.0 and (parent == -1).sum() == 1
    assert stamp.min() == 4 and parent[np.argmin(stamp)] == -1      # three level drops, then the first seed


def test_two_spheres_in_one_cloud():
    a, na = yard.fibonacci_sphere(600, (0.0, 0.0, 0.0))
    b, nb = yard.fibonacci_sphere(300, (3.0, 0.0, 0.5), 0.6)
    outward = np.concatenate([na, nb])
    o, stamp, parent, its = _alone(np.concatenate([a, b]), yard.random_signs(outward, 10), 8, 8)
    assert yard.outward_share(o, outward) == 1.0 and (parent == -1).sum() == 2


def test_on_a_plane_the_tie_rule_alone_picks_the_parents():
    p, n = yard.plane_grid(16)
    o, stamp, parent, its = _alone(p, n, 8, 8)
    assert (o[:, 2] == 1.0).all() and (parent == -1).sum() == 1 and stamp.max() == its[0] < 40


def test_a_cube_is_crossed_at_the_last_level():
    p, n = yard.cube(10)
    o, stamp, parent, its = _alone(p, yard.random_signs(n, 11), 8, 8)
    assert (parent == -1).sum() == 1
    has = parent >= 0
    across = has & ((o * o[np.clip(parent, 0, None)]).sum(1) == 0)     # a parent on another face: d = 0, below tau[2]
    assert across.sum() >= 5                                             # six faces: at least five crossings
    inside = has & ~across
    assert ((o * o[np.clip(parent, 0, None)]).sum(1)[inside] == 1).all()   # within a face every child agrees with its parent


def test_a_long_chain_of_iterations():
    p, n = yard.polyline(4000)
    o, stamp, parent, its = _alone(p, n, 3, 2)
    print("polyline: %d iterations for 4,000 points, %d seeds" % (its[0], (parent == -1).sum()))
    assert 4000 <= its[0] <= 5 * 4000 and (stamp >= 1).all()


def test_duplicate_points():
    base, outward = yard.fibonacci_sphere(40)
    p, n = np.tile(base, (5, 1)), yard.random_signs(np.tile(outward, (5, 1)), 12)
    o, stamp, parent, its = _alone(p, n, 8, 8)
    assert (stamp >= 1).all() and (np.abs(o) == np.abs(n)).all()


def test_tiny_clouds_and_zero_padded_lists():
    rng = np.random.default_rng(13)
    sizes = [1, 2, 5, 8, 9]
    clouds = [rng.standard_normal((s, 3)).astype(np.float32) for s in sizes]
    normals = rng.standard_normal((sum(sizes), 3)).astype(np.float32)
    idx = np.concatenate([yard.knn_lists(c, 8) for c in clouds])            # zeros behind the min(8, P_n) entries
    firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    o, stamp, parent, its = _check(normals, np.concatenate(clouds), idx, firsts, sizes, 8)
    assert (stamp >= 1).all() and parent[0] == -1 and its[0] == 4 and (parent[1:3] == -1).sum() == 1
    _check(normals, np.concatenate(clouds), idx, firsts, sizes, 40)         # KP above K and above every P_n
    _check(normals, np.concatenate(clouds), idx, firsts, sizes, 1)          # no neighbours: every point is a seed


def test_a_nan_normal_ends_as_a_seed_and_is_ignored():
    p, outward = yard.fibonacci_sphere(300)
    n = yard.random_signs(outward, 14)
    n[77] = np.nan
    o, stamp, parent, its = _alone(p, n, 8, 8)
    assert parent[77] == -1 and stamp[77] == its[0] and (parent != 77).all() and np.isnan(o[77]).all()
    keep = np.arange(300) != 77
    assert yard.outward_share(o[keep], outward[keep]) == 1.0


def test_a_nan_height_loses_the_seed():
    p, outward = yard.fibonacci_sphere(300)
    p[0, 2] = np.nan                                   # the point that would be the seed
    idx = yard.knn_lists(np.nan_to_num(p, nan=1.0), 8)
    o, stamp, parent, its = _check(yard.random_signs(outward, 15), p, idx, [0], [300], 8)
    assert parent[0] >= 0 and (parent == -1).sum() == 1
    q = np.full((6, 3), np.nan, np.float32)            # every z NaN: the smallest id seeds
    _, stamp, parent, _ = _check(np.tile(np.array([[0, 0, -1]], np.float32), (6, 1)), q, np.zeros((6, 1), np.int64), [0], [6], 8)
    assert np.argsort(stamp).tolist() == list(range(6))


def test_a_batch_is_every_cloud_alone_and_the_gap_is_not_read():
    sizes = [300, 0, 1, 1000]
    clouds = [yard.fibonacci_sphere(s, (n, 0.0, 0.0))[0] if s else np.zeros((0, 3), np.float32) for n, s in enumerate(sizes)]
    normals = [yard.random_signs(yard.fibonacci_sphere(s)[1], 20 + n) if s else np.zeros((0, 3), np.float32)
               for n, s in enumerate(sizes)]
    lists = [yard.knn_lists(c, 8) for c in clouds]
    gap3, gapk = np.full((17, 3), np.nan, np.float32), np.full((17, 8), 1 << 40, np.int64)
    points = np.concatenate([clouds[0], gap3, clouds[2], clouds[3]])
    nrm = np.concatenate([normals[0], gap3, normals[2], normals[3]])
    idx = np.concatenate([lists[0], gapk, lists[2], lists[3]])
    firsts = [0, 300, 317, 318]
    o, stamp, parent, its = _check(nrm, points, idx, firsts, sizes, 8)
    assert np.array_equal(o[300:317], np.tile(np.array([[0, 0, 1]], np.float32), (17, 1)))
    assert (stamp[300:317] == 0).all() and (parent[300:317] == -1).all()
    for n in (0, 3):   # and against the same cloud oriented alone on the GPU
        f, s = firsts[n], sizes[n]
        alone = _raw_orient(normals[n], clouds[n], lists[n], [0], [s], 8)
        assert _same_bits(o[f:f + s], alone[0]) and np.array_equal(stamp[f:f + s], alone[1])
        assert np.array_equal(parent[f:f + s], alone[2])


@pytest.fixture(scope="module")
def capacity_clouds():
    """a sphere that fills the LDS path to its last stamp and one of a point more, with their references"""
    from dss_amd import normals_ops
    made = []
    for n, P in enumerate((normals_ops.LDS_CAPACITY, normals_ops.LDS_CAPACITY + 1)):
        p, outward = yard.fibonacci_sphere(P)
        nrm, idx = yard.random_signs(outward, 30 + n), yard.tree_lists(p, 8)
        made.append((p, nrm, idx, outward, yard.orient(nrm, p, idx, [0], [P], 8)))
    return made


@pytest.mark.parametrize("which", [0, 1])
def test_both_sides_of_the_lds_capacity(capacity_clouds, which):
    p, nrm, idx, outward, want = capacity_clouds[which]
    _assert_equal(_raw_orient(nrm, p, idx, [0], [p.shape[0]], 8), want)
    assert yard.outward_share(want[0], outward) == 1.0


def test_both_paths_in_one_call(capacity_clouds):
    (pa, na, ia, _, wa), (pb, nb, ib, _, wb) = capacity_clouds
    got = _raw_orient(np.concatenate([na, nb]), np.concatenate([pa, pb]), np.concatenate([ia, ib]), [0, pa.shape[0]],
                      [pa.shape[0], pb.shape[0]], 8)
    _assert_equal(got, [np.concatenate([a, b]) for a, b in zip(wa[:3], wb[:3])])


def test_a_second_call_and_a_replayed_graph():
    """the operator twice: the same bits; captured after a warm-up, a replay on new inputs equals the yardstick"""
    from dss_amd import ops
    p, outward = yard.fibonacci_sphere(500)
    idx = yard.knn_lists(p, 8)
    first, num = _i64([0]), _i64([500])
    n1, n2 = yard.random_signs(outward, 40), yard.random_signs(outward, 41)
    static_n, pts, lists = _gpu(n1), _gpu(p), _gpu(idx)
    call = lambda: ops.orient_normals(static_n, pts, lists, first, num, 8, return_stamps=True, return_parents=True)   # noqa: E731
    a, b = call(), call()
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))
    _assert_equal([t.cpu().numpy() for t in a], yard.orient(n1, p, idx, [0], [500], 8))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                      # warm-up on the capturing stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = call()
    static_n.copy_(_gpu(n2))
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal([t.cpu().numpy() for t in out], yard.orient(n2, p, idx, [0], [500], 8))


def _raw_disambiguate(points, normals, idx, firsts, sizes, mode, view=None):
    from dss_amd import _lib
    dev, N, P = _dev(), len(sizes), normals.shape[0]
    out = torch.full((P, 3), float("nan"), dtype=torch.float32, device=dev)
    _lib.call("dss_disambiguate_normals", dev, _gpu(points), _gpu(normals), None if idx is None else _gpu(idx), _i64(firsts),
              _i64(sizes), N, P, 1 if idx is None else idx.shape[1], mode, None if view is None else _gpu(view), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_the_local_and_the_viewpoint_rule():
    rng = np.random.default_rng(50)
    sizes = [700, 5, 300]
    clouds = [rng.standard_normal((s, 3)).astype(np.float32) for s in sizes]
    gap3, gapk = np.full((9, 3), np.nan, np.float32), np.full((9, 12), -3, np.int64)
    points = np.concatenate([clouds[0], gap3, clouds[1], clouds[2]])
    normals = np.concatenate([rng.standard_normal((700, 3)).astype(np.float32), gap3,
                              rng.standard_normal((305, 3)).astype(np.float32)])
    idx = np.concatenate([yard.knn_lists(clouds[0], 12), gapk, yard.knn_lists(clouds[1], 12), yard.knn_lists(clouds[2], 12)])
    firsts = [0, 709, 714]
    got = _raw_disambiguate(points, normals, idx, firsts, sizes, 0)
    want = yard.disambiguate(points, normals, idx, firsts, sizes, 0)
    assert _same_bits(got, want) and 100 < (got[:700] != normals[:700]).any(1).sum() < 600
    view = np.array([[0, 0, 5], [1, 1, 1], [-4, 0, 0]], np.float32)          # one viewpoint per cloud
    got = _raw_disambiguate(points, normals, None, firsts, sizes, 1, view)
    want = yard.disambiguate(points, normals, None, firsts, sizes, 1, view)
    assert _same_bits(got, want)
    assert np.array_equal(got[700:709], np.tile(np.array([[0, 0, 1]], np.float32), (9, 1)))
    from dss_amd import ops
    op = ops.disambiguate_normals(_gpu(points), _gpu(normals), None, _i64(firsts), _i64(sizes), _gpu(view))
    assert _same_bits(op.cpu().numpy(), want)
    assert ops.disambiguate_normals(torch.zeros(0, 3, device=_dev()), torch.zeros(0, 3, device=_dev()),
                                    torch.zeros(0, 4, dtype=torch.int64, device=_dev()), _i64([0]), _i64([0])).shape == (0, 3)
    empty = ops.orient_normals(torch.zeros(0, 3, device=_dev()), torch.zeros(0, 3, device=_dev()),
                               torch.zeros(0, 4, dtype=torch.int64, device=_dev()), _i64([0]), _i64([0]), return_parents=True)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


def test_estimate_normals_end_to_end_on_the_bunny():
    """the public call equals the yardstick run on what ops.knn_points + ops.local_frames return for the same points"""
    import scenes
    from dss_amd import cloud_ops, ops
    from dss_amd.cloud import PointClouds3D
    pts, own = scenes.load_cloud("bunny")
    P = pts.shape[0]
    x = _gpu(pts)
    first, num = _i64([0]), _i64([P])
    _, knn_idx = ops.knn_points(x, first, num, 16)
    _, frame_normals, curvature = ops.local_frames(x, knn_idx, first, num, return_curvature=True)
    idx, pca = knn_idx.cpu().numpy(), frame_normals.cpu().numpy()
    want, _, parent, its = yard.orient(pca, pts, idx, [0], [P], 8)
    got, curv = cloud_ops.estimate_normals(x[None], [P], return_curvature=True)
    assert got.shape == (1, P, 3) and _same_bits(got[0].cpu().numpy(), want) and torch.equal(curv[0], curvature)
    assert np.abs(np.linalg.norm(want.astype(np.float64), axis=1) - 1.0).max() < 1e-5   # fp32 Jacobi rotations of a unit basis
    share = yard.outward_share(want, own)
    print("bunny on the GPU's frames: %.4f agree with the file's normals, %d iterations" % (max(share, 1 - share), its[0]))
    assert max(share, 1 - share) >= 0.99
    # the other orientations, padded rows, and the container's method
    padded = torch.full((2, P + 3, 3), float("nan"), device=_dev())
    padded[0, :P], padded[1, :500] = x, x[:500]
    none = cloud_ops.estimate_normals(padded, [P, 500], orientation="none")
    assert _same_bits(none[0, :P].cpu().numpy(), pca) and (none[0, P:] == 0).all() and (none[1, 500:] == 0).all()
    local = cloud_ops.estimate_normals(padded, [P, 500], orientation="local")
    assert _same_bits(local[0, :P].cpu().numpy(), yard.disambiguate(pts, pca, idx, [0], [P]))
    view = cloud_ops.estimate_normals(padded, [P, 500], orientation="viewpoint", viewpoint=torch.tensor([0.0, 0.0, 9.0]))
    assert _same_bits(view[0, :P].cpu().numpy(), yard.disambiguate(pts, pca, None, [0], [P], 1, np.array([[0, 0, 9]], np.float32)))
    cloud = PointClouds3D([x, x[:500]])
    assert cloud.normals_list() is None
    stored = cloud.estimate_normals(assign_to_self=True, orientation="consistent")
    assert _same_bits(stored[0].cpu().numpy(), want) and torch.equal(cloud.normals_padded(), stored[:, :P])
    assert torch.equal(cloud.normals_packed(), torch.cat([stored[0, :P], stored[1, :500]]))
    assert _same_bits(cloud.estimate_normals()[0].cpu().numpy(), local[0, :P].cpu().numpy())          # the reference's default
    assert _same_bits(cloud.estimate_normals(disambiguate_directions=False)[0].cpu().numpy(), pca)
    # orient_normals: normals that exist, here of random sign
    flipped = yard.random_signs(pca, 60)
    idx8 = ops.knn_points(x, first, num, 8)[1].cpu().numpy()
    fixed, parents = cloud_ops.orient_normals(x[None], _gpu(flipped)[None], neighborhood_size=8, return_parents=True)
    w_o, _, w_p, _ = yard.orient(flipped, pts, idx8, [0], [P], 8)
    assert _same_bits(fixed[0].cpu().numpy(), w_o) and np.array_equal(parents[0].cpu().numpy(), w_p)
