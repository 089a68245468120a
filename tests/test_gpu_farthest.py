"""GPU: farthest point sampling (`dss_farthest_points`, `ops.farthest_points`, `cloud_ops.sample_farthest_points`,
`cloud_ops.subsample`) against the float32 yardstick of tests/farthest_reference.py (checked on itself by
test_farthest_cpu.py).  Every step of the contract is an exactly defined fp32 operation, so ids AND `sel_sqdist` are compared
bit for bit; there is no tolerance in this file.  The raw entry is called on outputs pre-filled with -7 / NaN, so a slot that a
call leaves unwritten shows."""
import numpy as np
import pytest
import torch

import farthest_reference as yard

pytestmark = pytest.mark.gpu

CASES = yard.single_cloud_cases()


def _dev():
    return torch.device("cuda:0")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _i64(values):
    return torch.tensor(list(values), dtype=torch.int64, device=_dev())


def _raw(packed, firsts, sizes, counts, K_max, starts=None):
    """dss_farthest_points through the C ABI on pre-filled outputs -> (idx (N, K_max), sel_sqdist (N, K_max)) as numpy"""
    from dss_amd import _lib
    dev, N, P = _dev(), len(sizes), packed.shape[0]
    pts = _gpu(packed.astype(np.float32).reshape(P, 3))
    idx = torch.full((N, K_max), -7, dtype=torch.int64, device=dev)
    sqd = torch.full((N, K_max), float("nan"), dtype=torch.float32, device=dev)
    nbytes = _lib.load().dss_farthest_points_workspace(N, P)
    ws = _lib.workspace(dev, nbytes) if nbytes else None
    _lib.call("dss_farthest_points", dev, pts, _i64(firsts), _i64(sizes), _i64(counts), None if starts is None else _i64(starts),
              N, P, K_max, idx, sqd, ws, ws.numel() if ws is not None else 0)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sqd.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_alone(x, k, K_max, start=0):
    """one cloud against the yardstick, ids and radii bit for bit -> the GPU's ids"""
    idx, sqd = _raw(x, [0], [x.shape[0]], [k], K_max, None if start == 0 else [start])
    want_i, want_r = yard.rows([x], [k], K_max, [start])
    assert np.array_equal(idx, want_i), "ids differ first at step %d" % int(np.flatnonzero((idx != want_i)[0])[0])
    assert _same_bits(sqd, want_r)
    return idx[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_single_clouds_equal_the_yardstick(name):
    x, k, start = CASES[name]
    idx = _check_alone(x, k, k, start)
    kk = min(k, x.shape[0])
    assert len(set(idx[:kk].tolist())) == kk and (idx[kk:] == -1).all()
    if name in ("random_257_all", "duplicates", "lattice"):
        assert sorted(idx.tolist()) == list(range(x.shape[0]))   # k = P: a permutation, duplicate points or not


def test_no_samples_and_the_padding_of_a_wider_row():
    x = yard.random_cloud(10, 3)
    idx, sqd = _raw(x, [0], [10], [0], 4)
    assert (idx == -1).all() and (sqd == 0).all()
    _check_alone(x, 3, 8)               # K_max above the count: -1 / 0 behind the three samples
    idx, sqd = _raw(x, [0], [10], [99], 8)   # a count above K_max is clamped to it
    want_i, want_r = yard.rows([x], [8], 8)
    assert np.array_equal(idx, want_i) and _same_bits(sqd, want_r)
    from dss_amd import ops
    empty = ops.farthest_points(torch.zeros(0, 3, device=_dev()), _i64([0]), _i64([0]), _i64([3]), None, 3, return_sqdist=True)
    assert empty[0].tolist() == [[-1, -1, -1]] and empty[1].tolist() == [[0.0, 0.0, 0.0]]
    assert ops.farthest_points(_gpu(x), _i64([0]), _i64([10]), _i64([0]), None, 0).shape == (1, 0)


def test_a_nan_point_is_selected_second_and_never_again():
    x = yard.with_nan()
    idx = _check_alone(x, 50, 50)
    assert idx[1] == 13 and sorted(idx.tolist()) == list(range(50))


def test_a_start_outside_the_cloud_is_clamped_into_it():
    x = yard.random_cloud(100, 4)
    for start, used in ((1000, 99), (-5, 0)):
        idx, sqd = _raw(x, [0], [100], [20], 20, [start])
        want_i, want_r = yard.rows([x], [20], 20, [used])
        assert np.array_equal(idx, want_i) and _same_bits(sqd, want_r)


def test_a_batch_is_every_cloud_alone_and_the_gap_is_not_read():
    rng = np.random.default_rng(21)
    sizes, counts, K_max = [300, 0, 1, 1000], [50, 5, 5, 999], 999
    clouds = [rng.standard_normal((s, 3)).astype(np.float32) for s in sizes]
    gap = np.full((17, 3), 3e37, np.float32)                      # rows that no cloud owns: read, they would win every step
    packed = np.concatenate([clouds[0], gap, clouds[2], clouds[3]], 0)
    firsts = [0, 300, 317, 318]
    starts = [5, 0, 0, 77]
    idx, sqd = _raw(packed, firsts, sizes, counts, K_max, starts)
    want_i, want_r = yard.rows(clouds, counts, K_max, starts)
    assert np.array_equal(idx, want_i) and _same_bits(sqd, want_r)
    assert (idx[1] == -1).all() and idx[2].tolist() == [0] + [-1] * 998 and np.isfinite(sqd[:, 1:]).all()
    for n in (0, 3):   # and against the same cloud sampled alone on the GPU
        a_i, a_r = _raw(clouds[n], [0], [sizes[n]], [counts[n]], K_max, [starts[n]])
        assert np.array_equal(idx[n], a_i[0]) and _same_bits(sqd[n], a_r[0])


def _capacities():
    from dss_amd import sampling_ops
    return sampling_ops.REGISTER_CAPACITIES


def test_the_capacities_are_the_five_of_the_kernel():
    assert len(_capacities()) == 5 and list(_capacities()) == sorted(_capacities())


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("over", [0, 1])
def test_every_path_boundary(which, over):
    """a cloud that fills an instantiation to its last slot, and one point more: the next instantiation, behind the largest one
    the streaming path.  The last point lies far away, so step 1 must select id P - 1."""
    P = _capacities()[which] + over
    x = yard.boundary_cloud(P, 100 + 2 * which + over)
    idx = _check_alone(x, 64, 64)
    assert idx[1] == P - 1


def test_mixed_paths_in_one_call():
    caps = _capacities()
    sizes = [100, caps[2] + 1, caps[-1] + 300]     # a small, a boundary and a streaming-size cloud
    clouds = [yard.boundary_cloud(s, 300 + n) for n, s in enumerate(sizes)]
    counts, starts, K_max = [32, 64, 48], [0, 11, 7], 64
    firsts = [0, sizes[0], sizes[0] + sizes[1]]
    idx, sqd = _raw(np.concatenate(clouds, 0), firsts, sizes, counts, K_max, starts)
    want_i, want_r = yard.rows(clouds, counts, K_max, starts)
    assert np.array_equal(idx, want_i) and _same_bits(sqd, want_r)
    assert [int(idx[n, 1]) for n in range(3)] == [s - 1 for s in sizes]


@pytest.fixture(scope="module")
def large():
    x = yard.random_cloud(20000, 7)
    return x, yard.farthest(x, 2000)


def test_a_large_cloud_bit_for_bit_and_in_float64(large):
    from dss_amd import ops
    x, (want_i, want_r) = large
    P, k = x.shape[0], 2000
    call = lambda: ops.farthest_points(_gpu(x), _i64([0]), _i64([P]), _i64([k]), None, k, return_sqdist=True)   # noqa: E731
    idx, sqd = call()
    again_i, again_r = call()
    torch.cuda.synchronize()
    assert idx.dtype == torch.int64 and sqd.dtype == torch.float32
    assert torch.equal(idx, again_i) and _same_bits(sqd.cpu().numpy(), again_r.cpu().numpy())   # a second call: the same bits
    idx, sqd = idx[0].cpu().numpy(), sqd[0].cpu().numpy()
    assert np.array_equal(idx, want_i) and _same_bits(sqd, want_r)
    worst = yard.teacher_forced(x, idx)
    print("20,000 points, 2,000 samples: smallest d64[pick] / max d64 = 1 - %.3g" % (1.0 - worst))
    assert worst >= 1.0 - yard.REL
    assert (sqd[1:] <= sqd[:-1]).all() and len(set(idx.tolist())) == k


def test_the_public_call_pads_and_follows_pytorch3d_conventions():
    from dss_amd import cloud_ops
    from dss_amd.cloud import PointClouds3D
    rng = np.random.default_rng(31)
    sizes, P = [60, 10, 0], 60
    clouds = [rng.standard_normal((s, 3)).astype(np.float32) for s in sizes]
    padded = np.full((3, P, 3), 3e37, np.float32)              # junk in the padding rows: it must not be read
    for n, c in enumerate(clouds):
        padded[n, :sizes[n]] = c
    K, starts = [16, 16, 4], [3, 9, 0]
    want_i, _ = yard.rows(clouds, K, 16, starts)
    want_p = np.zeros((3, 16, 3), np.float32)
    for n, c in enumerate(clouds):
        kk = int((want_i[n] >= 0).sum())
        want_p[n, :kk] = c[want_i[n, :kk]]
    pts = _gpu(padded)
    keep = pts.clone()
    for lengths in (sizes, _i64(sizes)):
        sel, idx = cloud_ops.sample_farthest_points(pts, lengths, K, starts)
        assert sel.shape == (3, 16, 3) and idx.shape == (3, 16) and idx.dtype == torch.int64
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(sel.cpu().numpy(), want_p)
    assert torch.equal(pts, keep)
    cloud = PointClouds3D([_gpu(c) for c in clouds[:2]])
    sel, idx = cloud_ops.sample_farthest_points(cloud, K=16, start_idx=starts[:2])
    assert np.array_equal(idx.cpu().numpy(), want_i[:2]) and np.array_equal(sel.cpu().numpy(), want_p[:2])
    sel, idx = cloud_ops.sample_farthest_points(pts[:1], K=5)   # one K for all, lengths None: all P rows are points
    assert np.array_equal(idx[0].cpu().numpy(), yard.farthest(padded[0], 5)[0])
    sel, idx = cloud_ops.sample_farthest_points(pts, sizes, K=0)
    assert sel.shape == (3, 0, 3) and idx.shape == (3, 0)


def test_the_public_call_is_capturable_with_host_integers():
    """one linear stream, captured after a warm-up call; a replay on new coordinates reproduces the eager result"""
    from dss_amd import cloud_ops
    x = _gpu(np.stack([yard.random_cloud(500, 41), yard.random_cloud(500, 42)]))
    lengths, K, starts = [500, 333], [40, 25], [0, 17]
    eager_sel, eager_idx = cloud_ops.sample_farthest_points(x, lengths, K, starts)
    torch.cuda.synchronize()
    static = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cloud_ops.sample_farthest_points(static, lengths, K, starts)   # warm-up on the capturing stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sel, idx = cloud_ops.sample_farthest_points(static, lengths, K, starts)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager_idx) and torch.equal(sel, eager_sel)
    other = _gpu(np.stack([yard.random_cloud(500, 43), yard.random_cloud(500, 44)]))
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    want_sel, want_idx = cloud_ops.sample_farthest_points(other, lengths, K, starts)
    assert torch.equal(idx, want_idx) and torch.equal(sel, want_sel) and not torch.equal(want_idx, eager_idx)


def test_subsample_carries_normals_and_features_in_selection_order():
    from dss_amd import cloud_ops
    from dss_amd.cloud import PointClouds3D
    rng = np.random.default_rng(51)
    sizes = [400, 90]
    pts = [rng.standard_normal((s, 3)).astype(np.float32) for s in sizes]
    nrm = [rng.standard_normal((s, 3)).astype(np.float32) for s in sizes]
    feat = [rng.standard_normal((s, 2)).astype(np.float32) for s in sizes]
    cloud = PointClouds3D([_gpu(p) for p in pts], [_gpu(a) for a in nrm], [_gpu(a) for a in feat])
    out = cloud_ops.subsample(cloud, n_points=[50, 200], start_idx=[7, 0])
    for n, k in enumerate((50, 90)):   # the second cloud has only 90 points: all of them, in selection order
        want = yard.farthest(pts[n], k, (7, 0)[n])[0]
        assert np.array_equal(out.points_list()[n].cpu().numpy(), pts[n][want])
        assert np.array_equal(out.normals_list()[n].cpu().numpy(), nrm[n][want])
        assert np.array_equal(out.features_list()[n].cpu().numpy(), feat[n][want])
    by_ratio = cloud_ops.subsample(cloud, ratio=0.125)
    assert [int(p.shape[0]) for p in by_ratio.points_list()] == [50, 11]
    assert np.array_equal(by_ratio.points_list()[0].cpu().numpy(), pts[0][yard.farthest(pts[0], 50)[0]])
    assert [int(p.shape[0]) for p in cloud.points_list()] == sizes   # the input is not modified
    # method="random": int(ratio P_n) distinct rows, attributes following, the same rows under the same seed
    draw = lambda: cloud_ops.subsample(cloud, ratio=0.33, method="random",   # noqa: E731
                                       generator=torch.Generator(device=_dev()).manual_seed(9))
    a, b = draw(), draw()
    for n, s in enumerate(sizes):
        p = a.points_list()[n].cpu().numpy()
        assert p.shape == (int(0.33 * s), 3) and torch.equal(a.points_list()[n], b.points_list()[n])
        rows = [int(np.flatnonzero((pts[n] == q).all(-1))[0]) for q in p]
        assert len(set(rows)) == len(rows)
        assert np.array_equal(a.normals_list()[n].cpu().numpy(), nrm[n][rows])
        assert np.array_equal(a.features_list()[n].cpu().numpy(), feat[n][rows])
