"""GPU: nearest point in another cloud (`ops.nearest_points` / dss_nearest_points), the chamfer distance built on it
(`losses.chamfer_distance`) and its backward (dss_chamfer_backward), against the float64 yardstick of
tests/chamfer_reference.py (checked on the CPU by test_chamfer_cpu.py).

Tolerances.  d2: relative 2e-6 -- in the difference form the subtraction of two fp32 inputs is correctly rounded, the
bound of (dx dx + dy dy) + dz dz is ~6 * 2^-24 = 3.6e-7, the margin covers fused against unfused multiply-add.  idx: equal
to the reference outside the near-ties the reference itself marks (two nearest within 1e-5, at most 1 % of a scene:
test_chamfer_cpu.py), in full on the exact-tie scenes.  Loss values: relative 1e-5.  Gradients: rel-L2 <= 1e-6, the
project's gradient standard."""
import itertools

import numpy as np
import pytest
import torch

import chamfer_reference as cr

pytestmark = pytest.mark.gpu

D2_RTOL, LOSS_RTOL, GRAD_REL_L2 = 2e-6, 1e-5, 1e-6


def _dev():
    return torch.device("cuda:0")


def _pack(clouds, gap=0):
    """clouds -> packed (P,3) with `gap` NaN slots of no cloud in front of every cloud and behind the last, first, num"""
    rows, first, run = [], [], 0
    for c in clouds:
        rows.append(np.full((gap, 3), np.nan, np.float32))
        run += gap
        first.append(run)
        rows.append(np.asarray(c, np.float32).reshape(-1, 3))
        run += c.shape[0]
    rows.append(np.full((gap, 3), np.nan, np.float32))
    dev = _dev()
    return (torch.from_numpy(np.concatenate(rows)).to(dev), torch.tensor(first, dtype=torch.int64, device=dev),
            torch.tensor([c.shape[0] for c in clouds], dtype=torch.int64, device=dev))


_REF = {}


def _reference(name, n, direction):
    """the float64 search of one cloud pair of a scene, computed once per session"""
    key = (name, n, direction)
    if key not in _REF:
        sc = _scene(name)
        a, b = (sc["x"][n], sc["y"][n]) if direction == "xy" else (sc["y"][n], sc["x"][n])
        _REF[key] = cr.nearest_ref(a, b)
    return _REF[key]


_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = (cr.SMALL_SCENES.get(name) or cr.LARGE_SCENES[name])()
    return _SCENES[name]


def _check_search(name, directions=("xy", "yx"), gap=0, bit_equal=False):
    from dss_amd import ops
    sc = _scene(name)
    for direction in directions:
        q, t = (sc["x"], sc["y"]) if direction == "xy" else (sc["y"], sc["x"])
        Q, qf, qn = _pack(q, gap)
        T, tf, tn = _pack(t, gap)
        d2, idx = ops.nearest_points(Q, qf, qn, T, tf, tn)
        d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
        assert d2.dtype == np.float32 and idx.dtype == np.int64 and d2.shape == idx.shape == (Q.shape[0],)
        owned = np.zeros(Q.shape[0], bool)
        for n, c in enumerate(q):
            f = int(qf[n])
            owned[f:f + c.shape[0]] = True
            ref = _reference(name, n, direction)
            got_d, got_i = d2[f:f + c.shape[0]], idx[f:f + c.shape[0]]
            err = np.abs(got_d.astype(np.float64) - ref.d2) / np.maximum(ref.d2, 1e-300)
            print("%s %s cloud %d: max rel d2 error %.3g, %d of %d near-tied" % (name, direction, n, err.max(),
                                                                              int(ref.near_tie.sum()), c.shape[0]))
            if bit_equal:
                assert np.array_equal(got_d, ref.d2.astype(np.float32)) and np.array_equal(ref.d2.astype(np.float32), ref.d2)
            assert np.all(np.abs(got_d.astype(np.float64) - ref.d2) <= D2_RTOL * ref.d2), (name, direction, n, err.max())
            keep = np.ones(c.shape[0], bool) if name in cr.EXACT_TIE_SCENES else ~ref.near_tie
            assert np.array_equal(got_i[keep], ref.idx[keep]), (name, direction, n, int((got_i[keep] != ref.idx[keep]).sum()))
            assert np.all((got_i >= 0) & (got_i < t[n].shape[0]))
        # packed slots of no cloud: (0, -1), their (NaN) positions unread
        assert np.all(d2[~owned] == 0.0) and np.all(idx[~owned] == -1)


def test_exact_ties_lattice():
    """3x3x3 lattice in a 2x2x2 lattice, multiples of 1/4: bit-equal distances, the smaller id wins every tie"""
    _check_search("lattice", bit_equal=True)


def test_ragged_batch():
    """N = 3, sizes (1, 130, 1000) in (257, 1, 2049): wavefronts straddle cloud boundaries; with and without slots of no cloud"""
    _check_search("ragged")
    _check_search("ragged", gap=37)


def test_queries_outside_the_targets_box():
    _check_search("outside")


def test_empty_rings():
    _check_search("empty_rings")


@pytest.mark.parametrize("kind", ["coincident", "planar", "collinear"])
def test_degenerate_extents(kind):
    _check_search(kind)


def test_large_grid_build_route():
    """Py = KNN_SMALL_P + 1: the target's grid comes from the eight-launch build"""
    _check_search("large", directions=("xy",))


def test_clustered_target():
    """the trained cloud of configs[2] as target (outliers stretch its grid, most points share a few cells), the bunny as query"""
    _check_search("clustered", directions=("xy",))


def test_empty_target_cloud():
    """a query whose target cloud is empty gets (0, -1); the other clouds of the batch are searched as usual"""
    from dss_amd import ops
    rng = np.random.default_rng(20)
    x = [rng.uniform(-1, 1, (70, 3)).astype(np.float32), rng.uniform(-1, 1, (90, 3)).astype(np.float32)]
    y = [np.zeros((0, 3), np.float32), rng.uniform(-1, 1, (300, 3)).astype(np.float32)]
    X, xf, xn = _pack(x)
    Y, yf, yn = _pack(y)
    d2, idx = ops.nearest_points(X, xf, xn, Y, yf, yn)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert np.all(d2[:70] == 0.0) and np.all(idx[:70] == -1)
    ref = cr.nearest_ref(x[1], y[1])
    assert np.array_equal(idx[70:][~ref.near_tie], ref.idx[~ref.near_tie])
    assert np.all(np.abs(d2[70:].astype(np.float64) - ref.d2) <= D2_RTOL * ref.d2)
    # nothing to search at all
    d2, idx = ops.nearest_points(X, xf, xn, Y[:0], yf * 0, yn * 0)
    assert np.all(d2.cpu().numpy() == 0.0) and np.all(idx.cpu().numpy() == -1)


def _padded(clouds, dev):
    P = max(c.shape[0] for c in clouds)
    out = torch.zeros((len(clouds), P, 3), dtype=torch.float32, device=dev)
    for n, c in enumerate(clouds):
        out[n, : c.shape[0]] = torch.from_numpy(c).to(dev)
    return out, torch.tensor([c.shape[0] for c in clouds], dtype=torch.int64, device=dev)


@pytest.mark.parametrize("name", ["ragged", "outside", "empty_rings"])
def test_loss_values(name):
    """`losses.chamfer_distance` against chamfer_ref: every combination of reductions, with and without weights and normals,
    padded tensors with lengths and `PointClouds3D` input"""
    from dss_amd import losses
    from dss_amd.cloud import PointClouds3D
    dev = _dev()
    sc = _scene(name)
    N = len(sc["x"])
    x, xl = _padded(sc["x"], dev)
    y, yl = _padded(sc["y"], dev)
    xn, _ = _padded(sc["xn"], dev)
    yn, _ = _padded(sc["yn"], dev)
    weights = np.linspace(0.5, 2.0, N).astype(np.float32)
    worst = 0.0

    def close(got, want, what):
        nonlocal worst
        got = got.detach().cpu().numpy().astype(np.float64)
        assert got.shape == np.shape(want), what
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
        assert np.all(np.abs(got - want) <= LOSS_RTOL * np.abs(want)), (what, got, want)

    for batch, point, use_w, use_n in itertools.product(("mean", "sum", None), ("mean", "sum"), (False, True), (False, True)):
        what = (name, batch, point, use_w, use_n)
        w = weights if use_w else None
        want_d, want_n = cr.chamfer_ref(sc["x"], sc["y"], sc["xn"] if use_n else None, sc["yn"] if use_n else None, w, batch, point,
                                        idx_xy=[_reference(name, n, "xy").idx for n in range(N)],
                                        idx_yx=[_reference(name, n, "yx").idx for n in range(N)])
        got_d, got_n = losses.chamfer_distance(x, y, x_lengths=xl, y_lengths=yl, x_normals=xn if use_n else None,
                                               y_normals=yn if use_n else None,
                                               weights=None if w is None else torch.from_numpy(w).to(dev),
                                               batch_reduction=batch, point_reduction=point)
        close(got_d, want_d, what)
        if use_n:
            close(got_n, want_n, what)
        else:
            assert got_n is None
    # PointClouds3D pairs: lengths and normals from the clouds
    cx = PointClouds3D([torch.from_numpy(c).to(dev) for c in sc["x"]], [torch.from_numpy(c).to(dev) for c in sc["xn"]])
    cy = PointClouds3D([torch.from_numpy(c).to(dev) for c in sc["y"]], [torch.from_numpy(c).to(dev) for c in sc["yn"]])
    want_d, want_n = cr.chamfer_ref(sc["x"], sc["y"], sc["xn"], sc["yn"])
    got_d, got_n = losses.chamfer_distance(cx, cy)
    close(got_d, want_d, (name, "clouds"))
    close(got_n, want_n, (name, "clouds, normals"))
    print("%s: worst relative loss error %.3g" % (name, worst))


def _many_to_one():
    """4,096 queries whose nearest neighbour is ONE target point (and a few targets far away)"""
    rng = np.random.default_rng(21)
    x = rng.uniform(-0.1, 0.1, (4096, 3)).astype(np.float32)
    y = np.concatenate([np.zeros((1, 3)), rng.uniform(2, 3, (40, 3))]).astype(np.float32)
    return {"x": [x], "y": [y]}


def _rel_l2(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want))


@pytest.mark.parametrize("name", ["ragged", "many_to_one"])
def test_backward_against_float64_autograd(name):
    """dss_chamfer_backward against float64 torch autograd of sum gx d2_x + sum gy d2_y with the GPU's index lists held
    fixed; run twice, bit-identical"""
    from dss_amd import ops
    sc = _many_to_one() if name == "many_to_one" else _scene(name)
    X, xf, xn = _pack(sc["x"], gap=5)
    Y, yf, yn = _pack(sc["y"], gap=3)
    _, ixy = ops.nearest_points(X, xf, xn, Y, yf, yn)
    _, iyx = ops.nearest_points(Y, yf, yn, X, xf, xn)
    if name == "many_to_one":
        assert int((ixy == 0).sum()) == 4096
    rng = np.random.default_rng(22)
    gx = torch.from_numpy(rng.standard_normal(X.shape[0]).astype(np.float32)).to(X.device)
    gy = torch.from_numpy(rng.standard_normal(Y.shape[0]).astype(np.float32)).to(X.device)
    grad_x, grad_y = ops.chamfer_backward(X, xf, xn, Y, yf, yn, ixy, iyx, gx, gy)
    again_x, again_y = ops.chamfer_backward(X, xf, xn, Y, yf, yn, ixy, iyx, gx, gy)
    assert torch.equal(grad_x, again_x) and torch.equal(grad_y, again_y)
    only_x, none_y = ops.chamfer_backward(X, xf, xn, Y, yf, yn, ixy, iyx, gx, gy, want_y=False)
    assert none_y is None and torch.equal(only_x, grad_x)
    # reference: the packed ids of the neighbours from the GPU's cloud-local lists, everything else in float64 on the CPU
    cloud_x, cloud_y = ops.packed_cloud_ids(xf, xn, X.shape[0]).cpu(), ops.packed_cloud_ids(yf, yn, Y.shape[0]).cpu()
    own_x, own_y = cloud_x >= 0, cloud_y >= 0
    x64 = torch.nan_to_num(X.cpu().double()).requires_grad_(True)
    y64 = torch.nan_to_num(Y.cpu().double()).requires_grad_(True)
    jx = (yf.cpu()[cloud_x.clamp(min=0)] + ixy.cpu())[own_x]
    jy = (xf.cpu()[cloud_y.clamp(min=0)] + iyx.cpu())[own_y]
    total = (gx.cpu().double()[own_x] * ((x64[own_x] - y64[jx]) ** 2).sum(1)).sum() \
        + (gy.cpu().double()[own_y] * ((y64[own_y] - x64[jy]) ** 2).sum(1)).sum()
    total.backward()
    ex, ey = _rel_l2(grad_x.cpu().numpy(), x64.grad.numpy()), _rel_l2(grad_y.cpu().numpy(), y64.grad.numpy())
    print("%s: grad_x rel-L2 %.3g, grad_y rel-L2 %.3g" % (name, ex, ey))
    assert ex <= GRAD_REL_L2 and ey <= GRAD_REL_L2, (ex, ey)
    assert np.all(grad_x.cpu().numpy()[~own_x.numpy()] == 0.0) and np.all(grad_y.cpu().numpy()[~own_y.numpy()] == 0.0)


def test_chamfer_distance_is_one_differentiable_node():
    """the public loss on padded ragged input with weights: gradients of x and y against float64 autograd of the reference
    formula (GPU index lists), bit-identical on a second run, no graph on the normal term"""
    from dss_amd import losses, ops
    dev = _dev()
    sc = _scene("ragged")
    N = len(sc["x"])
    x, xl = _padded(sc["x"], dev)
    y, yl = _padded(sc["y"], dev)
    xn, _ = _padded(sc["xn"], dev)
    yn, _ = _padded(sc["yn"], dev)
    w = torch.tensor(np.linspace(0.5, 2.0, N).astype(np.float32), device=dev)
    grads = []
    for _ in range(2):
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        dist, normals = losses.chamfer_distance(xg, yg, x_lengths=xl, y_lengths=yl, x_normals=xn, y_normals=yn, weights=w)
        assert dist.requires_grad and not normals.requires_grad
        assert type(dist.grad_fn).__name__ == "_ChamferBackward"
        dist.backward()
        grads.append((xg.grad.clone(), yg.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # float64 reference with the GPU's index lists
    X, xf, xnum = _pack(sc["x"])
    Y, yf, ynum = _pack(sc["y"])
    _, ixy = ops.nearest_points(X, xf, xnum, Y, yf, ynum)
    _, iyx = ops.nearest_points(Y, yf, ynum, X, xf, xnum)
    ixy, iyx = ixy.cpu(), iyx.cpu()
    x64, y64 = x.cpu().double().requires_grad_(True), y.cpu().double().requires_grad_(True)
    total = 0.0
    for n in range(N):
        a, b = x64[n, : int(xl[n])], y64[n, : int(yl[n])]
        ia = ixy[int(xf[n]): int(xf[n]) + int(xl[n])]
        ib = iyx[int(yf[n]): int(yf[n]) + int(yl[n])]
        total = total + float(w[n]) * (((a - b[ia]) ** 2).sum(1).mean() + ((b - a[ib]) ** 2).sum(1).mean())
    (total / float(w.double().sum())).backward()
    ex, ey = _rel_l2(grads[0][0].cpu().numpy(), x64.grad.numpy()), _rel_l2(grads[0][1].cpu().numpy(), y64.grad.numpy())
    print("chamfer_distance: grad_x rel-L2 %.3g, grad_y rel-L2 %.3g" % (ex, ey))
    assert ex <= GRAD_REL_L2 and ey <= GRAD_REL_L2, (ex, ey)
    assert np.all(grads[0][0].cpu().numpy()[0, 1:] == 0.0)   # padding rows of the one-point cloud
