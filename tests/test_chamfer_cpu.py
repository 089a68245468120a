"""CPU: the cross-cloud nearest-point query and the chamfer distance built on it (include/dss_hip.h: dss_nearest_workspace,
dss_nearest_points, dss_chamfer_backward) -- the symbols and their argument checks, and the float64 yardstick the GPU
tests (test_gpu_chamfer.py) measure against: tests/chamfer_reference.py, checked here against the pure-torch stand-in
compat/pytorch3d/loss/chamfer.py and for the share of near-ties its scenes contain."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import chamfer_reference as cr
from dss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "compat") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "compat"))

INVALID, WORKSPACE = -1, -2   # DSS_ERR_INVALID_ARGUMENT, DSS_ERR_WORKSPACE


def test_symbols_and_argument_checks():
    """the three entries load and refuse NULL pointers, negative sizes and a short workspace before any launch (no GPU here)"""
    lib = _lib.load()
    for name in ("dss_nearest_workspace", "dss_nearest_points", "dss_chamfer_backward"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dss_nearest_workspace(3, 5000) == lib.dss_knn_workspace(3, 5000) > 0
    buf = ctypes.create_string_buffer(64)   # a non-NULL address that a rejected call never reads
    p = ctypes.addressof(buf)

    def nearest(x=p, xf=p, xn=p, Px=5, y=p, yf=p, yn=p, Py=7, N=1, d2=p, idx=p, ws=p, ws_bytes=1 << 30):
        return lib.dss_nearest_points(x, xf, xn, Px, y, yf, yn, Py, N, d2, idx, ws, ws_bytes, None)

    for kw in ({"N": 0}, {"N": -1}, {"Px": -1}, {"Py": -1}):
        assert nearest(**kw) == INVALID and b"bad sizes" in lib.dss_last_error(), kw
    for name in ("x", "xf", "xn", "y", "yf", "yn", "d2", "idx"):
        assert nearest(**{name: None}) == INVALID and b"NULL" in lib.dss_last_error(), name
    assert nearest(ws=None) == WORKSPACE
    assert nearest(ws_bytes=lib.dss_nearest_workspace(1, 7) - 1) == WORKSPACE and b"workspace" in lib.dss_last_error()
    assert nearest(ws_bytes=0) == WORKSPACE
    assert nearest(Px=0, x=None, d2=None, idx=None, ws=None) == 0   # nothing to write

    def backward(x=p, y=p, xf=p, xn=p, Px=5, yf=p, yn=p, Py=7, N=1, ixy=p, iyx=p, oxy=p, oyx=p, gx=p, gy=p, grad_x=p, grad_y=p):
        return lib.dss_chamfer_backward(x, y, xf, xn, Px, yf, yn, Py, N, ixy, iyx, oxy, oyx, gx, gy, grad_x, grad_y, None)

    for kw in ({"N": 0}, {"Px": -1}, {"Py": -3}):
        assert backward(**kw) == INVALID and b"bad sizes" in lib.dss_last_error(), kw
    for name in ("x", "y", "xf", "xn", "yf", "yn", "ixy", "iyx", "oxy", "oyx", "gx", "gy"):
        assert backward(**{name: None}) == INVALID and b"NULL" in lib.dss_last_error(), name
    assert backward(grad_x=None, grad_y=None) == 0   # no gradient asked for: nothing to do
    assert backward(grad_x=None, oxy=None) == INVALID   # grad_y needs order_xy ...
    assert backward(grad_y=None, oyx=None) == INVALID   # ... and grad_x order_yx


def _padded(clouds, dtype=torch.float64):
    P = max(c.shape[0] for c in clouds)
    out = torch.zeros((len(clouds), P, 3), dtype=dtype)
    for n, c in enumerate(clouds):
        out[n, : c.shape[0]] = torch.from_numpy(np.asarray(c)).to(dtype)
    return out, torch.tensor([c.shape[0] for c in clouds], dtype=torch.int64)


@pytest.mark.parametrize("name", sorted(cr.SMALL_SCENES))
def test_reference_matches_the_stand_in(name):
    """chamfer_ref == compat's chamfer_distance in float64: every reduction, with and without weights and normals; the ragged
    scene goes in padded with lengths"""
    from pytorch3d.loss import chamfer_distance
    sc = cr.SMALL_SCENES[name]()
    N = len(sc["x"])
    x, xl = _padded(sc["x"])
    y, yl = _padded(sc["y"])
    xn, _ = _padded(sc["xn"])
    yn, _ = _padded(sc["yn"])
    weights = np.linspace(0.5, 2.0, N)
    for batch, point, use_w, use_n in itertools.product(("mean", "sum", None), ("mean", "sum"), (False, True), (False, True)):
        w = weights if use_w else None
        want_d, want_n = cr.chamfer_ref(sc["x"], sc["y"], sc["xn"] if use_n else None, sc["yn"] if use_n else None, w, batch, point)
        got_d, got_n = chamfer_distance(x, y, x_lengths=xl, y_lengths=yl, x_normals=xn if use_n else None,
                                        y_normals=yn if use_n else None, weights=None if w is None else torch.from_numpy(w),
                                        batch_reduction=batch, point_reduction=point)
        np.testing.assert_allclose(got_d.numpy(), want_d, rtol=1e-12, atol=0, err_msg=str((batch, point, use_w, use_n)))
        if use_n:
            np.testing.assert_allclose(got_n.numpy(), want_n, rtol=1e-11, atol=0, err_msg=str((batch, point, use_w, use_n)))
        else:
            assert got_n is None and want_n is None


@pytest.mark.parametrize("name", sorted(set(cr.SMALL_SCENES) | set(cr.LARGE_SCENES)))
def test_scenes_stay_under_the_near_tie_cap(name):
    """on the reference alone: at most 1 % of a scene's queries have their two nearest targets within 1e-5 (relative, squared
    distance) and leave the index comparison -- in both directions, the chamfer distance searches both.  The exact-tie scenes
    are exempt: their ties are exact in fp32 too and the index is compared in full there"""
    sc = (cr.SMALL_SCENES.get(name) or cr.LARGE_SCENES[name])()
    for n, (a, b) in enumerate(zip(sc["x"], sc["y"])):
        for tag, q, t in (("x in y", a, b), ("y in x", b, a)):
            ref = cr.nearest_ref(q, t)
            share = float(ref.near_tie.mean())
            print("%s cloud %d %s: %d of %d queries near-tied" % (name, n, tag, int(ref.near_tie.sum()), q.shape[0]))
            if name in cr.EXACT_TIE_SCENES:
                continue
            assert share <= cr.NEAR_TIE_CAP, (name, n, tag, share)
            # the tree-backed reference agrees with brute force where both are affordable
            if q.shape[0] * t.shape[0] <= cr._BRUTE_MAX and t.shape[0] >= 2:
                from scipy.spatial import cKDTree
                dd, ii = cKDTree(np.asarray(t, np.float64)).query(np.asarray(q, np.float64), k=1)
                keep = ~ref.near_tie
                assert np.array_equal(ii[keep], ref.idx[keep])
                np.testing.assert_allclose(dd ** 2, ref.d2, rtol=1e-12, atol=1e-300)


def test_chamfer_distance_refuses_bad_input_without_a_gpu():
    """what `losses.chamfer_distance` decides on the host: reductions, shapes, empty clouds (the stand-in divides by zero
    there) -- and no quiet CPU fallback"""
    from dss_amd import losses
    from dss_amd.cloud import PointClouds3D
    x, y = torch.zeros(2, 5, 3), torch.zeros(2, 4, 3)
    with pytest.raises(ValueError, match="batch_reduction"):
        losses.chamfer_distance(x, y, batch_reduction="max")
    with pytest.raises(ValueError, match="point_reduction"):
        losses.chamfer_distance(x, y, point_reduction=None)
    with pytest.raises(ValueError, match="shape"):
        losses.chamfer_distance(x, torch.zeros(3, 4, 3))
    with pytest.raises(ValueError, match="empty cloud"):
        losses.chamfer_distance(x, y, x_lengths=torch.tensor([5, 0]))
    with pytest.raises(ValueError, match="empty cloud"):
        losses.chamfer_distance(x, torch.zeros(2, 0, 3))
    with pytest.raises(ValueError, match="empty cloud"):
        losses.chamfer_distance(PointClouds3D([torch.zeros(4, 3)]), PointClouds3D([torch.zeros(0, 3)]))
    with pytest.raises(ValueError, match="weights"):
        losses.chamfer_distance(x, y, weights=torch.tensor([1.0, -1.0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.chamfer_distance(x, y)


def test_cpu_tensors_are_refused_by_name():
    """the cross-cloud operators (dss_amd/cross_cloud.py, re-exported by `ops`) refuse CPU tensors like every operator of
    `ops` does, naming the first argument they look at (the pin tests/test_ops_checks_cpu.py gives the operators defined there)"""
    from dss_amd import ops
    x, y = torch.zeros(6, 3), torch.zeros(5, 3)
    first, nx, ny = torch.tensor([0]), torch.tensor([6]), torch.tensor([5])
    with pytest.raises(RuntimeError, match=r"dss_amd: x is on cpu; the HIP path needs GPU tensors \(no CPU fallback\)"):
        ops.nearest_points(x, first, nx, y, first, ny)
    with pytest.raises(RuntimeError, match=r"dss_amd: x is on cpu; the HIP path needs GPU tensors \(no CPU fallback\)"):
        ops.chamfer_backward(x, first, nx, y, first, ny, torch.zeros(6, dtype=torch.int64), torch.zeros(5, dtype=torch.int64),
                             torch.zeros(6), torch.zeros(5))
    with pytest.raises(TypeError, match="x must be a torch.Tensor"):
        ops.nearest_points(None, first, nx, y, first, ny)
