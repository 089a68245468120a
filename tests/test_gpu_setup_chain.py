"""GPU: the binning kernel's wave-uniform cloud lookup against the per-lane one.

setup_bin_kernel (dss_render_forward) fetches cloud, matrices, depth range and h once per wavefront when the wavefront's
64 points lie in one cloud, and per lane when it straddles a cloud boundary; point_setup_kernel (dss_point_setup) always
takes the per-lane path.  With cloud sizes that are not multiples of 64 both forms run in one launch, and every output of
the fused forward must equal the separate entry points bit for bit."""
import numpy as np
import pytest
import torch

import scenes
from dss_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, K = 128, 5
SIZES = (1000, 777, 1301)   # none a multiple of 64, and no prefix sum either: two wavefronts straddle a boundary


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cloud(count, seed):
    pts, nrm = scenes.load_cloud("teapot")
    pts = scenes.normalize_unit_sphere(pts)
    pick = np.random.default_rng(seed).permutation(pts.shape[0])[:count]
    return pts[pick], nrm[pick]


def _frames(nrm, seed):
    """Synthetic anisotropic inputs: a symmetric positive semi-definite Vrk per point (xx,xy,xz,yy,yz,zz) and a unit frame normal."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((nrm.shape[0], 3, 3)).astype(np.float32) * 0.02
    vr = a @ a.transpose(0, 2, 1)
    vr6 = np.stack([vr[:, 0, 0], vr[:, 0, 1], vr[:, 0, 2], vr[:, 1, 1], vr[:, 1, 2], vr[:, 2, 2]], 1).astype(np.float32)
    fn = nrm + 0.1 * rng.standard_normal(nrm.shape).astype(np.float32)
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    return vr6, fn.astype(np.float32)


def _check(world, normals, h, M, V, first, num, feat, shared, backface, vr6=None, fn=None):
    N = first.shape[0]
    zn, zf = torch.full((N,), 0.6, device=DEV), torch.full((N,), 100.0, device=DEV)   # the near plane cuts the clouds
    kw = dict(vr6=vr6, frame_normals=fn)
    for rows in (None, (32, 96)):
        f = ops.render_forward(world, normals, h, M, V, zn, zf, first, num, feat, S, K, 1.0, 0.05, 1.0, backface, shared,
                               rows=rows, **kw)
        info = ops.point_setup(world, normals, h, M, V, zn, zf, first, num, S, 1.0, 1.0, backface, shared, **kw)
        idx, zbuf, qv, occ, vis = ops.splat_points(info["pts_screen"], info["ellipse_params"], info["cutoff_threshold"],
                                                   info["radii"], first, num, 0.05, S, K, None, None, rows=rows,
                                                   return_visible=True)
        img, wsum = ops.blend_forward(idx, qv, occ, info["scaler"], feat, return_wsum=True)
        assert info["valid"].any() and not info["valid"].all()        # both sides of the culling
        assert (idx >= 0).any()
        for k in ("pts_screen", "ellipse_params", "radii", "scaler", "cutoff_threshold", "valid"):
            assert torch.equal(f[k], info[k]), k
        assert torch.equal(f["idx"], idx) and torch.equal(f["zbuf"], zbuf) and torch.equal(f["qvalue"], qv)
        assert torch.equal(f["occupancy"], occ) and torch.equal(f["visible"], vis)
        assert torch.equal(f["image"], img) and torch.equal(f["wsum"], wsum)


def _inputs(shared, mode, sizes):
    N = len(sizes)
    az = [45.0 + 70.0 * k for k in range(N)]
    M, V, _ = scenes.camera_matrices(1.2, 25.0, az, znear=0.6)
    if shared:
        Pw = sizes[-1]
        pts, nrm = _cloud(Pw, 0)
        counts = [Pw] * N
    else:
        parts = [_cloud(c, k) for k, c in enumerate(sizes)]
        pts, nrm = np.concatenate([p for p, _ in parts]), np.concatenate([n for _, n in parts])
        Pw, counts = pts.shape[0], list(sizes)
    P = sum(counts)
    first = torch.tensor(np.cumsum([0] + counts[:-1]), device=DEV, dtype=torch.int64)
    num = torch.tensor(counts, device=DEV, dtype=torch.int64)
    feat = _t(np.random.default_rng(7).uniform(0, 1, (P, 3)).astype(np.float32))
    h0 = scenes.global_h(pts)
    vr6 = fn = None
    if mode == "h_cloud":
        h = _t(np.array([h0 * (1.0 + 0.5 * k) for k in range(N)], np.float32))      # a different h per cloud
    elif mode == "h_point":
        h = _t((h0 * np.random.default_rng(3).uniform(0.5, 2.0, Pw)).astype(np.float32))
    else:
        h = torch.zeros(Pw, device=DEV)
        vr6, fn = (_t(a) for a in _frames(nrm, 5))
    return _t(pts), _t(nrm), h, _t(M), _t(V), first, num, feat, vr6, fn


@pytest.mark.parametrize("backface", [False, True])
@pytest.mark.parametrize("mode", ["h_cloud", "h_point", "aniso"])
@pytest.mark.parametrize("shared", [True, False])
def test_three_clouds_with_straddling_wavefronts_fused_equals_separate(shared, mode, backface):
    world, normals, h, M, V, first, num, feat, vr6, fn = _inputs(shared, mode, SIZES)
    assert all(int(f) % 64 for f in first[1:]) and int(num.sum()) % 64
    _check(world, normals, h, M, V, first, num, feat, shared, backface, vr6, fn)


def test_shared_cloud_with_one_h_per_packed_point_fused_equals_separate():
    """h_point AND h_cloud given (a shared cloud whose cameras cull differently): one h per (camera, point) pair."""
    world, normals, _, M, V, first, num, feat, _, _ = _inputs(True, "h_cloud", SIZES)
    P = int(num.sum())
    h = _t((scenes.global_h(world.cpu().numpy()) * np.random.default_rng(9).uniform(0.5, 2.0, P)).astype(np.float32))
    _check(world, normals, h, M, V, first, num, feat, True, False)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("mode", ["h_cloud", "h_point", "aniso"])
def test_one_cloud_of_a_size_that_is_no_multiple_of_64_fused_equals_separate(mode, shared):
    world, normals, h, M, V, first, num, feat, vr6, fn = _inputs(shared, mode, (1301,))
    _check(world, normals, h, M, V, first, num, feat, shared, True, vr6, fn)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("mode", ["h_cloud", "h_point"])
def test_one_cloud_that_owns_only_the_middle_of_the_packed_points_fused_equals_separate(mode, shared):
    """One cloud with first_idx = 37 and 50 packed points behind its end: the points in front of it and behind it belong to
    no cloud (culled), so the first and the last wavefronts fall back to the per-lane lookup although N == 1; the wavefronts
    in between are uniform, and for the shared cloud row p of the world arrays -- requested before the lookup returned -- is
    not the point's row (p - 37): it has to be requested again."""
    world, normals, h, M, V, first, num, feat, vr6, fn = _inputs(shared, mode, (1301,))
    first = torch.tensor([37], device=DEV, dtype=torch.int64)
    num = torch.tensor([1301 - 37 - 50], device=DEV, dtype=torch.int64)
    _check(world, normals, h, M, V, first, num, feat, shared, True)
    info = ops.point_setup(world, normals, h, M, V, torch.full((1,), 0.6, device=DEV), torch.full((1,), 100.0, device=DEV),
                           first, num, S, 1.0, 1.0, True, shared)
    assert not info["valid"][:37].any() and not info["valid"][-50:].any() and info["valid"][37:-50].any()
