"""GPU: every path of the per-camera kNN statistic (knn.hip) against the fp64 references of knn_reference.py.

What test_gpu_knn.py does not reach: a wavefront of knn_fill_kernel that straddles two clouds, packed slots outside every
cloud, the dispatch of knn_run at either side of its size thresholds and with DSS_OPT_KNN_QUERY forced, many clouds, and the
edges of the per-camera order (scaled depth axis, points exactly on a depth plane, cameras that keep next to nothing).

Which test reaches which launch of knn_run ("matrix" = test_every_query_path_gives_the_reference_at_every_size_threshold, run
under DSS_OPT_KNN_QUERY = 0, 1, 2, 3 each; "straddle" = the two sizes of the shared-wavefront test):

  small build (P <= 131072, N <= 16, at most 160 scan blocks)   matrix P = 65535 / 65536, straddle (1000, 1500), gap tests
  eight-launch build: by size                                   matrix P >= 120000, straddle (99790, 99790)
  eight-launch build: more than 16 clouds at a small P          test_many_small_clouds_take_the_large_build N = 17, 70
  skip structure off / on (P >= 65536)                          matrix P = 65535 | P >= 65536; option 3 turns it off
  dense_flag down / up with the structure built                 matrix even, lumpy | clustered
  cooperative query, no skip / skip instance                    matrix P = 65535 | 65536 .. 120000 (option 0), all (option 1)
  one-thread query alone (role 0)                               matrix option 2 at P = 65535, option 3 at P >= 120001
  one-thread role 1 + cooperative role 2 pair                   matrix P >= 120001 (option 0), P >= 65536 (option 2)
  one-thread query with 64 / 256 threads per workgroup          matrix P <= 131072 | P = 131073
  K-th distance instances <8> / <16>                            matrix K = 1, 7, 8 | 9, 16
  full lists <8> / <12> / <16> / one-thread <40>                matrix K = 8 | 12 | 16 | 17, 40
  per-camera: unmasked search + masked search, both kernels     matrix (shared: even, clustered, lumpy; per cloud: split3)
  per-camera: two-row persistent grid, knn_view_rows_kernel     matrix shared kinds (camera 1 drops nothing: its row is a copy)
  knn_fill_kernel's flag, one leader per camera of a wavefront  straddle, middle-camera and drops-nothing tests
  renderable_sum / renderable_mean (64-camera stride)           many clouds N = 70, edge tests, layouts test"""
import numpy as np
import pytest
import torch

import knn_reference as ref
import scenes
from dss_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K7, R02 = 7, 0.2


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _with_query_option(value, fn):
    _lib.set_option(_lib.OPT_KNN_QUERY, value)
    try:
        return fn()
    finally:
        _lib.set_option(_lib.OPT_KNN_QUERY, 0)


def _pack(clouds):
    pts = np.concatenate(clouds, 0).astype(np.float32)
    num = np.array([c.shape[0] for c in clouds], np.int64)
    return pts, np.cumsum(num) - num, num


def _sphere(rng, n, radius=0.5):
    v = rng.normal(size=(n, 3))
    return (radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _cut(depth_sorted, n_drop, ascending):
    """a near plane between the n_drop-th and the next point of a depth-sorted cloud (fp32), dropping the n_drop nearest"""
    d = depth_sorted.astype(np.float64)
    a, b = (d[n_drop - 1], d[n_drop]) if ascending else (d[-n_drop], d[-n_drop - 1])
    # three products below 1 and three sums below 2, each rounded once at most: the fp32 depth is within 2e-7 of the exact one
    # however the expression is contracted, and the plane is at least 5e-7 from both points -- the kept set is unambiguous
    assert b - a >= 1e-6, (a, b)
    return np.float32(0.5 * (a + b))


# ----------------------------------------------------------------------------------------------------------------------
# the reference itself
# ----------------------------------------------------------------------------------------------------------------------
def test_kdtree_reference_agrees_with_brute_force():
    """the KD-tree references against an O(P^2) fp64 brute force, once, on clouds of at most 4,000 points (surface, volume,
    duplicates, fewer points than K): the suite's reference does not rest on scipy alone"""
    rng = np.random.default_rng(3)
    clouds = [_sphere(rng, 4000), rng.uniform(-1, 1, (2500, 3)).astype(np.float32),
              np.repeat(rng.uniform(0, 1, (60, 3)), 4, 0).astype(np.float32), rng.uniform(0, 1, (4, 3)).astype(np.float32)]
    for c in clouds:
        for K in (1, 7, 8, 16):
            assert np.allclose(ref.kth(c, K), ref.brute_kth(c, K), rtol=1e-6, atol=1e-12)
        for r in (0.2, 0.05):
            a, b = ref.radius_stat(c, 7, r), ref.brute_radius_stat(c, 7, r)
            assert ((a < 0) == (b < 0)).all() and np.allclose(a, b, rtol=1e-6, atol=1e-12)
    # and the kernel against the brute force directly
    pts, first, num = _pack(clouds)
    got = ops.knn_kth_sqdist(t(pts), t(first), t(num), 7).cpu().numpy()
    ref.assert_stat_close(got, np.concatenate([ref.brute_kth(c, 7) for c in clouds]), "kernel vs brute force")


# ----------------------------------------------------------------------------------------------------------------------
# defect 1: a wavefront of knn_fill_kernel that straddles two clouds (one cloud per camera)
# ----------------------------------------------------------------------------------------------------------------------
_CAMS3 = ([1.6, 1.6, 1.6], [10.0, 40.0, -20.0], [0.0, 120.0, 250.0])


def _straddle_scene(sizes, drops, seed=21, radius=0.5):
    """Clouds on a sphere of `radius`, one camera each.  Cloud n is sorted by its camera's view depth -- descending for even
    n, ascending for odd n -- and `drops[n]` of its nearest points lie in front of the camera's near plane: the LAST points
    of an even cloud, the FIRST points of an odd one.  With sizes[n] % 64 != 0 the dropped points of an odd cloud share their
    wavefront with the dropped points of the even cloud before it, at higher lanes.
    -> clouds, V (N,4,4), znear, zfar"""
    N = len(sizes)
    rng = np.random.default_rng(seed)
    _, V, _ = scenes.camera_matrices(_CAMS3[0][:N], _CAMS3[1][:N], _CAMS3[2][:N])
    clouds, znear = [], []
    for n in range(N):
        c = _sphere(rng, sizes[n], radius)
        z = ref.view_depth32(c, V[n])
        order = np.argsort(z, kind="stable")
        order = order if n % 2 else order[::-1]
        c = np.ascontiguousarray(c[order])
        clouds.append(c)
        znear.append(_cut(ref.view_depth32(c, V[n]), drops[n], ascending=bool(n % 2)) if drops[n] else np.float32(0.01))
    return clouds, V, np.array(znear, np.float32), np.full(N, 100.0, np.float32)


def _hidden_drop_count(cloud, V_n, zn, zf):
    """kept points whose statistic among the kept points differs from the one in the whole cloud by more than ten times the
    tolerance (reference alone): what a lost "drops points" flag gets wrong"""
    ok, masked = ref.view_stat(cloud, V_n, zn, zf, K7, R02)
    plain = ref.radius_stat(cloud, K7, R02)[ok]
    return int((~np.isclose(masked, plain, rtol=10 * ref.DIST_RTOL, atol=ref.DIST_ATOL)).sum())


def _check_per_cloud(clouds, V, znear, zfar, got, what):
    pts, first, num = _pack(clouds)
    for n, c in enumerate(clouds):
        assert ref.plane_gap(c, V[n], znear[n], zfar[n]) > 4e-7
        _, row = ref.view_row(c, V[n], znear[n], zfar[n], K7, R02)
        ref.assert_stat_close(got[first[n]:first[n] + num[n]], row, (what, "cloud", n))


@pytest.mark.parametrize("sizes", [(1000, 1500), (99790, 99790)], ids=["small_build_coop", "large_build_one_thread"])
def test_camera_whose_drops_share_a_wavefront_with_the_previous_clouds_is_flagged(sizes):
    """One cloud per camera; camera 0 drops the last 5 points of cloud 0 and camera 1 exactly the first 12 of cloud 1: all of
    camera 1's dropped points sit in the wavefront of knn_fill_kernel that also holds dropped points of cloud 0 at lower
    lanes.  Camera 1's "drops points" flag must still go up, or every query of cloud 1 gets the statistic of the WHOLE
    cloud.  (1000, 1500): small build, cooperative query; (99790, 99790): large build, one-thread query + the role pair."""
    assert sizes[0] % 64 != 0 and 64 - sizes[0] % 64 >= 12
    clouds, V, znear, zfar = _straddle_scene(sizes, (5, 12))
    assert _hidden_drop_count(clouds[1], V[1], znear[1], zfar[1]) >= 10    # the scene shows the defect
    pts, first, num = _pack(clouds)
    for q in (0, 1, 2):
        got = _with_query_option(q, lambda: ops.knn_kth_sqdist_view(t(pts), t(first), t(num), K7, t(V), t(znear), t(zfar), False,
                                                                     radius=R02)).cpu().numpy()
        _check_per_cloud(clouds, V, znear, zfar, got, ("query option", q))


def test_middle_camera_whose_drops_are_hidden_between_two_flagged_ones():
    """three clouds; cameras 0 and 2 drop the last 5 points of their clouds (their own last wavefronts flag them), camera 1
    the first 12 of its cloud, behind cloud 0's in the same wavefront"""
    clouds, V, znear, zfar = _straddle_scene((1000, 1500, 700), (5, 12, 5))
    assert _hidden_drop_count(clouds[1], V[1], znear[1], zfar[1]) >= 10
    pts, first, num = _pack(clouds)
    for q in (1, 2):
        got = _with_query_option(q, lambda: ops.knn_kth_sqdist_view(t(pts), t(first), t(num), K7, t(V), t(znear), t(zfar), False,
                                                                     radius=R02)).cpu().numpy()
        _check_per_cloud(clouds, V, znear, zfar, got, ("query option", q))


def test_camera_that_drops_nothing_next_to_one_that_does_keeps_the_plain_search():
    """camera 0 drops the last 5 points of cloud 0, camera 1 nothing: its flag must stay down -- the slots of cloud 1 hold the
    plain search, bit for bit"""
    clouds, V, znear, zfar = _straddle_scene((1000, 1500), (5, 0))
    pts, first, num = _pack(clouds)
    got = ops.knn_kth_sqdist_view(t(pts), t(first), t(num), K7, t(V), t(znear), t(zfar), False, radius=R02)
    plain = ops.knn_kth_sqdist(t(pts), t(first), t(num), K7, radius=R02)
    assert torch.equal(got[1000:], plain[1000:])
    assert not torch.equal(got[:1000], plain[:1000])
    _check_per_cloud(clouds, V, znear, zfar, got.cpu().numpy(), "")


@pytest.mark.parametrize("mode", ["invariant", "isotropic"])
@pytest.mark.parametrize("sizes", [(1000, 1500), (99790, 99790)], ids=["small", "large"])
def test_render_of_two_clouds_whose_drops_share_a_wavefront(sizes, mode):
    """end to end: SurfaceSplatting with two DIFFERENT clouds, the masked path against the reference's drop-then-search order
    (`compact_culled=True`): same variance scale, same alpha plane"""
    from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
    from dss_amd.cloud import PointClouds3D
    from dss_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting
    from dss_amd.renderer import NormWeightedCompositor, SurfaceSplattingRenderer
    # (sphere radii at which neither mode's clamp of h hides the statistic: mean h = 5e-4 resp. 1.2e-4)
    clouds, V, znear, zfar = _straddle_scene(sizes, (5, 12), radius=0.25 if sizes[0] == 1000 else 1.0)
    assert _hidden_drop_count(clouds[1], V[1], znear[1], zfar[1]) >= 10
    R, T = look_at_view_transform(_CAMS3[0][:2], _CAMS3[1][:2], _CAMS3[2][:2])
    cams = FoVPerspectiveCameras(fov=60.0, R=R, T=T, device=DEV)
    assert np.array_equal(cams.get_world_to_view_transform().get_matrix().cpu().numpy().astype(np.float32), V)
    cams.znear, cams.zfar = t(znear), t(zfar)
    st = PointsRasterizationSettings(backface_culling=False, cutoff_threshold=1.0, depth_merging_threshold=0.05,
                                     Vrk_invariant=mode == "invariant", Vrk_isotropic=mode == "isotropic",
                                     radii_backward_scaler=5.0, image_size=128, points_per_pixel=5, bin_size=None,
                                     clip_pts_grad=0.05, antialiasing_sigma=1.0)
    gen = torch.Generator().manual_seed(1)
    cols = [torch.rand((c.shape[0], 3), generator=gen).to(DEV) for c in clouds]
    nrms = [t(c / np.linalg.norm(c, axis=1, keepdims=True)) for c in clouds]
    images, hs = {}, {}
    for compact in (False, True):
        ras = SurfaceSplatting(cameras=cams, raster_settings=st, compact_culled=compact)
        ren = SurfaceSplattingRenderer(ras, NormWeightedCompositor())
        with torch.no_grad():
            images[compact] = ren(PointClouds3D([t(c) for c in clouds], nrms, cols))
        hs[compact] = ras._Vrk_h.clone()
    if mode == "invariant":
        assert hs[False].numel() == 2
        assert torch.allclose(hs[False], hs[True], rtol=1e-6), (hs[False], hs[True])
        assert 5e-5 < float(hs[False].min()) and float(hs[False].max()) < 1e-3, hs[False]   # not clamped away
    else:   # one h per point: the masked path keeps the dropped points' slots, the other order has dropped them
        ok = np.concatenate([ref.view_stat(c, V[n], znear[n], zfar[n], K7, R02)[0] for n, c in enumerate(clouds)])
        assert hs[False].numel() == ok.size and hs[True].numel() == int(ok.sum())
        assert torch.allclose(hs[False][t(ok)], hs[True], rtol=1e-6), float((hs[False][t(ok)] - hs[True]).abs().max())
        assert float(((hs[True] > 5e-5) & (hs[True] < 0.01)).float().mean()) > 0.9   # not clamped away
    a, b = images[False], images[True]
    assert a.shape == b.shape and float(a[..., 3].sum()) > 500
    assert torch.equal(a[..., 3], b[..., 3]) and float((a - b).abs().max()) <= 1e-6, float((a - b).abs().max())


# ----------------------------------------------------------------------------------------------------------------------
# defect 2: packed slots outside every cloud
# ----------------------------------------------------------------------------------------------------------------------
def _raw_view(pts, first, num, K, V, znear, zfar, shared, radius):
    """dss_knn_kth_sqdist_view through the C ABI like ops.knn_kth_sqdist_view, into an output pre-filled with NaN"""
    lib = _lib.load()
    P_, F_, N_, V_, zn_, zf_ = t(pts), t(first), t(num), t(V), t(znear), t(zfar)
    N, P, n_cams = len(first), pts.shape[0], V.shape[0]
    dev = P_.device
    with torch.cuda.device(dev):
        out = torch.full((n_cams, P) if shared else (P,), float("nan"), dtype=torch.float32, device=dev)
        ws = _lib.workspace(dev, lib.dss_knn_workspace(N, P))
        rc = lib.dss_knn_kth_sqdist_view(_lib.ptr(P_), _lib.ptr(F_), _lib.ptr(N_), N, P, int(K), float(radius) if radius else -1.0,
                                         _lib.ptr(V_), _lib.ptr(zn_), _lib.ptr(zf_), n_cams, int(shared), _lib.ptr(out), _lib.ptr(ws),
                                         ws.numel(), _lib.stream_ptr(dev))
    _lib.check(rc, "dss_knn_kth_sqdist_view")
    return out.cpu().numpy()


def _raw_plain(pts, first, num, K, radius=None, full=False):
    """dss_knn_kth_sqdist[_radius] / dss_knn_points through the C ABI into outputs pre-filled with NaN (ids: -7)"""
    lib = _lib.load()
    P_, F_, N_ = t(pts), t(first), t(num)
    N, P = len(first), pts.shape[0]
    dev = P_.device
    with torch.cuda.device(dev):
        ws = _lib.workspace(dev, lib.dss_knn_workspace(N, P))
        if full:
            d = torch.full((P, K), float("nan"), dtype=torch.float32, device=dev)
            i = torch.full((P, K), -7, dtype=torch.int64, device=dev)
            rc = lib.dss_knn_points(_lib.ptr(P_), _lib.ptr(F_), _lib.ptr(N_), N, P, int(K), _lib.ptr(d), _lib.ptr(i), _lib.ptr(ws),
                                    ws.numel(), _lib.stream_ptr(dev))
            _lib.check(rc, "dss_knn_points")
            return d.cpu().numpy(), i.cpu().numpy()
        out = torch.full((P,), float("nan"), dtype=torch.float32, device=dev)
        if radius:
            rc = lib.dss_knn_kth_sqdist_radius(_lib.ptr(P_), _lib.ptr(F_), _lib.ptr(N_), N, P, int(K), float(radius), _lib.ptr(out),
                                               _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        else:
            rc = lib.dss_knn_kth_sqdist(_lib.ptr(P_), _lib.ptr(F_), _lib.ptr(N_), N, P, int(K), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                        _lib.stream_ptr(dev))
    _lib.check(rc, "dss_knn_kth_sqdist")
    return out.cpu().numpy()


def _with_gaps(clouds, gaps):
    """packed layout with gaps[n] unused slots before cloud n and gaps[-1] behind the last one; the unused slots hold NaN
    positions (nothing may read them) -> pts, first, num, covered (P,) bool"""
    parts, first = [], []
    at = 0
    for c, g in zip(clouds, gaps):
        parts.append(np.full((g, 3), np.nan, np.float32))
        at += g
        first.append(at)
        parts.append(c.astype(np.float32))
        at += c.shape[0]
    parts.append(np.full((gaps[-1], 3), np.nan, np.float32))
    pts = np.concatenate(parts, 0)
    num = np.array([c.shape[0] for c in clouds], np.int64)
    first = np.array(first, np.int64)
    covered = np.zeros(pts.shape[0], bool)
    for f, n in zip(first, num):
        covered[f:f + n] = True
    return pts, first, num, covered


@pytest.mark.parametrize("query", [0, 2], ids=["by_size", "one_thread"])
@pytest.mark.parametrize("P", [3000, 70000])
def test_slots_outside_the_shared_cloud_are_zero_in_every_cameras_row(P, query):
    """first_idx = [7], num_pts = [P - 20]: seven packed slots before the cloud and thirteen behind it; three cameras of which
    two drop points.  No row of the (cameras, P) result keeps what the output held before the call."""
    cloud = _sphere(np.random.default_rng(4), P - 20)
    pts, first, num, covered = _with_gaps([cloud], (7, 13))
    assert pts.shape[0] == P and first[0] == 7 and num[0] == P - 20
    _, V, _ = scenes.camera_matrices(*_CAMS3)
    znear, zfar = np.array([1.3, 0.01, 1.5], np.float32), np.array([100.0, 100.0, 1.9], np.float32)
    for r in (R02, None):
        got = _with_query_option(query, lambda: _raw_view(pts, first, num, K7, V, znear, zfar, True, r))
        assert got.shape == (3, P) and not np.isnan(got).any(), np.isnan(got).sum(1)
        assert (got[:, ~covered] == 0).all()
        for n in range(3):
            assert ref.plane_gap(cloud, V[n], znear[n], zfar[n]) > 4e-7
            ok, row = ref.view_row(cloud, V[n], znear[n], zfar[n], K7, r)
            assert bool(ok.all()) == (n == 1) and ok.sum() > 100
            ref.assert_stat_close(got[n, covered], row, ("camera", n, "radius", r))


@pytest.mark.parametrize("query", [0, 2], ids=["by_size", "one_thread"])
def test_slots_between_clouds_are_zero_in_every_entry(query):
    """gaps before, between and behind three clouds: the per-cloud view entry, the plain and fixed-radius K-th distance and the
    full lists write zeros there and the clouds' own results everywhere else"""
    rng = np.random.default_rng(8)
    clouds = [_sphere(rng, 1500), _sphere(rng, 777, 0.4), rng.uniform(-0.5, 0.5, (2101, 3)).astype(np.float32)]
    pts, first, num, covered = _with_gaps(clouds, (5, 70, 1, 130))
    _, V, _ = scenes.camera_matrices(*_CAMS3)
    znear, zfar = np.array([1.3, 0.01, 1.5], np.float32), np.array([100.0, 100.0, 1.9], np.float32)
    got = _with_query_option(query, lambda: _raw_view(pts, first, num, K7, V, znear, zfar, False, R02))
    assert not np.isnan(got).any() and (got[~covered] == 0).all()
    for n, c in enumerate(clouds):
        assert ref.plane_gap(c, V[n], znear[n], zfar[n]) > 4e-7
        ref.assert_stat_close(got[first[n]:first[n] + num[n]], ref.view_row(c, V[n], znear[n], zfar[n], K7, R02)[1], ("view", n))
    for r in (None, R02):
        got = _with_query_option(query, lambda: _raw_plain(pts, first, num, K7, r))
        assert not np.isnan(got).any() and (got[~covered] == 0).all()
        ref.assert_stat_close(got[covered], np.concatenate([ref.stat(c, K7, r) for c in clouds]), ("plain", r))
    for K in (8, 17):
        d, i = _with_query_option(query, lambda: _raw_plain(pts, first, num, K, full=True))
        assert not np.isnan(d).any() and (d[~covered] == 0).all() and (i[~covered] == 0).all()
        for n, c in enumerate(clouds):
            want = ref.sorted_sq(c, K)
            assert np.allclose(d[first[n]:first[n] + num[n]], want, rtol=ref.DIST_RTOL, atol=ref.DIST_ATOL)
            ids = i[first[n]:first[n] + num[n]]
            assert (ids >= 0).all() and (ids < num[n]).all() and (ids[:, 0] == np.arange(num[n])).all()


# ----------------------------------------------------------------------------------------------------------------------
# the dispatch of knn_run: every query option at either side of every size threshold, every entry
# ----------------------------------------------------------------------------------------------------------------------
def _plane_near(cloud, V_n, target):
    """a depth plane close to `target`, in the middle of the widest gap between the depths of the 200 points around it: the
    kept set does not hang on the rounding of a depth"""
    c, V = cloud.astype(np.float64), V_n.astype(np.float64)
    z = np.sort(c[:, 0] * V[0, 2] + c[:, 1] * V[1, 2] + c[:, 2] * V[2, 2] + V[3, 2])
    i = int(np.searchsorted(z, target))
    lo, hi = max(i - 100, 0), min(i + 100, len(z))
    if hi - lo < 2:
        return np.float32(target)
    w = z[lo:hi]
    j = int(np.argmax(np.diff(w)))
    return np.float32(0.5 * (w[j] + w[j + 1]))


def _clustered(P, seed=7):
    """the recipe of the synthetic clustered cloud of test_gpu_knn.py at P points (that one has 64,300): a blob with more than
    4,096 points in one cell (not sub-sorted), a shell, a clump, exact duplicates and far outliers, shuffled -- well over an
    eighth of the points live in dense cells, so `dense_flag` goes up from 65,536 points on"""
    rng = np.random.default_rng(seed)
    n_blob, n_far = 12000, 300
    n_dup = 4 * ((P - n_blob - n_far) // 100)
    n_shell = (P - n_blob - n_far - n_dup) * 3 // 5
    n_clump = P - n_blob - n_far - n_dup - n_shell
    blob = rng.normal(0, 0.004, (n_blob, 3))
    shell = rng.normal(0, 1, (n_shell, 3))
    shell = 0.4 * shell / np.linalg.norm(shell, axis=1, keepdims=True)
    clump = rng.normal(0, 0.02, (n_clump, 3)) + [0.3, 0.1, -0.2]
    dup = np.repeat(rng.uniform(-0.05, 0.05, (n_dup // 4, 3)), 4, 0)
    far = rng.uniform(-3, 3, (n_far, 3))
    out = np.concatenate([blob, shell, clump, dup, far]).astype(np.float32)
    assert out.shape[0] == P
    return out[rng.permutation(P)]


def _matrix_clouds(kind, P):
    if kind == "even":
        return [scenes.synthetic_cloud(P, seed=P % 89)[0]]
    if kind == "split3":   # the same P as three unequal clouds whose sizes are no multiples of 64
        base = scenes.synthetic_cloud(P, seed=P % 83)[0]
        n0, n1 = P // 2 + 3, (3 * P) // 10 + 1
        sizes = (n0, n1, P - n0 - n1)
        assert all(s % 64 != 0 for s in sizes), sizes
        return [base[:n0], base[n0:n0 + n1] * 0.8 + 0.1, base[n0 + n1:] * 1.1 - 0.2]
    if kind == "clustered":
        return [_clustered(P)]
    if kind == "lumpy":    # dense cells (listed, sub-sorted) that hold less than an eighth of the points: `dense_flag` stays down
        rng = np.random.default_rng(P % 79)
        blob = (rng.normal(0, 0.003, (5000, 3)) + [0.0, 0.0, 0.9]).astype(np.float32)
        return [np.concatenate([scenes.synthetic_cloud(P - 5000, seed=5)[0], blob])[rng.permutation(P)]]
    raise ValueError(kind)


_MATRIX = [(kind, P) for kind in ("even", "split3", "clustered") for P in (65535, 65536, 120000, 120001, 131072, 131073)] + \
          [("lumpy", 65536), ("lumpy", 131073)]


def _all_query_options(fn):
    """fn() under DSS_OPT_KNN_QUERY = 0 (by size), 1 (cooperative), 2 (one thread per query), 3 (by size, no skip structure):
    bit-identical results required; -> the result of option 0"""
    outs = [_with_query_option(q, fn) for q in (0, 1, 2, 3)]
    for q, o in enumerate(outs[1:], 1):
        for a, b in zip(outs[0] if isinstance(outs[0], tuple) else (outs[0],), o if isinstance(o, tuple) else (o,)):
            assert torch.equal(a, b), ("query option", q, int((a != b).sum()))
    return outs[0]


@pytest.mark.parametrize("kind,P", _MATRIX, ids=["%s-%d" % kp for kp in _MATRIX])
def test_every_query_path_gives_the_reference_at_every_size_threshold(kind, P):
    """knn_run chooses by size: the skip structure from 65,536 points, the cooperative query up to 120,000, the small build up to
    131,072 -- and by DSS_OPT_KNN_QUERY.  Every entry, at either side of every threshold, under every option: the fp64
    KD-tree's answer, and the same bits whatever the path."""
    clouds = _matrix_clouds(kind, P)
    pts, first, num = _pack(clouds)
    assert pts.shape[0] == P
    Pt, Ft, Nt = t(pts), t(first), t(num)
    tabs = [ref.sorted_sq(c, 40) for c in clouds]    # one KD-tree query per cloud serves every K
    # K-th distance (K = 8 / 9: the template instance changes), fixed radius
    for K, r in ((1, None), (7, None), (8, None), (9, None), (16, None), (7, R02)):
        got = _all_query_options(lambda: ops.knn_kth_sqdist(Pt, Ft, Nt, K, radius=r)).cpu().numpy()
        want = np.concatenate([ref.stat_from_sorted(tab, c.shape[0], K, r) for tab, c in zip(tabs, clouds)])
        ref.assert_stat_close(got, want, ("kth", K, r))
    # full lists (K = 8 / 12 / 16 / 17: the template instance changes)
    own_first = t(np.repeat(first, num))
    for K in (8, 12, 16, 17, 40):
        d, i = _all_query_options(lambda: ops.knn_points(Pt, Ft, Nt, K))
        want = np.concatenate([tab[:, :K] for tab in tabs])
        dn = d.cpu().numpy()
        assert np.allclose(dn, want, rtol=ref.DIST_RTOL, atol=ref.DIST_ATOL), (K, float(np.abs(dn - want).max()))
        assert bool((d[:, 1:] >= d[:, :-1]).all()) and bool((d[:, 0] == 0).all())
        assert bool((i >= 0).all()) and bool((i < t(np.repeat(num, num))[:, None]).all())
        # a listed neighbour really is at the listed distance
        diff = Pt[own_first[:, None] + i].double() - Pt[:, None, :].double()
        assert torch.allclose((diff ** 2).sum(-1), d.double(), rtol=ref.DIST_RTOL, atol=ref.DIST_ATOL), K
    # per-camera order: one shared cloud under three cameras, or one cloud per camera
    shared = len(clouds) == 1
    _, V, _ = scenes.camera_matrices(*_CAMS3)
    cam_cloud = [clouds[0] if shared else clouds[n] for n in range(3)]
    znear = np.array([_plane_near(cam_cloud[0], V[0], 1.3), -100.0, _plane_near(cam_cloud[2], V[2], 1.5)], np.float32)
    zfar = np.array([100.0, 100.0, _plane_near(cam_cloud[2], V[2], 1.9)], np.float32)
    # (camera 1 drops nothing, not even the outliers of the clustered cloud behind it)
    kept = []
    for n in range(3):
        assert ref.plane_gap(cam_cloud[n], V[n], znear[n], zfar[n]) > 4e-7
        z = ref.view_depth32(cam_cloud[n], V[n])
        ok = (z >= znear[n]) & (z <= zfar[n])
        assert bool(ok.all()) == (n == 1) and ok.sum() > 1000
        kept.append((ok, ref.sorted_sq(cam_cloud[n][ok], 8)))
    Vt, zn, zf = t(V), t(znear), t(zfar)
    for K, r in ((1, R02), (7, R02), (8, R02), (7, None)):
        got = _all_query_options(lambda: ops.knn_kth_sqdist_view(Pt, Ft, Nt, K, Vt, zn, zf, shared, radius=r)).cpu().numpy()
        assert got.shape == ((3, P) if shared else (P,))
        for n in range(3):
            ok, tab = kept[n]
            row = np.zeros(ok.size, np.float32)
            row[ok] = ref.stat_from_sorted(tab, int(ok.sum()), K, r)
            ref.assert_stat_close(got[n] if shared else got[first[n]:first[n] + num[n]], row, ("view", K, r, "camera", n))


def test_k_beyond_an_entrys_limit_is_refused_and_nothing_is_written():
    """K = 9 on the per-camera entry (DSS_ERR_UNSUPPORTED), K = 17 on the K-th distance and K = 41 on the full lists
    (DSS_ERR_INVALID_ARGUMENT): an error through `ops`, a negative status at the C ABI, and the outputs as they were"""
    lib = _lib.load()
    cloud = _sphere(np.random.default_rng(1), 3000)
    pts, first, num = _pack([cloud])
    Pt, Ft, Nt = t(pts), t(first), t(num)
    _, V, _ = scenes.camera_matrices(*_CAMS3)
    Vt, zn, zf = t(V), t(np.array([1.3, 0.01, 1.5], np.float32)), t(np.full(3, 100.0, np.float32))
    with pytest.raises(RuntimeError):
        ops.knn_kth_sqdist_view(Pt, Ft, Nt, 9, Vt, zn, zf, True, radius=R02)
    with pytest.raises(RuntimeError):
        ops.knn_kth_sqdist(Pt, Ft, Nt, 17)
    with pytest.raises(RuntimeError):
        ops.knn_kth_sqdist(Pt, Ft, Nt, 17, radius=R02)
    with pytest.raises(RuntimeError):
        ops.knn_points(Pt, Ft, Nt, 41)
    dev = Pt.device
    with torch.cuda.device(dev):
        ws = _lib.workspace(dev, lib.dss_knn_workspace(1, 3000))
        out = torch.full((3, 3000), float("nan"), device=dev)
        d = torch.full((3000, 41), float("nan"), device=dev)
        i = torch.full((3000, 41), -7, dtype=torch.int64, device=dev)
        st = _lib.stream_ptr(dev)
        rc = lib.dss_knn_kth_sqdist_view(_lib.ptr(Pt), _lib.ptr(Ft), _lib.ptr(Nt), 1, 3000, 9, 0.2, _lib.ptr(Vt), _lib.ptr(zn),
                                         _lib.ptr(zf), 3, 1, _lib.ptr(out), _lib.ptr(ws), ws.numel(), st)
        assert rc == -3, rc    # DSS_ERR_UNSUPPORTED
        rc = lib.dss_knn_kth_sqdist(_lib.ptr(Pt), _lib.ptr(Ft), _lib.ptr(Nt), 1, 3000, 17, _lib.ptr(out), _lib.ptr(ws), ws.numel(), st)
        assert rc == -1, rc    # DSS_ERR_INVALID_ARGUMENT
        rc = lib.dss_knn_points(_lib.ptr(Pt), _lib.ptr(Ft), _lib.ptr(Nt), 1, 3000, 41, _lib.ptr(d), _lib.ptr(i), _lib.ptr(ws),
                                ws.numel(), st)
        assert rc == -1, rc
        torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(d).all()) and bool((i == -7).all())


def _many_clouds(N, seed):
    """N small clouds of 20 to 900 points (no multiples of 64), some empty, some with fewer than K = 7 points; a few
    centimetres across, so that the variance scale of most of them lies inside its clamp"""
    rng = np.random.default_rng(seed)
    clouds = []
    for n in range(N):
        size = 0 if n % 9 == 4 else (int(rng.integers(1, 7)) if n % 7 == 2 else int(rng.integers(20, 901)))
        size += 1 if (size and size % 64 == 0) else 0
        kindn = n % 3
        c = _sphere(rng, size, 0.05 + 0.001 * n) if kindn == 0 else rng.uniform(-0.06, 0.06, (size, 3)).astype(np.float32)
        if kindn == 2 and size >= 8:
            c[size // 2:size // 2 + 4] = c[0]    # a few exact duplicates
        clouds.append(c)
    return clouds


@pytest.mark.parametrize("N", [17, 70])
def test_many_small_clouds_take_the_large_build(N):
    """more than 16 clouds: the eight-launch build at a small P, find_cloud over many clouds, one camera per cloud, and (70
    cameras) the 64-camera stride of renderable_mean_kernel"""
    clouds = _many_clouds(N, 40 + N)
    pts, first, num = _pack(clouds)
    assert (num == 0).sum() >= 1 and ((num > 0) & (num < K7)).sum() >= 2 and (num % 64 != 0)[num > 0].all()
    Pt, Ft, Nt = t(pts), t(first), t(num)
    for K, r in ((7, None), (7, R02), (16, None)):
        got = _all_query_options(lambda: ops.knn_kth_sqdist(Pt, Ft, Nt, K, radius=r)).cpu().numpy()
        ref.assert_stat_close(got, np.concatenate([ref.stat(c, K, r) for c in clouds]), ("kth", K, r))
    d, i = _all_query_options(lambda: ops.knn_points(Pt, Ft, Nt, 12))
    want = np.concatenate([ref.sorted_sq(c, 12) for c in clouds])
    assert np.allclose(d.cpu().numpy(), want, rtol=ref.DIST_RTOL, atol=ref.DIST_ATOL)
    assert bool((i >= 0).all()) and bool((i < t(np.repeat(np.maximum(num, 1), num))[:, None]).all())
    # one camera per cloud, all looking down +z from z = -2 + 0.01 n with their own depth ranges
    V = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    V[:, 3, 2] = 2.0 + 0.01 * np.arange(N, dtype=np.float32)
    znear = np.array([0.01 if n % 4 == 0 else _plane_near(clouds[n], V[n], V[n, 3, 2] - 0.02) for n in range(N)], np.float32)
    zfar = np.array([100.0 if n % 3 else _plane_near(clouds[n], V[n], V[n, 3, 2] + 0.03) for n in range(N)], np.float32)
    got = _all_query_options(lambda: ops.knn_kth_sqdist_view(Pt, Ft, Nt, K7, t(V), t(znear), t(zfar), False, radius=R02)).cpu().numpy()
    stats, counts = [], []
    for n, c in enumerate(clouds):
        assert ref.plane_gap(c, V[n], znear[n], zfar[n]) > 4e-7
        ok, row = ref.view_row(c, V[n], znear[n], zfar[n], K7, R02)
        ref.assert_stat_close(got[first[n]:first[n] + num[n]], row, ("view", n))
        stats.append(row[ok])
        counts.append(int(ok.sum()))
    assert min(counts) == 0 and sum(0 < c < K7 for c in counts) >= 2 and sum(c < s for c, s in zip(counts, num)) >= N // 3
    h = ops.renderable_mean_clamp(t(got), Pt, t(V), t(znear), t(zfar), Ft, Nt, False, 0.5, 5e-5, 1e-3, 0.5e-3, 7).cpu().numpy()
    want_h = ref.padded_mean_clamp(stats, counts, 0.5, 5e-5, 1e-3, 0.5e-3, 7)
    assert np.allclose(h, want_h, rtol=ref.MEAN_RTOL, atol=0), (h, want_h)
    assert ((want_h > 5e-5) & (want_h < 1e-3) & (want_h != np.float32(0.5e-3))).sum() >= N // 3    # not all clamped away


# ----------------------------------------------------------------------------------------------------------------------
# edges of the per-camera order
# ----------------------------------------------------------------------------------------------------------------------
_H = (0.5, 5e-5, 1e-3, 0.5e-3, 7)    # scale, lo, hi, fallback, min_points: what the rasterizer passes


def _view_both_kernels(pts, first, num, K, V, znear, zfar, shared, r):
    """the per-camera entry under the cooperative and the one-thread query: same bits -> numpy"""
    a = _with_query_option(1, lambda: ops.knn_kth_sqdist_view(t(pts), t(first), t(num), K, t(V), t(znear), t(zfar), shared, radius=r))
    b = _with_query_option(2, lambda: ops.knn_kth_sqdist_view(t(pts), t(first), t(num), K, t(V), t(znear), t(zfar), shared, radius=r))
    assert torch.equal(a, b), int((a != b).sum())
    return a.cpu().numpy()


def _check_view(clouds, shared, V, znear, zfar, got, K=K7, r=R02, gap=4e-7):
    """rows against `view_stat` -> (statistic of the kept points, kept count) per camera"""
    _, first, num = _pack(clouds)
    stats, counts = [], []
    for n in range(V.shape[0]):
        c = clouds[0] if shared else clouds[n]
        assert gap is None or ref.plane_gap(c, V[n], znear[n], zfar[n]) > gap
        ok, row = ref.view_row(c, V[n], znear[n], zfar[n], K, r)
        ref.assert_stat_close(got[n] if shared else got[first[n]:first[n] + num[n]], row, ("camera", n))
        stats.append(row[ok])
        counts.append(int(ok.sum()))
    return stats, counts


def _mean_clamp(got, clouds, shared, V, znear, zfar):
    pts, first, num = _pack(clouds)
    N = V.shape[0]
    f1 = np.zeros(N, np.int64) if shared else first
    n1 = np.full(N, num[0], np.int64) if shared else num
    return ops.renderable_mean_clamp(t(got), t(pts), t(V), t(znear), t(zfar), t(f1), t(n1), shared, *_H).cpu().numpy()


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_cloud"])
@pytest.mark.parametrize("scale", [2.5, 0.3])
def test_depth_axis_that_is_no_unit_vector_gives_the_rigid_cameras_statistic(scale, shared):
    """the depth column of the view matrix times 2.5 / 0.3, znear and zfar scaled alike: the same kept set, so the same
    statistic as the rigid camera's, bit for bit -- the shortcut's margin must scale with the axis (knn_view_shortcut)"""
    base = scenes.synthetic_cloud(30011, seed=2)[0]
    clouds = [base] if shared else [base[:14001], base[14001:23003] * 0.8, base[23003:] * 1.1]
    _, V, _ = scenes.camera_matrices(*_CAMS3)
    cc = [clouds[0] if shared else clouds[n] for n in range(3)]
    znear = np.array([_plane_near(cc[0], V[0], 1.3), 0.01, _plane_near(cc[2], V[2], 1.5)], np.float32)
    zfar = np.array([100.0, _plane_near(cc[1], V[1], 1.8), _plane_near(cc[2], V[2], 1.9)], np.float32)
    pts, first, num = _pack(clouds)
    rigid = _view_both_kernels(pts, first, num, K7, V, znear, zfar, shared, R02)
    _, counts = _check_view(clouds, shared, V, znear, zfar, rigid)
    Vs = V.copy()
    Vs[:, :, 2] *= np.float32(scale)
    zn_s, zf_s = (znear * np.float32(scale)).astype(np.float32), (zfar * np.float32(scale)).astype(np.float32)
    scaled = _view_both_kernels(pts, first, num, K7, Vs, zn_s, zf_s, shared, R02)
    _, counts_s = _check_view(clouds, shared, Vs, zn_s, zf_s, scaled, gap=4e-7 * min(scale, 1.0))
    assert counts == counts_s and all(0 < k < c.shape[0] for k, c in zip(counts, cc))
    assert np.array_equal(rigid, scaled)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_cloud"])
def test_points_exactly_on_a_depth_plane_are_kept_and_counted(shared):
    """identity rotation, translation 2 along z: a point with z = -0.5 has view depth 1.5 = znear and one with z = 0.25 has
    2.25 = zfar, exactly, in fp32 -- the bounds are inclusive, in the search and in the count of renderable_mean_clamp"""
    rng = np.random.default_rng(13)

    def cloud(n):
        c = (rng.uniform(-1, 1, (n, 3)) * [0.1, 0.1, 0.6]).astype(np.float32)
        c[100:140, 2], c[300:340, 2] = -0.5, 0.25
        return c
    clouds = [cloud(6000)] if shared else [cloud(6000), cloud(2500)]
    N = 2
    V = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    V[:, 3, 2] = 2.0
    znear, zfar = np.array([1.5, 1.5], np.float32), np.array([2.25, 100.0], np.float32)
    pts, first, num = _pack(clouds)
    got = _view_both_kernels(pts, first, num, K7, V, znear, zfar, shared, R02)
    stats, counts = _check_view(clouds, shared, V, znear, zfar, got, gap=None)   # (z + 2 is ONE rounding: no ambiguity)
    for n in range(N):
        c = clouds[0] if shared else clouds[n]
        ok, _ = ref.view_stat(c, V[n], znear[n], zfar[n], K7, R02)
        assert ok[100:140].all() and ok[300:340].all() and 0 < ok.sum() < c.shape[0]
        mine = got[n] if shared else got[first[n]:first[n] + num[n]]
        assert (mine[100:140] != 0).all() and (mine[300:340] != 0).all() and (mine[~ok] == 0).all()
    h = _mean_clamp(got, clouds, shared, V, znear, zfar)
    want = ref.padded_mean_clamp(stats, counts, *_H)
    # a count that missed the 40 on-plane points of the largest kept set would move the mean by 40 / ~2000
    assert np.allclose(h, want, rtol=ref.MEAN_RTOL, atol=0) and ((want > 5e-5) & (want < 1e-3)).all(), (h, want)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_cloud"])
def test_cameras_that_keep_next_to_nothing(shared):
    """cameras that keep 0 points, 1, K - 1 = min_points - 1, min_points and all of them: rows, the fallback of the cameras
    below min_points, and the mean over the padded batch; then every camera keeping nothing (largest kept count 0)"""
    rng = np.random.default_rng(14)
    keeps = (0, 1, K7 - 1, _H[4], None, 400)
    N = len(keeps)
    clouds = [_sphere(rng, 3001, 0.45)] if shared else [_sphere(rng, 900 + 101 * n, 0.2) for n in range(N)]
    V = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    V[:, 3, 2] = 2.0
    znear, zfar = np.full(N, 0.01, np.float32), np.full(N, 100.0, np.float32)
    for n, k in enumerate(keeps):
        c = clouds[0] if shared else clouds[n]
        z = np.sort(c[:, 2].astype(np.float64) + 2.0)
        if k is not None:
            zfar[n] = np.float32(z[0] - 0.01 if k == 0 else 0.5 * (z[k - 1] + z[k]))
    pts, first, num = _pack(clouds)
    got = _view_both_kernels(pts, first, num, K7, V, znear, zfar, shared, R02)
    stats, counts = _check_view(clouds, shared, V, znear, zfar, got, gap=None)
    assert counts[:4] == [0, 1, K7 - 1, _H[4]] and counts[4] == (clouds[0] if shared else clouds[4]).shape[0] and counts[5] == 400
    h = _mean_clamp(got, clouds, shared, V, znear, zfar)
    want = ref.padded_mean_clamp(stats, counts, *_H)
    assert np.allclose(h, want, rtol=ref.MEAN_RTOL, atol=0), (h, want)
    assert (h[:3] == np.float32(_H[3])).all() and h[3] != np.float32(_H[3])
    assert 5e-5 < h[5] < h[4] < 1e-3, h     # (the padded mean: 400 kept points divided by the largest kept count)
    # nobody keeps anything
    zfar[:] = 0.5
    got = _view_both_kernels(pts, first, num, K7, V, znear, zfar, shared, R02)
    assert (got == 0).all()
    h = _mean_clamp(got, clouds, shared, V, znear, zfar)
    assert (h == np.float32(_H[3])).all() and (ref.padded_mean_clamp([[]] * N, [0] * N, *_H) == h).all()


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_cloud"])
def test_thin_slab_and_duplicates_on_the_kept_side(shared):
    """camera 0: a slab thinner than the spacing of the points (nearly every kept query is within reach of both planes: none
    may take the shortcut); camera 1: groups of eight identical points on the kept side (K-th distance 0: the shortcut with
    a reach of 0) next to a cut through the cloud"""
    rng = np.random.default_rng(15)

    def cloud(n):
        c = scenes.synthetic_cloud(n, seed=n % 71)[0]
        c[:320] = np.repeat(c[320:360], 8, 0)    # forty groups of eight identical points
        return c
    clouds = [cloud(60001)] if shared else [cloud(60001), cloud(20003)]
    _, V, _ = scenes.camera_matrices(_CAMS3[0][:2], _CAMS3[1][:2], _CAMS3[2][:2])
    c0, c1 = clouds[0], clouds[0] if shared else clouds[1]
    znear = np.array([_plane_near(c0, V[0], 1.600), _plane_near(c1, V[1], 1.45)], np.float32)
    zfar = np.array([_plane_near(c0, V[0], 1.604), 100.0], np.float32)
    pts, first, num = _pack(clouds)
    got = _view_both_kernels(pts, first, num, K7, V, znear, zfar, shared, R02)
    stats, counts = _check_view(clouds, shared, V, znear, zfar, got)
    assert 50 < counts[0] < 400 and 0 < counts[1] < c1.shape[0], counts
    ok1, _ = ref.view_stat(c1, V[1], znear[1], zfar[1], K7, R02)
    assert ok1[:320].sum() >= 80 and (stats[1] == 0).sum() >= 80      # kept duplicates: statistic 0 (not "dropped": kept and 0)
    got_plain = _view_both_kernels(pts, first, num, K7, V, znear, zfar, shared, None)
    _check_view(clouds, shared, V, znear, zfar, got_plain, r=None)
    h = _mean_clamp(got, clouds, shared, V, znear, zfar)
    assert np.allclose(h, ref.padded_mean_clamp(stats, counts, *_H), rtol=ref.MEAN_RTOL, atol=0)


def test_renderable_mean_clamp_layouts_against_an_fp64_sum():
    """values as (Pw,) and as (N, Pw), a shared cloud and one cloud per camera with first_idx[0] > 0, a cloud of more than
    4 * 32 * 1024 points (the four-way unrolled loop and its tail), the same bits on a second call"""
    rng = np.random.default_rng(16)
    big = scenes.synthetic_cloud(4 * 32 * 1024 + 4321, seed=4)[0]
    _, V, _ = scenes.camera_matrices(*_CAMS3)

    def want(vals_per_cam, cam_clouds, znear, zfar):
        stats, counts = [], []
        for n, c in enumerate(cam_clouds):
            assert ref.plane_gap(c, V[n], znear[n], zfar[n]) > 4e-7
            z = ref.view_depth32(c, V[n])
            ok = (z >= znear[n]) & (z <= zfar[n])
            stats.append(vals_per_cam[n][ok])
            counts.append(int(ok.sum()))
        assert len(set(counts)) == len(counts) and min(counts) > 1000
        return ref.padded_mean_clamp(stats, counts, *_H)

    # shared cloud
    znear = np.array([_plane_near(big, V[0], 1.3), 0.01, _plane_near(big, V[2], 1.5)], np.float32)
    zfar = np.array([100.0, _plane_near(big, V[1], 1.9), _plane_near(big, V[2], 2.0)], np.float32)
    f1, n1 = np.zeros(3, np.int64), np.full(3, big.shape[0], np.int64)
    v1 = rng.uniform(1e-4, 1.5e-3, big.shape[0]).astype(np.float32)
    v2 = rng.uniform(1e-4, 1.5e-3, (3, big.shape[0])).astype(np.float32)
    for vals, per_cam in ((v1, [v1] * 3), (v2, list(v2))):
        args = (t(vals), t(big), t(V), t(znear), t(zfar), t(f1), t(n1), True) + _H
        h = ops.renderable_mean_clamp(*args)
        assert torch.equal(h, ops.renderable_mean_clamp(*args))
        w = want(per_cam, [big] * 3, znear, zfar)
        assert np.allclose(h.cpu().numpy(), w, rtol=ref.MEAN_RTOL, atol=0) and ((w > 5e-5) & (w < 1e-3)).all(), (h, w)
    # one cloud per camera, 11 unused slots in front of the first one
    clouds = [big, big[:50001] * 0.9, big[50001:80003] * 1.1]
    pts = np.concatenate([np.full((11, 3), np.nan, np.float32)] + clouds)
    num = np.array([c.shape[0] for c in clouds], np.int64)
    first = np.cumsum(num) - num + 11
    znear = np.array([_plane_near(clouds[n], V[n], 1.4) for n in range(3)], np.float32)
    zfar = np.full(3, 100.0, np.float32)
    vals = rng.uniform(1e-4, 1.5e-3, pts.shape[0]).astype(np.float32)
    vals[:11] = np.nan
    args = (t(vals), t(pts), t(V), t(znear), t(zfar), t(first), t(num), False) + _H
    h = ops.renderable_mean_clamp(*args)
    assert torch.equal(h, ops.renderable_mean_clamp(*args))
    w = want([vals[f:f + n] for f, n in zip(first, num)], clouds, znear, zfar)
    assert np.allclose(h.cpu().numpy(), w, rtol=ref.MEAN_RTOL, atol=0) and ((w > 5e-5) & (w < 1e-3)).any(), (h, w)
