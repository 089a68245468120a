"""GPU: point-to-mesh distance (`ops.point_face_distance`, `ops.face_point_distance`, `ops.mesh_distance_backward`), the loss
`losses.point_mesh_face_distance` and `dss_amd.evaluate_cloud`, against tests/mesh_distance_reference.py (checked on the
CPU by test_mesh_distance_cpu.py).

Bars.  d2 and idx of both searches: BIT-EQUAL to the float32 restatement of the definition (same operations, same order, no
contraction, correctly rounded division), ties to the smaller id -- no tolerance.  Gradients: rel-L2 <= 1e-6 against fp64
autograd at the kernel's own index lists, the project's gradient standard.  Loss value: relative 1e-5, chamfer's bar."""
import os

import numpy as np
import pytest
import torch

import mesh_distance_reference as mr

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_REL_L2 = 1e-5, 1e-6


def _dev():
    return torch.device("cuda:0")


def _pack_clouds(clouds, gap=0):
    """clouds -> packed (P,3) with `gap` NaN slots of no cloud in front of every cloud and behind the last, first, num"""
    rows, first, run = [], [], 0
    for c in clouds:
        rows.append(np.full((gap, 3), np.nan, np.float32))
        run += gap
        first.append(run)
        rows.append(np.asarray(c, np.float32).reshape(-1, 3))
        run += len(c)
    rows.append(np.full((gap, 3), np.nan, np.float32))
    dev = _dev()
    return (torch.from_numpy(np.concatenate(rows)).to(dev), torch.tensor(first, dtype=torch.int64, device=dev),
            torch.tensor([len(c) for c in clouds], dtype=torch.int64, device=dev))


def _pack_meshes(meshes):
    """[(verts, faces with mesh-local ids)] -> verts (V,3), faces (F,3) with packed ids, first, num, vertex offsets"""
    dev = _dev()
    starts = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])[:-1]]).astype(np.int64)
    verts = np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])
    faces = np.concatenate([np.asarray(f, np.int64).reshape(-1, 3) + s for (_, f), s in zip(meshes, starts)])
    nf = [len(f) for _, f in meshes]
    first = np.concatenate([[0], np.cumsum(nf)[:-1]]).astype(np.int64)
    return (torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(first).to(dev),
            torch.tensor(nf, dtype=torch.int64, device=dev), starts)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(tag, got_d, got_i, want_d, want_i):
    bad = np.nonzero((_bits(got_d) != _bits(want_d)) | (got_i != want_i))[0]
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got (%r, %d) want (%r, %d)" % (
        tag, bad.size, len(want_i), bad[0], got_d[bad[0]], got_i[bad[0]], want_d[bad[0]], want_i[bad[0]])


def _run(clouds, meshes, gap=0):
    from dss_amd import ops
    P, pf, pn = _pack_clouds(clouds, gap)
    V, F, ff, fn, _ = _pack_meshes(meshes)
    dp, ip = ops.point_face_distance(P, pf, pn, V, F, ff, fn)
    df, jf = ops.face_point_distance(P, pf, pn, V, F, ff, fn)
    torch.cuda.synchronize()
    assert dp.dtype == torch.float32 and ip.dtype == torch.int64 and dp.shape == ip.shape == (P.shape[0],)
    assert df.dtype == torch.float32 and jf.dtype == torch.int64 and df.shape == jf.shape == (F.shape[0],)
    return (dp.cpu().numpy(), ip.cpu().numpy(), df.cpu().numpy(), jf.cpu().numpy(), pf.cpu().numpy(), ff.cpu().numpy())


def _check(clouds, meshes, gap=0, directions=("pf", "fp"), pruned=False):
    """both searches of a batch, bit for bit; slots of no cloud get (0, -1)"""
    dp, ip, df, jf, pf, ff = _run(clouds, meshes, gap)
    owned = np.zeros(len(dp), bool)
    for n, (q, (v, f)) in enumerate(zip(clouds, meshes)):
        a, b = int(pf[n]), int(ff[n])
        owned[a:a + len(q)] = True
        if len(q) == 0 or len(f) == 0:
            assert (ip[a:a + len(q)] == -1).all() and (dp[a:a + len(q)] == 0).all()
            assert (jf[b:b + len(f)] == -1).all() and (df[b:b + len(f)] == 0).all()
            continue
        if pruned:
            want_p, want_f = mr.nearest_face(q, v, f, pruned=True), None
        else:
            want_p, want_f = mr.nearest_both(q, v, f, chunk=4096 if len(q) > 20000 else 256)
        if "pf" in directions:
            _same("pair %d point -> face" % n, dp[a:a + len(q)], ip[a:a + len(q)], *want_p)
        if "fp" in directions and want_f is not None:
            _same("pair %d face -> point" % n, df[b:b + len(f)], jf[b:b + len(f)], *want_f)
    assert (ip[~owned] == -1).all() and (dp[~owned] == 0).all()
    return dp, ip, df, jf


def test_lattice_sheet_exact_ties():
    """vertices, edge midpoints, quarter points at heights 0, 1/2, 2 and outside the sheet by 1/2, 3 and 50 cells: up to six
    faces tie exactly and the smaller id must win, in both directions"""
    v, f = mr.lattice_sheet()
    _check([mr.lattice_queries()], [(v, f)])


@pytest.mark.parametrize("level", [0, 1, 3])
def test_icospheres(level):
    """20, 80 and 1,280 faces; queries inside, outside, 50 radii away, exactly on 64 vertices and 32 edge midpoints"""
    rng = np.random.default_rng(100 + level)
    v, f = mr.icosphere(level)
    q = np.concatenate([mr.sphere_queries(rng, 600), mr.on_mesh_queries(rng, v, f, 64, 32)])
    _check([q], [(v, f)])


def test_ragged_batch_and_empty_sides():
    """meshes of 20 / 1,280 / 2 faces against clouds of 65 / 300 / 1 points with NaN gap slots between the clouds (wavefronts
    straddle clouds); then a 0-face mesh and a 0-point cloud: (0, -1)"""
    rng = np.random.default_rng(3)
    quad = (np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), np.asarray([[0, 1, 2], [0, 2, 3]]))
    meshes = [mr.icosphere(0), mr.icosphere(3, radius=0.7, center=(0.1, -0.2, 0.3)), quad]
    clouds = [mr.sphere_queries(rng, 65), mr.sphere_queries(rng, 300), np.asarray([[0.25, 0.5, 1.0]], np.float32)]
    _check(clouds, meshes, gap=7)
    empty_mesh = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    _check([clouds[0], clouds[1][:5], np.zeros((0, 3), np.float32)], [meshes[0], empty_mesh, mr.icosphere(1)], gap=3)


def test_nan_query_and_nan_point():
    """a point with a NaN position gets (0, -1) and is nobody's nearest point"""
    rng = np.random.default_rng(4)
    v, f = mr.icosphere(1)
    q = mr.sphere_queries(rng, 130)
    q[[3, 64, 129]] = np.nan
    dp, ip, df, jf = _check([q], [(v, f)])
    assert (ip[[3, 64, 129]] == -1).all() and not np.isin(jf, [3, 64, 129]).any()


def test_degenerate_faces_and_slivers():
    """collinear, two equal and three equal vertices mixed into an icosphere: the union of their edges, no NaN"""
    rng = np.random.default_rng(5)
    v, f = mr.icosphere(1)
    v, deg = mr.degenerate_faces(v)
    faces = np.concatenate([f[:30], deg, f[30:]])
    q = np.concatenate([mr.sphere_queries(rng, 400), v[:12], ((v[0] + v[1]) * np.float32(0.5))[None]])
    _check([q], [(v, faces)])


@pytest.mark.parametrize("aspect", [1e2, 1e4])
def test_slivers(aspect):
    """slivers of aspect 100 (kappa ~ 100: searched through the grid, the walk's floor widened by K_grid) and 1e4 (kappa ~ 1e4:
    on the large list), alone and mixed into an icosphere; queries anywhere in the cube AND above the slivers' interiors, where
    the plane term decides and its float32 error is ~kappa times a well-shaped triangle's -- both directions"""
    rng = np.random.default_rng(int(aspect))
    sv, sf = mr.sliver_mesh(rng, aspect=aspect)
    above = mr.above_interiors(rng, sv, sf)
    q = np.concatenate([rng.uniform(-1.5, 1.5, (500, 3)).astype(np.float32), above])
    (_, ip), _ = mr.nearest_both(above, sv, sf)
    assert (ip == np.repeat(np.arange(len(sf)), 8)).mean() > 0.5     # most of them do have their own sliver as the answer
    _check([q], [(sv, sf)])
    v, f = mr.icosphere(2, radius=1.2)
    _check([q], [(np.concatenate([v, sv]), np.concatenate([f, sf + len(v)]))])


def test_absent_faces_are_never_read_or_answered():
    """faces with vertex ids -1 and V, and with a NaN and an Inf vertex, mixed into an icosphere: the answers of the mesh
    without them (ids mapped), (0, -1) for those faces, and the run ends clean.  Ordinary wrong data: the kernels check ids
    before any load (mesh_load_face)"""
    from dss_amd import ops
    rng = np.random.default_rng(6)
    v, f = mr.icosphere(2)
    bad_v = np.concatenate([v, [[np.nan, 0.5, 0.5], [np.inf, 0.0, 0.0]]]).astype(np.float32)
    V = len(bad_v)
    bad_f = np.concatenate([[[0, 1, -1]], f[:100], [[0, V, 1], [5, 6, V - 2], [V - 1, 7, 8]], f[100:], [[-1, -1, -1], [V, V + 5, 2 ** 40]]])
    usable = mr.usable_faces(bad_v, bad_f)
    assert usable.sum() == len(f)
    q = np.concatenate([mr.sphere_queries(rng, 500), v[:40]])
    dp, ip, df, jf = _check([q], [(bad_v, bad_f)])
    d0, i0, df0, jf0, _, _ = _run([q], [(v, f)])
    keep = np.nonzero(usable)[0]
    _same("against the mesh without them", dp, ip, d0, keep[i0])
    _same("faces", df[keep], jf[keep], df0, jf0)
    assert (jf[~usable] == -1).all() and (df[~usable] == 0).all()
    # the backward names no absent face either: gradients of the clean mesh, zero rows for the two bad vertices
    P, pf, pn = _pack_clouds([q])
    Vt, Ft, ff, fn, _ = _pack_meshes([(bad_v, bad_f)])
    gp, gf = torch.ones(len(q), device=_dev()), torch.ones(len(bad_f), device=_dev())
    grad_p, grad_v = ops.mesh_distance_backward(P, pf, pn, Vt, Ft, ff, fn, torch.from_numpy(ip).to(_dev()), torch.from_numpy(jf).to(_dev()), gp, gf)
    torch.cuda.synchronize()
    assert torch.isfinite(grad_p).all() and torch.isfinite(grad_v).all() and (grad_v[-2:] == 0).all()


def test_large_list():
    """an icosphere of 1,280 faces plus one triangle 100 times its extent (tested by every query, outside the grid); a mesh
    that is only a two-triangle quad under 4,096 points (one wavefront per face strides the whole cloud)"""
    rng = np.random.default_rng(8)
    v, f = mr.icosphere(3)
    big_v = np.concatenate([v, [[-100, -100, 0.3], [100, -100, 0.3], [0, 100, 0.3]]]).astype(np.float32)
    big_f = np.concatenate([f[:640], [[len(v), len(v) + 1, len(v) + 2]], f[640:]])
    q = np.concatenate([mr.sphere_queries(rng, 500), rng.uniform(-3, 3, (200, 3)).astype(np.float32)])
    dp, ip, _, _ = _check([q], [(big_v, big_f)])
    assert (ip == 640).sum() > 50          # the large triangle is the answer for many queries
    quad = (np.asarray([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32), np.asarray([[0, 1, 2], [0, 2, 3]]))
    cloud = rng.uniform(-2, 2, (4096, 3)).astype(np.float32)
    cloud[:, 2] = np.abs(cloud[:, 2]) + 0.01
    _check([cloud], [quad])


def test_large_list_multiple_does_not_change_results():
    """DSS_OPT_MESH_LARGE from everything-on-the-list to nothing-on-it: the same bits"""
    from dss_amd import _lib
    rng = np.random.default_rng(9)
    v, f = mr.icosphere(2)
    q = mr.sphere_queries(rng, 300)
    want = _run([q], [(v, f)])[:2]
    for quarters in (1, 2, 64, 4096):
        old = _lib.set_option(_lib.OPT_MESH_LARGE, quarters)
        try:
            got = _run([q], [(v, f)])[:2]
        finally:
            _lib.set_option(_lib.OPT_MESH_LARGE, old)
        _same("quarters %d" % quarters, got[0], got[1], want[0], want[1])


def test_planar_mesh_and_collinear_cloud():
    """zero extent along z in the mesh's grid, and a cloud on one line (its grid has zero extent along two axes)"""
    v, f = mr.lattice_sheet(6, 5)
    t = np.linspace(-2, 9, 257, dtype=np.float32)
    line = np.stack([t, 0.37 * t + 0.2, 0.11 * t], 1).astype(np.float32)
    _check([line], [(v, f)])


def test_grid_large_route_faces():
    """more faces than build_grid's small route takes (131,072): a 257 x 256 sheet, 131,584 faces, 256 queries.  Point ->
    face only: that is the direction whose grid is built over the faces; face -> point would build the small grid of the 256
    points here (its large route is the next test) at 33 million reference pairs"""
    rng = np.random.default_rng(10)
    v, f = mr.lattice_sheet(257, 256)
    assert len(f) == 131584
    v = v.copy()
    v[:, 2] = (0.3 * np.sin(v[:, 0] * 0.1) * np.cos(v[:, 1] * 0.07)).astype(np.float32)
    q = np.stack([rng.uniform(-5, 262, 256), rng.uniform(-5, 261, 256), rng.uniform(-2, 2, 256)], 1).astype(np.float32)
    _check([q], [(v, f)], directions=("pf",), pruned=True)


def test_grid_large_route_points():
    """more points than the small route takes: 131,073 points against 64 faces, both directions"""
    rng = np.random.default_rng(11)
    v, f = mr.icosphere(1)
    q = (rng.normal(size=(131073, 3)) * 0.8).astype(np.float32)
    _check([q], [(v, f[:64])])


# ---- backward
def _backward_case(clouds, meshes, seed):
    from dss_amd import ops
    rng = np.random.default_rng(seed)
    P, pf, pn = _pack_clouds(clouds)
    V, F, ff, fn, _ = _pack_meshes(meshes)
    _, ip = ops.point_face_distance(P, pf, pn, V, F, ff, fn)
    _, jf = ops.face_point_distance(P, pf, pn, V, F, ff, fn)
    gp = torch.from_numpy(rng.uniform(0.5, 1.5, P.shape[0]).astype(np.float32)).to(_dev())
    gf = torch.from_numpy(rng.uniform(0.5, 1.5, F.shape[0]).astype(np.float32)).to(_dev())
    grad_p, grad_v = ops.mesh_distance_backward(P, pf, pn, V, F, ff, fn, ip, jf, gp, gf)
    again_p, again_v = ops.mesh_distance_backward(P, pf, pn, V, F, ff, fn, ip, jf, gp, gf)
    assert torch.equal(grad_p, again_p) and torch.equal(grad_v, again_v)          # a second call: the same bits
    only_p, none_v = ops.mesh_distance_backward(P, pf, pn, V, F, ff, fn, ip, jf, gp, gf, want_verts=False)
    none_p, only_v = ops.mesh_distance_backward(P, pf, pn, V, F, ff, fn, ip, jf, gp, gf, want_points=False)
    assert none_v is None and none_p is None and torch.equal(only_p, grad_p) and torch.equal(only_v, grad_v)
    # the same pairs in fp64 autograd
    ipn, jfn, pfn, ffn = ip.cpu().numpy(), jf.cpu().numpy(), pf.cpu().numpy(), ff.cpu().numpy()
    cloud_of = np.concatenate([np.full(len(c), n) for n, c in enumerate(clouds)])
    mesh_of = np.concatenate([np.full(len(f), n) for n, (_, f) in enumerate(meshes)])
    assert (ipn >= 0).all() and (jfn >= 0).all()
    pair_point = np.concatenate([np.arange(len(ipn)), pfn[mesh_of] + jfn])
    pair_face = np.concatenate([ffn[cloud_of] + ipn, np.arange(len(jfn))])
    g = np.concatenate([gp.cpu().numpy(), gf.cpu().numpy()])
    want_p, want_v = mr.gradients_fp64(P.cpu().numpy(), V.cpu().numpy(), F.cpu().numpy(), pair_point, pair_face, g)
    for tag, got, want in (("points", grad_p, want_p), ("verts", grad_v, want_v)):
        rel = np.linalg.norm(got.double().cpu().numpy() - want) / np.linalg.norm(want)
        print("grad %s rel-L2 %.3g" % (tag, rel))
        assert rel <= GRAD_REL_L2, (tag, rel)
    return ipn, jfn


def test_backward_against_fp64_autograd():
    rng = np.random.default_rng(12)
    meshes = [mr.icosphere(0), mr.icosphere(2, radius=0.7, center=(0.1, -0.2, 0.3)), mr.sliver_mesh(rng, n=16)]
    clouds = [mr.sphere_queries(rng, 65, radius=0.2), mr.sphere_queries(rng, 300, radius=0.2), rng.uniform(-1, 1, (40, 3)).astype(np.float32)]
    _backward_case(clouds, meshes, 13)


def test_backward_many_points_one_face():
    """4,096 points whose nearest face is the one triangle: each of its vertices sums 4,097 pairs"""
    rng = np.random.default_rng(14)
    tri = (np.asarray([[0, 0, 0], [1, 0, 0], [0.2, 0.9, 0.1]], np.float32), np.asarray([[0, 1, 2]]))
    ip, _ = _backward_case([rng.uniform(-1, 2, (4096, 3)).astype(np.float32)], [tri], 15)
    assert (ip == 0).all()


def test_backward_many_faces_one_point():
    """64 faces whose nearest point is the one point: its row sums 65 pairs"""
    v, f = mr.icosphere(1)
    _, jf = _backward_case([np.asarray([[0.3, 0.1, 2.0]], np.float32)], [(v, f[:64])], 16)
    assert (jf == 0).all()


# ---- loss and evaluation
def test_point_mesh_face_distance_value_and_gradients():
    from dss_amd import losses, ops
    from dss_amd.cloud import PointClouds3D
    rng = np.random.default_rng(17)
    meshes = [mr.icosphere(1), mr.icosphere(2, radius=0.6, center=(0.2, 0.0, -0.1))]
    clouds = [mr.sphere_queries(rng, 200, radius=0.1), mr.sphere_queries(rng, 333, radius=0.1)]
    dev = _dev()
    pts = [torch.nn.Parameter(torch.from_numpy(c).to(dev)) for c in clouds]
    verts = [torch.nn.Parameter(torch.from_numpy(v).to(dev)) for v, _ in meshes]
    faces = [torch.from_numpy(f).to(dev) for _, f in meshes]
    loss = losses.point_mesh_face_distance((verts, faces), PointClouds3D(pts), min_triangle_area=5e-3)
    want = mr.loss_fp64(clouds, meshes)
    print("loss %.9g want %.9g" % (loss.item(), want))
    assert loss.dim() == 0 and abs(loss.item() - want) <= LOSS_RTOL * want
    loss.backward()
    # fp64 autograd of the same sum at the kernel's own index lists
    P, pf, pn = _pack_clouds(clouds)
    V, F, ff, fn, _ = _pack_meshes(meshes)
    _, ip = ops.point_face_distance(P, pf, pn, V, F, ff, fn)
    _, jf = ops.face_point_distance(P, pf, pn, V, F, ff, fn)
    ipn, jfn, pfn, ffn = ip.cpu().numpy(), jf.cpu().numpy(), pf.cpu().numpy(), ff.cpu().numpy()
    cloud_of = np.concatenate([np.full(len(c), n) for n, c in enumerate(clouds)])
    mesh_of = np.concatenate([np.full(len(f), n) for n, (_, f) in enumerate(meshes)])
    N = len(clouds)
    g = np.concatenate([1.0 / (np.asarray([len(c) for c in clouds])[cloud_of] * N), 1.0 / (np.asarray([len(f) for _, f in meshes])[mesh_of] * N)])
    want_p, want_v = mr.gradients_fp64(P.cpu().numpy(), V.cpu().numpy(), F.cpu().numpy(), np.concatenate([np.arange(len(ipn)), pfn[mesh_of] + jfn]),
                                       np.concatenate([ffn[cloud_of] + ipn, np.arange(len(jfn))]), g)
    got_p = torch.cat([p.grad for p in pts]).double().cpu().numpy()
    got_v = torch.cat([v.grad for v in verts]).double().cpu().numpy()
    for tag, got, ref in (("points", got_p, want_p), ("verts", got_v, want_v)):
        rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print("loss grad %s rel-L2 %.3g" % (tag, rel))
        assert rel <= GRAD_REL_L2, (tag, rel)


def test_evaluate_cloud(golden_dir):
    """the reference script's row on the bunny against an icosphere: all four keys, 0-dim device tensors, no host read; the
    values against float64 on a 2,000-point subsample.  Bars: CD, hausdorff, p2f avg relative 1e-5 (fp32 distances carry
    ~1e-6, a pairwise fp32 mean adds ~1e-7); p2f std relative 1e-4 (the variance cancels mean^2 against the mean of squares,
    which amplifies the same errors by (mean^2 + var) / var, below 10 here)"""
    import chamfer_reference as cr
    import dss_amd
    from scipy.spatial import cKDTree
    dev = _dev()
    bunny = cr.read_ply_points(os.path.join(golden_dir, "bunny-8000.ply")).astype(np.float32)
    bunny = (bunny - bunny.mean(0)) / np.abs(bunny - bunny.mean(0)).max()
    v, f = mr.icosphere(3)
    gt = mr.icosphere(2)[0]
    pred, gtc, vt, ft = (torch.from_numpy(a).to(dev) for a in (bunny, gt, v, f))
    dss_amd.evaluate_cloud(pred, gt_cloud=gtc, gt_mesh=(vt, ft))   # (sizes the workspace)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        row = dss_amd.evaluate_cloud(pred, gt_cloud=gtc, gt_mesh=(vt, ft))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sorted(row) == ["CD", "hausdorff", "p2f avg", "p2f std"]
    assert all(t.dim() == 0 and t.is_cuda and bool(torch.isfinite(t)) for t in row.values())
    assert sorted(dss_amd.evaluate_cloud(pred, gt_mesh=(vt, ft))) == ["p2f avg", "p2f std"]
    assert sorted(dss_amd.evaluate_cloud(pred, gt_cloud=gtc)) == ["CD", "hausdorff"]
    sub = bunny[::4][:2000]
    row = dss_amd.evaluate_cloud(torch.from_numpy(sub).to(dev), gt_cloud=gtc, gt_mesh=(vt, ft))
    a, b = sub.astype(np.float64), gt.astype(np.float64)
    dab, dba = cKDTree(b).query(a)[0] ** 2, cKDTree(a).query(b)[0] ** 2
    d = np.sqrt(mr.nearest_face(a, v.astype(np.float64), f, np.float64)[0])
    want = {"CD": dab.mean() + dba.mean(), "hausdorff": dab.max() + dba.max(), "p2f avg": d.mean(), "p2f std": d.std()}
    for k, rtol in (("CD", 1e-5), ("hausdorff", 1e-5), ("p2f avg", 1e-5), ("p2f std", 1e-4)):
        print("%s: %.9g want %.9g" % (k, float(row[k]), want[k]))
        assert abs(float(row[k]) - want[k]) <= rtol * want[k], k
