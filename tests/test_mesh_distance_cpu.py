"""CPU: the point-to-mesh distance (include/dss_hip.h: dss_point_face_workspace, dss_point_face_distance,
dss_face_point_distance, dss_mesh_distance_backward) -- the symbols and their argument checks, the refusals of the Python
layers, the loss's reductions, and the yardsticks the GPU tests (test_gpu_mesh_distance.py) measure against:
tests/mesh_distance_reference.py, whose float32 restatement is checked here against its float64 one on every scene."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_distance_reference as mr
from dss_amd import _lib

INVALID, WORKSPACE = -1, -2   # DSS_ERR_INVALID_ARGUMENT, DSS_ERR_WORKSPACE
SCENES = mr.cpu_scenes()


def _both(name):
    q, v, f = SCENES[name]
    tri32 = mr.triangles(v, f)
    return q, v, f, mr.d2_matrix(q, tri32, np.float32), mr.d2_matrix(q, tri32.astype(np.float64), np.float64)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float32_restatement_within_derived_error(name):
    """|d2_f32 - d2_f64| <= c EPS k (d2 + L sqrt(d2) + EPS k L^2) for the nearest face's distance of every query, k = the
    larger kappa of the two faces the two precisions name, with c = BAR x the scene's recorded worst value (printed here:
    mr.ERROR_C holds what this test measured); the sliver scenes include queries above the triangles' interiors"""
    q, v, f, D32, D64 = _both(name)
    d32, i32 = mr._pick(D32)
    d64, i64 = mr._pick(D64)
    k = mr.kappa(v, f)
    unit = mr.error_bar(d64, mr.longest_edge(v, f), 1.0, np.maximum(k[i32], k[i64]))
    plain = float((np.abs(d32.astype(np.float64) - d64) / mr.error_bar(d64, mr.longest_edge(v, f), 1.0)).max())
    print("%s: kappa up to %.3g; without it c = %.3g; plane term decides %d queries" % (
        name, k.max(), plain, int((D64.min(1) < np.minimum.reduce([mr.d2_matrix(q, mr.triangles(v, f).astype(np.float64)[:, [a, b, b]], np.float64).min(1)
                                                                  for a, b in ((0, 1), (1, 2), (2, 0))])).sum())))
    worst = float((np.abs(d32.astype(np.float64) - d64) / unit).max())
    print("%s: worst c = %.3f over %d queries x %d faces (recorded %.2f)" % (name, worst, len(q), len(f), mr.ERROR_C[name]))
    assert not np.isnan(D32[:, mr.usable_faces(v, f)]).any()
    assert worst <= mr.BAR * mr.ERROR_C[name]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_named_face_attains_the_float64_minimum(name):
    """the face the float32 restatement names is, in float64, as near as the float64 minimum within the same bar -- for
    every query, ties included (a quarter of the queries of an icosphere are exact ties between faces)"""
    q, v, f, D32, D64 = _both(name)
    _, i32 = mr._pick(D32)
    d64, i64 = mr._pick(D64)
    assert (i32 >= 0).all()
    at_named = D64[np.arange(len(q)), i32]
    k = mr.kappa(v, f)
    bar = mr.error_bar(d64, mr.longest_edge(v, f), mr.BAR * mr.ERROR_C[name], np.maximum(k[i32], k[i64]))
    print("%s: worst use of the bar %.3g" % (name, float(((at_named - d64) / np.maximum(bar, 1e-300)).max())))
    assert (at_named - d64 <= bar).all(), float((at_named - d64 - bar).max())
    ties = (D32 == D32.min(1, keepdims=True)).sum(1)
    print("%s: %d of %d queries have several exact float32 minimisers" % (name, int((ties > 1).sum()), len(q)))


def test_lattice_is_exact():
    """integer vertices and dyadic queries: every operation of the definition is exact, so float32 == float64 on the full
    distance matrix, and many queries have 2 to 6 exact minimisers"""
    q, v, f, D32, D64 = _both("lattice")
    assert len(f) == 32 and len(q) > 1500
    assert np.array_equal(D32.astype(np.float64), D64)
    ties = (D32 == D32.min(1, keepdims=True)).sum(1)
    assert (ties > 1).sum() > len(q) // 4 and ties.max() <= 6
    d, i = mr._pick(D32)
    assert np.array_equal(i, mr._pick(D64)[1])   # first minimum = smaller id in both


def test_pruned_reference_equals_brute_force():
    q, v, f = SCENES["ico3"]
    a, b = mr.nearest_face(q, v, f), mr.nearest_face(q, v, f, pruned=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_absent_faces_in_the_reference():
    v, f = mr.icosphere(1)
    bad_v = np.concatenate([v, [[np.nan, 0, 0], [np.inf, 0, 0]]]).astype(np.float32)
    V = len(bad_v)
    bad_f = np.concatenate([[[0, 1, -1]], f[:40], [[0, V, 1], [0, 1, V - 2], [V - 1, 1, 2]], f[40:]])
    assert mr.usable_faces(bad_v, bad_f).sum() == len(f)
    q = SCENES["ico2"][0][:200]
    d, i = mr.nearest_face(q, bad_v, bad_f)
    d0, i0 = mr.nearest_face(q, v, f)
    keep = np.nonzero(mr.usable_faces(bad_v, bad_f))[0]
    assert np.array_equal(d, d0) and np.array_equal(i, keep[i0])
    df, jf = mr.nearest_point(q, bad_v, bad_f)
    assert (jf[~mr.usable_faces(bad_v, bad_f)] == -1).all() and (df[~mr.usable_faces(bad_v, bad_f)] == 0).all()


def test_symbols_and_argument_checks():
    """the four entries load and refuse NULL pointers, bad sizes and a short workspace before any launch (no GPU here)"""
    lib = _lib.load()
    for name in ("dss_point_face_workspace", "dss_point_face_distance", "dss_face_point_distance", "dss_mesh_distance_backward"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dss_version() == 103
    assert lib.dss_point_face_workspace(3, 5000) > lib.dss_knn_workspace(3, 5000) + 5000 * (12 + 4 + 48 + 4)
    assert lib.dss_point_face_workspace(1, 0) > 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def search(fn, pts=p, pf=p, pn=p, P=5, verts=p, V=9, faces=p, ff=p, fn_=p, F=7, N=1, d2=p, idx=p, ws=p, ws_bytes=1 << 30):
        return getattr(lib, fn)(pts, pf, pn, P, verts, V, faces, ff, fn_, F, N, d2, idx, ws, ws_bytes, None)

    for fn in ("dss_point_face_distance", "dss_face_point_distance"):
        for kw in ({"N": 0}, {"N": -1}, {"P": -1}, {"F": -1}, {"V": -1}, {"F": 1 << 31}, {"P": 1 << 31}):
            assert search(fn, **kw) == INVALID and b"bad sizes" in lib.dss_last_error(), (fn, kw)
        for name in ("pts", "pf", "pn", "verts", "faces", "ff", "fn_", "d2", "idx"):
            assert search(fn, **{name: None}) == INVALID and b"NULL" in lib.dss_last_error(), (fn, name)
        assert search(fn, ws=None) == WORKSPACE
        assert search(fn, ws_bytes=0) == WORKSPACE and b"workspace" in lib.dss_last_error()
    assert search("dss_point_face_distance", ws_bytes=lib.dss_point_face_workspace(1, 7) - 1) == WORKSPACE
    assert search("dss_face_point_distance", ws_bytes=lib.dss_nearest_workspace(1, 5) - 1) == WORKSPACE
    assert search("dss_point_face_distance", P=0, pts=None, d2=None, idx=None, ws=None) == 0   # nothing to write
    assert search("dss_face_point_distance", F=0, faces=None, d2=None, idx=None, ws=None) == 0

    def backward(pts=p, pf=p, pn=p, P=5, verts=p, V=9, faces=p, ff=p, fn_=p, F=7, N=1, ipf=p, ifp=p, of=p, ov=p, gp=p, gf=p,
                 grad_p=p, grad_v=p):
        return lib.dss_mesh_distance_backward(pts, pf, pn, P, verts, V, faces, ff, fn_, F, N, ipf, ifp, of, ov, gp, gf, grad_p,
                                              grad_v, None)

    for kw in ({"N": 0}, {"P": -1}, {"F": -3}, {"V": -1}):
        assert backward(**kw) == INVALID and b"bad sizes" in lib.dss_last_error(), kw
    for name in ("pts", "pf", "pn", "verts", "faces", "ff", "fn_", "ipf", "ifp", "of", "ov", "gp", "gf"):
        assert backward(**{name: None}) == INVALID and b"NULL" in lib.dss_last_error(), name
    assert backward(grad_p=None, grad_v=None) == 0   # no gradient asked for: nothing to do
    assert backward(grad_p=None, of=None, grad_v=None) == 0
    assert backward(grad_p=None, ov=None) == INVALID   # grad_verts needs order_v ...
    assert backward(grad_v=None, of=None) == INVALID   # ... and grad_points order_f
    # the large-list multiple is an explicit option with a checked range
    assert lib.dss_get_option(_lib.OPT_MESH_LARGE) == 0
    assert lib.dss_set_option(_lib.OPT_MESH_LARGE, -1) == INVALID and b"DSS_OPT_MESH_LARGE" in lib.dss_last_error()
    assert lib.dss_set_option(_lib.OPT_MESH_LARGE, 4097) == INVALID


def test_exports():
    import dss_amd
    from dss_amd import losses, mesh_ops, ops
    for name in ("point_face_distance", "face_point_distance", "mesh_distance_backward"):
        assert getattr(ops, name) is getattr(mesh_ops, name)
    assert callable(losses.point_mesh_face_distance) and callable(dss_amd.evaluate_cloud)


def test_cpu_tensors_and_wrong_shapes_are_refused():
    from dss_amd import ops
    pts, verts, faces = torch.zeros(6, 3), torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    one = torch.tensor([0])
    for fn in (ops.point_face_distance, ops.face_point_distance):
        with pytest.raises(RuntimeError, match=r"dss_amd: points is on cpu; the HIP path needs GPU tensors \(no CPU fallback\)"):
            fn(pts, one, torch.tensor([6]), verts, faces, one, torch.tensor([4]))
        with pytest.raises(TypeError, match="points must be a torch.Tensor"):
            fn(None, one, torch.tensor([6]), verts, faces, one, torch.tensor([4]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_distance_backward(pts, one, torch.tensor([6]), verts, faces, one, torch.tensor([4]), torch.zeros(6, dtype=torch.int64),
                                   torch.zeros(4, dtype=torch.int64), torch.zeros(6), torch.zeros(4))


class _FakeGpu:
    """lets the shape and dtype checks of mesh_ops run on CPU tensors: `require_gpu` without the device test"""

    def __enter__(self):
        self.old = _lib.require_gpu

        def fake(t, name, dtype=None):
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch.Tensor" % name)
            if dtype is not None and t.dtype != dtype:
                raise RuntimeError("dss_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
            return t.contiguous()
        _lib.require_gpu = fake
        return self

    def __exit__(self, *a):
        _lib.require_gpu = self.old
        return False


def test_wrong_shapes_and_dtypes_raise_runtime_error():
    """reachable without a GPU: every refusal happens before the library is entered"""
    from dss_amd import mesh_ops
    pts, verts, faces = torch.zeros(6, 3), torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    one, n6, n4 = torch.tensor([0]), torch.tensor([6]), torch.tensor([4])
    with _FakeGpu():
        for bad in (dict(points=torch.zeros(6, 2)), dict(verts=torch.zeros(5, 4)), dict(faces=torch.zeros(4, 4, dtype=torch.int64)),
                    dict(faces=torch.zeros(12, dtype=torch.int64)), dict(f_first=torch.tensor([0, 2])), dict(p_num=torch.tensor([3, 3]))):
            kw = dict(points=pts, p_first=one, p_num=n6, verts=verts, faces=faces, f_first=one, f_num=n4)
            kw.update(bad)
            with pytest.raises(RuntimeError, match="points \\(P,3\\), verts \\(V,3\\)"):
                mesh_ops._mesh_inputs(**kw)
        for bad in (dict(points=pts.double()), dict(faces=faces.int()), dict(p_first=one.int()), dict(verts=verts.half())):
            kw = dict(points=pts, p_first=one, p_num=n6, verts=verts, faces=faces, f_first=one, f_num=n4)
            kw.update(bad)
            with pytest.raises(RuntimeError, match="must be torch"):
                mesh_ops._mesh_inputs(**kw)
        with pytest.raises(RuntimeError, match="idx_pf, g_p \\(P,\\)"):
            mesh_ops.mesh_distance_backward(pts, one, n6, verts, faces, one, n4, torch.zeros(5, dtype=torch.int64),
                                            torch.zeros(4, dtype=torch.int64), torch.zeros(6), torch.zeros(4))


def test_contributor_orders():
    """the keys of `mesh_distance_orders` (plain torch, runs anywhere): faces by their point, entries by their vertex; pairs
    that do not exist and vertex ids outside [0, V) go last"""
    from dss_amd import mesh_ops
    faces = torch.tensor([[0, 1, 2], [2, 1, 3], [3, -1, 9], [0, 0, 0]])
    V = 4
    p_first, p_num, f_first, f_num = torch.tensor([0]), torch.tensor([3]), torch.tensor([0]), torch.tensor([4])
    idx_pf = torch.tensor([1, -1, 0])          # point 1 has no face
    idx_fp = torch.tensor([2, 2, -1, 0])       # face 2 has no point
    order_f, order_v = mesh_ops.mesh_distance_orders(faces, V, idx_pf, idx_fp, p_first, p_num, f_first, f_num)
    assert order_f.tolist() == [3, 0, 1, 2]
    P, F = 3, 4
    pairs = [(0, 1), None, (2, 0), (2, 0), (2, 1), None, (0, 3)]   # (point, face) of pair k
    key = []
    for k, pr in enumerate(pairs):
        for c in range(3):
            v = int(faces[pr[1], c]) if pr is not None else -1
            key.append(v if 0 <= v < V else 1 << 62)
    want = sorted(range(3 * (P + F)), key=lambda e: (key[e], e))
    assert order_v.tolist() == want


def _loss_fp64(clouds, meshes):
    """the plain evaluation: each direction by its own brute-force search; `mr.loss_fp64` (one pass) must agree"""
    N, total = len(clouds), 0.0
    for q, (v, f) in zip(clouds, meshes):
        q64, v64 = np.asarray(q, np.float64), np.asarray(v, np.float64)
        total += mr.nearest_face(q64, v64, f, np.float64)[0].sum() / (len(q) * N)
        total += mr.nearest_point(q64, v64, f, np.float64)[0].sum() / (len(f) * N)
    assert abs(total - mr.loss_fp64(clouds, meshes)) <= 1e-14 * total
    return total


class _Meshes:
    """the accessors of pytorch3d's Meshes the loss reads, over a list of (verts, faces)"""

    def __init__(self, meshes):
        self.v = [torch.as_tensor(v) for v, _ in meshes]
        self.f = [torch.as_tensor(f) for _, f in meshes]

    def _first(self, sizes):
        return torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), dtype=torch.int64)

    def verts_packed(self): return torch.cat(self.v)
    def faces_packed(self): return torch.cat([f + o for f, o in zip(self.f, self._first([len(v) for v in self.v]).tolist())])
    def mesh_to_faces_packed_first_idx(self): return self._first([len(f) for f in self.f])
    def num_faces_per_mesh(self): return torch.tensor([len(f) for f in self.f])
    def mesh_to_verts_packed_first_idx(self): return self._first([len(v) for v in self.v])
    def num_verts_per_mesh(self): return torch.tensor([len(v) for v in self.v])


def test_loss_reductions_against_fp64(monkeypatch):
    """`losses.point_mesh_face_distance` with the three operators replaced by the numpy restatement (no GPU here): packing
    of ragged clouds and meshes, both mesh forms, the two normalisations -- against a plain float64 evaluation"""
    from dss_amd import losses, ops
    from dss_amd.cloud import PointClouds3D
    rng = np.random.default_rng(5)
    meshes = [mr.icosphere(0), mr.icosphere(1, radius=0.5, center=(0.2, 0, 0)), mr.lattice_sheet(2, 1)]
    clouds = [rng.normal(size=(n, 3)).astype(np.float32) for n in (65, 30, 7)]

    def per_mesh(fn, points, pf, pn, verts, faces, ff, fn_):
        d, i = [], []
        for n in range(len(pf)):
            q = points[pf[n]:pf[n] + pn[n]].numpy()
            dd, ii = fn(q, verts.numpy(), faces[ff[n]:ff[n] + fn_[n]].numpy())
            d.append(dd), i.append(ii)
        return torch.from_numpy(np.concatenate(d)), torch.from_numpy(np.concatenate(i))

    monkeypatch.setattr(ops, "point_face_distance", lambda *a: per_mesh(mr.nearest_face, *a))
    monkeypatch.setattr(ops, "face_point_distance", lambda *a: per_mesh(mr.nearest_point, *a))
    want = _loss_fp64(clouds, meshes)
    pcl = PointClouds3D([torch.from_numpy(c) for c in clouds])
    as_lists = ([torch.from_numpy(v) for v, _ in meshes], [torch.from_numpy(f) for _, f in meshes])
    for form in (as_lists, _Meshes(meshes)):
        got = losses.point_mesh_face_distance(form, pcl, min_triangle_area=5e-3)
        assert got.dim() == 0 and abs(float(got) - want) <= 1e-5 * want
    padded = torch.from_numpy(np.stack([clouds[0], clouds[0]]))   # a padded (N,P,3) tensor, as chamfer_distance takes one
    got = losses.point_mesh_face_distance(([as_lists[0][0]] * 2, [as_lists[1][0]] * 2), padded)
    assert abs(float(got) - _loss_fp64([clouds[0]] * 2, [meshes[0]] * 2)) <= 1e-5 * float(got)


def test_loss_refuses_bad_input_without_a_gpu():
    from dss_amd import losses
    from dss_amd.cloud import PointClouds3D
    v, f = (torch.from_numpy(a) for a in mr.icosphere(0))
    pcl = PointClouds3D([torch.zeros(4, 3)])
    with pytest.raises(ValueError, match="empty mesh"):
        losses.point_mesh_face_distance(([v], [f[:0]]), pcl)
    with pytest.raises(ValueError, match="empty cloud"):
        losses.point_mesh_face_distance(([v], [f]), PointClouds3D([torch.zeros(0, 3)]))
    with pytest.raises(ValueError, match="1 clouds against 2 meshes"):
        losses.point_mesh_face_distance(([v, v], [f, f]), pcl)
    with pytest.raises(ValueError, match="packed accessors"):
        losses.point_mesh_face_distance(v, pcl)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.point_mesh_face_distance(([v], [f]), pcl)
    import dss_amd
    with pytest.raises(ValueError, match="empty"):
        dss_amd.evaluate_cloud(torch.zeros(0, 3), gt_cloud=torch.zeros(3, 3))
    assert dss_amd.evaluate_cloud(torch.zeros(3, 3)) == {}
