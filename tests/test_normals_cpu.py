"""CPU: the yardstick of the normal orientation (tests/normals_reference.py) on itself -- closed shapes come out outward at
every point, the golden clouds agree with their own normals, the local rule is the stand-in's -- and, without a GPU, the
refusals of the public calls and of the entries, the exports and the ABI conventions of the three new entries, and the
compiler's resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import normals_reference as yard
import scenes
from dss_amd import cloud_ops, normals_ops
from dss_amd.cloud import PointClouds3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("dss_disambiguate_normals", "int"), ("dss_orient_normals_workspace", "size_t"), ("dss_orient_normals", "int"))


def _oriented_pca(points, K=16, KP=8, fp32=False, lists=yard.knn_lists):
    idx = lists(points, K)
    return yard.orient(yard.pca_normals(points, idx, fp32), points, idx, [0], [points.shape[0]], KP)


def _check_tree(stamp, parent, its):
    """stamps >= 1, seeds are the points without a parent, and a parent was oriented strictly earlier"""
    assert (stamp >= 1).all() and stamp.max() <= its
    has = parent >= 0
    assert (stamp[parent[has]] < stamp[has]).all()


def test_a_torus_comes_out_outward_everywhere():
    p, outward = yard.torus(2000)
    o, stamp, parent, its = _oriented_pca(p)
    assert yard.outward_share(o, outward) == 1.0
    assert (parent == -1).sum() == 1 and its[0] <= 5 * 2000
    _check_tree(stamp, parent, its[0])


def test_two_spheres_in_one_cloud_have_two_seeds():
    a, na = yard.fibonacci_sphere(600, (0.0, 0.0, 0.0))
    b, nb = yard.fibonacci_sphere(300, (3.0, 0.0, 0.5), 0.6)
    p, outward = np.concatenate([a, b]), np.concatenate([na, nb])
    o, stamp, parent, its = _oriented_pca(p)
    assert yard.outward_share(o, outward) == 1.0
    assert (parent == -1).sum() == 2
    _check_tree(stamp, parent, its[0])


def test_a_sphere_of_257_points():
    p, outward = yard.fibonacci_sphere(257)
    o, stamp, parent, its = _oriented_pca(p)
    assert yard.outward_share(o, outward) == 1.0 and (parent == -1).sum() == 1
    # and from normals of random sign: the result is every input normal or its negative
    n = yard.random_signs(outward, 9)
    idx = yard.knn_lists(p, 8)
    o, stamp, parent, _ = yard.orient(n, p, idx, [0], [257], 8)
    assert yard.outward_share(o, outward) == 1.0
    assert (np.abs(o) == np.abs(n)).all()


@pytest.mark.parametrize("name,measured", [("bunny", 0.9995), ("teapot", 0.9975), ("yoga6", 0.9999)])
@pytest.mark.parametrize("fp32", [False, True])
def test_golden_clouds_agree_with_their_own_normals(name, measured, fp32):
    p, own = scenes.load_cloud(name)
    o, stamp, parent, its = _oriented_pca(p, fp32=fp32, lists=yard.tree_lists)
    share = yard.outward_share(o, own)
    share = max(share, 1.0 - share)
    print("%s (%s covariances): %.4f of the normals agree, %d iterations, %d seeds"
          % (name, "float32" if fp32 else "float64", share, its[0], (parent == -1).sum()))
    assert share >= 0.99
    assert abs(share - measured) < 5e-4         # the figures of DESIGN 4.17
    _check_tree(stamp, parent, its[0])


def test_the_local_rule_is_the_stand_ins():
    from compat.pytorch3d.ops.points_normals import _disambiguate_vector_directions
    rng = np.random.default_rng(4)
    p = rng.standard_normal((500, 3)).astype(np.float32)
    n = rng.standard_normal((500, 3)).astype(np.float32)
    idx = yard.knn_lists(p, 12)
    got = yard.disambiguate(p, n, idx, [0], [500])
    want = _disambiguate_vector_directions(torch.from_numpy(p)[None], torch.from_numpy(p[idx])[None], torch.from_numpy(n)[None])
    assert np.array_equal(got, want[0].numpy())
    assert 0 < (got != n).any(1).sum() < 500


def test_the_viewpoint_rule_and_unowned_rows():
    p, outward = yard.fibonacci_sphere(100)
    n = yard.random_signs(outward, 2)
    packed = np.concatenate([p, np.full((5, 3), np.nan, np.float32), p + np.float32(4.0)])
    nrm = np.concatenate([n, np.full((5, 3), np.nan, np.float32), n])
    view = np.array([[0, 0, 0], [4, 4, 4]], np.float32)          # the centres: every normal is turned inward
    got = yard.disambiguate(packed, nrm, None, [0, 105], [100, 100], 1, view)
    assert yard.outward_share(got[:100], outward) == 0.0 and yard.outward_share(got[105:], outward) == 0.0
    assert np.array_equal(got[100:105], np.tile(np.array([[0, 0, 1]], np.float32), (5, 1)))


def test_seed_rules():
    assert [yard.seed_sign_flip(np.array(v, np.float32)) for v in
            ([0, 0, 1], [0, 0, -1], [1, -1, 0], [-1, 0, 0], [1, 0, -0.0], [0, 0, 0], [np.nan, np.nan, np.nan], [-1, np.nan, 0])] \
        == [False, True, True, True, False, False, False, True]
    # the highest point seeds; a NaN z loses to every number; ties go to the smallest id
    p = np.array([[0, 0, 0], [1, 0, np.nan], [2, 0, 0.0], [3, 0, -0.0]], np.float32)
    n = np.tile(np.array([[0, 0, -1]], np.float32), (4, 1))
    idx = np.tile(np.arange(4)[:, None], (1, 1))                 # no neighbours at all: every point is a seed
    o, stamp, parent, its = yard.orient(n, p, idx, [0], [4], 8)
    assert np.argsort(stamp).tolist() == [0, 2, 3, 1] and (parent == -1).all() and (o[:, 2] == 1).all()
    assert its[0] == 16 <= 5 * 4


def test_exports_and_abi_conventions():
    import dss_amd
    from dss_amd import _lib, ops
    assert dss_amd.estimate_normals is cloud_ops.estimate_normals and dss_amd.orient_normals is cloud_ops.orient_normals
    assert ops.orient_normals is normals_ops.orient_normals and ops.disambiguate_normals is normals_ops.disambiguate_normals
    assert callable(PointClouds3D.estimate_normals)
    header = open(os.path.join(ROOT, "include", "dss_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret in ENTRIES:
        decl = re.search(r"DSS_API\s+%s\s+%s\s*\(([^;]*)\);" % (ret, name), header)
        assert decl, "%s is not declared in include/dss_hip.h" % name
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int) and len(argtypes) == len(args)
        for a, t in zip(args, argtypes):   # pointers as void *, sizes as their C type
            want = (ctypes.c_void_p if "*" in a else ctypes.c_int64 if a.startswith("int64_t") else
                    ctypes.c_size_t if a.startswith("size_t") else ctypes.c_float if a.startswith("float") else ctypes.c_int)
            assert t is want, (name, a)
        assert hasattr(lib, name)
        if ret == "int":
            assert args[-1] == "void *stream"
    assert _lib.load().dss_version() == 103
    assert normals_ops.THRESHOLDS == tuple(float(t) for t in yard.TAU.astype(np.float64).round(2))


def test_refusals_of_the_entries_are_reached_without_a_gpu():
    from dss_amd import _lib
    lib = _lib.load()
    host = ctypes.create_string_buffer(64)          # stands for device memory: a refused call launches nothing
    p = ctypes.addressof(host)
    q = p + 16
    orient = lambda N, P, K, KP, out=q, ws=None, nb=0, nin=p: lib.dss_orient_normals(nin, p, p, p, p, N, P, K, KP, out, None,   # noqa: E731
                                                                                      None, ws, nb, None)
    for N, P, K, KP in ((0, 10, 8, 8), (1, -1, 8, 8), (1, 10, 0, 8), (1, 10, 8, 0), (1, (2 ** 31 - 1) // 5 + 1, 8, 8)):
        assert orient(N, P, K, KP) == -1
        assert b"dss_orient_normals: bad sizes" in lib.dss_last_error()
    assert orient(1, 10, 8, 8, nin=None) == -1 and b"NULL" in lib.dss_last_error()
    assert orient(1, 10, 8, 8, out=None) == -1 and b"NULL" in lib.dss_last_error()
    assert orient(1, 10, 8, 8, out=p) == -1 and b"must not be normals_in" in lib.dss_last_error()
    # the workspace: the int32 copy of the lists always, the stamps once a cloud can be too large for LDS
    big, lists = normals_ops.LDS_CAPACITY + 1, 4 * (normals_ops.FAST_LIST - 1)
    fits = lib.dss_orient_normals_workspace(1, normals_ops.LDS_CAPACITY)
    assert lists * normals_ops.LDS_CAPACITY <= fits < lists * normals_ops.LDS_CAPACITY + 512
    need = lib.dss_orient_normals_workspace(3, big)
    assert (lists + 4) * big <= need < (lists + 4) * big + 512
    for P, nbytes in ((10, lib.dss_orient_normals_workspace(1, 10)), (big, need)):
        assert orient(1, P, 8, 8) == -1 and b"workspace" in lib.dss_last_error()
        assert orient(1, P, 8, 8, ws=p, nb=nbytes - 1) == -1 and b"workspace" in lib.dss_last_error()
    assert orient(1, 0, 8, 8, nin=None) == 0                      # the empty call returns 0 without a launch
    dis = lambda N, P, K, mode, view=None, out=q: lib.dss_disambiguate_normals(p, p, p, p, p, N, P, K, mode, view, out, None)   # noqa: E731
    for N, P, K, mode in ((0, 10, 8, 0), (1, -1, 8, 0), (1, 10, 0, 0), (1, 10, 8, 2), (1, 10, 8, -1), (1, 1 << 31, 8, 0)):
        assert dis(N, P, K, mode) == -1 and b"dss_disambiguate_normals: bad sizes" in lib.dss_last_error()
    assert dis(1, 10, 8, 1) == -1 and b"viewpoint" in lib.dss_last_error()
    assert dis(1, 10, 8, 0, view=p) == -1 and b"viewpoint" in lib.dss_last_error()
    assert dis(1, 10, 8, 0, out=None) == -1 and b"NULL" in lib.dss_last_error()
    assert dis(1, 0, 8, 0) == 0


def _no_library(monkeypatch):
    from dss_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)


@pytest.mark.parametrize("args,kw,what", [
    ((torch.zeros(1, 50, 3),), dict(neighborhood_size=0), "neighborhood_size must be in 1 .. 40"),
    ((torch.zeros(1, 50, 3),), dict(neighborhood_size=41), "neighborhood_size must be in 1 .. 40"),
    ((torch.zeros(1, 16, 3),), {}, "cloud 0 has 16 points, the neighbourhood size is 16"),
    ((torch.zeros(2, 50, 3), [50, 10]), {}, "cloud 1 has 10 points"),
    ((torch.zeros(1, 50, 3),), dict(orientation_neighbours=1), "orientation_neighbours must be in 2 .. neighborhood_size = 16"),
    ((torch.zeros(1, 50, 3),), dict(orientation_neighbours=17), "orientation_neighbours must be in 2 .. neighborhood_size = 16"),
    ((torch.zeros(1, 50, 3),), dict(orientation="tombari"), "orientation must be one of"),
    ((torch.zeros(1, 50, 3),), dict(orientation="viewpoint"), "needs a viewpoint"),
    ((torch.zeros(1, 50, 3),), dict(viewpoint=torch.zeros(3)), "no other orientation takes one"),
    ((torch.zeros(2, 50, 3),), dict(orientation="viewpoint", viewpoint=torch.zeros(3, 3)), r"viewpoint must be \(3,\) or \(N,3\)"),
    ((torch.zeros(1, 50, 3), [51]), {}, "num_points must lie"),
    ((torch.zeros(1, 50, 3), [50, 50]), {}, "num_points must be"),
    ((torch.zeros(50, 3),), {}, "expects padded points"),
])
def test_estimate_normals_refusals_come_before_the_library(args, kw, what, monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=what):
        cloud_ops.estimate_normals(*args, **kw)


@pytest.mark.parametrize("args,kw,what", [
    ((torch.zeros(1, 50, 3), torch.zeros(1, 50, 3)), dict(neighborhood_size=1), "neighborhood_size must be in 2 .. 40"),
    ((torch.zeros(1, 50, 3), torch.zeros(1, 50, 3)), dict(neighborhood_size=41), "neighborhood_size must be in 2 .. 40"),
    ((torch.zeros(1, 8, 3), torch.zeros(1, 8, 3)), {}, "cloud 0 has 8 points, the neighbourhood size is 8"),
    ((torch.zeros(1, 50, 3), torch.zeros(1, 49, 3)), {}, "expects normals of the points' shape"),
    ((torch.zeros(1, 50, 3), None), {}, "expects normals of the points' shape"),
    ((torch.zeros(50, 3), torch.zeros(50, 3)), {}, "expects padded points"),
])
def test_orient_normals_refusals_come_before_the_library(args, kw, what, monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=what):
        cloud_ops.orient_normals(*args, **kw)


def test_cpu_tensors_are_refused(monkeypatch):
    _no_library(monkeypatch)
    g = torch.Generator().manual_seed(0)
    cloud = PointClouds3D([torch.rand(40, 3, generator=g), torch.rand(30, 3, generator=g)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_ops.estimate_normals(torch.zeros(1, 50, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_ops.estimate_normals(cloud)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud.estimate_normals()
    with pytest.raises(ValueError, match="orientation must be one of"):
        cloud.estimate_normals(orientation="tombari")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_ops.orient_normals(torch.zeros(1, 50, 3), torch.zeros(1, 50, 3))
    from dss_amd import ops
    one, fifty = torch.zeros(1, dtype=torch.int64), torch.full((1,), 50, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.orient_normals(torch.zeros(50, 3), torch.zeros(50, 3), torch.zeros(50, 8, dtype=torch.int64), one, fifty)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disambiguate_normals(torch.zeros(50, 3), torch.zeros(50, 3), torch.zeros(50, 8, dtype=torch.int64), one, fifty)


def test_the_new_kernels_stay_in_registers():
    """ScratchSize 0 for the four kernels of csrc/normals.hip; the propagation kernel's LDS is the capacity that normals_ops
    states, four bytes a point, within a compute unit's 160 KiB; its 1024 threads leave 128 VGPRs."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "dss_amd", "csrc", "normals.hip"),
                          "-o", os.devnull], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    scratch, vgprs, lds, name = {}, {}, {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for table, pattern in ((scratch, r"ScratchSize \[bytes/lane\]: (\d+)"), (vgprs, r" VGPRs: (\d+)"),
                               (lds, r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pattern, line)
            if m and name:
                table[name] = int(m.group(1))
    print({k: (vgprs[k], scratch[k], lds[k]) for k in scratch})
    orient = sorted(k for k in scratch if "orient_normals_kernel" in k)
    assert len(orient) == 2 and len(scratch) == 4
    assert any("disambiguate_normals_kernel" in k for k in scratch) and any("normals_unowned_kernel" in k for k in scratch)
    assert all(v == 0 for v in scratch.values()), scratch
    assert all(vgprs[k] <= 128 for k in orient)
    in_lds, in_ws = sorted(orient, key=lambda k: -lds[k])
    assert 4 * normals_ops.LDS_CAPACITY <= lds[in_lds] <= 4 * normals_ops.LDS_CAPACITY + 1024 and lds[in_lds] <= 160 * 1024
    assert lds[in_ws] <= 1024
