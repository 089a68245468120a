"""CPU: the yardstick of farthest point sampling (tests/farthest_reference.py) on itself -- distinct ids, non-increasing radii,
the tie rule on the integer lattice against exact integer arithmetic, duplicate points, and the float64 teacher-forced check on
every scene of the GPU tests; the exports and the ABI conventions of the two new entries; the refusals of the entry, reached
without a GPU, and of the public calls; the compiler's resource report of every instantiation of the kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import farthest_reference as yard
from dss_amd import cloud_ops, sampling_ops
from dss_amd.cloud import PointClouds3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = yard.single_cloud_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_yardstick_invariants_and_the_float64_check(name):
    x, k, start = CASES[name]
    idx, rad = yard.farthest(x, k, start)
    assert len(idx) == min(k, x.shape[0]) and idx[0] == start and np.isinf(rad[0])
    assert len(set(idx.tolist())) == len(idx)                      # distinct
    assert (idx >= 0).all() and (idx < x.shape[0]).all()
    assert (rad[1:] <= rad[:-1]).all() and (rad >= 0).all()          # d only ever decreases
    worst = yard.teacher_forced(x, idx)
    print("%s: smallest d64[pick] / max d64 = 1 - %.3g" % (name, 1.0 - worst))
    assert worst >= 1.0 - yard.REL


def test_the_float64_check_refuses_a_wrong_sequence():
    x, k, _ = CASES["random_257_all"]
    idx, _ = yard.farthest(x, k)
    bad = idx.copy()
    bad[[1, 200]] = bad[[200, 1]]          # the farthest point is taken late
    with pytest.raises(AssertionError):
        yard.teacher_forced(x, bad)
    with pytest.raises(AssertionError, match="again"):
        yard.teacher_forced(x, np.concatenate([idx[:5], idx[2:3]]))


def test_ties_go_to_the_smallest_id_on_the_lattice():
    x = yard.lattice()
    idx, rad = yard.farthest(x, 125)
    assert idx[:3].tolist() == [0, 124, 14]       # (0,0,0), (4,4,4), then (0,2,4): the smallest id of the six at distance 20
    assert rad[1] == 48.0 and rad[2] == 20.0
    assert np.array_equal(idx, yard.exact_integer_fps(x, 125))
    assert sorted(idx.tolist()) == list(range(125))


def test_duplicate_points_are_never_selected_twice():
    x = yard.duplicates()
    idx, rad = yard.farthest(x, 200)
    assert sorted(idx.tolist()) == list(range(200))
    assert (rad[:40] > 0).all() and (rad[40:] == 0).all()
    assert sorted((idx[:40] % 40).tolist()) == list(range(40))     # the first 40 picks are the 40 distinct points


def test_a_nan_point_is_selected_second_and_never_again():
    x = yard.with_nan()
    idx, rad = yard.farthest(x, 50)
    assert idx[1] == 13 and np.isinf(rad[1]) and np.isfinite(rad[2:]).all()
    assert sorted(idx.tolist()) == list(range(50))
    # the step whose centre is the NaN point changes nothing: the third pick is the farthest from point 0 alone
    d0 = ((x.astype(np.float64) - x[0]) ** 2).sum(-1)
    d0[[0, 13]] = -1
    assert idx[2] == int(np.argmax(d0))


def test_rows_pad_and_clamp():
    a, b = yard.random_cloud(10, 3), yard.random_cloud(0, 0)
    idx, rad = yard.rows([a, b], [16, 5], 12)
    assert idx.shape == (2, 12) and (idx[0, :10] >= 0).all() and (idx[0, 10:] == -1).all() and (idx[1] == -1).all()
    assert (rad[0, 10:] == 0).all() and (rad[1] == 0).all()


def test_exports_and_abi_conventions():
    import dss_amd
    from dss_amd import _lib, ops
    assert dss_amd.sample_farthest_points is cloud_ops.sample_farthest_points
    assert dss_amd.subsample is cloud_ops.subsample
    assert callable(ops.farthest_points) and ops.farthest_points is sampling_ops.farthest_points
    header = open(os.path.join(ROOT, "include", "dss_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret in (("dss_farthest_points_workspace", "size_t"), ("dss_farthest_points", "int")):
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
    args = re.search(r"DSS_API\s+int\s+dss_farthest_points\s*\(([^;]*)\);", header).group(1)
    assert args.strip().endswith("void *stream") and _lib.SIGNATURES["dss_farthest_points"][1][-1] is ctypes.c_void_p
    assert _lib.load().dss_version() == 103


def _entry(lib, ptrs, N, P, K_max, ws=None, ws_bytes=0, idx=None):
    return lib.dss_farthest_points(ptrs, ptrs, ptrs, ptrs, None, N, P, K_max, ptrs if idx is None else idx, None, ws, ws_bytes,
                                   None)


def test_refusals_of_the_entry_are_reached_without_a_gpu():
    from dss_amd import _lib
    lib = _lib.load()
    host = ctypes.create_string_buffer(64)          # stands for device memory: a refused call launches nothing
    p = ctypes.addressof(host)
    for N, P, K_max in ((0, 10, 4), (-1, 10, 4), (1, -1, 4), (1, 10, -1), (1, 1 << 31, 4)):
        assert _entry(lib, p, N, P, K_max) == -1
        msg = lib.dss_last_error()
        assert b"dss_farthest_points: bad sizes" in msg and (b"N=%d P=%d K_max=%d" % (N, P, K_max)) in msg
    assert _entry(lib, None, 1, 10, 4) == -1 and b"NULL" in lib.dss_last_error()
    assert lib.dss_farthest_points(p, p, p, p, None, 1, 10, 4, None, None, None, 0, None) == -1     # idx is required
    assert b"NULL" in lib.dss_last_error()
    # the workspace: none is needed while every cloud fits the registers
    big = sampling_ops.MAX_REGISTER_POINTS + 1
    assert lib.dss_farthest_points_workspace(1, sampling_ops.MAX_REGISTER_POINTS) == 0
    need = lib.dss_farthest_points_workspace(3, big)
    assert need >= 4 * big
    assert _entry(lib, p, 1, big, 4) == -1 and b"workspace" in lib.dss_last_error()
    assert _entry(lib, p, 1, big, 4, ws=p, ws_bytes=need - 1) == -1 and b"workspace" in lib.dss_last_error()
    # the empty calls return 0 without a launch
    assert _entry(lib, None, 1, 0, 4) == 0
    assert _entry(lib, None, 2, 10, 0) == 0


def _no_library(monkeypatch):
    from dss_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)


@pytest.mark.parametrize("args,kw,what", [
    ((torch.zeros(1, 50, 3),), dict(K=-1), "negative count"),
    ((torch.zeros(2, 50, 3),), dict(K=[5, -2]), "negative count"),
    ((torch.zeros(1, 50, 3),), dict(start_idx=50), "start_idx 50 lies outside"),
    ((torch.zeros(1, 50, 3),), dict(start_idx=-1), "start_idx -1 lies outside"),
    ((torch.zeros(2, 50, 3), [50, 20]), dict(start_idx=torch.tensor([0, 20])), "start_idx 20 lies outside cloud 1"),
    ((torch.zeros(1, 50, 3), [51]), {}, "lengths must lie"),
    ((torch.zeros(1, 50, 3), [50, 50]), {}, "lengths must be"),
    ((torch.zeros(1, 50, 3),), dict(K=[1, 2, 3]), "K must be"),
    ((torch.zeros(50, 3),), {}, "expects padded points"),
    ((torch.zeros(1, 50, 2),), {}, "expects padded points"),
])
def test_sampling_refusals_come_before_the_library(args, kw, what, monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=what):
        cloud_ops.sample_farthest_points(*args, **kw)


def _cpu_cloud():
    g = torch.Generator().manual_seed(0)
    sizes = (40, 30)
    return PointClouds3D([torch.rand(s, 3, generator=g) for s in sizes], [torch.rand(s, 3, generator=g) for s in sizes],
                         [torch.rand(s, 2, generator=g) for s in sizes])


@pytest.mark.parametrize("kw,what", [
    (dict(n_points=-1), "negative count"),
    (dict(ratio=1.5), "ratio must lie"),
    (dict(ratio=-0.1), "ratio must lie"),
    (dict(ratio=[0.5, float("nan")]), "ratio must lie"),
    (dict(n_points=10, ratio=0.5), "exactly one"),
    (dict(), "exactly one"),
    (dict(n_points=10, method="poisson"), "method must be"),
    (dict(n_points=10, start_idx=[0, 30]), "start_idx 30 lies outside cloud 1"),
    (dict(n_points=[1, 2, 3]), "n_points must be"),
])
def test_subsample_refusals_come_before_the_library(kw, what, monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=what):
        cloud_ops.subsample(_cpu_cloud(), **kw)


def test_cpu_tensors_are_refused(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_ops.sample_farthest_points(torch.zeros(1, 50, 3), K=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_ops.sample_farthest_points(_cpu_cloud(), K=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_ops.subsample(_cpu_cloud(), n_points=5)
    from dss_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.farthest_points(torch.zeros(50, 3), torch.zeros(1, dtype=torch.int64), torch.full((1,), 50, dtype=torch.int64),
                            torch.full((1,), 5, dtype=torch.int64), None, 5)


def test_random_subsampling_is_the_reference_rule(monkeypatch):
    """method="random" launches no kernel of the library: int(ratio P_n) distinct rows of a randperm, attributes following"""
    _no_library(monkeypatch)
    cloud = _cpu_cloud()
    out = cloud_ops.subsample(cloud, ratio=0.33, method="random", generator=torch.Generator().manual_seed(5))
    again = cloud_ops.subsample(cloud, ratio=0.33, method="random", generator=torch.Generator().manual_seed(5))
    for n, s in enumerate((40, 30)):
        p, nr, f = out.points_list()[n], out.normals_list()[n], out.features_list()[n]
        assert p.shape == (int(0.33 * s), 3) and nr.shape == p.shape and f.shape == (p.shape[0], 2)
        rows = [int((cloud.points_list()[n] == q).all(-1).nonzero()[0, 0]) for q in p]
        assert len(set(rows)) == len(rows)
        assert torch.equal(nr, cloud.normals_list()[n][rows]) and torch.equal(f, cloud.features_list()[n][rows])
        assert torch.equal(p, again.points_list()[n])


def test_every_instantiation_stays_in_registers():
    """x, y, z, d of R points per thread are statically indexed: ScratchSize 0 everywhere, and a workgroup of T threads
    (T / 256 wavefronts per SIMD, 512 registers per SIMD lane) needs at most 512 / (T / 256) VGPRs, of which an instruction
    addresses the first 256: 128 for a 1024-thread workgroup.  The instantiations found are those that sampling_ops exports."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "dss_amd", "csrc", "sampling.hip"),
                          "-o", os.devnull], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    scratch, vgprs, name = {}, {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r" VGPRs: (\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
    reg = {k: re.search(r"fps_register_kernelILi(\d+)ELi(\d+)EE", k) for k in scratch if "fps_register_kernel" in k}
    stream = [k for k in scratch if "fps_stream_kernel" in k]
    assert len(reg) == len(sampling_ops.REGISTER_CAPACITIES) == 5 and len(stream) == 1
    shapes = sorted((int(m.group(1)), int(m.group(2))) for m in reg.values())
    assert tuple(sorted(t * r for t, r in shapes)) == sampling_ops.REGISTER_CAPACITIES
    assert sampling_ops.MAX_REGISTER_POINTS == max(t * r for t, r in shapes)
    print({k: (vgprs[k], scratch[k]) for k in list(reg) + stream})
    assert all(scratch[k] == 0 for k in list(reg) + stream), scratch
    for k, m in reg.items():
        T = int(m.group(1))
        assert vgprs[k] <= min(256, 512 // max(T // 256, 1)), (k, vgprs[k])
    assert vgprs[stream[0]] <= 128   # the 1024-thread instantiation
