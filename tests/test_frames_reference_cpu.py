"""CPU: the fp64 reference of the PCA frames (frames_reference.py) pinned before the GPU tests lean on it."""
import os

import numpy as np
from scipy.spatial import cKDTree

import frames_reference as fr
import oracle


def _teapot(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_setup_teapot.npz"))
    pts = z["points"]
    _, idx = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=8)
    return z, pts, idx.astype(np.int64)


def test_reference_agrees_with_the_oracle_and_with_the_reference_python_golden(golden_dir):
    """One cloud, K = 8, where `oracle.local_frames` (fp64 Jacobi, packed ids, 1/K) states the same thing: vr6 and the
    curvatures agree to the rounding of the oracle's float32 outputs (half an ulp of a value below the trace, 2^-24 tr) plus
    fp64 round-off over the smallest gap of the cloud (8.6e-3); and vr6 agrees with the reference's own
    `_compute_anisotropic_Vrk` (golden `aniso_Vr`) under the bound and the gap mask of
    test_gpu_setup.py::test_local_frames_match_oracle_and_reference_golden."""
    z, pts, idx = _teapot(golden_dir)
    P = len(pts)
    ref = fr.local_frames_reference(pts, idx, [0], [P])
    o_vr6, o_fn, o_cv = oracle.local_frames(pts, idx)
    assert ref.owned.all() and ref.C.dtype == ref.lam.dtype == ref.vr6.dtype == np.float64
    tr = np.trace(ref.C, axis1=1, axis2=2)
    assert (tr > 0).all() and np.allclose(ref.lam.sum(1), tr, rtol=1e-12)
    assert (ref.lam[:, 0] <= ref.lam[:, 1]).all() and (ref.lam[:, 1] <= ref.lam[:, 2]).all()
    tol = (2.0 ** -24 + 1e-12) * tr[:, None]
    assert (np.abs(ref.lam - o_cv) <= tol).all(), float((np.abs(ref.lam - o_cv) / tr[:, None]).max())
    assert (np.abs(ref.vr6 - o_vr6) <= tol).all(), float((np.abs(ref.vr6 - o_vr6) / tr[:, None]).max())
    gap = (ref.lam[:, 1] - ref.lam[:, 0]) / ref.lam[:, 2]
    assert (1 - np.abs((ref.vec[:, :, 0] * o_fn).sum(1)) <= 1e-6)[gap > 1e-2].all()
    # the eigenpairs are eigenpairs of C, and vr6 = C - lam0 e0 e0^T annihilates e0
    assert np.abs(np.einsum("pab,pbk->pak", ref.C, ref.vec) - ref.vec * ref.lam[:, None, :]).max() <= 1e-15 * tr.max()
    assert np.abs(np.einsum("pab,pb->pa", fr.mat33(ref.vr6), ref.vec[:, :, 0])).max() <= 1e-15 * tr.max()
    ref_vr = z["aniso_Vr"]
    ok = gap > 1e-2
    assert ok.mean() > 0.99
    assert np.abs(fr.mat33(ref.vr6) - ref_vr)[ok].max() <= 3e-4 * np.abs(ref_vr).max()


def test_reference_follows_the_packed_layout_and_clouds_shorter_than_k():
    """cloud-local ids plus first[n]; kk = min(K, num[n]) entries divided by kk (against numpy.cov of the whole small cloud);
    the documented constants in the slots that no cloud owns; the float32 yardstick stays close to the reference"""
    rng = np.random.default_rng(2)
    a, b = rng.normal(size=(40, 3)).astype(np.float32), (rng.normal(size=(5, 3)) + 9).astype(np.float32)
    gap = np.full((3, 3), np.nan, np.float32)
    pts = np.concatenate([gap[:2], a, gap, b, gap[:1]])
    first, num = np.array([2, 45]), np.array([40, 5])
    idx = np.zeros((len(pts), 8), np.int64)
    idx[2:42] = cKDTree(a.astype(np.float64)).query(a.astype(np.float64), k=8)[1]
    idx[45:50, :5] = cKDTree(b.astype(np.float64)).query(b.astype(np.float64), k=5)[1]
    ref = fr.local_frames_reference(pts, idx, first, num)
    covered = np.zeros(len(pts), bool)
    covered[2:42] = covered[45:50] = True
    assert np.array_equal(ref.owned, covered) and np.isfinite(ref.vr6).all() and np.isfinite(ref.vec).all()
    assert (ref.C[~covered] == 0).all() and (ref.lam[~covered] == fr.CONST_CURV).all() and (ref.vr6[~covered] == fr.CONST_VR6).all()
    assert (ref.vec[~covered][:, :, 0] == fr.CONST_NORMAL).all()
    assert np.allclose(ref.C[45:50], np.cov(b.astype(np.float64).T, bias=True), rtol=1e-12, atol=0)
    alone = fr.local_frames_reference(a, idx[2:42], [0], [40])
    assert np.array_equal(alone.C, ref.C[2:42]) and np.array_equal(alone.vr6, ref.vr6[2:42])
    p7 = a.astype(np.float64)[idx[9]]
    assert np.allclose(ref.C[9], np.cov(p7.T, bias=True), rtol=1e-12, atol=1e-15)
    C32, l32 = fr.local_frames_fp32(pts, idx, first, num)
    assert C32.dtype == l32.dtype == np.float32 and (C32[~covered] == 0).all()
    tr = np.trace(ref.C, axis1=1, axis2=2)[covered]
    assert (np.abs(C32 - ref.C)[covered].reshape(45, -1).max(1) <= 1e-6 * tr).all()
    assert (np.abs(l32 - ref.lam)[covered].max(1) <= 1e-6 * tr).all()
