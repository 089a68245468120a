"""CPU: the restatement of the surface sampler's rule (tests/mesh_sample_reference.py) is sound before the GPU tests hold
the kernels to it bit for bit -- Philox4x32-10 reproduces the published known answers, the table never yields a key-0
face, the face counts follow the areas (conditions at 5 and 4 standard deviations on fixed inputs: deterministic), every
point lies on its face, and the result has the invariances the integer key and the counter were chosen for.  Also the
new entries' ABI and their refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mesh_distance_reference as md
import mesh_sample_reference as ms

SCENES = [(1, (1.0, 1.0, 1.0), 4096, 80), (2, (1.0, 0.5, 2.0), 20000, 320), (3, (1.0, 1.0, 1.0), 20000, 1280)]
SEEDS = [0, 1, 2 ** 40 + 7]


@functools.lru_cache(maxsize=None)
def _sample(level, scale, S, seed):
    verts, faces = ms.icosphere(level, scale)
    return (verts, faces) + ms.sample_mesh(verts, faces, S, seed)


def test_philox_known_answers():
    """the three known answers of the Random123 distribution (kat_vectors: philox4x32 10)"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = " ".join("%08x" % int(w[0]) for w in ms.philox4x32_10(counter, key))
        assert got == want, (counter, key, got)
    # an array of counters gives what the counters give one by one
    r = ms.sample_words(3, 5, 2 ** 40 + 7)
    for s in range(5):
        one = ms.philox4x32_10((s, 0, 3, 0), (7, 2 ** 8))
        assert [int(w[s]) for w in r] == [int(w[0]) for w in one]


@pytest.mark.parametrize("keys", [[0, 0, 5, 3, 0, 2], [4, 0, 0, 1, 7], [1, 2, 3, 0, 0], [0, 9, 0], [0, 0, 1]])
def test_pick_never_returns_a_key_zero_face(keys):
    cum = ms.cumulate(keys)
    total = cum[-1]
    nonzero = [f for f, k in enumerate(keys) if k]
    for target in range(total):
        f = ms.pick(cum, target)
        assert keys[f] > 0 and cum[f] > target and (f == 0 or cum[f - 1] <= target), (target, f)
    for c in cum:                                   # a target equal to an entry of cum goes past every key-0 face behind it
        if c < total:
            assert keys[ms.pick(cum, c)] > 0 and cum[ms.pick(cum, c)] > c
    assert ms.pick(cum, total - 1) == nonzero[-1]
    assert ms.pick(cum, 0) == nonzero[0]
    hits = [sum(1 for t in range(total) if ms.pick(cum, t) == f) for f in range(len(keys))]
    assert hits == keys                             # every face owns exactly key_f of the total targets


def test_keys_are_scaled_by_a_power_of_two():
    ln = np.asarray([1.0, 2.0 ** -12, 2.0 ** -34, 0.0, 0.75, 2.0 ** -31, 2.0 ** -31 * 1.5], np.float32)
    assert ms.area_keys(ln) == [2 ** 31, 2 ** 19, 0, 0, 3 * 2 ** 29, 1, 1]
    for scale in (2.0 ** 7, 2.0 ** -9, 2.0 ** -60):
        assert ms.area_keys(ln * np.float32(scale)) == ms.area_keys(ln)
    assert ms.area_keys(np.asarray([1.9999999], np.float32)) == [2 ** 32 - 2 ** 8] and ms.area_keys(np.zeros(3, np.float32)) == [0, 0, 0]
    big = np.asarray([3e38, 1e38], np.float32)
    assert max(ms.area_keys(big)) <= 2 ** 32 and min(ms.area_keys(big)) >= 2 ** 29
    assert ms.area_keys(np.zeros(0, np.float32)) == []


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("level,scale,S,F", SCENES)
def test_counts_follow_areas(level, scale, S, F, seed):
    verts, faces, points, normals, fi, bary = _sample(level, scale, S, seed)
    assert len(faces) == F
    keys = np.asarray(ms.area_keys(ms.face_lengths(verts, faces)[0]), np.float64)
    expected = S * keys / keys.sum()
    count = np.bincount(fi, minlength=F).astype(np.float64)
    sigma = np.sqrt(expected * (1.0 - expected / S))
    worst = np.abs(count - expected) / sigma
    dof = F - 1
    chi2 = ((count - expected) ** 2 / expected).sum()
    print("level %d seed %d: worst face %.2f sigma, chi2 %.1f for %d dof = %.2f sigma"
          % (level, seed, worst.max(), chi2, dof, (chi2 - dof) / np.sqrt(2 * dof)))
    assert (np.abs(count - expected) <= 5.0 * sigma).all()
    assert abs(chi2 - dof) <= 4.0 * np.sqrt(2.0 * dof)


@pytest.mark.parametrize("level,scale,S,F", SCENES)
def test_points_lie_on_their_faces_with_unit_normals(level, scale, S, F):
    verts, faces, points, normals, fi, bary = _sample(level, scale, S, 1)
    assert (bary >= 0).all() and np.abs(bary.astype(np.float64).sum(-1) - 1.0).max() <= 2.0 ** -23
    assert (fi >= 0).all() and (fi < F).all()
    tri = verts[faces[fi]].astype(np.float64)
    n64 = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert np.abs(normals - n64).max() <= 1e-6
    if scale == (1.0, 1.0, 1.0):                    # the bar is stated for the unit sphere
        step = max(1, S // 2048)                    # (a fixed stride of the samples: the distance is a (Q,F) matrix)
        sel = np.arange(0, S, step)
        for lo in range(0, len(sel), 256):
            part = sel[lo:lo + 256]
            D = md.d2_matrix(points[part], verts[faces[fi[part]]], np.float64)
            assert np.sqrt(np.diagonal(D)).max() <= 1e-6
    assert (np.linalg.norm(points / np.asarray(scale, np.float32), axis=1) <= 1.0 + 1e-6).all()


def test_invariances():
    verts, faces = ms.icosphere(2, (1.0, 0.5, 2.0))
    base = ms.sample_mesh(verts, faces, 4096, 5)
    for scale in (2.0 ** 7, 2.0 ** -9):             # the point of the power-of-two key
        other = ms.sample_mesh(verts * np.float32(scale), faces, 4096, 5)
        assert (other[2] == base[2]).all() and (other[3].view(np.uint32) == base[3].view(np.uint32)).all()
        assert (other[0].view(np.uint32) == (base[0] * np.float32(scale)).view(np.uint32)).all()
    # a mesh's samples depend on its place in the batch through the counter's n alone
    a, b = ms.icosphere(1), (verts, faces)
    ab, ba = ms.sample_batch(*ms.pack([a, b]), 512, 9), ms.sample_batch(*ms.pack([b, a]), 512, 9)
    alone = ms.sample_mesh(verts, faces, 512, 9, n=1)
    for k in range(4):
        assert (ab[k][1] == alone[k]).all()
    assert not (ba[2][0] == ab[2][1]).all()         # the same mesh as mesh 0 draws other faces
    first = ms.sample_mesh(verts, faces, 512, 9, n=0)
    for k in range(4):
        assert (ba[k][0] == first[k]).all()
    # two seeds; a seed that differs in the high word only
    assert not (ms.sample_mesh(verts, faces, 512, 6)[2] == base[2][:512]).all()
    assert not (ms.sample_mesh(verts, faces, 512, 5 + 2 ** 32)[2] == base[2][:512]).all()
    # sample s does not depend on S
    short = ms.sample_mesh(verts, faces, 100, 5)
    for k in range(4):
        assert (short[k] == base[k][:100]).all()


def test_meshes_with_nothing_to_sample_and_the_hostile_mesh():
    for verts, faces in (ms.empty_mesh(), ms.degenerate_mesh()):
        p, nrm, fi, bary = ms.sample_mesh(verts, faces, 7, 3)
        assert (p == 0).all() and (nrm == 0).all() and (bary == 0).all() and (fi == -1).all() and fi.shape == (7,)
    out = ms.sample_batch(*ms.pack(ms.batch_of_five()), 300, 11)
    assert [bool((out[2][n] >= 0).all()) for n in range(5)] == [True, False, True, False, True]
    assert (out[2][1] == -1).all() and (out[0][3] == 0).all() and (out[2][2] == 0).all()
    verts, faces, undrawable = ms.hostile_mesh()
    ln, _ = ms.face_lengths(verts, faces)
    keys = ms.area_keys(ln)
    assert max(keys) == 2 ** 31 and sorted(np.nonzero(np.asarray(keys) == 0)[0]) == sorted(undrawable)
    assert 2 ** 19 in keys and ln[40 + 3] > 0        # the 2^-34 face is present and still never drawn
    p, nrm, fi, bary = ms.sample_mesh(verts, faces, 20000, 4)
    assert not np.isin(fi, undrawable).any() and np.isfinite(p).all() and np.isfinite(nrm).all() and np.isfinite(bary).all()
    assert (fi == 41).sum() > 2000                   # the large face (about a seventh of the total) takes its share


def test_backward_restatements_agree():
    meshes = ms.batch_of_five()
    verts, faces, first, num = ms.pack(meshes)
    _, _, fi, bary = ms.sample_batch(verts, faces, first, num, 200, 2)
    g = np.random.default_rng(0).standard_normal((5, 200, 3)).astype(np.float32)
    g32 = ms.backward(len(verts), faces, first, num, fi, bary, g, np.float32)
    g64 = ms.backward(len(verts), faces, first, num, fi, bary, g, np.float64)
    assert np.linalg.norm(g32 - g64) <= 1e-6 * np.linalg.norm(g64)
    # sum_v grad_verts[v] = sum over the samples of g (the weights of a sample sum to 1)
    assert np.abs(g64.sum(0) - g[fi >= 0].astype(np.float64).sum(0)).max() <= 1e-4
    deg_first = len(meshes[0][0]) + len(meshes[2][0])
    assert (g32[deg_first:deg_first + 4] == 0).all()  # the vertices of the degenerate mesh


def test_abi_of_the_sampler_entries_and_their_refusals():
    from dss_amd import _lib, ops
    import dss_amd
    lib = _lib.load()
    for name in ("dss_mesh_sample_workspace", "dss_sample_mesh_surface", "dss_mesh_sample_backward"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["dss_sample_mesh_surface"][1][8] is ctypes.c_uint64
    small, big = lib.dss_mesh_sample_workspace(1, 100), lib.dss_mesh_sample_workspace(8, 1 << 20)
    assert 0 < small < big and lib.dss_mesh_sample_workspace(1, 0) > 0
    for bad in ((0, 10), (1, -1), (1, 1 << 31), (70000, 10)):
        assert lib.dss_mesh_sample_workspace(*bad) == 0 and b"dss_mesh_sample_workspace" in lib.dss_last_error()
    rc = lib.dss_sample_mesh_surface(None, 3, None, None, None, 1, 1, 4, 0, None, None, None, None, None, 0, None)
    assert rc == -1 and b"dss_sample_mesh_surface: NULL" in lib.dss_last_error()
    rc = lib.dss_sample_mesh_surface(None, 3, None, None, None, 1, 1, -1, 0, None, None, None, None, None, 0, None)
    assert rc == -1 and b"dss_sample_mesh_surface: bad sizes" in lib.dss_last_error()
    assert lib.dss_sample_mesh_surface(None, 3, None, None, None, 1, 1, 0, 0, None, None, None, None, None, 0, None) == 0
    rc = lib.dss_mesh_sample_backward(None, None, None, 1, 1, 4, 3, None, None, None, None, None, None)
    assert rc == -1 and b"dss_mesh_sample_backward: NULL" in lib.dss_last_error()
    assert callable(ops.sample_mesh_surface) and callable(ops.mesh_sample_backward)
    assert callable(dss_amd.sample_points_from_meshes) and callable(dss_amd.sample_mesh_evenly)
    verts, faces = (torch.from_numpy(a) for a in ms.icosphere(0))
    one = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_mesh_surface(verts, faces, one, one + 20, 16, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_sample_backward(faces, one, one + 20, 12, torch.zeros(1, 16, dtype=torch.int64), torch.zeros(1, 16, 3),
                                 torch.zeros(1, 16, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dss_amd.sample_points_from_meshes((verts, faces), 16, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dss_amd.sample_mesh_evenly((verts, faces), 16, seed=0)
    import inspect
    assert list(inspect.signature(dss_amd.evaluate_cloud).parameters) == ["pred", "gt_cloud", "gt_mesh", "gt_samples", "seed"]
