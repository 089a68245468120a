"""CPU: the restatement of the mesh rasteriser's rule (tests/mesh_raster_reference.py) is sound before the GPU tests hold
the kernels to it bit for bit -- float32 and float64 pick the same face on every pixel of the icosphere scenes, a convex
silhouette has no hole, the inclusive edge rule covers a lattice quad completely and gives its diagonal to the smaller id,
and pytorch3d's strict rule, put in as a mutation, fails that test.  Also the new entries' ABI and their refusals."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_raster_reference as mr

SCENES = [(1, 32), (3, 64), (3, 33), (4, 128)]   # (icosphere level, image size)


def _scene(level, S):
    verts, faces = mr.icosphere(level)
    M, V, cam, zn, zf = mr.look_at_camera(2.0, 17.0, 33.0, fov=60.0, znear=0.1, zfar=10.0)
    return mr.screen_verts(verts, M, V), faces, zn, zf


@pytest.mark.parametrize("level,S", SCENES)
def test_icosphere_float32_and_float64_agree_and_silhouette_has_no_hole(level, S):
    sv, faces, zn, zf = _scene(level, S)
    p32, z32, b32 = mr.rasterize(sv, faces, zn, zf, S, np.float32)
    p64, z64, b64 = mr.rasterize(sv, faces, zn, zf, S, np.float64)
    assert z32.dtype == np.float32 and b32.dtype == np.float32 and z64.dtype == np.float64
    diff = np.argwhere(p32 != p64)
    assert len(diff) == 0, "%d pixels differ, first %s: %d vs %d" % (len(diff), diff[0], p32[tuple(diff[0])], p64[tuple(diff[0])])
    mask = p32 >= 0
    assert mask.any() and 0.5 < mask.mean() <= 1.0     # a unit sphere at distance 2 under a 60 degree field of view
    for name, lines in (("row", mask), ("column", mask.T)):
        for i, line in enumerate(lines):
            on = np.nonzero(line)[0]
            assert len(on) == 0 or len(on) == on[-1] - on[0] + 1, "%s %d of the mask has a hole" % (name, i)
    cov = mask
    assert np.abs(z32[cov] - z64[cov]).max() <= 1e-5 * z64[cov].max()
    assert np.abs(b32[cov].sum(-1) - 1).max() <= 1e-5 and (b32[cov] >= 0).all()
    assert (z32[~cov] == -1).all() and (b32[~cov] == 0).all()
    # the order in which the faces are visited does not show
    order = np.random.default_rng(level).permutation(len(faces))
    p_perm, z_perm, b_perm = mr.rasterize(sv, faces, zn, zf, S, np.float32, order=list(order))
    assert (p_perm == p32).all() and (z_perm.view(np.uint32) == z32.view(np.uint32)).all()
    assert (b_perm.view(np.uint32) == b32.view(np.uint32)).all()


QUADS = [dict(diagonal=0), dict(diagonal=1), dict(diagonal=0, reverse_second=True), dict(diagonal=1, reverse_second=True),
         dict(diagonal=0, welded=False), dict(diagonal=1, welded=False, reverse_second=True)]


def check_lattice_quad(rasterize, **quad):
    """the quad test, for any rasteriser with `mr.rasterize`'s signature: all 36 pixels covered, both faces seen, the pixels
    of the diagonal (covered by both faces) go to face 0"""
    S = 8
    verts, faces = mr.lattice_quad(S, 1, 6, **quad)
    p, z, b = rasterize(verts, faces, np.float32(0.1), np.float32(10.0), S)
    inside = np.zeros((S, S), bool)
    inside[1:7, 1:7] = True
    assert ((p >= 0) == inside).all(), "%d of 36 pixels covered" % int((p >= 0).sum())
    rows, cols = np.nonzero(inside)
    on_diag = (rows == cols) if quad.get("diagonal", 0) == 0 else (rows + cols == S - 1)
    # image column c <-> NDC index S - 1 - c in both axes: the lattice is symmetric under that flip, and so is either diagonal
    assert (p[rows[on_diag], cols[on_diag]] == 0).all(), "a pixel of the shared edge went to the larger face id"
    assert set(np.unique(p[inside])) == {0, 1}
    assert np.abs(z[inside] - 1.0).max() <= 4e-7          # b0 + b1 + b2 = 1 to a few roundings


@pytest.mark.parametrize("quad", QUADS)
def test_lattice_quad_is_covered_and_its_diagonal_goes_to_the_smaller_id(quad):
    check_lattice_quad(lambda *a: mr.rasterize(*a, dtype=np.float32), **quad)
    check_lattice_quad(lambda *a: mr.rasterize(*a, dtype=np.float64), **quad)


def test_strict_rule_mutation_fails_the_quad_test():
    strict = lambda *a: mr.rasterize(*a, dtype=np.float32, strict=True)
    verts, faces = mr.lattice_quad(8, 1, 6)
    p, _, _ = strict(verts, faces, np.float32(0.1), np.float32(10.0), 8)
    assert int((p >= 0).sum()) == 12          # the pixels strictly inside one of the two triangles
    for quad in QUADS:
        with pytest.raises(AssertionError, match="pixels covered"):
            check_lattice_quad(strict, **quad)


def test_absent_faces_and_ties_in_the_restatement():
    S = 16
    verts = np.asarray([(-0.9, -0.9, 1), (0.9, -0.9, 1), (0.0, 0.9, 1), (0.0, 0.0, np.nan), (0.5, 0.5, 0.05), (0.5, 0.5, 11)],
                       np.float32)
    good = (0, 1, 2)
    faces = np.asarray([(0, 1, -1), (0, 1, 6), (0, 1, 3), (0, 1, 4), (0, 1, 5), (0, 1, 1), good, good], np.int64)
    assert mr.present_faces(verts, faces, np.float32(0.1), np.float32(10)) == [6, 7]
    p, z, b = mr.rasterize(verts, faces, np.float32(0.1), np.float32(10), S)
    assert set(np.unique(p)) == {-1, 6}                      # coincident faces: the smaller id
    world = verts.copy()
    # seen from the origin the normal (B - A) x (C - A) = +z of face 6 points away: a back face; reversed it is a front face
    assert mr.present_faces(verts, faces[6:7], np.float32(0.1), np.float32(10), cull=(world, np.zeros(3))) == []
    assert mr.present_faces(verts, faces[6:7, ::-1], np.float32(0.1), np.float32(10), cull=(world, np.zeros(3))) == [0]


def test_abi_of_the_mesh_entries_and_their_refusals():
    from dss_amd import _lib, ops
    import dss_amd
    lib = _lib.load()
    for name in ("dss_mesh_raster_workspace", "dss_rasterize_meshes", "dss_mesh_flat_shade"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["dss_rasterize_meshes"][1][-1] is ctypes.c_void_p
    small, big = lib.dss_mesh_raster_workspace(1, 100, 60, 64), lib.dss_mesh_raster_workspace(8, 81920, 40962, 512)
    assert 0 < small < big and lib.dss_mesh_raster_workspace(2, 100, 60, 64) > small
    assert lib.dss_mesh_raster_workspace(1, 100, 60, 33) == lib.dss_mesh_raster_workspace(1, 100, 60, 40)
    assert lib.dss_mesh_raster_workspace(1, 0, 0, 1) > 0
    for bad in ((0, 10, 10, 8), (1, -1, 10, 8), (1, 10, 10, 0), (1, 1 << 31, 10, 8), (1, 10, 1 << 31, 8), (1, 10, 10, 40000)):
        assert lib.dss_mesh_raster_workspace(*bad) == 0 and b"dss_mesh_raster_workspace" in lib.dss_last_error()
    rc = lib.dss_rasterize_meshes(None, 3, None, None, None, 1, None, None, None, None, None, 1, 1, 0, 8, None, None, None, None,
                                  None, 0, None)
    assert rc == -1 and b"dss_rasterize_meshes: NULL" in lib.dss_last_error()
    rc = lib.dss_rasterize_meshes(None, 0, None, None, None, 0, None, None, None, None, None, 1, 1, 0, 0, None, None, None, None,
                                  None, 0, None)
    assert rc == -1 and b"dss_rasterize_meshes: bad sizes" in lib.dss_last_error()
    rc = lib.dss_mesh_flat_shade(None, None, None, 0, None, None, None, 0, None, 1, 1, 8, None, None, None, None, -1, 0, None,
                                 64.0, 1.0, 1.0, 1.0, None, None)
    assert rc == -1 and b"dss_mesh_flat_shade" in lib.dss_last_error()
    assert ops.rasterize_meshes is not None and ops.shade_mesh_flat is not None and callable(dss_amd.render_mesh_targets)
    verts, faces = (torch.from_numpy(a) for a in mr.icosphere(0))
    one = torch.zeros(1, dtype=torch.int64)
    eye = torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rasterize_meshes(verts, faces, one, one + 20, eye, eye, torch.ones(1), torch.ones(1), torch.zeros(1, 3), 8)
    from dss_amd.cameras import FoVPerspectiveCameras
    from dss_amd.texture import PointLights
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dss_amd.render_mesh_targets((verts, faces), FoVPerspectiveCameras(), PointLights(), image_size=8)
