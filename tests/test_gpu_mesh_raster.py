"""GPU: meshes to target images (`ops.rasterize_meshes`, `ops.shade_mesh_flat`, `dss_amd.render_mesh_targets`) against
tests/mesh_raster_reference.py (checked on the CPU by test_mesh_raster_cpu.py).

Bars.  pix_to_face, zbuf, bary and screen_verts: BIT-EQUAL to the float32 restatement of the rule of include/dss_hip.h (same
operations, same order, no contraction, correctly rounded division) -- no tolerance, on every path: binned and large faces,
chunked lists, several workgroups, image sizes that are no multiple of the tile.  Colours: rtol 2e-4, atol 1e-6 against the
float64 shader at the kernel's own pix_to_face and bary -- the bar tests/test_gpu_shading.py:78 holds the Phong forward to
(powf is why this is not bit-equal); background and alpha exact."""
import functools

import numpy as np
import pytest
import torch

import mesh_raster_reference as mr

pytestmark = pytest.mark.gpu

COLOUR_RTOL, COLOUR_ATOL = 2e-4, 1e-6     # tests/test_gpu_shading.py:78
TILE, BIN_TILES = 8, 16                   # csrc/mesh_raster.hip: DSS_TILE, MESH_BIN_TILES


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_floats(tag, got, want):
    """bit-equal, any NaN equal to any NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere((_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want)))
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got %r want %r" % (
        tag, len(bad), want.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _pack(meshes):
    """[(verts, faces with mesh-local vertex ids)] -> packed verts, faces with packed ids, first, num"""
    starts = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])[:-1]]).astype(np.int64)
    verts = np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])
    faces = np.concatenate([np.asarray(f, np.int64).reshape(-1, 3) + s for (_, f), s in zip(meshes, starts)])
    num = np.asarray([len(np.asarray(f).reshape(-1, 3)) for _, f in meshes], np.int64)
    first = np.concatenate([[0], np.cumsum(num)[:-1]]).astype(np.int64)
    return verts, faces, first, num


def _cams(cams):
    M, V, c, zn, zf = (np.stack([np.asarray(cam[k], np.float32) for cam in cams]) for k in range(5))
    return M, V, c, zn, zf


def _raster(verts, faces, first, num, cams, S, shared, cull=False):
    from dss_amd import ops
    M, V, c, zn, zf = _cams(cams)
    out = ops.rasterize_meshes(_t(verts), _t(faces), _t(first), _t(num), _t(M), _t(V), _t(zn), _t(zf), _t(c), S,
                               shared_mesh=shared, cull_backfaces=cull)
    torch.cuda.synchronize()
    N, nV = len(cams), len(verts)
    p, z, b, sv = out
    assert p.dtype == torch.int64 and p.shape == (N, S, S) and z.dtype == torch.float32 and z.shape == (N, S, S)
    assert b.dtype == torch.float32 and b.shape == (N, S, S, 3) and sv.dtype == torch.float32 and sv.shape == (N, nV, 3)
    return tuple(a.cpu().numpy() for a in out)


def _reference(verts, faces, first, num, cams, S, shared, cull=False):
    """the float32 restatement, camera by camera -> pix_to_face, zbuf, bary, screen_verts"""
    ps, zs, bs, svs = [], [], [], []
    for n, (M, V, c, zn, zf) in enumerate(cams):
        sv = mr.screen_verts(verts, M, V)
        m = 0 if shared else n
        fm = faces[first[m]:first[m] + num[m]]
        p, z, b = mr.rasterize(sv, fm, zn, zf, S, np.float32, cull=(verts, c) if cull else None)
        ps.append(p); zs.append(z); bs.append(b); svs.append(sv)
    return np.stack(ps), np.stack(zs), np.stack(bs), np.stack(svs)


def _compare(tag, got, want):
    p, z, b, sv = got
    wp, wz, wb, wsv = want
    _same_floats(tag + " screen_verts", sv, wsv)
    bad = np.argwhere(p != wp)
    assert len(bad) == 0, "%s pix_to_face: %d pixels differ, first at %s: got %d want %d" % (
        tag, len(bad), bad[0], p[tuple(bad[0])], wp[tuple(bad[0])])
    _same_floats(tag + " zbuf", z, wz)
    _same_floats(tag + " bary", b, wb)


def _check(tag, meshes, cams, S, shared=True, cull=False):
    packed = _pack(meshes)
    got = _raster(*packed, cams, S, shared, cull)
    _compare(tag, got, _reference(*packed, cams, S, shared, cull))
    return got


LOOK = dict(dist=2.0, elev=17.0, azim=33.0, fov=60.0, znear=0.1, zfar=10.0)


@functools.lru_cache(maxsize=None)
def _ico(level):
    return mr.icosphere(level)


@functools.lru_cache(maxsize=None)
def _ico_reference(level, S):
    """the restatement of an icosphere scene, computed once and shared"""
    return _reference(*_pack([_ico(level)]), [mr.look_at_camera(**LOOK)], S, True)


# ---- bit equality

@pytest.mark.parametrize("level,S", [(1, 32), (3, 64), (3, 33), (4, 128), (1, 1), (1, 7), (2, 33)])
def test_icosphere_scenes_bit_equal(level, S):
    got = _raster(*_pack([_ico(level)]), [mr.look_at_camera(**LOOK)], S, True)
    _compare("icosphere %d at %d" % (level, S), got, _ico_reference(level, S))
    assert (got[0] >= 0).any()


@pytest.mark.parametrize("quad", [dict(diagonal=0), dict(diagonal=1), dict(diagonal=0, reverse_second=True),
                                  dict(diagonal=1, reverse_second=True), dict(diagonal=0, welded=False),
                                  dict(diagonal=1, welded=False, reverse_second=True)])
def test_lattice_quads_bit_equal_and_fully_covered(quad):
    p, z, b, sv = _check("quad", [mr.lattice_quad(8, 1, 6, **quad)], [mr.identity_camera()], 8)
    assert int((p >= 0).sum()) == 36 and (p[0, 1:7, 1:7] >= 0).all()
    rows, cols = np.nonzero(p[0] >= 0)
    on_diag = (rows == cols) if quad["diagonal"] == 0 else (rows + cols == 7)
    assert (p[0, rows[on_diag], cols[on_diag]] == 0).all()


def test_triangle_larger_than_the_screen_coincident_faces_and_depth_order():
    cam = [mr.identity_camera()]
    big = (np.asarray([(-5, -4, 1), (6, -3, 1.5), (0, 7, 2)], np.float32), [(0, 1, 2)])
    p, z, b, _ = _check("all three vertices off screen", [big], cam, 33)
    assert (p == 0).all()
    tri = np.asarray([(-0.8, -0.7, 1), (0.9, -0.6, 1.3), (0.1, 0.8, 2)], np.float32)
    p, _, _, _ = _check("coincident faces", [(tri, [(0, 1, 2), (0, 1, 2)])], cam, 24)
    assert set(np.unique(p)) == {-1, 0}
    p, _, _, _ = _check("coincident faces behind a rotated copy", [(tri, [(1, 2, 0), (0, 1, 2), (0, 1, 2)])], cam, 24)
    assert 2 not in p and (p >= 0).any()                      # face 2 ties with face 1 everywhere and always loses
    near = np.asarray([(-0.8, -0.7, 1), (0.9, -0.6, 1), (0.1, 0.8, 1)], np.float32)
    far = near * np.asarray([1.1, 1.1, 3], np.float32)
    verts = np.concatenate([near, far])
    p01, _, _, _ = _check("near then far", [(verts, [(0, 1, 2), (3, 4, 5)])], cam, 24)
    p10, _, _, _ = _check("far then near", [(verts, [(3, 4, 5), (0, 1, 2)])], cam, 24)
    assert ((p01 == 0) == (p10 == 1)).all() and (p01 == 0).any() and (p01 == 1).any()   # the far one shows around the near one


def test_three_thousand_faces_in_one_tile():
    """a list of 47 chunks of 64 for one wavefront"""
    S, rng = 64, np.random.default_rng(5)
    lo, hi = mr.pix_to_ndc(24, S), mr.pix_to_ndc(31, S)          # NDC indices 24 .. 31 in both axes: one 8x8 tile
    n = 3000
    centre = rng.uniform(lo + 0.03, hi - 0.03, (n, 1, 2))
    xy = centre + rng.uniform(-0.03, 0.03, (n, 3, 2))
    zz = rng.uniform(1.0, 3.0, (n, 3, 1))
    verts = np.concatenate([xy, zz], axis=-1).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    p, _, _, _ = _check("stack", [(verts, faces)], [mr.identity_camera()], S)
    rows, cols = np.nonzero(p[0] >= 0)
    assert len(rows) > 30 and rows.min() // TILE == rows.max() // TILE and cols.min() // TILE == cols.max() // TILE


def test_icosphere_level_5_many_faces_per_tile():
    verts, faces = _ico(5)
    assert len(faces) == 20480
    _check("icosphere 5", [(verts, faces)], [mr.look_at_camera(**LOOK)], 64)


def _routes(verts, faces, S):
    """True where a face is binned, False where it travels on the large list (all faces present, identity camera)"""
    out = []
    for f in faces:
        c0, c1, r0, r1 = mr.face_rect(verts[f], S)
        out.append((c1 // TILE - c0 // TILE + 1) * (r1 // TILE - r0 // TILE + 1) <= BIN_TILES)
    return np.asarray(out)


def test_faces_on_both_sides_of_the_binned_large_threshold():
    S, rng, n = 64, np.random.default_rng(9), 40
    centre = rng.uniform(-0.15, 0.15, (n, 1, 2))
    shape = np.asarray([(0, 0), (1, 0), (0, 1)], np.float64)[None] + rng.uniform(0.0, 0.05, (n, 3, 2)) - 0.35
    xy = centre + shape * rng.uniform(0.45, 1.0, (n, 1, 2))          # 14 .. 32 pixels and the slack: 3 .. 5 tiles a side at 64^2
    verts = np.concatenate([xy, rng.uniform(1.0, 3.0, (n, 3, 1))], axis=-1).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    binned = _routes(verts, faces, S)
    assert 8 <= binned.sum() <= n - 8, binned.sum()                  # as is: both routes
    _check("mixed routes", [(verts, faces)], [mr.identity_camera()], S)
    for scale, want in ((0.4, True), (2.2, False)):                  # every face binned; every face large
        v = verts * np.asarray([scale, scale, 1], np.float32)
        assert (_routes(v, faces, S) == want).all()
        _check("scale %g" % scale, [(v, faces)], [mr.identity_camera()], S)
    # and the same faces at a size where the other route takes them all: the picture is the same rule either way
    assert _routes(verts, faces, 16).all() and not _routes(verts, faces, 256).any()
    _check("all binned at 16", [(verts, faces)], [mr.identity_camera()], 16)


# ---- absent faces, empty meshes

def test_absent_faces_are_ignored_and_their_neighbours_render():
    verts, faces = _ico(1)
    cam = mr.look_at_camera(**LOOK)
    nV = len(verts)
    axis = cam[2] / np.linalg.norm(cam[2])                                         # the camera sits at 2 axis
    extra = np.stack([np.asarray([0, 0, np.nan]), axis * 1.95, axis * -9.0]).astype(np.float32)   # NaN; in front of znear; beyond zfar
    v2 = np.concatenate([verts, extra])
    bad = np.asarray([(0, 1, -1), (0, 1, nV + 3), (0, 1, nV), (0, 1, nV + 1), (0, 1, nV + 2), (0, 1, 1), (5, 5, 5)], np.int64)
    sv = mr.screen_verts(v2, cam[0], cam[1])
    assert sv[nV + 1, 2] < cam[3] and sv[nV + 2, 2] > cam[4]
    plain = _check("plain", [(verts, faces)], [cam], 32)
    for where, f2 in (("behind", np.concatenate([faces, bad])), ("in front", np.concatenate([bad, faces]))):
        got = _check("bad faces " + where, [(v2, f2)], [cam], 32)
        shift = len(bad) if where == "in front" else 0
        assert (np.where(got[0] >= 0, got[0] - shift, -1) == plain[0]).all()
        _same_floats("zbuf", got[1], plain[1])
    culled = _check("culled", [(verts, faces)], [cam], 32, cull=True)
    assert (culled[0] == plain[0]).all()                                          # a closed surface: no back face ever won
    inside_out = _check("inside out, culled", [(verts, faces[:, ::-1])], [cam], 32, cull=True)
    assert (inside_out[0] >= 0).any() and not (inside_out[0] == plain[0]).all()   # now the far side is what is seen
    far_side = _check("inside out", [(verts, faces[:, ::-1])], [cam], 32)
    assert (far_side[0] == plain[0]).all()


def test_faces_cut_by_znear_or_zfar_are_absent_where_they_would_be_seen():
    """a face with one vertex in front of znear and a face with one vertex beyond zfar, each beside the face that renders
    and hidden by nothing: with the bound moved out of the way the face wins pixels, with the bound in place it wins none"""
    S = 32
    verts = np.asarray([(-0.9, -0.8, 1), (-0.1, -0.7, 1.5), (-0.5, 0.8, 2),        # face 0 renders
                        (0.1, -0.8, 0.05), (0.9, -0.8, 1), (0.5, -0.1, 1),         # face 1: a vertex at z = 0.05 < znear = 0.1
                        (0.1, 0.1, 11), (0.9, 0.1, 2), (0.5, 0.8, 2)], np.float32)  # face 2: a vertex at z = 11 > zfar = 10
    faces = np.arange(9, dtype=np.int64).reshape(3, 3)
    seen = {}
    for zn, zf in ((0.01, 100.0), (0.1, 100.0), (0.01, 10.0), (0.1, 10.0)):
        p, _, _, _ = _check("znear %g zfar %g" % (zn, zf), [(verts, faces)], [mr.identity_camera(zn, zf)], S)
        seen[zn, zf] = {f: int((p == f).sum()) for f in range(3)}
        assert seen[zn, zf][0] > 20
    assert seen[0.01, 100.0][1] > 20 and seen[0.01, 100.0][2] > 20      # both would be seen
    assert seen[0.1, 100.0][1] == 0 and seen[0.1, 100.0][2] > 20        # znear alone takes face 1
    assert seen[0.01, 10.0][1] > 20 and seen[0.01, 10.0][2] == 0        # zfar alone takes face 2
    assert seen[0.1, 10.0][1] == 0 and seen[0.1, 10.0][2] == 0


def test_empty_meshes_give_empty_images():
    verts, faces = _ico(1)
    cam = [mr.look_at_camera(**LOOK)]
    zero = np.zeros(1, np.int64)
    for v, f in ((verts, faces), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))):
        p, z, b, sv = _raster(v, f, zero, zero, cam, 20, True)
        assert (p == -1).all() and (z == -1).all() and (b == 0).all()
    got = _check("second mesh empty", [(verts, faces), (verts, faces[:0])], cam * 2, 20, shared=False)
    assert (got[0][0] >= 0).any() and (got[0][1] == -1).all()


# ---- batching, repeatability

def test_shared_mesh_equals_single_camera_calls_and_packed_meshes_equal_separate_renders():
    cams = [mr.look_at_camera(**LOOK), mr.look_at_camera(2.5, -40.0, 120.0), mr.look_at_camera(1.8, 60.0, -75.0, fov=75.0)]
    mesh = _pack([_ico(2)])
    batch = _raster(*mesh, cams, 40, True)
    for n, cam in enumerate(cams):
        one = _raster(*mesh, [cam], 40, True)
        for k, name in enumerate(("pix_to_face", "zbuf", "bary", "screen_verts")):
            assert (batch[k][n].view(np.uint32 if k else np.int64) == one[k][0].view(np.uint32 if k else np.int64)).all(), (n, name)
    _compare("three cameras", batch, _reference(*mesh, cams, 40, True))
    meshes = [_ico(1), (_ico(2)[0] * np.float32(0.7), _ico(2)[1])]
    both = _check("two meshes", meshes, cams[:2], 40, shared=False)
    for n in range(2):
        one = _raster(*_pack([meshes[n]]), [cams[n]], 40, True)
        assert (both[0][n] == one[0][0]).all() and (_bits(both[1][n]) == _bits(one[1][0])).all()
        assert (_bits(both[2][n]) == _bits(one[2][0])).all()


def test_repeated_calls_and_a_small_call_after_a_large_one_on_the_same_workspace():
    cam = [mr.look_at_camera(**LOOK)]
    large, small = _pack([_ico(4)]), _pack([_ico(1)])
    first = _raster(*large, cam, 128, True)
    _compare("large", first, _ico_reference(4, 128))
    _compare("small after large", _raster(*small, cam, 32, True), _ico_reference(1, 32))
    again = _raster(*large, cam, 128, True)
    for a, b in zip(first, again):
        assert (a.view(np.uint32 if a.dtype == np.float32 else np.int64) == b.view(np.uint32 if b.dtype == np.float32 else np.int64)).all()


# ---- a vertex and a cloud point at the same position

def test_screen_verts_equal_the_per_point_setup_bitwise():
    from dss_amd import ops
    verts, faces = _ico(3)
    cams = [mr.look_at_camera(2.0, 17.0, 33.0, zfar=2.2), mr.look_at_camera(2.5, -40.0, 120.0, znear=2.0)]   # some points cut
    M, V, c, zn, zf = _cams(cams)
    N, P = len(cams), len(verts)
    first = np.arange(N, dtype=np.int64) * P
    num = np.full(N, P, np.int64)
    setup = ops.point_setup(_t(verts), _t(verts), _t(np.full(P, 0.01, np.float32)), _t(M), _t(V), _t(zn), _t(zf), _t(first),
                            _t(num), 64, 1.0, shared_cloud=True)
    _, _, _, sv = _raster(*_pack([(verts, faces)]), cams, 64, True)
    valid = setup["valid"].cpu().numpy().reshape(N, P)
    pts = setup["pts_screen"].cpu().numpy().reshape(N, P, 3)
    assert valid.any(axis=1).all() and (~valid).any(axis=1).all()
    assert (_bits(pts)[valid] == _bits(sv)[valid]).all()


# ---- colours

def _lights(L, point, specular):
    if L == 3:
        amb, kd, ks, direction = mr.tri_color_lights(specular)
    else:
        amb = np.asarray([0.5, 0.5, 0.5], np.float32)
        kd = np.asarray([(0.3, 0.3, 0.3)], np.float32)
        ks = np.asarray([(0.2, 0.2, 0.2) if specular else (0, 0, 0)], np.float32)
        direction = np.asarray([(0.3, 0.8, 0.52)], np.float32)
    return amb, kd, ks, (direction * np.float32(5)).astype(np.float32) if point else direction


@pytest.mark.parametrize("point", [True, False])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("specular", [True, False])
def test_flat_shading_against_float64(point, L, specular):
    from dss_amd import ops
    verts, faces = _ico(2)
    cams = [mr.look_at_camera(**LOOK), mr.look_at_camera(2.5, -40.0, 120.0)]
    M, V, c, zn, zf = _cams(cams)
    S, N = 40, len(cams)
    packed = _pack([(verts, faces)])
    tv, tf, t1, tn = (_t(a) for a in packed)
    p, z, b, _ = ops.rasterize_meshes(tv, tf, t1, tn, _t(M), _t(V), _t(zn), _t(zf), _t(c), S)
    amb, kd, ks, vec = _lights(L, point, specular)
    colours = np.random.default_rng(3).uniform(0.2, 1.0, (len(faces), 3)).astype(np.float32) if L == 3 and point else None
    rep = lambda a: _t(np.broadcast_to(a, (N,) + a.shape))
    shininess, bg = 12.0, (0.25, 0.5, 0.75)
    rgba = ops.shade_mesh_flat(p, b, tv, tf, t1, tn, _t(c), rep(amb), rep(kd), rep(ks), rep(vec), point, shininess, bg,
                               None if colours is None else _t(colours))
    torch.cuda.synchronize()
    assert rgba.dtype == torch.float32 and rgba.shape == (N, S, S, 4)
    rgba, p, b = rgba.cpu().numpy(), p.cpu().numpy(), b.cpu().numpy()
    mask = p >= 0
    assert mask.any() and (~mask).any()
    assert (rgba[..., 3] == mask.astype(np.float32)).all()
    assert (rgba[~mask][:, :3] == np.asarray(bg, np.float32)).all()
    for n in range(N):
        want = mr.flat_shade64(p[n], b[n], verts, faces, c[n], amb, kd, ks, vec, point, shininess, colours)
        got = rgba[n, ..., :3].astype(np.float64)
        err = np.abs(got - want)[mask[n]]
        print("camera %d: max abs error %.3g, max value %.3g" % (n, err.max(), want[mask[n]].max()))
        assert np.allclose(got[mask[n]], want[mask[n]], rtol=COLOUR_RTOL, atol=COLOUR_ATOL)
    if specular:
        assert (rgba[mask][:, :3].max(axis=-1) > 0).all()


# ---- the whole way

def test_render_mesh_targets():
    import dss_amd
    from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
    from dss_amd.texture import DirectionalLights, PointLights
    verts, faces = _ico(2)
    R, T = look_at_view_transform(2.0, [17.0, -30.0], [33.0, 140.0])
    cameras = FoVPerspectiveCameras(znear=0.1, zfar=10.0, fov=60.0, R=R, T=T, device=_dev())
    amb, kd, ks, direction = mr.tri_color_lights(True)
    lights = DirectionalLights(ambient_color=amb[None, None], diffuse_color=kd[None], specular_color=ks[None],
                               direction=direction[None])
    S = 48
    rgba, mask, depth, pix_to_face = dss_amd.render_mesh_targets((_t(verts), _t(faces)), cameras, lights, image_size=S)
    torch.cuda.synchronize()
    assert rgba.shape == (2, S, S, 4) and rgba.dtype == torch.float32 and mask.shape == (2, S, S) and mask.dtype == torch.bool
    assert depth.shape == (2, S, S) and depth.dtype == torch.float32 and pix_to_face.shape == (2, S, S)
    assert pix_to_face.dtype == torch.int64 and all(t.is_cuda for t in (rgba, mask, depth, pix_to_face))
    assert (mask == (pix_to_face >= 0)).all() and mask.any() and (~mask).any()
    assert (depth[~mask] == 10.0).all() and (depth[mask] > 0.9).all() and (depth[mask] < 2.1).all()
    assert (rgba[..., 3] == mask.float()).all() and (rgba[~mask][:, :3] == 1.0).all()
    # the same picture through the operator, from the cameras' own matrices, and the restatement of it
    from dss_amd import ops
    M = cameras.get_full_projection_transform().get_matrix().contiguous()
    V = cameras.get_world_to_view_transform().get_matrix().contiguous()
    centre = cameras.get_camera_center().contiguous()
    zero = torch.zeros(1, dtype=torch.int64, device=_dev())
    p2, z2, _, _ = ops.rasterize_meshes(_t(verts), _t(faces), zero, zero + len(faces), M, V, cameras.znear, cameras.zfar, centre, S)
    assert (p2 == pix_to_face).all() and (z2[mask] == depth[mask]).all()
    cams = [(M[n].cpu().numpy(), V[n].cpu().numpy(), centre[n].cpu().numpy(), np.float32(0.1), np.float32(10.0)) for n in range(2)]
    want = _reference(*_pack([(verts, faces)]), cams, S, True)
    assert (pix_to_face.cpu().numpy() == want[0]).all()
    other = dss_amd.render_mesh_targets((_t(verts), _t(faces)), cameras, PointLights(location=((0.0, 3.0, 3.0),)), image_size=S,
                                        background=(0, 0, 0), cull_backfaces=True)
    assert (other[3] == pix_to_face).all() and (other[0][~mask] == 0).all()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dss_amd.render_mesh_targets((torch.from_numpy(verts), torch.from_numpy(faces)), cameras, lights, image_size=S)


class _PackedMeshes:
    """stand-in for pytorch3d's Meshes: the four packed accessors `render_mesh_targets` reads"""

    def __init__(self, meshes):
        self._packed = [_t(a) for a in _pack(meshes)]

    def verts_packed(self):
        return self._packed[0]

    def faces_packed(self):
        return self._packed[1]

    def mesh_to_faces_packed_first_idx(self):
        return self._packed[2]

    def num_faces_per_mesh(self):
        return self._packed[3]


def test_render_mesh_targets_takes_an_object_of_one_or_of_n_meshes():
    import dss_amd
    from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
    from dss_amd.texture import PointLights
    R, T = look_at_view_transform(2.0, [17.0, -30.0], [33.0, 140.0])
    cameras = FoVPerspectiveCameras(znear=0.1, zfar=10.0, fov=60.0, R=R, T=T, device=_dev())
    lights = PointLights(location=((0.0, 3.0, 3.0),))
    small = (_ico(2)[0] * np.float32(0.6), _ico(2)[1])
    S = 40
    alone = [dss_amd.render_mesh_targets((_t(v), _t(f)), cameras, lights, image_size=S) for v, f in (_ico(1), small)]
    one = dss_amd.render_mesh_targets(_PackedMeshes([_ico(1)]), cameras, lights, image_size=S)      # one mesh, both cameras
    for a, b in zip(one, alone[0]):
        assert torch.equal(a, b)
    two = dss_amd.render_mesh_targets(_PackedMeshes([_ico(1), small]), cameras, lights, image_size=S)   # camera n sees mesh n
    for n in range(2):
        for a, b in zip(two, alone[n]):
            assert torch.equal(a[n], b[n])
    assert not torch.equal(two[1][0], two[1][1]) and two[3][1].max() >= len(_ico(1)[1])   # mesh 1's own local face ids
    with pytest.raises(ValueError, match="need 1 or 2 meshes"):
        dss_amd.render_mesh_targets(_PackedMeshes([_ico(1)] * 3), cameras, lights, image_size=S)
