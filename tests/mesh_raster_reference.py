"""The mesh rasteriser's rule (include/dss_hip.h, "Triangle meshes -> target images") restated in numpy, operation for
operation: in float32 it is what `dss_rasterize_meshes` must return to the bit; the same code in float64, evaluated on the
float32 screen vertices and pixel centres, shows how far rounding moves the answer; `flat_shade64` is the shader in float64.
Also the meshes the tests use (icosphere, lattice quads).  Checked on the CPU by test_mesh_raster_cpu.py."""
import numpy as np

f32 = np.float32
NO_FACE = np.iinfo(np.int64).max


# ---- meshes

def icosphere(level):
    """unit icosphere -> verts (V,3) float32, faces (F,3) int64, F = 20 * 4^level, outward winding"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float32), np.asarray(f, np.int64)


def lattice_quad(S=8, lo=1, hi=6, diagonal=0, reverse_second=False, welded=True, z=1.0):
    """A quad of two triangles whose corners sit on the pixel centres lo and hi of an S^2 image, in SCREEN coordinates
    (identity cameras make them world coordinates as well).  diagonal 0: split along (lo,lo)-(hi,hi), 1: the other one;
    reverse_second: the second face wound the other way; welded False: six vertices, the diagonal's two duplicated."""
    a, b = pix_to_ndc(lo, S), pix_to_ndc(hi, S)
    corners = np.asarray([(a, a, z), (b, a, z), (b, b, z), (a, b, z)], np.float32)
    tris = [(0, 1, 2), (0, 2, 3)] if diagonal == 0 else [(0, 1, 3), (1, 2, 3)]
    if reverse_second:
        tris[1] = tris[1][::-1]
    if welded:
        return corners, np.asarray(tris, np.int64)
    verts = np.concatenate([corners[list(tris[0])], corners[list(tris[1])]])
    return verts, np.arange(6, dtype=np.int64).reshape(2, 3)


# ---- cameras

def look_at_camera(dist=2.0, elev=17.0, azim=33.0, fov=60.0, znear=0.1, zfar=10.0):
    """-> M, V (4,4) float32 (full projection, world-to-view; row-vector convention), camera centre (3,), znear, zfar"""
    from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform
    R, T = look_at_view_transform(dist, elev, azim)
    cam = FoVPerspectiveCameras(znear=znear, zfar=zfar, fov=fov, R=R, T=T)
    M = cam.get_full_projection_transform().get_matrix()[0].numpy().astype(np.float32)
    V = cam.get_world_to_view_transform().get_matrix()[0].numpy().astype(np.float32)
    return M, V, cam.get_camera_center()[0].numpy().astype(np.float32), f32(znear), f32(zfar)


def identity_camera(znear=0.1, zfar=10.0):
    """screen = world: NDC x, y = world x, y and view z = world z"""
    return np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), np.zeros(3, np.float32), f32(znear), f32(zfar)


# ---- the rule

def pix_to_ndc(i, S):
    return f32(-1) + f32(2 * i + 1) / f32(S)


def screen_verts(verts, M, V):
    """(V,3) world -> (V,3) (ndc x, ndc y, view z), float32, in the per-point setup's order of operations"""
    p = np.asarray(verts, np.float32)
    ph0, ph1, ph2, ph3 = p[:, 0], p[:, 1], p[:, 2], f32(1)
    m, v = np.asarray(M, np.float32).reshape(16), np.asarray(V, np.float32).reshape(16)
    with np.errstate(all="ignore"):
        z = ph0 * v[2] + ph1 * v[6] + ph2 * v[10] + ph3 * v[14]
        clip = [ph0 * m[j] + ph1 * m[4 + j] + ph2 * m[8 + j] + ph3 * m[12 + j] for j in range(4)]
        out = np.stack([clip[0] / clip[3], clip[1] / clip[3], z], axis=1)
    assert out.dtype == np.float32
    return out


def ndc_index_range(x, r, S):
    """csrc/tile_rect.h, float32 -> (lo, hi) NDC pixel indices or None"""
    with np.errstate(all="ignore"):
        flo = ((x - r + f32(1)) * f32(S) - f32(1)) * f32(0.5)
        fhi = ((x + r + f32(1)) * f32(S) - f32(1)) * f32(0.5)
    lo, hi = 0, S - 1
    if flo == flo and fhi == fhi:
        if fhi < f32(-2) or flo > f32(S) + f32(1):
            return None
        a, b = max(flo, f32(-2)), min(fhi, f32(S) + f32(1))
        lo, hi = max(0, int(np.floor(a)) - 1), min(S - 1, int(np.ceil(b)) + 1)
    return (lo, hi) if lo <= hi else None


def edge(ax, ay, bx, by, px, py):
    """edge function of (a, b) at p; a, b scalars, p scalars or arrays, all of one dtype"""
    swap = bx < ax or (bx == ax and by < ay)
    ux, uy, vx, vy = (bx, by, ax, ay) if swap else (ax, ay, bx, by)
    e = (vx - ux) * (py - uy) - (vy - uy) * (px - ux)
    return -e if swap else e


def face_rect(s, S):
    """the pixel rectangle of a face with screen vertices s (3,3) float32 -> (c0, c1, r0, r1) image columns / rows or None"""
    with np.errstate(all="ignore"):
        xmin, xmax = min(min(s[0, 0], s[1, 0]), s[2, 0]), max(max(s[0, 0], s[1, 0]), s[2, 0])
        ymin, ymax = min(min(s[0, 1], s[1, 1]), s[2, 1]), max(max(s[0, 1], s[1, 1]), s[2, 1])
        xr = ndc_index_range((xmin + xmax) * f32(0.5), (xmax - xmin) * f32(0.5), S)
        yr = ndc_index_range((ymin + ymax) * f32(0.5), (ymax - ymin) * f32(0.5), S)
    if xr is None or yr is None:
        return None
    return S - 1 - xr[1], S - 1 - xr[0], S - 1 - yr[1], S - 1 - yr[0]


def present_faces(sv, faces, znear, zfar, cull=None):
    """-> the ids of the faces that are not absent, ascending.  cull = (world verts (V,3), camera centre (3,)) or None"""
    nV, keep = len(sv), []
    for f, ids in enumerate(np.asarray(faces, np.int64).reshape(-1, 3)):
        if (ids < 0).any() or (ids >= nV).any():
            continue
        s = sv[ids]
        if not np.isfinite(s).all() or (s[:, 2] < znear).any() or (s[:, 2] > zfar).any():
            continue
        with np.errstate(all="ignore"):
            if edge(s[0, 0], s[0, 1], s[1, 0], s[1, 1], s[2, 0], s[2, 1]) == 0:
                continue
            if cull is not None:
                w, e = np.asarray(cull[0], np.float32), np.asarray(cull[1], np.float32)
                a, b, c = w[ids[0]], w[ids[1]], w[ids[2]]
                u, v, g = b - a, c - a, e - a
                n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
                if not (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2] > 0:
                    continue
        keep.append(f)
    return keep


def rasterize(sv, faces, znear, zfar, S, dtype=np.float32, strict=False, cull=None, order=None):
    """One camera: sv (V,3) float32 screen vertices, faces (F,3) ids into sv -> pix_to_face (S,S) int64, zbuf (S,S),
    bary (S,S,3) in `dtype`.  strict: pytorch3d's rule (every w > 0) instead of the inclusive one -- the mutation the tests
    must catch.  order: the order in which the faces are visited (the result must not depend on it)."""
    sv = np.asarray(sv, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cen = np.asarray([pix_to_ndc(S - 1 - c, S) for c in range(S)], np.float32).astype(dtype)   # by image column / row
    best_z = np.full((S, S), np.inf, dtype)
    best_f = np.full((S, S), NO_FACE, np.int64)
    best_b = np.zeros((S, S, 3), dtype)
    keep = present_faces(sv, faces, znear, zfar, cull)
    if order is not None:
        present = set(keep)
        keep = [f for f in order if f in present]
    for f in keep:
        s32 = sv[faces[f]]
        rect = face_rect(s32, S)
        if rect is None:
            continue
        c0, c1, r0, r1 = rect
        s = s32.astype(dtype)
        (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = s
        px, py = cen[None, c0:c1 + 1], cen[r0:r1 + 1, None]
        with np.errstate(all="ignore"):
            area = edge(x0, y0, x1, y1, x2, y2)
            sg = dtype(1) if area > 0 else dtype(-1)
            w0 = sg * edge(x1, y1, x2, y2, px, py)
            w1 = sg * edge(x2, y2, x0, y0, px, py)
            w2 = sg * edge(x0, y0, x1, y1, px, py)
            bs = (w0 + w1) + w2
            cov = ((w0 > 0) & (w1 > 0) & (w2 > 0) if strict else (w0 >= 0) & (w1 >= 0) & (w2 >= 0)) & (bs > 0)
            if not cov.any():
                continue
            q0, q1, q2 = (w0 / bs) / z0, (w1 / bs) / z1, (w2 / bs) / z2
            t = (q0 + q1) + q2
            zb = dtype(1) / t
            bz, bf = best_z[r0:r1 + 1, c0:c1 + 1], best_f[r0:r1 + 1, c0:c1 + 1]
            win = cov & ((zb < bz) | ((zb == bz) & (f < bf)))
            bz[win], bf[win] = zb[win], f
            best_b[r0:r1 + 1, c0:c1 + 1][win] = np.stack([q0 * zb, q1 * zb, q2 * zb], axis=-1)[win]
        assert zb.dtype == dtype
    found = best_f != NO_FACE
    return np.where(found, best_f, -1), np.where(found, best_z, dtype(-1)), best_b


# ---- the flat shader, float64

def _unit(a):
    return a / np.maximum(np.sqrt((a * a).sum(-1, keepdims=True)), 1e-6)


def flat_shade64(pix_to_face, bary, verts, faces, cam, ambient, kd, ks, lvec, point_lights, shininess, colors=None):
    """One camera, float64: pix_to_face (S,S) ids into faces (F,3) (ids into verts), bary (S,S,3); ambient (3,), kd / ks /
    lvec (L,3) -> rgb (S,S,3) on the covered pixels (0 elsewhere) by dss_phong_forward's formula on the face normal"""
    d = lambda a: np.asarray(a, np.float64)
    verts, bary, cam, ambient, kd, ks, lvec = map(d, (verts, bary, cam, ambient, kd, ks, lvec))
    cov = pix_to_face >= 0
    tri = verts[np.asarray(faces, np.int64)[pix_to_face[cov]]]                 # (K,3,3)
    b = bary[cov]
    x = (b[:, 0:1] * tri[:, 0] + b[:, 1:2] * tri[:, 1]) + b[:, 2:3] * tri[:, 2]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nh = _unit(nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True)))
    v = _unit(cam[None] - x)
    dif, spec = np.zeros_like(x), np.zeros_like(x)
    for l in range(len(kd)):
        u = lvec[l][None] - x if point_lights else np.broadcast_to(lvec[l][None], x.shape)
        dh = _unit(u)
        ca = (nh * dh).sum(-1, keepdims=True)
        r = -dh + 2.0 * (ca * nh)
        a0 = (v * r).sum(-1, keepdims=True)
        alpha = np.where(ca > 0, np.maximum(a0, 0.0), 0.0)
        dif += kd[l][None] * np.maximum(ca, 0.0)
        spec += ks[l][None] * alpha ** float(shininess)
    col = np.ones_like(x) if colors is None else d(colors)[pix_to_face[cov]]
    out = np.zeros(pix_to_face.shape + (3,), np.float64)
    out[cov] = col * (ambient[None] + dif) + spec
    return out


def tri_color_lights(has_specular):
    """the colours of the reference's get_tri_color_lights_for_view (common.py:74-81) and three fixed directions"""
    ambient = np.asarray([0.2, 0.2, 0.2], np.float32)
    kd = np.asarray([(0.0, 0.0, 0.8), (0.0, 0.8, 0.0), (0.8, 0.0, 0.0)], np.float32)
    ks = np.zeros((3, 3), np.float32)
    if has_specular:
        ks, kd = (f32(0.15) * kd).astype(np.float32), (kd * f32(0.85)).astype(np.float32)
    el, az = np.radians([30.0, 30.0, 30.0]), np.radians([-60.0, 60.0, 180.0])
    direction = np.stack([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)], axis=-1).astype(np.float32)
    return ambient, kd, ks, direction
