"""CPU: the argument checks of dss_amd.ops, pinned without a device (libdss_hip.so loads without a GPU).

Every public operator refuses CPU tensors, naming the first argument it looks at; the operators that check shapes first
say so first; a non-tensor is a TypeError.  The table records what each operator does, exceptions included: `clip_grad_`
and the two band-partials operators have their own message, `_rasterize_fine` cannot get past its registry without a
device (its shape checks, `_check_raster_inputs`, are called directly), and `_splat_points_occ_backward` looks at the
devices before the shapes.  The `h` mode (per cloud / per world point / per packed point) is compared with literal
copies of the two expressions it replaced.
"""
import itertools

import pytest
import torch

from dss_amd import ops

N, P, S, K, C, KNN = 2, 6, 16, 3, 3, 4
f32, i32, i64, f64 = torch.float32, torch.int32, torch.int64, torch.float64


def z(*shape, dtype=f32):
    return torch.zeros(shape, dtype=dtype)


pts, nrm, ell, rad, cut, scaler, feats = z(P, 3), z(P, 3), z(P, 3), z(P, 2), z(P), z(P), z(P, C)
first, num = torch.tensor([0, 4]), torch.tensor([4, 2])
vis = torch.ones(P, dtype=torch.bool)
idx, q, occ, wsum, g_img = z(N, S, S, K, dtype=i32), z(N, S, S, K), z(N, S, S), z(N, S, S), z(N, S, S, C + 1)
M, V, zn, zf, h, rs = z(N, 4, 4), z(N, 4, 4), z(N), z(N), z(N), z(N)
kd_, ki_ = z(P, KNN), z(P, KNN, dtype=i64)
amb, lights, cam = z(N, 3), z(N, 1, 3), z(N, 3)
rgba, tgt, mask, band, sums = z(N, S, S, 4), z(N, S, S, 3), z(N, S, S), z(N, 8, S, 4), z(N + 1, 5, dtype=f64)
phong = (pts, nrm, z(P, 3), first, num, amb, lights, lights, lights, False, cam)
proj = (pts, M, V, first, num, z(P, 3), vis)

# operator, well-shaped CPU arguments, the argument it refuses first (None: see OWN_MESSAGE), index of that argument
TABLE = [
    ("splat_points", (pts, ell, cut, rad, first, num, 0.05, S, K), "points", None),
    ("_splat_points_naive", (pts, ell, cut, rad, first, num, 0.05, S, K), "points", None),
    ("_rasterize_coarse", (pts, rad, first, num, S, 16, 100), "points", None),
    ("_rasterize_fine", (pts, ell, cut, rad, z(8, dtype=torch.uint8), 0.05, S, 16, K), None, None),
    ("_splat_points_occ_backward", (pts, rad, occ, first, num, 5.0), "points", 0),
    ("_splat_points_occ_fast_cuda_backward", (pts, rad, rs, occ, num, first), "points", None),
    ("backward_radius", (rad, vis, first, num, 5.0), "radii", 0),
    ("occ_backward", (pts, rad, vis, rs, occ, first, num), "points", 0),
    ("_backward_zbuf", (idx, q, z(P, 3)), "idx", 0),
    ("clip_grad_", (z(P, 3), 0.05), None, None),
    ("splat_backward", (pts, rad, vis, idx, occ, q, first, num, 5.0), "points", 0),
    ("blend_forward", (idx, q, occ, scaler, feats), "idx", 0),
    ("blend_backward", (g_img, idx, q, scaler, P), "grad_out", 0),
    ("render_forward", (pts, nrm, h, M, V, zn, zf, first, num, feats, S, K, 1.0, 0.05), "world", 0),
    ("render_backward", (g_img, idx, q, wsum, scaler, pts, rad, vis, first, num, 5.0), "grad_out", 0),
    ("gather_rows", (z(N * S * 8), z(S, dtype=i32), N, S, 8), "src", 0),
    ("local_frames", (pts, ki_, first, num), "points", 0),
    ("point_setup", (pts, nrm, h, M, V, zn, zf, first, num, S, 1.0), "world", 0),
    ("project_backward", proj, "world", 0),
    ("camera_backward", proj, "world", 0),
    ("knn_kth_sqdist", (pts, first, num, KNN), "points", 0),
    ("knn_points", (pts, first, num, KNN), "points", 0),
    ("cloud_mean_clamp", (z(P), first, num, 1.0, 0.0, 1.0, 0.5, 2), "values", 0),
    ("renderable_mean_clamp", (z(P), pts, V, zn, zf, first, num, False, 1.0, 0.0, 1.0, 0.5, 2), "values", 0),
    ("knn_kth_sqdist_view", (pts, first, num, KNN, V, zn, zf, False), "points", 0),
    ("phong_forward", phong, "world", 0),
    ("phong_backward", (z(P, 3),) + phong, "world", 1),
    ("phong_backward_camera", (z(P, 3),) + phong, "world", 1),
    ("phong_backward_lights", (z(P, 3),) + phong, "world", 1),
    ("mollify_normals", (nrm, kd_, ki_, None, first, num), "normals", 0),
    ("projection_loss", (pts, nrm, kd_, ki_, vis, first, num, 0.5), "points", 0),
    ("repulsion_loss", (pts, nrm, ki_, first, num, 0.5, 1.0), "points", 0),
    ("image_loss_forward", (rgba, tgt, mask, 1.0, 1.0), "rgba", 0),
    ("image_loss_backward", (rgba, tgt, mask, 1.0, 1.0, sums), "rgba", 0),
    ("points_inmask", (pts, M, mask), "points", 0),
    ("image_loss_band_sums", (band, tgt, mask, (0, 8)), "rgba_band", 0),
    ("image_loss_from_sums", (sums, (S, S), 1.0, 1.0), "sums", 0),
    ("image_loss_band_backward", (band, tgt, mask, (0, 8), 1.0, 1.0, sums), "rgba_band", 0),
    ("image_loss_band_partials", (band, tgt, mask, (0, 8)), None, None),
    ("image_loss_band_backward_partials", (band, tgt, mask, (0, 8), 1.0, 1.0, z(N, 64, 5, dtype=f64)), None, None),
]
OWN_MESSAGE = {
    "_rasterize_fine": "bin_points must be the tensor dss_amd.ops._rasterize_coarse returned",
    "clip_grad_": "grad_pts must be a contiguous float32 GPU tensor",
    "image_loss_band_partials": "dss_amd: rgba_band must be a float32 GPU tensor (no CPU fallback)",
    "image_loss_band_backward_partials": "dss_amd: rgba_band must be a float32 GPU tensor (no CPU fallback)",
}
# public callables that are no operators over the C ABI's tensors (host arithmetic, the plan class, a torch-only helper)
NOT_OPERATORS = {"fuse_projection", "band_rows", "band_targets", "FusedPlan"}


def test_the_table_covers_every_public_operator():
    own = {n: f for n, f in vars(ops).items() if callable(f) and getattr(f, "__module__", None) == ops.__name__}
    # the reference's own bindings keep their leading underscore (``DSS._C._rasterize_fine``, ...)
    public = {n for n, f in own.items() if not n.startswith("_") or (f.__doc__ or "").startswith("``DSS._C.")}
    assert public - NOT_OPERATORS == {row[0] for row in TABLE}


@pytest.mark.parametrize("name,args,arg,_pos", TABLE, ids=[r[0] for r in TABLE])
def test_cpu_tensors_are_refused_by_name(name, args, arg, _pos):
    with pytest.raises(RuntimeError) as e:
        getattr(ops, name)(*args)
    msg = str(e.value)
    if arg is None:
        assert OWN_MESSAGE[name] in msg
    else:
        assert msg == "dss_amd: %s is on cpu; the HIP path needs GPU tensors (no CPU fallback)" % arg


@pytest.mark.parametrize("name,args,arg,pos", [r for r in TABLE if r[3] is not None], ids=[r[0] for r in TABLE if r[3] is not None])
def test_a_non_tensor_is_a_type_error(name, args, arg, pos):
    args = list(args)
    args[pos] = [0.0]
    with pytest.raises(TypeError, match="%s must be a torch.Tensor" % arg):
        getattr(ops, name)(*args)


def test_shape_checks_that_precede_the_device_checks():
    for fn in (ops.splat_points, ops._splat_points_naive):
        with pytest.raises(RuntimeError, match=r"points must have shape \(P, 3\), got \(6, 2\)"):
            fn(z(P, 2), ell, cut, rad, first, num, 0.05, S, K)
        with pytest.raises(RuntimeError, match=r"radii must have shape \(6, 2\), got \(6, 3\)"):
            fn(pts, ell, cut, z(P, 3), first, num, 0.05, S, K)
        with pytest.raises(RuntimeError, match=r"ellipse_params must have shape \(6, 3\), got \(5, 3\)"):
            fn(pts, z(5, 3), cut, rad, first, num, 0.05, S, K)
        with pytest.raises(RuntimeError, match=r"cutoff_thres must have shape \(6,\), got \(6, 1\)"):
            fn(pts, ell, z(P, 1), rad, first, num, 0.05, S, K)
        with pytest.raises(RuntimeError, match=r"cloud_to_packed_first_idx and num_points_per_cloud must both be \(N,\)"):
            fn(pts, ell, cut, rad, first, num[:1], 0.05, S, K)
    # _rasterize_fine runs the same checks after its registry lookup (which needs a device tensor)
    assert ops._check_raster_inputs(pts, ell, cut, rad, first, num) == P
    with pytest.raises(RuntimeError, match=r"radii must have shape \(6, 2\)"):
        ops._check_raster_inputs(pts, ell, cut, z(P, 3), first, num)
    # _splat_points_occ_backward looks at the devices first
    with pytest.raises(RuntimeError, match="points is on cpu"):
        ops._splat_points_occ_backward(z(P, 2), rad, occ, first, num, 5.0)


def test_non_bool_masks_are_true_where_nonzero():
    """`keep` / `visible` of any dtype mean what the reference's .bool() means; .to(uint8) made 0.5 and 256.0 false"""
    vals = [0.0, 0.5, 256.0, -1.0, -0.0, float("nan"), 1.0]
    assert ops._nonzero_u8(torch.tensor(vals)).tolist() == [int(b) for b in torch.tensor(vals).bool().tolist()] == [0, 1, 1, 1, 0, 1, 1]
    assert ops._nonzero_u8(torch.tensor([0, 256, 3], dtype=i32)).tolist() == [0, 1, 1]
    flags = torch.tensor([True, False, True])
    assert ops._nonzero_u8(flags).dtype == torch.uint8 and ops._nonzero_u8(flags).data_ptr() == flags.data_ptr()


def test_rasterize_fine_refuses_foreign_bin_points():
    for foreign in (z(8, dtype=torch.uint8), None, [1, 2]):
        with pytest.raises(RuntimeError, match="a clone / device copy is not accepted"):
            ops._rasterize_fine(pts, ell, cut, rad, foreign, 0.05, S, 16, K)


def test_band_parser_and_band_rows():
    assert ops._band(None, 32) == (0, 32, 1)
    assert ops._band((2, 10), 32) == (2, 10, 1)
    assert ops._band((0, 32, 2), 32) == (0, 32, 2)
    assert ops._band([3.0, 9.0, 4.0], None) == (3, 9, 4)
    assert [ops.band_rows(*b) for b in ((0, 32), (5, 5), (9, 3), (0, 32, 2), (8, 30, 2), (0, 20, 4))] == [32, 0, 0, 16, 14, 8]


def _parent_ops_mode(numel, N, Pw, P, shared):
    """literal copy of the expression render_forward and point_setup carried"""
    per_point = numel == Pw and not (numel == N and Pw == N)
    packed_h = (not per_point) and shared and N > 1 and numel == P
    if not per_point and not packed_h and numel != N:
        raise RuntimeError("h must have %d (per point), %d (per cloud) or, for a shared cloud, %d (per packed point) entries" % (Pw, N, P))
    return 1 if per_point else 2 if packed_h else 0


def _parent_lean_mode(numel, N, Pw, P, shared):
    """literal copy of the expression SurfaceSplatting._lean_plan carried; None = fall back to the general path"""
    per_point = 1 if (numel == Pw and not (numel == N and Pw == N)) else 0
    if not per_point and shared and N > 1 and numel == P:
        per_point = 2
    if not per_point and numel != N:
        return None
    return per_point


H_CASES = [(n, pw, sh, k) for (n, pw, sh) in ((1, 1, False), (1, 5, False), (3, 3, False), (3, 3, True), (3, 5, True), (3, 5, False))
           for k in ("1", "N", "Pw", "P", "P+1")]


@pytest.mark.parametrize("N_,Pw,shared,which", H_CASES, ids=["N%d-Pw%d-%s-h%s" % (c[0], c[1], "shared" if c[2] else "own", c[3]) for c in H_CASES])
def test_h_mode_is_the_parents_expression(N_, Pw, shared, which):
    P_ = N_ * Pw if shared else Pw
    numel = {"1": 1, "N": N_, "Pw": Pw, "P": P_, "P+1": P_ + 1}[which]
    hh = torch.zeros(numel)
    lean = _parent_lean_mode(numel, N_, Pw, P_, shared)
    try:
        want = _parent_ops_mode(numel, N_, Pw, P_, shared)
    except RuntimeError as e:
        assert lean is None                                   # where the operators raise, _lean_plan falls back
        with pytest.raises(RuntimeError) as got:
            ops._h_mode(hh, N_, Pw, P_, shared)
        assert str(got.value) == str(e)
        return
    assert lean == want
    assert ops._h_mode(hh, N_, Pw, P_, shared) == want
    if numel == N_ and Pw == N_:
        assert want == 0                                      # the tie: as many clouds as points reads h per cloud


def test_h_mode_table_has_the_tie_and_the_fallbacks():
    outcomes = set()
    for (n, pw, sh), k in itertools.product(((1, 1, False), (3, 3, False), (3, 3, True), (3, 5, True), (3, 5, False)), (0, 1, 2)):
        p = n * pw if sh else pw
        outcomes.update(_parent_lean_mode(m, n, pw, p, sh) for m in (1, n, pw, p, p + 1))
    assert outcomes == {None, 0, 1, 2}
    assert _parent_ops_mode(3, 3, 3, 3, False) == 0 and _parent_ops_mode(3, 3, 3, 9, True) == 0
