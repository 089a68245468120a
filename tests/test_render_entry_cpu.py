"""The render entry (`SurfaceSplatting.forward` / `render_fused`, `SurfaceSplattingRenderer.forward`) on CPU tensors:
every `ops` function it reaches is replaced by a recording stand-in that returns tensors of the right shapes, so that
WHICH operators a call runs, in which order, with which tensor shapes and scalar arguments, is compared with literals
(`TRACES`, recorded once from the entry as it stood before its stages were separated).  CPU tensors are no
`FusedPlan.lean_input`, so `render_fused` takes the general node; the lean / graphed / sharded routes need a GPU
(tests/test_gpu_setup.py, test_gpu_camera_grad.py, test_gpu_sharded.py)."""
import types

import pytest
import torch

from dss_amd import neighbours, ops
from dss_amd.cameras import FoVPerspectiveCameras
from dss_amd.cloud import PointClouds3D
from dss_amd.rasterizer import PointFragments, PointsRasterizationSettings, SurfaceSplatting
from dss_amd.renderer import NormWeightedCompositor, SurfaceSplattingRenderer

N, S, K = 2, 16, 3


def _d(a):
    if torch.is_tensor(a):
        return "[%s]" % ",".join(str(int(s)) for s in a.shape)
    if isinstance(a, (tuple, list)):
        return "(%s)" % ", ".join(_d(x) for x in a)
    if isinstance(a, float) and a.is_integer():
        return repr(int(a))             # (10 and 10.0 are the same scalar argument to an operator)
    return repr(a)


class Recorder:
    def __init__(self):
        self.raw = []

    def note(self, name, args, kw):
        self.raw.append((name, args, kw))

    @property
    def lines(self):
        return ["%s(%s)" % (name, ", ".join([_d(a) for a in args] + ["%s=%s" % (k, _d(v)) for k, v in sorted(kw.items())]))
                for name, args, kw in self.raw]

    def of(self, name):
        return [(args, kw) for n, args, kw in self.raw if n == name]


def _z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def _render_forward(world, normals, h, M, V, znear, zfar, first, num, features, image_size, points_per_pixel, cutoff,
                    thr, sigma=1.0, backface=False, shared_cloud=False, **kw):
    n, pw, c, s, k = M.shape[0], world.shape[0], features.shape[1], int(image_size), int(points_per_pixel)
    p = n * pw if shared_cloud else pw
    image = torch.arange(c + 1, dtype=torch.float32).expand(n, s, s, c + 1).contiguous()   # (channel c holds the value c)
    return dict(image=image, idx=_z(n, s, s, k, dtype=torch.int32), zbuf=_z(n, s, s, k), qvalue=_z(n, s, s, k),
                occupancy=_z(n, s, s), wsum=_z(n, s, s), scaler=_z(p), pts_screen=_z(p, 3), radii=_z(p, 2),
                ellipse_params=_z(p, 3), cutoff_threshold=_z(p), visible=_z(p, dtype=torch.bool), valid=_z(p, dtype=torch.bool))


def _point_setup(world, normals, h, M, V, znear, zfar, first, num, image_size, cutoff, sigma=1.0, backface=False,
                 shared_cloud=False, **kw):
    p = M.shape[0] * world.shape[0] if shared_cloud else world.shape[0]
    return dict(pts_screen=_z(p, 3), ellipse_params=_z(p, 3), radii=_z(p, 2), scaler=_z(p), cutoff_threshold=_z(p),
                valid=_z(p, dtype=torch.bool))


def _splat_points(points, ellipse, cutoff, radii, first, num, thr, image_size, points_per_pixel, *a, **kw):
    n, s, k = first.shape[0], int(image_size), int(points_per_pixel)
    return (_z(n, s, s, k, dtype=torch.int32), _z(n, s, s, k), _z(n, s, s, k), _z(n, s, s),
            _z(points.shape[0], dtype=torch.uint8))


def _blend_forward(idx, qvalue, occupancy, scaler, features, return_wsum=False):
    return _z(*idx.shape[:3], features.shape[1] + 1), _z(*idx.shape[:3])


STAND_INS = {
    "knn_kth_sqdist_view": lambda pts, first, num, k, V, znear, zfar, shared, radius=None:
        _z(V.shape[0], pts.shape[0]) if shared else _z(pts.shape[0]),
    "renderable_mean_clamp": lambda d, pts, V, *a: _z(V.shape[0]),
    "cloud_mean_clamp": lambda d, first, num, *a: _z(first.shape[0]),
    "knn_points": lambda pts, first, num, k: (_z(pts.shape[0], k), _z(pts.shape[0], k, dtype=torch.int64)),
    "local_frames": lambda pts, idx, first, num: (_z(pts.shape[0], 6), _z(pts.shape[0], 3)),
    "render_forward": _render_forward,
    "render_backward": lambda g, idx, qv, wsum, scaler, pts, *a, **kw: (_z(pts.shape[0], g.shape[-1] - 1), _z(pts.shape[0], 3)),
    "point_setup": _point_setup,
    "splat_points": _splat_points,
    "splat_backward": lambda pts, *a, **kw: _z(pts.shape[0], 3),
    "project_backward": lambda world, *a, **kw: _z(world.shape[0], 3),
    "camera_backward": lambda world, M, V, *a, **kw: (_z(M.shape[0], 4, 4), _z(M.shape[0], 4, 4)),
    "blend_forward": _blend_forward,                   # (the renderer's unfused blend, not part of the rasterizer's entry)
    "blend_backward": lambda g, idx, qv, scaler, p, **kw: (_z(p, g.shape[-1] - 1), _z(*idx.shape[:3])),
}


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()

    def wrap(name, fn):
        def stand_in(*args, **kw):
            r.note(name, args, kw)
            return fn(*args, **kw)
        return stand_in
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, wrap(name, fn))
    monkeypatch.setattr(neighbours, "kth_sqdist", wrap("neighbours.kth_sqdist", lambda pts, *a, **kw: _z(pts.shape[0])))
    return r


# -- scenes -------------------------------------------------------------------------------------------------------------
def _cams(n=N):
    T = torch.tensor([[0.0, 0.0, 3.0]]).repeat(n, 1)
    return FoVPerspectiveCameras(znear=0.1, zfar=50.0, R=torch.eye(3)[None].repeat(n, 1, 1), T=T)


def _tensors(p, c=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(p, 3, generator=g) - 0.5).requires_grad_()
    nrm = torch.nn.functional.normalize(torch.rand(p, 3, generator=g) - 0.5, dim=1)
    return pts, nrm, torch.rand(p, c, generator=g).requires_grad_()


def _clouds(arrangement, c=3):
    if arrangement == "one":                       # one cloud shared by the cameras
        return PointClouds3D(*[[t] for t in _tensors(9, c)])
    if arrangement == "distinct":                  # 9 and 5 points
        a, b = _tensors(9, c), _tensors(5, c, seed=1)
        return PointClouds3D([a[0], b[0]], [a[1], b[1]], [a[2], b[2]])
    if arrangement == "copies":                    # two tensors, the same positions
        a = _tensors(9, c)
        return PointClouds3D([a[0], a[0].detach().clone().requires_grad_()], [a[1], a[1].clone()], [a[2], a[2].detach().clone().requires_grad_()])
    if arrangement == "extended":                  # extend(2): the same tensor objects twice
        return PointClouds3D(*[[t] for t in _tensors(9, c)]).extend(N)
    if arrangement == "small":                     # fewer than 7 points, shared
        return PointClouds3D(*[[t] for t in _tensors(5, c)])
    raise KeyError(arrangement)


def _settings(**kw):
    kw = dict(dict(backface_culling=False, image_size=S, points_per_pixel=K), **kw)
    return PointsRasterizationSettings(**kw)


def _run(rec, entry, arrangement, settings=None, rast_kw=None, **kwargs):
    """one forward + backward through `entry` -> the recorded lines"""
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=settings or _settings(), **(rast_kw or {}))
    pc = _clouds(arrangement)
    if entry == "render_fused":
        image, fragments, out = rast.render_fused(pc, **kwargs)
        assert tuple(image.shape) == (N, S, S, 4) and isinstance(fragments, PointFragments) and len(out) == N
        image.sum().backward()
    else:
        fragments, out = rast(pc, **kwargs)
        assert isinstance(fragments, PointFragments) and len(out) == N
        fragments.occupancy.sum().backward()
    return rec.lines


SCENARIOS = {
    # cloud arrangements (per-point variance, the settings' default) through both entries
    **{"%s-%s%s" % (e, a, "" if det else "-nodetect"): (e, a, {}, {} if det else {"detect_identical_clouds": False}, {})
       for e in ("render_fused", "forward") for a, det in (("one", True), ("distinct", True), ("copies", True), ("copies", False),
                                                         ("extended", True), ("small", True))},
    # variance modes
    "invariant-one": ("render_fused", "one", {"Vrk_invariant": True}, {}, {}),
    "invariant-distinct": ("render_fused", "distinct", {"Vrk_invariant": True}, {}, {}),
    "invariant-copies": ("render_fused", "copies", {"Vrk_invariant": True}, {}, {}),
    "frames-one": ("render_fused", "one", {"Vrk_invariant": False, "Vrk_isotropic": False}, {}, {}),
    "frames-distinct": ("forward", "distinct", {"Vrk_invariant": False, "Vrk_isotropic": False}, {}, {}),
    "h-given": ("render_fused", "one", {"Vrk_invariant": True}, {}, {"Vrk_h": torch.full((1,), 1e-3)}),
    "h-given-forward": ("forward", "distinct", {}, {}, {"Vrk_h": torch.full((14,), 1e-3)}),
    "radius-none": ("render_fused", "one", {}, {"frnn_radius": None}, {}),
    "radius-zero": ("forward", "one", {}, {"frnn_radius": 0}, {}),
    # the (radii_s, clip) pair as it reaches the backward operators
    "clip-none": ("render_fused", "one", {"clip_pts_grad": None, "radii_backward_scaler": 5}, {}, {}),
    "clip-0.05": ("render_fused", "one", {"clip_pts_grad": 0.05}, {}, {}),
    "clip-none-forward": ("forward", "one", {"clip_pts_grad": None, "radii_backward_scaler": 5}, {}, {}),
    "clip-0.05-forward": ("forward", "one", {"clip_pts_grad": 0.05}, {}, {}),
}

_VIEW = "knn_kth_sqdist_view(%s, 7, [2,4,4], [2], [2], %s, radius=%s)"
_RF = "render_forward(%s, [2,4,4], [2,4,4], [2], [2], [2], [2], %s, 16, 3, 1, 0.05, 1, False, %s, frame_normals=%s, order_refresh=0, vr6=%s)"
_RB = "render_backward([2,16,16,4], [2,16,16,3], [2,16,16,3], [2,16,16], %s, [2], [2], %s, %s, project=%s)"
_PS = "point_setup(%s, [2,4,4], [2,4,4], [2], [2], [2], [2], 16, 1, 1, False, %s, frame_normals=%s, vr6=%s)"
_SP = "splat_points(%s, [2], [2], 0.05, 16, 3, 0, None, return_visible=True)"
_SB = "splat_backward(%s, [2,16,16,3], [2,16,16], None, [2], [2], %s, %s)"
_PB = "project_backward(%s, [2,4,4], [2,4,4], [2], [2], %s, %s, %s)"


def _fused(view, world, h, p, shared, radii_s=10, clip=-1, pre=(), frames=False):
    """the lines of one render_fused forward + backward on the general route"""
    aniso = ("[%d,3]" % world, "[%d,6]" % world) if frames else ("None", "None")
    project = "None" if shared else "([%d,3], [2,4,4])" % world
    out = list(pre) + ([view] if view else [])
    out.append(_RF % ("[%d,3], [%d,3], [%d]" % (world, world, h), "[%d,3]" % p, shared, *aniso))
    out.append(_RB % ("[%d], [%d,3], [%d,2], [%d]" % (p, p, p, p), radii_s, clip, project))
    if shared:
        out.append(_PB % ("[%d,3]" % world, "[%d,3]" % p, "[%d]" % p, True))
    return out


def _masked(view, world, h, p, shared, radii_s=10, clip=-1, pre=(), frames=False):
    """the lines of one masked forward() + backward"""
    aniso = ("[%d,3]" % world, "[%d,6]" % world) if frames else ("None", "None")
    out = list(pre) + ([view] if view else [])
    out.append(_PS % ("[%d,3], [%d,3], [%d]" % (world, world, h), shared, *aniso))
    out.append(_SP % ("[%d,3], [%d,3], [%d], [%d,2]" % (p, p, p, p)))
    out.append(_SB % ("[%d,3], [%d,2], [%d]" % (p, p, p), radii_s, clip))
    out.append(_PB % ("[%d,3]" % world, "[%d,3]" % p, "[%d]" % p, shared))
    return out


_V_ONE = _VIEW % ("[9,3], [1], [1]", True, 0.2)
_V_TWO = _VIEW % ("[14,3], [2], [2]", False, 0.2)
_V_COPIES = _VIEW % ("[18,3], [2], [2]", False, 0.2)
_V_SMALL = _VIEW % ("[5,3], [1], [1]", True, 0.2)
_MEAN = "renderable_mean_clamp(%s, [2,4,4], [2], [2], [2], [2], %s, 0.5, 5e-05, 0.001, 0.0005, 7)"
_FRAMES = lambda p: ["knn_points([%d,3], [%s], [%s], 8)" % (p, 1 if p == 9 else 2, 1 if p == 9 else 2),
                     "local_frames([%d,3], [%d,8], [%s], [%s])" % (p, p, 1 if p == 9 else 2, 1 if p == 9 else 2)]

TRACES = {
    "render_fused-one": _fused(_V_ONE, 9, 18, 18, True),
    "render_fused-distinct": _fused(_V_TWO, 14, 14, 14, False),
    "render_fused-copies": _fused(_V_ONE, 18, 18, 18, False),          # searched as ONE cloud shared by the cameras
    "render_fused-copies-nodetect": _fused(_V_COPIES, 18, 18, 18, False),
    "render_fused-extended": _fused(_V_ONE, 9, 18, 18, True),          # the same tensor objects: shared geometry
    "render_fused-small": _fused(_V_SMALL, 5, 10, 10, True),
    "forward-one": _masked(_V_ONE, 9, 18, 18, True),
    "forward-distinct": _masked(_V_TWO, 14, 14, 14, False),
    "forward-copies": _masked(_V_ONE, 18, 18, 18, False),
    "forward-copies-nodetect": _masked(_V_COPIES, 18, 18, 18, False),
    "forward-extended": _masked(_V_ONE, 9, 18, 18, True),
    "forward-small": _masked(_V_SMALL, 5, 10, 10, True),
    "invariant-one": _fused(_V_ONE, 9, 2, 18, True, pre=(), frames=False)[:1] + [_MEAN % ("[2,9], [9,3]", True)]
                     + _fused(None, 9, 2, 18, True),
    "invariant-distinct": [_V_TWO, _MEAN % ("[14], [14,3]", False)] + _fused(None, 14, 2, 14, False),
    "invariant-copies": [_V_ONE, _MEAN % ("[2,9], [9,3]", True)] + _fused(None, 18, 2, 18, False),
    "frames-one": _fused(None, 9, 9, 18, True, pre=_FRAMES(9), frames=True),
    "frames-distinct": _masked(None, 14, 14, 14, False, pre=_FRAMES(14), frames=True),
    "h-given": _fused(None, 9, 2, 18, True),
    "h-given-forward": _masked(None, 14, 14, 14, False),
    "radius-none": _fused(_VIEW % ("[9,3], [1], [1]", True, -1), 9, 18, 18, True),
    "radius-zero": _masked(_VIEW % ("[9,3], [1], [1]", True, -1), 9, 18, 18, True),
    "clip-none": _fused(_V_ONE, 9, 18, 18, True, radii_s=5, clip=-1),
    "clip-0.05": _fused(_V_ONE, 9, 18, 18, True, radii_s=10, clip=0.05),
    "clip-none-forward": _masked(_V_ONE, 9, 18, 18, True, radii_s=5, clip=-1),
    "clip-0.05-forward": _masked(_V_ONE, 9, 18, 18, True, radii_s=10, clip=0.05),
}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_operator_trace(rec, name):
    entry, arrangement, settings, rast_kw, kwargs = SCENARIOS[name]
    assert _run(rec, entry, arrangement, _settings(**settings), rast_kw, **kwargs) == TRACES[name]


def test_every_scenario_has_its_literal():
    assert sorted(SCENARIOS) == sorted(TRACES)


# -- the variance scale ---------------------------------------------------------------------------------------------------
def test_small_clouds_take_the_fixed_h_in_both_layouts(rec):
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=_settings())
    rast.render_fused(_clouds("distinct"))                   # own clouds: 9 points searched, 5 points overridden
    h = rec.of("render_forward")[0][0][2]
    assert torch.equal(h, torch.cat([torch.full((9,), 5e-5), torch.full((5,), 0.5e-3)])) and rast._Vrk_h is h
    rast.render_fused(_clouds("small"))                      # a shared cloud: one value per (camera, point)
    assert torch.equal(rec.of("render_forward")[1][0][2], torch.full((10,), 0.5e-3))
    rast.render_fused(_clouds("one"))
    assert torch.equal(rec.of("render_forward")[2][0][2], torch.full((18,), 5e-5))   # (the stand-in's d = 0, clamped)


def test_refresh_false_searches_once(rec):
    # (per point the stored h is reused when it has one entry per point of the clouds handed over: own clouds)
    for st, arrangement in ((_settings(), "distinct"), (_settings(Vrk_invariant=True), "one")):
        rast, pc = SurfaceSplatting(cameras=_cams(), raster_settings=st), _clouds(arrangement)
        rast.render_fused(pc)
        first = len(rec.of("knn_kth_sqdist_view"))
        h = rast._Vrk_h
        rast.render_fused(pc, refresh=False)
        rast(pc, refresh=False)
        assert len(rec.of("knn_kth_sqdist_view")) == first and rast._Vrk_h is h
        rast.render_fused(pc)
        assert len(rec.of("knn_kth_sqdist_view")) == first + 1


def test_variance_scale_without_a_view_searches_the_whole_clouds(rec):
    pc = _clouds("distinct")
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=_settings())
    h = rast._variance_scale(pc, _settings())
    assert torch.equal(h, torch.cat([torch.full((9,), 5e-5), torch.full((5,), 0.5e-3)])) and rast._Vrk_h is h
    h = rast._variance_scale(pc, _settings(Vrk_invariant=True))
    assert tuple(h.shape) == (2,) and rast._Vrk_h is h
    assert rast._variance_scale(pc, _settings(Vrk_invariant=True), refresh=False) is h
    h = rast._variance_scale(pc, _settings(Vrk_invariant=False, Vrk_isotropic=False))
    assert torch.equal(h, torch.zeros(14)) and rast._Vrk_h is h
    SurfaceSplatting(cameras=_cams(), frnn_radius=None)._variance_scale(pc, _settings())
    assert rec.lines == ["neighbours.kth_sqdist([14,3], [2], [2], (9, 5), 7, radius=0.2)",
                         "neighbours.kth_sqdist([14,3], [2], [2], (9, 5), 7, radius=0.2)",
                         "cloud_mean_clamp([14], [2], [2], 0.5, 5e-05, 0.001, 0.0005, 7)",
                         "neighbours.kth_sqdist([14,3], [2], [2], (9, 5), 7, radius=-1)"]


# -- camera gradients -------------------------------------------------------------------------------------------------------
_CAM_REFUSAL = ("%s does not carry gradients to the cameras (a camera tensor requires grad): render without it, or detach "
                "the cameras")


def test_camera_gradients_take_the_general_node_and_the_other_routes_refuse(rec):
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=_settings())
    rast.render_fused(_clouds("distinct"))[0].sum().backward()
    assert not rec.of("camera_backward")
    cams = _cams()
    cams.T.requires_grad_()
    rast = SurfaceSplatting(cameras=cams, raster_settings=_settings())
    del rec.raw[:]
    rast.render_fused(_clouds("distinct"))[0].sum().backward()
    assert rec.lines[1:] == [      # (differentiable cameras: no fused projection, the screen-space gradient feeds both)
        _RF % ("[14,3], [14,3], [14]", "[14,3]", False, "None", "None"),
        _RB % ("[14], [14,3], [14,2], [14]", 10, -1, "None"),
        _PB % ("[14,3]", "[14,3]", "[14]", False),
        "camera_backward([14,3], [2,4,4], [2,4,4], [2], [2], [14,3], [14], False)"]
    assert cams.T.grad is not None and tuple(cams.T.grad.shape) == (2, 3)
    del rec.raw[:]
    rast(_clouds("distinct"))[0].occupancy.sum().backward()
    assert [ln.split("(")[0] for ln in rec.lines] == ["knn_kth_sqdist_view", "point_setup", "splat_points", "splat_backward",
                                                     "project_backward", "camera_backward"]
    with pytest.raises(NotImplementedError) as e:
        rast.render_fused(_clouds("distinct"), graphed=True)
    assert str(e.value) == _CAM_REFUSAL % "graphed=True"
    with pytest.raises(NotImplementedError) as e:
        rast.render_fused(_clouds("distinct"), row_partition=object())
    assert str(e.value) == _CAM_REFUSAL % "row_partition=..."


# -- the memo of _prepare -------------------------------------------------------------------------------------------------------
def test_prepare_memo(rec):
    cams, st, h = _cams(), _settings(Vrk_invariant=True), torch.full((1,), 1e-3)
    rast = SurfaceSplatting(cameras=cams, raster_settings=st)
    pts, nrm, col = _tensors(9)
    M = lambda: rec.of("render_forward")[-1][0][3]
    render = lambda: rast.render_fused(PointClouds3D([pts], [nrm], [col]), Vrk_h=h)   # (a fresh cloud object per call)
    render()
    assert rast._prepare_memo is not None
    m1, h1 = M(), rec.of("render_forward")[-1][0][2]
    _, _, out = render()
    assert M() is m1 and rec.of("render_forward")[-1][0][2] is h1 and len(out) == N    # a hit: the same tensors go in
    assert out.points_list()[0] is pts
    cams.T.add_(1)                                      # modified in place: the version misses
    render()
    m2 = M()
    assert m2 is not m1 and not torch.equal(m2, m1)
    cams.R = cams.R.clone()                             # re-assigned: the identity misses
    render()
    m3 = M()
    assert m3 is not m2 and torch.equal(m3, m2)
    render()
    assert M() is m3
    st.image_size = 8                                   # settings change in place: re-attached on a hit
    image, _, _ = render()
    assert M() is m3 and rec.of("render_forward")[-1][0][10] == 8 and tuple(image.shape) == (N, 8, 8, 4)
    assert not rec.of("knn_kth_sqdist_view")
    # two different tensors per cloud: the packed geometry is a copy, nothing is memoised
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=_settings(Vrk_invariant=True))
    pc = _clouds("distinct")
    rast.render_fused(pc, Vrk_h=torch.full((2,), 1e-3))
    rast.render_fused(pc, Vrk_h=torch.full((2,), 1e-3))
    assert getattr(rast, "_prepare_memo", None) is None
    # differentiable cameras are never memoised
    cams = _cams()
    cams.T.requires_grad_()
    rast = SurfaceSplatting(cameras=cams, raster_settings=_settings(Vrk_invariant=True))
    rast.render_fused(PointClouds3D([pts], [nrm], [col]), Vrk_h=h)
    assert getattr(rast, "_prepare_memo", None) is None


# -- empty clouds, errors, verbose ------------------------------------------------------------------------------------------------
def test_empty_cloud(rec):
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=_settings())
    pc = PointClouds3D([torch.zeros(0, 3)], [torch.zeros(0, 3)], [torch.zeros(0, 3)])
    image, frag, out = rast.render_fused(pc)
    frag2, out2 = rast(pc)
    assert out is pc and out2 is pc and not rec.raw
    assert tuple(image.shape) == (N, S, S, 4) and image.dtype == torch.float32 and not image.any()
    for f in (frag, frag2):
        assert isinstance(f, PointFragments)
        assert [(tuple(t.shape), t.dtype) for t in f] == [((N, S, S, K), torch.int32)] + [((N, S, S, K), torch.float32)] * 3 \
            + [((N, S, S), torch.float32)]
        assert (f.idx == -1).all() and (f.zbuf == -1).all() and (f.qvalue == -1).all() and not f.scaler.any() \
            and not f.occupancy.any()


def test_error_messages(rec):
    rast = SurfaceSplatting(raster_settings=_settings())
    for call in (rast.render_fused, rast, lambda pc: SurfaceSplatting(raster_settings=_settings(), compact_culled=True)(pc)):
        with pytest.raises(ValueError) as e:
            call(_clouds("one"))
        assert str(e.value) == "Cameras must be specified either at initialization or in the forward pass"
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=_settings())
    three = PointClouds3D(*[[t[i] for t in (_tensors(9), _tensors(9, seed=1), _tensors(9, seed=2))] for i in range(3)])
    for call in (rast.render_fused, rast):
        with pytest.raises(ValueError) as e:
            call(three)
        assert str(e.value) == "need 1 or 2 point clouds for 2 cameras, got 3"
    with pytest.raises(ValueError) as e:
        rast.render_fused(_clouds("one", c=9))
    assert str(e.value) == ("render_fused blends at most 8 feature channels, got 9 (use the unfused forward() + renderer for "
                            "wider features)")


def test_cameras_and_settings_given_per_call(rec):
    rast = SurfaceSplatting(raster_settings=_settings())
    cams = _cams()
    image, _, _ = rast.render_fused(_clouds("one"), cameras=cams, raster_settings=_settings(image_size=8, points_per_pixel=2))
    assert tuple(image.shape) == (N, 8, 8, 4) and rast.cameras is cams and rast.raster_settings.image_size == S
    frag, _ = rast(_clouds("one"), raster_settings=_settings(image_size=8, points_per_pixel=2))
    assert tuple(frag.idx.shape) == (N, 8, 8, 2)


def test_verbose_returns_the_per_point_info(rec):
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=_settings())
    frag, out, info = rast(_clouds("one"), verbose=True)
    assert sorted(info) == ["cutoff_threshold", "ellipse_params", "radii", "scaler"] and len(out) == N
    assert {k: tuple(v.shape) for k, v in info.items()} == {"radii": (18, 2), "ellipse_params": (18, 3),
                                                           "cutoff_threshold": (18,), "scaler": (18,)}
    assert frag.scaler_packed is info["scaler"] and rast._last_valid.dtype == torch.bool


# -- SurfaceSplattingRenderer.forward -------------------------------------------------------------------------------------------------
def _renderer(settings=None, rast_kw=None, compositor=None, **kw):
    rast = SurfaceSplatting(cameras=_cams(), raster_settings=settings or _settings(), **(rast_kw or {}))
    return SurfaceSplattingRenderer(rast, NormWeightedCompositor() if compositor is None else compositor, **kw)


def test_renderer_fused_call(rec):
    r = _renderer(fused=True)
    images = r(_clouds("one"))
    assert torch.is_tensor(images) and tuple(images.shape) == (N, S, S, 4)
    images, fragments = r(_clouds("one"), verbose=True)
    assert tuple(images.shape) == (N, S, S, 4) and isinstance(fragments, PointFragments)
    assert [ln.split("(")[0] for ln in rec.lines] == ["knn_kth_sqdist_view", "render_forward"] * 2
    # wider features: RGBA = the first three channels + the occupancy (the stand-in's channel c holds the value c)
    images = r(_clouds("one", c=5))
    assert tuple(images.shape) == (N, S, S, 4) and torch.equal(images[0, 0, 0], torch.tensor([0.0, 1.0, 2.0, 5.0]))
    assert rec.of("render_forward")[-1][0][9].shape[1] == 5
    # order_refresh of the renderer reaches the operator unless the call names its own
    r = _renderer(fused=True, order_refresh=4)
    r(_clouds("one"))
    r(_clouds("one"), order_refresh=2)
    assert [kw["order_refresh"] for _a, kw in rec.of("render_forward")[-2:]] == [4, 2]
    assert r(PointClouds3D([torch.zeros(0, 3)], [torch.zeros(0, 3)], [torch.zeros(0, 3)])) is None


@pytest.mark.parametrize("which", ["fused=False", "fused=None+verbose", "compact_culled", "points_per_pixel=33", "C=9"])
def test_renderer_unfused_branch(rec, which):
    r = _renderer(settings=_settings(points_per_pixel=33) if which == "points_per_pixel=33" else None,
                  rast_kw={"compact_culled": True} if which == "compact_culled" else None,
                  fused=False if which == "fused=False" else None if which == "fused=None+verbose" else True)
    out = r(_clouds("one", c=9 if which == "C=9" else 3), verbose=which == "fused=None+verbose")
    images = out[0] if which == "fused=None+verbose" else out
    assert tuple(images.shape) == (N, S, S, 4)
    names = [ln.split("(")[0] for ln in rec.lines]
    assert names == ["knn_kth_sqdist_view", "point_setup", "splat_points", "blend_forward"]
    if which == "fused=None+verbose":
        assert isinstance(out[1], PointFragments)
    if which == "compact_culled":      # two filtered clouds of their own, found to hold the same positions
        assert rec.lines[:2] == [_V_ONE, _PS % ("[18,3], [18,3], [18]", False, "None", "None")]


def test_row_partition_needs_the_fused_path(rec):
    part = types.SimpleNamespace(S=S, world_size=2, rank=0, cyclic=False)
    r = _renderer(compositor=torch.nn.Identity(), row_partition=part)
    with pytest.raises(RuntimeError) as e:
        r(_clouds("one"))
    assert str(e.value) == ("a row-partitioned render needs dss_amd's SurfaceSplatting, a NormWeightedCompositor and "
                            "the masked culling path (backface_culling off or compact_culled=False)")
    assert not rec.raw
