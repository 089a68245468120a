"""Dealing of the backward gather's groups in the two-launch form (render_backward_kernel<..., PREP>, raster_backward.hip):
full rounds are dealt, an incomplete last round behind them is claimed from global counters by the wavefronts that have
finished their dealt groups.  Which wavefront runs a task must not change the task: every dealing case gives the gradients
of the automatic grid BIT FOR BIT, where every wavefront has at most one group and nothing is claimed, and those of the
static three-launch form (DSS_OPT_BACKWARD_FUSED = 5).  DSS_OPT_BACKWARD_GRID caps the persistent grid so that a few
thousand points reach several rounds; the `visible` mask is an input of the backward and is trimmed to exact list lengths.
The counters are zeroed by fb_prep_kernel of the same call: a captured forward + backward must replay to the eager result."""
import numpy as np
import pytest
import torch

import scenes
from dss_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 5


def _scene(P, S, N):
    """the shapes of test_render_backward_with_fused_projection_equals_project_backward: the bunny cut to P points, N distinct
    clouds, one forward, grad_out = randn"""
    pts, nrm = scenes.load_cloud("bunny")
    pts = scenes.normalize_unit_sphere(pts)
    pts, nrm = pts[:P], nrm[:P]
    Pc = len(pts)
    h = scenes.global_h(pts)
    az = [30.0, 150.0, 260.0][:N]
    M = np.concatenate([scenes.camera_matrices(2.0, 20.0, a)[0] for a in az])
    V = np.concatenate([scenes.camera_matrices(2.0, 20.0, a)[1] for a in az])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    sc = dict(N=N, S=S, Pc=Pc, M=t(M), V=t(V))
    sc["world"] = t(np.tile(pts, (N, 1)) + np.repeat(np.arange(N, dtype=np.float32)[:, None] * 0.01, Pc, 0))
    sc["normals"] = t(np.tile(nrm, (N, 1)))
    sc["first"] = torch.arange(N, device=DEV, dtype=torch.int64) * Pc
    sc["num"] = torch.full((N,), Pc, dtype=torch.int64, device=DEV)
    sc["h"] = torch.full((N,), float(h), device=DEV)
    sc["znear"], sc["zfar"] = torch.full((N,), 0.1, device=DEV), torch.full((N,), 100.0, device=DEV)
    sc["feat"] = torch.rand((N * Pc, 3), generator=torch.Generator().manual_seed(7)).to(DEV)
    sc["f"] = ops.render_forward(sc["world"], sc["normals"], sc["h"], sc["M"], sc["V"], sc["znear"], sc["zfar"], sc["first"],
                                 sc["num"], sc["feat"], S, K, 1.0, 0.05, 1.0, False, False)
    sc["go"] = torch.randn((N, S, S, 4), generator=torch.Generator().manual_seed(8)).to(DEV)
    return sc


_SCENES = {}


def _get_scene(key):
    if key not in _SCENES:
        _SCENES[key] = _scene(*key)
    return _SCENES[key]


def _trim(visible, count):
    """the mask with only its first `count` set flags kept"""
    on = torch.nonzero(visible.view(-1) != 0).view(-1)
    assert len(on) >= count, (len(on), count)
    out = torch.zeros_like(visible)
    out.view(-1)[on[:count]] = 1
    return out


def _backward(sc, vis, project):
    f = sc["f"]
    a = (sc["go"], f["idx"], f["qvalue"], f["wsum"], f["scaler"], f["pts_screen"], f["radii"], vis, sc["first"], sc["num"], 4.0, 0.05)
    gf, gp = ops.render_backward(*a, project=(sc["world"], sc["M"]) if project else None)
    return gf.clone(), gp.clone()


def _dealing_cases(W, tpw):
    """(name, list length): n_groups = ceil(length / tpw) against W wavefronts"""
    return [("n_groups < W", (W - 1) * tpw), ("n_groups == W", W * tpw), ("n_groups == 2W", 2 * W * tpw),
            ("2W + 1", (2 * W + 1) * tpw), ("3W - 1", (3 * W - 1) * tpw),
            ("last group holds a single task", (2 * W + 3) * tpw + 1)]


@pytest.mark.parametrize("tpw", [1, 2, 4])
@pytest.mark.parametrize("P,S,N", [(4000, 128, 1), (3000, 96, 3)])
def test_every_dealing_case_equals_the_automatic_grid_bit_for_bit(P, S, N, tpw):
    sc = _get_scene((P, S, N))
    n_vis = int((sc["f"]["visible"] != 0).sum())
    # worker workgroups of the capped grid: three rounds of W = 4 x workers wavefronts must fit the visible list; more than
    # 128 wavefronts when the list allows it, so that several wavefronts share a claim counter
    workers = max(8, min(40, (n_vis // tpw) // 12))
    W = 4 * workers
    assert 3 * W * tpw <= n_vis, "scene too small for three rounds: %d visible, W = %d, tpw = %d" % (n_vis, W, tpw)
    try:
        _lib.set_option(_lib.OPT_BACKWARD_TPW, tpw)
        for name, count in _dealing_cases(W, tpw):
            vis = _trim(sc["f"]["visible"], count)
            for project in (False, True):
                _lib.set_option(_lib.OPT_BACKWARD_GRID, 0)
                want_f, want_p = _backward(sc, vis, project)
                assert float(want_p.abs().max()) > 0 and float(want_f.abs().max()) > 0
                _lib.set_option(_lib.OPT_BACKWARD_GRID, N + workers)
                got_f, got_p = _backward(sc, vis, project)
                assert torch.equal(got_f, want_f) and torch.equal(got_p, want_p), (name, project, "capped grid vs automatic")
                _lib.set_option(_lib.OPT_BACKWARD_FUSED, 5)   # the static three-launch form, same cap
                try:
                    st_f, st_p = _backward(sc, vis, project)
                finally:
                    _lib.set_option(_lib.OPT_BACKWARD_FUSED, 0)
                assert torch.equal(st_f, want_f) and torch.equal(st_p, want_p), (name, project, "three-launch form")
    finally:
        _lib.set_option(_lib.OPT_BACKWARD_GRID, 0)
        _lib.set_option(_lib.OPT_BACKWARD_TPW, 0)
        _lib.set_option(_lib.OPT_BACKWARD_FUSED, 0)


def test_grid_option_is_clamped_and_checked():
    lib = _lib.load()
    assert lib.dss_set_option(_lib.OPT_BACKWARD_GRID, -1) == -1 and b"DSS_OPT_BACKWARD_GRID" in lib.dss_last_error()
    assert lib.dss_get_option(_lib.OPT_BACKWARD_GRID) == 0
    sc = _get_scene((4000, 128, 1))
    vis = sc["f"]["visible"]
    want = _backward(sc, vis, False)
    try:
        for grid in (1, 1 << 30):   # below N + 8 and above the automatic grid: clamped, same results
            _lib.set_option(_lib.OPT_BACKWARD_GRID, grid)
            got = _backward(sc, vis, False)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), grid
    finally:
        _lib.set_option(_lib.OPT_BACKWARD_GRID, 0)


def test_captured_step_with_a_claimed_round_replays_to_the_eager_result():
    """FusedPlan forward + backward captured on a side stream with a capped grid and an incomplete last round: the claim
    counters are left used up by every launch and must be zeroed again by the replayed fb_prep_kernel."""
    sc = _get_scene((4000, 128, 1))
    S, Pc, tpw = sc["S"], sc["Pc"], 2
    n_groups = (int((sc["f"]["visible"] != 0).sum()) + tpw - 1) // tpw
    workers = next(w for w in range(40, 7, -1) if n_groups > 4 * w and n_groups % (4 * w) != 0)
    plan = ops.FusedPlan(torch.device(DEV), 1, Pc, Pc, S, K, 3, False, False, False, False, 1.0, 1.0, 0.05)

    def step():
        arena = plan.forward(sc["world"], sc["normals"], sc["h"], sc["M"], sc["V"], sc["znear"], sc["zfar"], sc["first"],
                             sc["num"], sc["feat"])
        gf, gw = plan.backward(arena, sc["go"], sc["first"], sc["num"], 4.0, 0.05, sc["world"], sc["M"])
        return plan.image(arena), gf, gw
    try:
        _lib.set_option(_lib.OPT_BACKWARD_TPW, tpw)
        want = [x.clone() for x in step()]   # automatic grid: nothing is claimed
        assert torch.equal(plan.view(plan.forward(sc["world"], sc["normals"], sc["h"], sc["M"], sc["V"], sc["znear"], sc["zfar"],
                                                  sc["first"], sc["num"], sc["feat"]), "visible"), sc["f"]["visible"])
        _lib.set_option(_lib.OPT_BACKWARD_GRID, 1 + workers)
        eager = [x.clone() for x in step()]
        for e, w in zip(eager, want):
            assert torch.equal(e, w)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = step()
        for rep in range(3):
            for x in out:
                x.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            for o, e in zip(out, eager):
                assert torch.equal(o, e), rep
    finally:
        _lib.set_option(_lib.OPT_BACKWARD_GRID, 0)
        _lib.set_option(_lib.OPT_BACKWARD_TPW, 0)
