"""GPU: the bilateral filter of the normals and the RIMLS projection (`cloud_ops.denoise_normals`,
`cloud_ops.project_to_latent_surface`, dss_denoise_normals / dss_rimls_step) against the float64 yardstick of
tests/smoothing_reference.py (checked against the reference's own filter run and against fp32 arithmetic by
test_smoothing_cpu.py) and the fixture tests/golden/ref_smoothing.npz.

Tolerances.  Normals and positions: 1e-6 absolute per component (the yardstick evaluated in fp32 differs from float64 by
1.0e-7 / 6.5e-8; the bound leaves room for another summation order and exp).  Decisions -- `converged`, the live mask after
every single step -- are compared exactly: the yardstick's convergence margin is at least 5e-4 on both scenes at the
defaults and its radius margin at least 1e-4 where a test passes `search_radius`, so no point is excluded.  Whatever is said
to be bit-equal is compared with array_equal.
Observed on an MI355X (largest errors; every test prints its own): filter against the yardstick 1.2e-7 (sphere; 1.1e-7 plane,
1.0e-7 paraboloid) and against the reference's run 1.2e-7; projection at the defaults 6.5e-8 (plane) and 5.5e-8
(paraboloid), the same over all single steps, no decision differs (convergence margins 5.8e-4 / 8.7e-4); max_est_iter = 1
5.9e-8 / 5.6e-8, no decision differs (margins 1.2e-4 / 1.9e-4); search_radius = 0.05: filter 1.2e-7, projection 6.4e-8;
the 701-point cloud of the ragged batch 4.6e-8; 20 points at K = 31: filter 8.7e-8, positions 4.9e-9."""
import os

import numpy as np
import pytest
import torch

import smoothing_reference as yard

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_smoothing.npz")
ATOL = 1e-6
EXPLICIT_RADIUS = 0.05   # test_smoothing_cpu.py: radius margin >= 1e-4 for both tools on the plane


def _dev():
    return torch.device("cuda:0")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def refs(z):
    """the yardstick's runs, computed once and left unchanged"""
    out = {}
    for name in yard.SCENES:
        x, n = z[name + "_points"], z[name + "_normals"]
        f = yard.denoise(x, n)
        nf = f["normals"].astype(np.float32)
        out[name] = dict(x=x, n=n, f=f, nf=nf, p=yard.project(x, nf), p_est1=yard.project(x, nf, max_est_iter=1))
    out["sphere"] = dict(x=z["sphere_points"], n=z["sphere_normals"], f=yard.denoise(z["sphere_points"], z["sphere_normals"]))
    r = out["plane"]
    r["f_radius"] = yard.denoise(r["x"], r["n"], search_radius=EXPLICIT_RADIUS)
    r["p_radius"] = yard.project(r["x"], r["nf"], search_radius=EXPLICIT_RADIUS)
    return out


def _filter(x, n, **kw):
    from dss_amd import cloud_ops
    out = cloud_ops.denoise_normals(_gpu(x)[None], _gpu(n)[None], **kw)
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


def _project(x, n, **kw):
    from dss_amd import cloud_ops
    pts, conv = cloud_ops.project_to_latent_surface(_gpu(x)[None], _gpu(n)[None], return_converged=True, **kw)
    torch.cuda.synchronize()
    assert conv.dtype == torch.bool
    return pts[0].cpu().numpy(), conv[0].cpu().numpy()


def _check_projection(what, got, conv, want):
    err = float(np.abs(got - want["points"]).max())
    flips = int((conv != want["converged"]).sum())
    print("%s: positions max abs error %.3g, converged %d of %d, decisions that differ %d, convergence margin %.3g"
          % (what, err, int(conv.sum()), conv.shape[0], flips, want["margin"]))
    assert err <= ATOL
    assert flips == 0


@pytest.mark.parametrize("name", ["plane", "paraboloid", "sphere"])
def test_filter_against_the_yardstick_and_the_golden(refs, z, name):
    r = refs[name]
    got = _filter(r["x"], r["n"])
    e_y, e_g = float(np.abs(got - r["f"]["normals"]).max()), float(np.abs(got - z[name + "_filtered"]).max())
    print("%s: filter max abs error, yardstick %.3g, reference's run %.3g" % (name, e_y, e_g))
    assert e_y <= ATOL
    assert e_g <= ATOL
    assert float(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max()) <= 1e-6
    assert np.array_equal(got, _filter(r["x"], r["n"]))   # a repeated call returns the same bits


@pytest.mark.parametrize("name", ["plane", "paraboloid"])
def test_projection_at_the_defaults(refs, name):
    r = refs[name]
    assert r["p"]["margin"] >= 5e-4
    got, conv = _project(r["x"], r["nf"])
    _check_projection(name, got, conv, r["p"])
    again, _ = _project(r["x"], r["nf"])
    assert np.array_equal(got, again)


@pytest.mark.parametrize("name", ["plane", "paraboloid"])
def test_projection_step_by_step_through_the_operators(refs, name):
    """the ops-level call: the live mask and the positions after every single step; the first step is max_proj_iters = 1"""
    from dss_amd import cloud_ops, ops
    r, K = refs[name], 31
    x, n = _gpu(r["x"]), _gpu(r["nf"])
    P = x.shape[0]
    first, num = cloud_ops._ranges([P], _dev())
    radius = torch.full((1,), float(r["p"]["radius"]), dtype=torch.float32, device=_dev())
    d, idx = ops.knn_points(x, first, num, K + 1)
    assert np.array_equal(idx[:, 1:].cpu().numpy(), r["p"]["nb"]), "neighbour lists differ from the yardstick's"
    assert np.array_equal(d[:, 1:].cpu().numpy(), r["p"]["d"]), "list distances differ from the yardstick's"
    state, live, worst = x, None, 0.0
    for t in range(10):
        new, live = ops.rimls_step(state, n, d, idx, first, num, radius, K, live, 5)
        assert new.data_ptr() != state.data_ptr() and live.dtype == torch.uint8
        state = new
        got_live = live.cpu().numpy().astype(bool)
        assert np.array_equal(got_live, r["p"]["alive"][t]), "live mask differs after step %d" % (t + 1)
        worst = max(worst, float(np.abs(state.cpu().numpy() - r["p"]["states"][t]).max()))
        if t == 0:
            one, conv = _project(r["x"], r["nf"], max_proj_iters=1)
            assert np.array_equal(one, state.cpu().numpy()) and np.array_equal(conv, ~got_live)
    print("%s: live after every step %s, positions max abs error over all steps %.3g"
          % (name, [int(a.sum()) for a in r["p"]["alive"]], worst))
    assert worst <= ATOL
    assert np.array_equal(x.cpu().numpy(), r["x"])   # the input state was not written
    # a state without live points: the step changes nothing
    none = torch.zeros(P, dtype=torch.uint8, device=_dev())
    same, still = ops.rimls_step(state, n, d, idx, first, num, radius, K, none, 5)
    assert torch.equal(same, state) and int(still.sum()) == 0


@pytest.mark.parametrize("name", ["plane", "paraboloid"])
def test_projection_with_a_single_pass(refs, name):
    r = refs[name]
    got, conv = _project(r["x"], r["nf"], max_est_iter=1)
    _check_projection(name + ", max_est_iter = 1", got, conv, r["p_est1"])


def test_explicit_search_radius(refs):
    r = refs["plane"]
    f, p = r["f_radius"], r["p_radius"]
    assert f["radius_margin"] >= 1e-4 and p["radius_margin"] >= 1e-4 and f["live"].mean() < 0.8 and p["live"].mean() < 0.8
    got = _filter(r["x"], r["n"], search_radius=EXPLICIT_RADIUS)
    err = float(np.abs(got - f["normals"]).max())
    print("filter, radius %.3g (%.0f %% of the entries live): max abs error %.3g" % (EXPLICIT_RADIUS, 100 * f["live"].mean(), err))
    assert err <= ATOL
    assert float(np.abs(got - r["f"]["normals"]).max()) > 1e-4   # the radius changed the result
    pts, conv = _project(r["x"], r["nf"], search_radius=EXPLICIT_RADIUS)
    _check_projection("projection, radius %.3g (%.0f %% live)" % (EXPLICIT_RADIUS, 100 * p["live"].mean()), pts, conv, p)


def test_ragged_batch_is_every_cloud_alone(refs):
    from dss_amd import cloud_ops
    a, b = refs["paraboloid"], refs["plane"]
    sizes, P = [1500, 701], 1500
    pts = torch.full((2, P, 3), 7.0, device=_dev())      # junk in the padding rows: it must not be read
    nrm = torch.full((2, P, 3), 7.0, device=_dev())
    pts[0], nrm[0] = _gpu(a["x"]), _gpu(a["nf"])
    pts[1, :701], nrm[1, :701] = _gpu(b["x"][:701]), _gpu(b["nf"][:701])
    pts0, nrm0 = pts.clone(), nrm.clone()
    for as_tensor in (False, True):
        num = torch.tensor(sizes, device=_dev()) if as_tensor else sizes
        f = cloud_ops.denoise_normals(pts, nrm, num)
        p, conv = cloud_ops.project_to_latent_surface(pts, nrm, num, return_converged=True)
        torch.cuda.synchronize()
        assert f.shape == (2, P, 3) and p.shape == (2, P, 3) and conv.shape == (2, P)
        for n, s in enumerate(sizes):
            f1 = cloud_ops.denoise_normals(pts[n:n + 1, :s].contiguous(), nrm[n:n + 1, :s].contiguous())
            p1, c1 = cloud_ops.project_to_latent_surface(pts[n:n + 1, :s].contiguous(), nrm[n:n + 1, :s].contiguous(),
                                                         return_converged=True)
            assert torch.equal(f[n, :s], f1[0]) and torch.equal(p[n, :s], p1[0]) and torch.equal(conv[n, :s], c1[0])
        assert int((f[1, 701:] != 0).sum()) == 0 and int((p[1, 701:] != 0).sum()) == 0 and not bool(conv[1, 701:].any())
        assert torch.equal(pts, pts0) and torch.equal(nrm, nrm0)   # the inputs are not modified
    # the second cloud against the yardstick on its own
    want = yard.project(b["x"][:701], b["nf"][:701])
    assert want["margin"] >= 5e-4
    _check_projection("cloud of 701 points in a ragged batch", p[1, :701].cpu().numpy(), conv[1, :701].cpu().numpy(), want)


def test_a_container_uses_its_own_normals(refs):
    from dss_amd import cloud_ops
    from dss_amd.cloud import PointClouds3D
    a, b = refs["plane"], refs["paraboloid"]
    cloud = PointClouds3D([_gpu(a["x"]), _gpu(b["x"][:701])], [_gpu(a["n"]), _gpu(b["n"][:701])])
    f = cloud_ops.denoise_normals(cloud)
    assert torch.equal(f[0], cloud_ops.denoise_normals(_gpu(a["x"])[None], _gpu(a["n"])[None])[0])
    p = cloud_ops.project_to_latent_surface(cloud, f, max_proj_iters=2)
    want = cloud_ops.project_to_latent_surface(_gpu(b["x"][:701])[None], f[1:2, :701].contiguous(), max_proj_iters=2)
    assert torch.equal(p[1, :701], want[0])


def test_short_lists_a_single_point_and_an_isolated_point(refs):
    from dss_amd import cloud_ops
    r = refs["plane"]
    # 20 points, K = 31: the lists are shorter than K
    x, n = r["x"][:20].copy(), r["nf"][:20].copy()
    x = (x * np.float32(0.2)).astype(np.float32)   # inside the radius of 0.2, so that the 19 real entries are live
    f = yard.denoise(x, n, K=31)
    p = yard.project(x, n, K=31)
    assert f["live"][:, :19].all() and not f["live"][:, 19:].any()
    got_f = _filter(x, n, neighborhood_size=31)
    got_p, conv = _project(x, n)
    print("20 points, K = 31: filter %.3g, positions %.3g, convergence margin %.3g"
          % (np.abs(got_f - f["normals"]).max(), np.abs(got_p - p["points"]).max(), p["margin"]))
    assert float(np.abs(got_f - f["normals"]).max()) <= ATOL
    assert float(np.abs(got_p - p["points"]).max()) <= ATOL
    assert p["margin"] >= 5e-4 and np.array_equal(conv, p["converged"])
    # one point
    one_x, one_n = np.array([[0.25, -0.5, 2.0]], np.float32), np.array([[0.0, 3.0, 4.0]], np.float32)
    assert np.array_equal(_filter(one_x, one_n), np.array([[0.0, 0.6, 0.8]], np.float32))
    got, conv = _project(one_x, one_n)
    assert np.array_equal(got, one_x) and conv.tolist() == [True]
    # one point moved 1.0 away from the rest
    x, n = r["x"].copy(), (r["n"] * np.float32(2.0)).astype(np.float32)
    x[7, 2] += np.float32(1.0)
    got_f = _filter(x, n)
    unit = torch.nn.functional.normalize(torch.from_numpy(n[7:8]).double(), dim=-1).numpy()[0]
    assert float(np.abs(got_f[7] - unit).max()) <= 1e-7
    want_f = yard.denoise(x, n)
    assert not want_f["live"][7].any() and float(np.abs(got_f - want_f["normals"]).max()) <= ATOL
    nf = want_f["normals"].astype(np.float32)
    got, conv = _project(x, nf)
    assert np.array_equal(got[7], x[7]) and bool(conv[7])
    want = yard.project(x, nf)
    assert want["margin"] >= 5e-4
    _check_projection("plane with one point 1.0 away", got, conv, want)


def test_both_tools_improve_the_plane(refs):
    r = refs["plane"]
    _, _, n_true = yard.scene("plane")
    f = _filter(r["x"], r["n"])
    before, after = yard.normal_error(r["n"], n_true), yard.normal_error(f, n_true)
    p, _ = _project(r["x"], f)
    d0, d1 = yard.surface_distance("plane", r["x"]), yard.surface_distance("plane", p)
    print("normal error %.4f -> %.4f (%.2f), rms distance %.4f -> %.4f (%.2f)" % (before, after, after / before, d0, d1, d1 / d0))
    assert after < 0.25 * before
    assert d1 < 0.5 * d0
