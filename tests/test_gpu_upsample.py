"""GPU: sparsity upsampling (`cloud_ops.upsample`, dss_upsample_candidates / dss_upsample_insert) and `remove_outliers`
against the float64 yardstick of tests/upsample_reference.py (checked against the reference's own run by
test_upsample_cpu.py) and the fixture tests/golden/ref_upsample.npz.

Tolerances.  `father`: equal wherever the yardstick's two best candidates are at least 1e-5 apart (relative, on the
distance); the share below that is capped at 2 %.  sparsity_sq: 2e-6 relative -- the candidate (q + 2 p) / 3 carries ~1e-7
absolute per coordinate at unit scale against distances of ~0.1 (test_upsample_cpu.py evaluates the kernel's arithmetic in
numpy fp32 against the same bound).  Rows of the grown cloud: 1e-6 absolute.  Point sets of multi-round runs: a new point
is matched within 1e-5, at most 2 % unmatched.  Whatever is said to be bit-equal is compared with array_equal.
Observed on an MI355X: unmatched new points against the reference's run, either direction, 0 of 43 (257 -> 300), 0 of 300
(600 -> 900), 0 of 1000 (1000 -> 2000); points excluded as near-ties on the grown cloud 4 of 798; sparsity_sq relative error at
most 1.3e-6 (K = 4), 6.6e-7 at K = 16."""
import os

import numpy as np
import pytest
import torch

import upsample_reference as yard

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S_RTOL, ROW_ATOL, MARGIN, SET_TOL = 2e-6, 1e-6, 1e-5, 1e-5


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "ref_upsample.npz"))


def _i64(v):
    return torch.tensor(v, dtype=torch.int64, device=_dev())


def gpu_round(x, K, n_new):
    """one round of one cloud through the operators, as numpy"""
    from dss_amd import ops
    pts = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(_dev())
    P = pts.shape[0]
    first, num = _i64([0]), _i64([P])
    d2, idx = ops.knn_points(pts, first, num, K + 1)
    s, father, key = ops.upsample_candidates(pts, idx, first, num, K)
    sel = torch.sort(key).indices[P - n_new:]
    out, _ = ops.upsample_insert(pts, None, idx, father, sel, first, num, first, _i64([P + n_new]), _i64([n_new]), K)
    torch.cuda.synchronize()
    return dict(s=s.cpu().numpy(), father=father.cpu().numpy(), key=key.cpu().numpy(), sel=sel.cpu().numpy(),
                points=out.cpu().numpy(), nb=idx[:, 1:].cpu().numpy(), d2=d2.cpu().numpy())


def _upsample(x, target, K=16, num_points=None, attributes=None):
    from dss_amd import cloud_ops
    x = np.asarray(x, np.float32)
    pts = torch.from_numpy(x if x.ndim == 3 else x[None]).to(_dev())
    out = cloud_ops.upsample(pts, target, num_points=num_points, neighborhood_size=K, attributes=attributes)
    torch.cuda.synchronize()
    return out


def check_candidates(g, c, only=None):
    ok = np.ones(c["s"].shape[0], bool) if only is None else only
    assert np.array_equal(g["nb"], c["nb"]), "neighbour lists differ from the yardstick's"
    bad = int((g["father"][ok] != c["father"][ok]).sum())
    rel = float((np.abs(g["s"] - c["s"]) / c["s"]).max())
    print("father mismatches %d of %d, sparsity_sq max relative error %.3g" % (bad, int(ok.sum()), rel))
    assert bad == 0
    assert rel <= S_RTOL
    want = np.array([yard.pack_key(s, i) for i, s in enumerate(g["s"])], dtype=np.uint64).view(np.int64)
    assert np.array_equal(g["key"], want)


def test_one_round_on_a_fresh_cloud(fixture):
    x, K, n_new = fixture["s1_in"], 16, 25
    c = yard.one_round(x, n_new, K)
    assert float(c["father_margin"].min()) >= MARGIN and c["cut_margin"] >= MARGIN
    g = gpu_round(x, K, n_new)
    check_candidates(g, c)
    assert np.array_equal(g["sel"], c["sel"])
    assert g["points"].shape == (257 + n_new, 3)
    assert float(np.abs(g["points"] - c["points"]).max()) <= ROW_ATOL
    assert np.array_equal(g["points"][n_new:], x)
    out, num = _upsample(x, 257 + n_new)                      # the public entry runs the same round
    assert num.tolist() == [282] and np.array_equal(out[0].cpu().numpy(), g["points"])


@pytest.fixture(scope="module")
def grown(fixture):
    """the yardstick's state after three rounds of the seed-0 scene: it holds collinear thirds, exact ties in real arithmetic"""
    state, rounds = yard.upsample(fixture["s0_in"], 900, K=16, max_rounds=3)
    assert state.shape[0] == 798 and min(float(r["father_margin"].min()) for r in rounds[1:]) == 0.0
    return state.astype(np.float32)


def test_one_round_on_a_grown_cloud(grown):
    K, n_new = 16, grown.shape[0] // 10
    c = yard.one_round(grown, n_new, K)
    ok = c["father_margin"] >= MARGIN
    print("excluded as near-ties: %d of %d" % (int((~ok).sum()), ok.shape[0]))
    assert (~ok).mean() <= 0.02
    g = gpu_round(grown, K, n_new)
    check_candidates(g, c, only=ok)
    assert c["cut_margin"] >= MARGIN
    assert set(g["sel"][ok[g["sel"]]].tolist()) == set(c["sel"][ok[c["sel"]]].tolist())
    again = gpu_round(grown, K, n_new)
    for k in ("s", "father", "key", "sel", "points"):
        assert np.array_equal(g[k], again[k]), k


def test_exact_ties_follow_the_tie_rules():
    """6 x 6 planar lattice with spacing 3/8: (q + 2 p) / 3 and every squared distance are exact in fp32 and in float64, so
    the many ties are ties in both and the rules decide: smallest j for the father, smaller id for the selection"""
    K = 8
    i, j = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    lattice = np.stack([0.375 * i.ravel(), 0.375 * j.ravel(), np.zeros(36)], 1).astype(np.float32)
    c = yard.one_round(lattice, 3, K)
    assert (c["father_margin"] == 0.0).sum() >= 4 and c["cut_margin"] == 0.0          # ties everywhere they matter
    g = gpu_round(lattice, K, 3)
    assert np.array_equal(g["nb"], c["nb"])
    assert np.array_equal(g["father"], c["father"])
    assert np.array_equal(g["s"], c["s"].astype(np.float32)) and np.array_equal(g["s"].astype(np.float64), c["s"])
    assert np.array_equal(g["sel"], c["sel"])
    assert np.array_equal(g["points"], c["points"].astype(np.float32))
    padded = np.full((1, 40, 3), 7.0, np.float32)              # the lattice padded to a cloud of 40 columns
    padded[0, :36] = lattice
    out, num = _upsample(padded, 39, K=K, num_points=[36])
    assert num.tolist() == [39] and np.array_equal(out[0].cpu().numpy(), g["points"])


def test_ragged_batch_equals_every_cloud_alone(fixture):
    """257, 64 + 3 and 130 points: the 16-lane groups of a wavefront and the wavefronts themselves straddle the clouds"""
    clouds = [fixture["s1_in"], fixture["s0_in"][:67], fixture["s2_in"][:130]]
    targets = [300, 67, 143]
    padded = np.zeros((3, 257, 3), np.float32)
    for n, c in enumerate(clouds):
        padded[n, :c.shape[0]] = c
    out, num = _upsample(padded, targets, num_points=[c.shape[0] for c in clouds])
    assert num.tolist() == targets and tuple(out.shape) == (3, 300, 3)
    out = out.cpu().numpy()
    for n, (c, t) in enumerate(zip(clouds, targets)):
        if t > c.shape[0]:
            alone, _ = _upsample(c, t)
            assert np.array_equal(out[n, :t], alone[0].cpu().numpy()), "cloud %d" % n
        assert np.array_equal(out[n, t - c.shape[0]:t], c) and not out[n, t:].any()
    assert np.array_equal(out[1, :67], clouds[1])


@pytest.mark.parametrize("K", [4, 16, 17, 39])
def test_every_group_width(fixture, K):
    x = fixture["s1_in"]
    c = yard.one_round(x, 25, K)
    assert float(c["father_margin"].min()) >= MARGIN
    g = gpu_round(x, K, 25)
    check_candidates(g, c)
    assert np.array_equal(g["sel"], c["sel"]) and float(np.abs(g["points"] - c["points"]).max()) <= ROW_ATOL


@pytest.mark.parametrize("seed,P,target", [(1, 257, 300), (0, 600, 900), (2, 1000, 2000)])
def test_full_operation_against_the_reference_run(fixture, seed, P, target):
    x, ref = fixture["s%d_in" % seed], fixture["s%d_out" % seed]
    out, num = _upsample(x, target)
    out = out[0].cpu().numpy()
    n_new = target - P
    assert num.tolist() == [target] and out.shape == ref.shape
    assert np.array_equal(out[n_new:], x)
    a, b = yard.unmatched(ref[:n_new], out), yard.unmatched(out[:n_new], ref)
    print("seed %d: unmatched new points, reference in ours %d, ours in reference %d, of %d" % (seed, a, b, n_new))
    assert a <= 0.02 * n_new and b <= 0.02 * n_new


def test_attributes_ride_along(fixture):
    x = fixture["s1_in"]
    rng = np.random.default_rng(3)
    normals = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    colours = rng.uniform(0, 1, (257, 3)).astype(np.float32)
    dev = _dev()
    attrs = [torch.from_numpy(a[None]).to(dev) for a in (normals, colours, x)]   # the positions themselves as a third attribute
    out, num, grown = _upsample(x, 282, attributes=attrs)
    c = yard.one_round(x, 25, 16, attrs=np.concatenate([normals, colours], 1))
    assert num.tolist() == [282] and [tuple(a.shape) for a in grown] == [(1, 282, 3)] * 3
    got = torch.cat(grown[:2], -1)[0].cpu().numpy()
    assert float(np.abs(got[:25] - c["attrs"][:25]).max()) <= 1e-6          # (a_q + 2 a_p) / 3 of the two parents, float64
    assert np.array_equal(got[25:, :3], normals) and np.array_equal(got[25:, 3:], colours)
    assert np.abs(np.linalg.norm(got[:25, :3], axis=1) - 1).max() > 1e-4    # the kernel does not renormalise
    plain, _ = _upsample(x, 282)
    assert np.array_equal(out.cpu().numpy(), plain.cpu().numpy())           # attributes do not change the points
    # several rounds: an attribute that IS the position goes through the same arithmetic as the position
    out, num, grown = _upsample(x, 300, attributes=attrs)
    assert np.array_equal(grown[2].cpu().numpy(), out.cpu().numpy())
    assert np.array_equal(grown[0][0, 43:].cpu().numpy(), normals)


def test_upsample_clouds_interpolates_and_renormalises(fixture):
    from dss_amd import cloud_ops
    from dss_amd.cloud import PointClouds3D
    x = fixture["s1_in"]
    dev = _dev()
    normals = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    feats = np.random.default_rng(4).uniform(0, 1, (257, 4)).astype(np.float32)
    cloud = PointClouds3D([torch.from_numpy(x).to(dev)], [torch.from_numpy(normals).to(dev)], [torch.from_numpy(feats).to(dev)])
    big = cloud_ops.upsample_clouds(cloud, 282)
    c = yard.one_round(x, 25, 16, attrs=np.concatenate([normals, feats], 1))
    assert big.num_points_per_cloud().tolist() == [282]
    assert float(np.abs(big.points_packed().cpu().numpy() - c["points"]).max()) <= ROW_ATOL
    n64 = c["attrs"][:, :3] / np.linalg.norm(c["attrs"][:, :3], axis=1, keepdims=True)
    assert float(np.abs(big.normals_packed().cpu().numpy() - n64).max()) <= 1e-6
    assert float(np.abs(big.features_packed().cpu().numpy() - c["attrs"][:, 3:]).max()) <= 1e-6


def test_refusals_on_the_device(fixture):
    from dss_amd import _lib, cloud_ops, ops
    dev = _dev()
    pts = torch.from_numpy(fixture["s1_in"]).to(dev)
    with pytest.raises(ValueError):
        cloud_ops.upsample(pts[None], 256)
    with pytest.raises(ValueError):
        cloud_ops.upsample(pts[None, :9], 10, neighborhood_size=4)
    first, num = _i64([0]), _i64([257])
    for K in (0, 40):   # the C ABI refuses what it can see: K, through RuntimeError with the entry's message
        with pytest.raises(RuntimeError, match="dss_upsample_candidates"):
            ops.upsample_candidates(pts, torch.zeros((257, K + 1), dtype=torch.int64, device=dev), first, num, K)
    lib = _lib.load()
    assert lib.dss_upsample_insert(None, None, 0, None, None, None, None, None, None, None, None, 1, 16, 257, 256, 0, None, None,
                                   None) == -1   # DSS_ERR_INVALID_ARGUMENT: a grown cloud smaller than the old one


def test_no_host_read_the_call_runs_under_stream_capture(fixture):
    """every size of every round follows from host integers: the whole call, two rounds with their kNN builds, sorts and
    fill kernels, is captured into a graph on a side stream; the replay returns the eager result bit for bit"""
    x = fixture["s1_in"]
    eager, _ = _upsample(x, 300)
    pts = torch.from_numpy(x[None]).to(_dev())
    from dss_amd import cloud_ops
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cloud_ops.upsample(pts, 300)            # warm-up on the capturing stream: workspaces, caches
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, num = cloud_ops.upsample(pts, 300)
    graph.replay()
    torch.cuda.synchronize()
    assert num.tolist() == [300]
    assert np.array_equal(out.cpu().numpy(), eager.cpu().numpy())


@pytest.fixture(scope="module")
def trained():
    return np.load(os.path.join(GOLDEN, "trained_cloud_cfg3.npz"))


def test_large_cloud_smoke(trained):
    """99,790 points of a trained model (dense bulk, thin halo) -> + 10 % in one round"""
    from dss_amd import ops
    x, K = trained["points"], 16
    P, n_new = x.shape[0], x.shape[0] // 10
    out, num = _upsample(x, P + n_new)
    assert num.tolist() == [P + n_new] and tuple(out.shape) == (1, P + n_new, 3)
    out = out[0]
    assert torch.equal(out[n_new:].cpu(), torch.from_numpy(x)) and bool(torch.isfinite(out).all())
    pts = torch.from_numpy(x).to(_dev())
    first, num1 = _i64([0]), _i64([P])
    d2, idx = ops.knn_points(pts, first, num1, K + 1)
    _, _, key = ops.upsample_candidates(pts, idx, first, num1, K)
    sel = torch.sort(key).indices[P - n_new:]                 # the fathers, in emission order
    step = (out[:n_new] - pts[sel]).norm(dim=1)
    assert bool((step <= 2.0 * d2[sel, K].sqrt()).all())
    before = d2[sel, 1].double().sqrt().mean().item()
    d2_after, _ = ops.knn_points(out.contiguous(), first, _i64([P + n_new]), 2)
    after = d2_after[sel + n_new, 1].double().sqrt().mean().item()
    print("mean nearest-neighbour distance of the fathers: %.6g -> %.6g" % (before, after))
    assert after < before


def _ratio64(x, K):
    """float64 restatement: smallest eigenvalue of the covariance of the K nearest points (self included) over the trace"""
    nb = np.concatenate([np.arange(x.shape[0])[:, None], yard.knn_lists(x, K - 1)], 1)
    q = x.astype(np.float64)[nb]
    d = q - q.mean(1, keepdims=True)
    lam = np.linalg.eigvalsh(np.einsum("pka,pkb->pab", d, d) / K)
    return lam[:, 0] / lam.sum(1)


def test_remove_outliers(trained):
    from dss_amd import cloud_ops
    from dss_amd.cloud import PointClouds3D
    K, tol = 16, 0.05
    bulk = trained["points"][:4096]
    rng = np.random.default_rng(5)
    centre = np.array([bulk[:, 0].max() + 0.5, bulk[:, 1].mean(), bulk[:, 2].mean()])
    planted = (centre + 0.01 * rng.standard_normal((32, 3))).astype(np.float32)   # tight, isotropic, 0.5 away from the rest
    x = np.concatenate([bulk, planted], 0)
    nrm = np.concatenate([trained["normals"][:4096], np.zeros((32, 3), np.float32)], 0)
    ids = np.arange(x.shape[0], dtype=np.float32)[:, None]
    dev = _dev()
    cloud = PointClouds3D([torch.from_numpy(x).to(dev)], [torch.from_numpy(nrm).to(dev)], [torch.from_numpy(ids).to(dev)])
    kept = cloud_ops.remove_outliers(cloud, neighborhood_size=K, tolerance=tol)
    got = np.zeros(x.shape[0], bool)
    got[kept.features_packed()[:, 0].cpu().numpy().astype(np.int64)] = True
    ratio = _ratio64(x, K)
    want = ratio < tol
    clear = np.abs(ratio - tol) >= 1e-4 * tol
    print("kept %d of %d, near the tolerance %d, disagreements %d" % (got.sum(), got.shape[0], (~clear).sum(), (got != want)[clear].sum()))
    assert (~clear).mean() <= 0.01
    assert np.array_equal(got[clear], want[clear])
    assert not got[4096:].any() and 0 < got.sum() < 4096
    assert np.array_equal(kept.points_packed().cpu().numpy(), x[got]) and np.array_equal(kept.normals_packed().cpu().numpy(), nrm[got])
    small = PointClouds3D([torch.from_numpy(x[:16]).to(dev)])
    with pytest.raises(ValueError):
        cloud_ops.remove_outliers(small, neighborhood_size=16)
