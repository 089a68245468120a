"""CPU: the yardstick of the per-point setup forward (`tests/setup_reference.py`) is pinned before
`tests/test_gpu_setup_reference.py` measures the kernels with it.

* Self-check: the reference agrees with independent fp64 arithmetic -- the projection of `camera_reference.project`, Vr and
  det Mk from an explicit tangent basis, G^-1 from `torch.linalg.inv` -- to 1e-13 of every entry's scale, and with the
  closed forms of a zero normal, of culled and unowned rows and of the cutoff.
* The cases are what they say: the planted points sit where the header of the reference says, the exact boundaries are exact
  in fp32 too, and the reference lists at most 1 % of a case's owned pairs as within rounding of a threshold, no plant
  among them.
* The oracle (`oracle.point_setup`, the fp32 C mirror that the kernel follows operation by operation) keeps the bars on
  every case: the first time the mirror meets these branches.
* The bars are tied to what plain fp32 torch loses on the same formula: 4 x the figure, rounded up, and re-measured here.
* Discrimination: fourteen wrong formulas, each switched on in the reference in fp64, go through the GPU test's check with the
  GPU test's bars; each misses it at least tenfold on some case -- but for sqrt(det Vk) / h, which IS |det Mk| in exact
  arithmetic: fp64 tells it apart only where det Vk happens to round below zero, fp32 on every isotropic case.
"""
import math

import pytest
import torch

import setup_reference as sr

F64 = torch.float64
ROUND_OFF = 1e-13     # both sides fp64, two different orders of ~200 operations, relative to the entry's scale

_ids = [sr.case_id(k) for k in sr.CASES]


@pytest.fixture(scope="module", params=sr.CASES, ids=_ids)
def loaded(request):
    key = request.param
    return key, sr.case(*key), sr.reference(*key)


def test_reference_equals_independent_arithmetic(loaded):
    key, c, ref = loaded
    rows, _cam, _wi = sr.pairs_of(c)
    indep = sr.definition(c)
    use = (ref.valid & ~ref.near)[rows]
    assert bool(use.any())
    for name in sr.OUTPUTS:
        v, a, d = ref.vals[name][rows][use], ref.A[name][rows][use], indep[name][use]
        assert bool((a >= v.abs()).all()) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(v).all())
        worst = float(((v - d).abs()[a > 0] / a[a > 0]).max())
        assert worst <= ROUND_OFF and bool(((v - d).abs()[a == 0] <= 1e-300).all()), (name, worst)


def test_closed_forms(loaded):
    key, c, ref = loaded
    # culled pairs and rows that no cloud owns: the defaults, exactly, and without a scale; the cutoff is the constant
    off = ~ref.valid
    assert not bool(ref.valid[~ref.owned].any()) and bool((ref.cutoff == sr.CUTOFF).all())
    for name in sr.OUTPUTS:
        dflt = torch.tensor(sr.DEFAULTS[name], dtype=F64)
        assert bool((ref.vals[name][off] == dflt[None]).all()) and float(ref.A[name][off].abs().sum()) == 0
    if c.layout in ("ragged", "shared_partial"):
        assert int((~ref.owned).sum()) == {"ragged": 500 - 301, "shared_partial": 1500 - 623}[c.layout]
    # a zero normal (anisotropic: a zero Vr): the pure antialiasing circle; a zero normal of the frame: no weight
    p = c.plants["vr6_zero" if c.mode == "aniso" else "zero_normal"]
    zero = c.plants["zero_normal"]
    if bool(ref.valid[zero]):
        assert float(ref.vals["scaler"][zero]) == 0 and float(ref.A["scaler"][zero]) == 0
    else:
        assert c.backface       # (n_z = 0 is not < 0)
    if bool(ref.valid[p]):
        px = 2.0 / c.S
        a, b, cc = ref.vals["ellipse"][p].tolist()
        want = 1.0 / (sr.SIGMA * px * px)
        assert abs(a / want - 1) <= 1e-15 and abs(cc / want - 1) <= 1e-15 and b == 0
        r = px * math.sqrt(sr.CUTOFF * sr.SIGMA)
        assert all(abs(x / r - 1) <= 1e-15 for x in ref.vals["radii"][p].tolist())
        assert (float(ref.vals["scaler"][p]) > 0) == (c.mode == "aniso")


def test_the_cases_are_what_they_say(loaded):
    key, c, ref = loaded
    rows, cam, wi = sr.pairs_of(c)
    own = int(ref.owned.sum())
    assert own == int(c.num.sum()) and int(ref.near.sum()) <= 0.01 * own
    planted = torch.tensor(sorted(c.plants.values()))
    assert planted.unique().numel() == len(c.plants) and not bool(ref.near[planted].any())
    kept = ref.valid[ref.owned]
    assert bool(kept.any()) and bool((~kept).any())        # both sides of the culling
    assert float(c.h.min()) >= sr.H_MIN * (1 - 1e-6) or c.mode == "aniso"
    assert float(c.h.max()) <= sr.H_MAX * (1 + 1e-6)
    lens = c.normals.to(F64).norm(dim=1)
    assert float(lens[lens > 1e-6].min()) < 2e-3 and float(lens.max()) > 500
    f32 = sr.setup(c, dtype=torch.float32)
    world_row = lambda p: int(wi[rows == p])
    P = lambda name: c.plants[name]
    n = lambda name: c.normals[world_row(P(name))].to(F64)
    assert float(n("zero_normal").norm()) == 0
    assert 0.9e-13 < float(n("normal_1e-13").norm()) < 1.1e-13 and 0.9e-11 < float(n("normal_1e-11").norm()) < 1.1e-11
    star = c.cam_names.index("mirror") if "mirror" in c.cam_names else 0
    for name, bound in (("edge_on", 1e-6), ("edge_on_1e-4", 1.1e-4), ("big_h_edge_on", 1e-6)):
        ray = sr._ray(c.M[star], c.world[world_row(P(name))])
        sin = abs(float(n(name) @ ray)) / float(n(name).norm())
        assert sin <= bound and (name != "edge_on_1e-4" or sin >= 0.9e-4), (name, sin)
        assert bool(ref.valid[P(name)])
    ndc = ref.vals["screen"][P("off_screen")][:2].abs()
    assert bool(ref.valid[P("off_screen")]) and 4.0 <= float(ndc.min()) and float(ndc.max()) <= 6.0
    if c.mode != "aniso":
        h_of = {"h_cloud": lambda p: c.h[star], "h_point": lambda p: c.h[world_row(p)], "h_packed": lambda p: c.h[p]}[c.mode]
        assert float(h_of(P("big_h_edge_on"))) == float(torch.tensor(sr.H_MAX))
    else:
        w = world_row(P("vr6_zero"))
        assert float(c.vr6[w].abs().sum()) == 0 and float(c.fn[w].norm()) > 0.99
        q = c.vr6[world_row(P("vr6_rank_one"))].to(F64)
        m = torch.stack([q[[0, 1, 2]], q[[1, 3, 4]], q[[2, 4, 5]]])
        ev = torch.linalg.eigvalsh(m)
        assert float(ev[2]) > 0 and float(ev[:2].abs().max()) <= 1e-6 * float(ev[2])
        w = world_row(P("frame_normal_other_side"))
        view = c.V[star][:3, 2].to(F64)
        assert float(c.normals[w].to(F64) @ view) < 0 < float(c.fn[w].to(F64) @ view)
        assert bool(ref.valid[P("frame_normal_other_side")])        # the cloud normal decides, with and without culling
    if c.mode == "h_packed":
        # the values of one world point differ between its cameras
        by_cam = [c.h[lo:hi] for lo, hi in sr._ranges(c.first, c.num)]
        k = min(by_cam[0].numel(), by_cam[1].numel())
        assert k > 100 and float((by_cam[0][:k] != by_cam[1][:k]).float().mean()) > 0.9
    if "mirror" in c.cam_names:
        assert torch.equal(c.V[star], torch.eye(4)) and float(torch.linalg.det(c.M[star][:3, :3].to(F64))) < 0
        for name, z in (("z_at_near", sr.MIRROR_NEAR), ("z_at_far", sr.MIRROR_FAR)):
            assert bool(ref.valid[P(name)]) and float(ref.vals["screen"][P(name), 2]) == z
            assert float(f32.vals["screen"][P(name), 2]) == z and float(c.znear[star] if "near" in name else c.zfar[star]) == z
        assert float(n("nz_zero")[2]) == 0 and bool(ref.valid[P("nz_zero")]) == (not c.backface)
        x = c.world[world_row(P("edge_on_exact"))].to(F64)
        assert float(n("edge_on_exact") @ x) == 0 and bool(ref.valid[P("edge_on_exact")])
    if "ortho" in c.cam_names:
        assert c.M[c.cam_names.index("ortho")][:, 3].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_the_oracle_keeps_the_bars(loaded):
    key, c, ref = loaded
    got = sr.oracle_outputs(c, ref.valid)
    worst, wrong = sr.ratios(got, ref)
    print("oracle     %-40s max |err| / A: %s" % (sr.case_id(key), "  ".join(
        "%s %.1e (bar %.0e)" % (n, w, b) for n, w, b in zip(sr.OUTPUTS, worst, sr.BARS[key]))))
    assert not wrong, wrong
    assert sr.violation(got, ref, sr.BARS[key]) <= 1.0, (worst, sr.BARS[key])


def test_bars_are_the_fp32_figures(loaded):
    """A bar is 4 x what the formula loses in plain fp32 torch, rounded up to one significant digit (`print_bars`): re-measured
    here, figure <= bar <= 10 x figure with one fp32 rounding (2^-24) of slack on the figure, so that a stale or a padded bar
    fails.  (Not `==`, and the slack: the vectorised fp32 square root of torch's CPU kernels differs in the last bit between
    CPUs -- seen on two -- and one such bit in the radii or the scaler moves an entry's ratio by up to 2^-24 |entry| / scale,
    which is the size of these figures: the `ragged` scaler measures 3.5e-8 on one CPU and 1.9e-8 on the other.)"""
    key, c, ref = loaded
    figs, bars = sr.fp32_figures(key), sr.BARS[key]
    print("fp32 torch %-40s max |err| / A: %s" % (sr.case_id(key), "  ".join(
        "%s %.1e (bar %.0e)" % (n, f, b) for n, f, b in zip(sr.OUTPUTS, figs, bars))))
    for name, fig, bar in zip(sr.OUTPUTS, figs, bars):
        assert fig > 0 and fig - 2.0 ** -24 <= bar <= 10 * (fig + 2.0 ** -24), (name, fig, bar)
    assert set(sr.BARS) == set(sr.CASES)


# ---------------------------------------------------------------------------------------------------------------------
# discrimination.  The mutants run on the cases at S = 1024 of the two layouts that between them have every camera kind,
# every mode and every plant (an entry is a function of its own pair alone: more cases of the same kind add nothing).
# `shared_partial` is there for one mutant: sqrt(det Vk) / h IS |det Mk| in exact arithmetic, and in fp64 it differs from
# the reference only by its conditioning (edge-on it keeps half its digits, about a tenth of a bar) -- until det Vk rounds
# below zero, as it does on that layout's `edge_on` plant on the CPUs tried, and the root is NaN (printed, not asserted).  In
# fp32, the format a kernel would evaluate it in, it misses every isotropic case (test_the_sqrt_det_vk_mutant_in_fp32).
MUTANT_CASES = [k for k in sr.CASES if k[3] == 1024 and (k[0] in ("shared", "ragged") or (k[0] == "shared_partial" and k[1] == "h_point"))]


def test_no_mutation_is_the_reference():
    key = MUTANT_CASES[0]
    a, b = sr.setup(sr.case(*key)), sr.reference(*key)
    assert all(torch.equal(a.vals[n], b.vals[n]) for n in sr.OUTPUTS) and torch.equal(a.valid, b.valid)
    assert sr.violation(sr.as_got(a), b, sr.BARS[key]) == 0.0


@pytest.mark.parametrize("mut", sr.MUTANTS)
def test_the_check_kills_the_mutant(mut):
    """the mutant's output through `violation` (the GPU test's check) with the GPU test's bars"""
    assert {k[1] for k in MUTANT_CASES} == set(sr.MODES) and {k[2] for k in MUTANT_CASES} == {False, True}
    missed = {}
    for key in MUTANT_CASES:
        c = sr.case(*key)
        missed[sr.case_id(key)] = sr.violation(sr.as_got(sr.setup(c, mut=mut)), sr.reference(*key), sr.BARS[key])
    hits = {k: v for k, v in missed.items() if v > 1.0}
    print("mutant %-30s misses the check on %2d of %d cases, at the most %.3g-fold" % (mut, len(hits), len(missed), max(missed.values())))
    if mut == "scaler_sqrt_detVk_over_h":
        return          # (see MUTANT_CASES: in fp64 a matter of which way det Vk rounds; test_the_sqrt_det_vk_mutant_in_fp32 holds it)
    assert hits and max(hits.values()) >= 10.0, (mut, missed)


@pytest.mark.parametrize("key", [k for k in MUTANT_CASES if k[1] != "aniso"], ids=sr.case_id)
def test_the_sqrt_det_vk_mutant_in_fp32(key):
    got = sr.as_got(sr.setup(sr.case(*key), dtype=torch.float32, mut="scaler_sqrt_detVk_over_h"))
    assert sr.violation(got, sr.reference(*key), sr.BARS[key]) >= 10.0


def test_violation_counts_what_the_gpu_check_counts():
    key = ("ragged", "h_point", True, 64)
    c, ref = sr.case(*key), sr.reference(*key)
    bars = sr.BARS[key]
    good = sr.as_got(ref)
    assert sr.violation(good, ref, bars) == 0.0
    p = int(torch.nonzero(ref.valid & ~ref.near)[0])
    culled = int(torch.nonzero(ref.owned & ~ref.valid & ~ref.near)[0])

    def with_entry(name, row, col, value):
        g = {k: v.clone() for k, v in good.items()}
        g[name][row, col] = value
        return g
    at = lambda f: float(ref.vals["radii"][p, 0] + f * bars[2] * ref.A["radii"][p, 0])
    assert sr.violation(with_entry("radii", p, 0, at(0.5)), ref, bars) == pytest.approx(0.5, rel=1e-6)
    assert sr.violation(with_entry("radii", p, 0, at(2.0)), ref, bars) == pytest.approx(2.0, rel=1e-6)
    assert sr.violation(with_entry("radii", p, 0, math.nan), ref, bars) == math.inf
    assert sr.violation(with_entry("ellipse", culled, 0, 1.0 + 1e-7), ref, bars) == math.inf       # a default: exact
    assert sr.violation(with_entry("screen", culled, 2, 0.5), ref, bars) == math.inf
    flipped = dict(good, valid=good["valid"].clone())
    flipped["valid"][culled] = True
    assert sr.violation(flipped, ref, bars) == math.inf                                              # a decision
