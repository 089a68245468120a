"""CPU: the yardstick of the projection backward (`tests/projection_reference.py`) is pinned before
`tests/test_gpu_projection_grad.py` measures the two kernels with it.

* Agreement: the fp64 closed form and torch.autograd of `camera_reference.project` agree to 1e-12 of every entry's sum of
  absolute products, on every case of the GPU test.
* The inputs can tell wrong formulas apart: perspective cameras that differ, no zero g_z, a real mixture of valid and
  culled pairs, norms on both sides of the clip, the planted gradients where they are said to be.
* The bars of the GPU test are tied to what plain fp32 torch loses on the same formula.
* Discrimination: eleven wrong versions of the closed form -- each a one-line mutation of a copy kept here -- go through
  the GPU test's per-entry check with the GPU test's bars, and each misses it at least tenfold on every case it can affect
  (and equals the closed form bit for bit on the cases it cannot).
"""
import math

import pytest
import torch

import camera_reference as cref
import projection_reference as pr

F64 = torch.float64
ROUND_OFF = 1e-12     # both sides fp64: an entry is a sum of <= 17 terms of ~30 operations, relative to its absolute products
# a mutant of a 262,145-point case is evaluated on the case's first points: an entry is a function of its own point alone
MUTANT_POINTS = 4099


@pytest.fixture(scope="module", params=pr.CASES, ids=["%s-%s" % (n, "clip" if c else "noclip") for n, c in pr.CASES])
def loaded(request):
    name, clipped = request.param
    return pr.case(name, clipped), pr.reference(name, clipped)


def _own(c):
    own = torch.zeros(c.grad.shape[0], dtype=torch.bool)
    own[pr.owned_rows(c.first, c.num)] = True
    return own


def test_closed_form_equals_autograd(loaded):
    c, ((gw, A), (fs, fA)) = loaded
    auto = pr.project_backward_autograd(c.world, c.M, c.V, c.first, c.num, c.grad, c.valid, c.shared, c.clip)
    assert (A >= gw.abs() * (1 - 1e-15)).all()
    worst, zeros_ok = pr.entry_ratio(auto, gw, A)
    assert zeros_ok and worst <= ROUND_OFF, worst
    # the feature sum against the obvious view(N, Pw, C).sum(0) where every camera owns every point
    N, Pw = len(c.num), c.world.shape[0]
    if c.shared and c.num.tolist() == [Pw] * N and c.first.tolist() == [n * Pw for n in range(N)]:
        worst, zeros_ok = pr.entry_ratio(c.feat.to(F64).view(N, Pw, 8).sum(0), fs, fA)
        assert zeros_ok and worst <= ROUND_OFF, worst
    if not c.shared:
        own = _own(c)
        assert torch.equal(fs[own], c.feat.to(F64)[own]) and float(fs[~own].abs().sum()) == 0


def test_entries_without_a_term_are_zeros(loaded):
    c, ((gw, A), (fs, fA)) = loaded
    has = torch.zeros(c.world.shape[0], dtype=torch.bool)
    owned = torch.zeros(c.world.shape[0], dtype=torch.bool)
    for lo, hi in cref._ranges(c.first, c.num):
        wr = slice(0, hi - lo) if c.shared else slice(lo, hi)
        has[wr] |= c.valid[lo:hi] & (c.grad[lo:hi].abs().sum(1) > 0)       # (the planted zero gradient is no term either)
        owned[wr] = True
    assert float(gw[~has].abs().sum()) == 0 and float(A[~has].abs().sum()) == 0 and bool((A[has] > 0).all())
    assert float(fs[~owned].abs().sum()) == 0 and float(fA[~owned].abs().sum()) == 0
    if c.name.startswith("all_culled"):
        assert not has.any()
    if c.name == "gap":
        assert int((~owned).sum()) == 300 - 128
    if c.name == "shared_partial":
        assert int(has[123:].sum()) > 0 and int((~has).sum()) > 0


def test_the_inputs_can_tell_the_formulas_apart(loaded):
    c, _ref = loaded
    N, own = len(c.num), _own(c)
    expected = "eight-lane" if (c.name.startswith("lanes") or c.name in ("shared_partial", "all_culled_shared")) else "one-thread"
    assert pr.kernel_of(c) == expected
    assert bool((c.M[:, :3, 3] != 0).all()), "perspective: M[:, i, 3] != 0 for i = 0, 1, 2"
    assert all(not torch.equal(c.M[a], c.M[b]) and not torch.equal(c.V[a], c.V[b]) for a in range(N) for b in range(a))
    assert not c.valid[~own].any()
    free = torch.ones(c.grad.shape[0], dtype=torch.bool)
    free[c.planted] = False
    assert bool((c.grad[free][:, 2] != 0).all()), "every g_z is non-zero"
    if c.name == "one" or c.name.startswith("all_culled"):
        assert int(c.valid.sum()) == (1 if c.name == "one" else 0) and c.planted.numel() == 0
        return
    frac = float(c.valid[own].float().mean())
    assert 0.2 <= frac <= 0.8, "valid is a real mixture"
    if c.clip > 0:
        norms = c.grad.to(F64).norm(dim=1)[c.valid]
        assert float((norms < c.clip).float().mean()) >= 0.25 and float((norms > c.clip).float().mean()) >= 0.25
        assert c.planted.numel() == len(pr.PLANTS) and bool(c.valid[c.planted].all())
        g = c.grad[c.planted]
        clip32 = torch.tensor(c.clip, dtype=torch.float32)
        assert float(clip32) == c.clip
        assert float(g[0].abs().sum()) == 0
        assert abs(float(g[1].to(F64).norm()) / 1e-25 - 1) < 1e-6 and float((g[1] * g[1]).sum()) == 0   # fp32 squares it to 0
        assert torch.equal((g[2] * g[2]).sum().sqrt(), clip32) and float(g[2].to(F64).norm()) == c.clip
        assert abs(float(g[3].to(F64).norm()) / c.clip - 1) <= 2.0 ** -23 and bool((g[3] != 0).all())
        assert abs(float(g[4].to(F64).norm()) / (1e6 * c.clip) - 1) < 1e-6
    else:
        assert c.planted.numel() == 0


def test_w_spans_two_decades():
    c = pr.case("lanes17_3001", False)
    w = []
    for n, (lo, hi) in enumerate(cref._ranges(c.first, c.num)):
        xh = torch.cat([c.world, torch.ones(c.world.shape[0], 1)], 1).to(F64)
        w.append((xh @ c.M[n].to(F64))[:, 3][c.valid[lo:hi]])
    w = torch.cat(w)
    assert 0.3 <= float(w.min()) <= 0.35 and 29.0 <= float(w.max()) <= 31.0


def test_bars_follow_the_fp32_figures(loaded):
    """A bar is 4 x what the closed form loses in plain fp32 torch, rounded up to one significant digit: figure <= bar <=
    10 x figure, so that a stale or a padded bar fails (a figure of 0 -- nothing is added -- has the bar 0)."""
    c, _ref = loaded
    clipped = c.clip > 0
    figs, bars = pr.fp32_figures(c.name, clipped), pr.BARS[(c.name, clipped)]
    each = "  ".join("%s %.1e (bar %.0e)" % (n, f, b) for n, f, b in zip(pr.OUTPUTS, figs, bars))
    print("fp32 torch %-20s %-6s max |err| / A: %s" % (c.name, "clip" if clipped else "noclip", each))
    for out_name, fig, bar in zip(pr.OUTPUTS, figs, bars):
        assert fig <= bar <= 10 * fig, (out_name, fig, bar)


# ---------------------------------------------------------------------------------------------------------------------
# discrimination
MUTATIONS = ("ndc_term_dropped", "w_applied_once", "M_transposed", "V_column_1", "clip_after_projection", "clip_over_xy",
             "valid_ignored", "next_cameras_matrices", "first_eight_cameras", "first_idx_ignored", "features_masked_by_valid")


def _mutant_ranges(mut, c):
    if mut != "first_idx_ignored":
        return cref._ranges(c.first, c.num)
    # the pair index is n Pw + wi (shared) / the clouds follow each other without a gap (not shared)
    starts = [n * c.world.shape[0] for n in range(len(c.num))] if c.shared else (torch.cumsum(c.num, 0) - c.num).tolist()
    return [(s, s + k) for s, k in zip(starts, c.num.tolist())]


def _mutant(mut, c):
    """A COPY of `projection_reference.project_backward` and `feature_reduce` (values only, fp64) with one mutation switched
    on by name -> (grad_world (Pw,3), feature sum (Pw,8)); `mut=None` is the closed form itself (asserted below)."""
    world, M, V, g, f = (t.to(F64) for t in (c.world, c.M, c.V, c.grad, c.feat))
    N, Pw = len(c.num), world.shape[0]
    if mut == "clip_over_xy" and c.clip > 0:
        nrm = g[:, :2].norm(dim=1, keepdim=True)
        g = g / nrm.clamp_min(1e-12) * nrm.clamp_max(c.clip)
    elif mut != "clip_after_projection":
        g = cref.clip_screen_grad(g, c.clip)
    val, feat = torch.zeros(Pw, 3, dtype=F64), torch.zeros(Pw, 8, dtype=F64)
    for n, (lo, hi) in enumerate(_mutant_ranges(mut, c)):
        if hi == lo:
            continue
        wr = slice(0, hi - lo) if c.shared else slice(lo, hi)
        ok = c.valid[lo:hi]
        feat[wr] += f[lo:hi] * ok[:, None] if mut == "features_masked_by_valid" else f[lo:hi]
        if mut == "first_eight_cameras" and n >= 8:
            continue
        k = (n + 1) % N if mut == "next_cameras_matrices" else n
        m, v = (M[k].T if mut == "M_transposed" else M[k]), V[k]
        x, y, z = world[wr].unbind(1)
        col = lambda j: x * m[0, j] + y * m[1, j] + z * m[2, j] + m[3, j].expand_as(x)
        w = col(3)
        nx, ny = (col(0), col(1)) if mut == "w_applied_once" else (col(0) / w, col(1) / w)
        if mut == "ndc_term_dropped":
            nx, ny = nx * 0, ny * 0
        gx, gy, gz = g[lo:hi].unbind(1)
        zc = 1 if mut == "V_column_1" else 2
        t = torch.stack([((m[i, 0] - nx * m[i, 3]) * gx + (m[i, 1] - ny * m[i, 3]) * gy) / w + v[i, zc] * gz for i in range(3)], 1)
        if mut == "clip_after_projection":
            t = cref.clip_screen_grad(t, c.clip)
        if mut == "valid_ignored":
            ok = torch.ones_like(ok)
        val[wr] += torch.where(ok[:, None], t, torch.zeros_like(t))
    return val, feat


def _affects(mut, c):
    """-> (whether the mutation can change grad_world of the case, whether it can change its feature sum)"""
    own = _own(c)
    terms, culled, N = bool(c.valid.any()), bool((~c.valid[own]).any()), len(c.num)
    moved = any(k > 0 and a != b for (a, _), (b, _), k in zip(_mutant_ranges(mut, c), cref._ranges(c.first, c.num), c.num.tolist()))
    world = {"clip_after_projection": terms and c.clip > 0, "clip_over_xy": terms and c.clip > 0, "valid_ignored": culled,
             "next_cameras_matrices": terms and N >= 2, "first_eight_cameras": terms and N > 8, "first_idx_ignored": moved,
             "features_masked_by_valid": False}.get(mut, terms)
    feat = {"first_idx_ignored": moved, "features_masked_by_valid": culled}.get(mut, False)
    return world, feat


def _for_mutants(c, ref):
    if c.world.shape[0] <= MUTANT_POINTS:
        return c, ref
    (gw, A), (fs, fA) = ref
    return pr.truncated(c, MUTANT_POINTS), ((gw[:MUTANT_POINTS], A[:MUTANT_POINTS]), (fs[:MUTANT_POINTS], fA[:MUTANT_POINTS]))


def test_the_copy_is_the_closed_form(loaded):
    c, ref = _for_mutants(*loaded)
    (gw, _A), (fs, _fA) = ref
    val, feat = _mutant(None, c)
    assert torch.equal(val, gw) and torch.equal(feat, fs)


def test_the_per_entry_check_kills_every_mutant(loaded):
    """each mutant's output through `violation` (the GPU test's check) with the GPU test's bars: at least 10 on every output
    of every case the mutation can affect; the bits of the closed form where it cannot"""
    c, ref = _for_mutants(*loaded)
    bars = pr.BARS[(c.name, c.clip > 0)]
    for mut in MUTATIONS:
        got = _mutant(mut, c)
        for out_name, g, (r, a), bar, hit in zip(pr.OUTPUTS, got, ref, bars, _affects(mut, c)):
            if not hit:
                assert torch.equal(g, r), (mut, out_name)
                continue
            v = pr.violation(g, r, a, bar)
            print("mutant %-26s %-18s %-6s %-13s misses the check %.3g-fold"
                  % (mut, c.name, "clip" if c.clip > 0 else "noclip", out_name, v))
            assert v >= 10.0, (mut, c.name, out_name, v)


def test_every_mutant_is_killed_somewhere():
    """(the loop above is per case: this counts, per mutation, the small cases of the table that it can affect)"""
    small = [pr.case(name, True) for name in pr.LAYOUTS if not name.startswith("big")]
    for mut in MUTATIONS:
        hits = [c.name for c in small if any(_affects(mut, c))]
        assert len(hits) >= 2, (mut, hits)


def test_violation_counts_what_the_gpu_check_counts():
    ref, A = torch.tensor([[1.0, 0.0]], dtype=F64), torch.tensor([[2.0, 0.0]], dtype=F64)
    assert pr.violation(ref.clone(), ref, A, 1e-6) == 0.0 and pr.violation(ref.clone(), ref, A, 0) == 0.0
    assert pr.violation(ref + torch.tensor([[2e-6, 0.0]], dtype=F64), ref, A, 1e-6) == pytest.approx(1.0, rel=1e-9)
    assert pr.violation(ref + torch.tensor([[0.0, 1e-20]], dtype=F64), ref, A, 1e-6) == math.inf      # no term: exact zero
    assert pr.violation(ref + torch.tensor([[1e-9, 0.0]], dtype=F64), ref, A, 0) == math.inf          # a bar of 0: exact
    assert pr.violation(ref + torch.tensor([[1e-31, 0.0]], dtype=F64), ref, A, 0) == 0.0              # below UNDERFLOW
    assert pr.violation(torch.tensor([[math.nan, 0.0]], dtype=F64), ref, A, 1e-6) == math.inf
