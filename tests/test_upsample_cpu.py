"""CPU: the float64 yardstick of sparsity upsampling (tests/upsample_reference.py) against the reference's own run
(tests/golden/ref_upsample.npz, made by tests/golden/make_golden_upsample.py), the refusals of `cloud_ops.upsample`, and
the packing of the sort key.

The reference runs in fp32 and its stand-in kNN orders near-equal distances its own way, so from the second round on -- when
the cloud holds collinear thirds (p, mid, q) that tie exactly in real arithmetic -- single decisions may differ and the
clouds are compared as point SETS: a new point is matched if the other cloud has a point within 1e-5, and at most 2 % of
the new points may be unmatched.  Observed: 0 of 43 (257 -> 300), 2 of 300 (600 -> 900), 3 of 1000 (1000 -> 2000), the same
in both directions.
"""
import os
import random

import numpy as np
import pytest
import torch

import upsample_reference as yard
from dss_amd import cloud_ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_upsample.npz")
SCENES = {1: (257, 300), 0: (600, 900), 2: (1000, 2000)}


@pytest.fixture(scope="module")
def runs():
    z = np.load(GOLDEN)
    out = {}
    for seed, (P, target) in SCENES.items():
        mine, rounds = yard.upsample(z["s%d_in" % seed], target, K=int(z["K"]))
        out[seed] = (z["s%d_in" % seed], z["s%d_out" % seed], mine, rounds)
    return out


def test_scene_generator_is_the_fixtures(runs):
    for seed, (P, _) in SCENES.items():
        assert np.array_equal(yard.sphere_scene(seed, P), runs[seed][0])


def test_fresh_scene_equals_the_reference_row_by_row(runs):
    x, ref, mine, rounds = runs[1]
    assert mine.shape == ref.shape == (300, 3) and [r["sel"].shape[0] for r in rounds] == [25, 18]
    err = float(np.abs(mine - ref).max())
    print("257 -> 300: max abs difference to the reference %.3g" % err)
    assert err <= 1e-6
    assert np.array_equal(mine[43:], x.astype(np.float64))   # the old points, in their order, behind the new ones


@pytest.mark.parametrize("seed", [0, 2])
def test_multi_round_scenes_match_the_reference_as_point_sets(runs, seed):
    x, ref, mine, rounds = runs[seed]
    P, target = SCENES[seed]
    n_new = target - P
    assert mine.shape == ref.shape and len(rounds) == {0: 5, 2: 8}[seed]
    assert np.array_equal(ref[n_new:], x) and np.array_equal(mine[n_new:], x.astype(np.float64))
    a, b = yard.unmatched(ref[:n_new], mine), yard.unmatched(mine[:n_new], ref)
    print("seed %d: unmatched new points, reference in yardstick %d, yardstick in reference %d, of %d" % (seed, a, b, n_new))
    assert a <= 0.02 * n_new and b <= 0.02 * n_new


def test_ties_are_not_rare_after_the_first_round(runs):
    """why the tie rules are part of the contract: the smallest margin between a point's two best candidates is exactly 0
    in the multi-round runs, while a fresh cloud has none below 1e-5"""
    for seed in (0, 2):
        assert min(float(r["father_margin"].min()) for r in runs[seed][3]) == 0.0
    assert float(runs[1][3][0]["father_margin"].min()) >= 1e-5


@pytest.mark.parametrize("K", [4, 16, 17, 39])
def test_fp32_restatement_is_within_the_bounds_asked_of_the_kernel(runs, K):
    """the kernel's arithmetic, every operation rounded to fp32 in numpy, against the yardstick: `father` equal and
    sparsity_sq within 2e-6 relative on the fresh scene -- the bounds of the GPU test follow from the number format"""
    x = runs[1][0]
    c = yard.candidates(x, K)
    s32, f32 = yard.round_fp32(x, K)
    assert float(c["father_margin"].min()) >= 1e-5
    assert np.array_equal(f32, c["father"])
    assert float((np.abs(s32 - c["s"]) / c["s"]).max()) <= 2e-6


def test_selection_order_and_tie_rules():
    s = np.array([0.5, 0.25, 0.5, 0.125, 0.5, 0.25])
    # largest s first, ties to the smaller id: 0, 2, 4, 1, 5; emitted in reverse
    assert yard.emission_order(s, 3).tolist() == [4, 2, 0]
    assert yard.emission_order(s, 4).tolist() == [1, 4, 2, 0]
    m = np.array([[1.0, 3.0, 3.0, 2.0]])
    assert int(m.argmax(-1)[0]) == 1   # the smallest j of a tied maximum


@pytest.mark.parametrize("sizes,targets,K,what", [
    ([257], [256], 16, "more than its target"),
    ([257, 300], [300, 299], 16, "more than its target"),
    ([9], [10], 4, "at least max"),
    ([16], [17], 16, "at least max"),
    ([257], [300], 0, "neighborhood_size"),
    ([257], [300], 40, "neighborhood_size"),
])
def test_refusals_come_before_the_library(sizes, targets, K, what, monkeypatch):
    from dss_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    pts = torch.zeros(len(sizes), max(sizes), 3)
    with pytest.raises(ValueError, match=what):
        cloud_ops.upsample(pts, targets, num_points=sizes, neighborhood_size=K)
    with pytest.raises(ValueError, match=what):
        cloud_ops.upsample(pts, torch.tensor(targets), num_points=torch.tensor(sizes), neighborhood_size=K)


def test_a_cloud_at_its_target_may_be_small_and_cpu_tensors_have_no_fallback():
    cloud_ops.check_upsample([67, 257], [67, 300], 16)
    cloud_ops.check_upsample([3], [3], 16)
    assert cloud_ops.round_sizes([257, 67, 130], [300, 67, 143]) == [25, 0, 13]
    assert cloud_ops.round_sizes([282, 67, 143], [300, 67, 143]) == [18, 0, 0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_ops.upsample(torch.zeros(1, 257, 3), 300)


def test_exports():
    import dss_amd
    from dss_amd import ops
    assert dss_amd.upsample is cloud_ops.upsample and dss_amd.upsample_clouds is cloud_ops.upsample_clouds
    assert dss_amd.remove_outliers is cloud_ops.remove_outliers
    assert callable(ops.upsample_candidates) and callable(ops.upsample_insert)


def test_key_order_is_the_order_of_sparsity_then_descending_id():
    """pure Python: ascending keys = ascending (s, -id), on random values, on tied values, and at the ends of the range"""
    rng = random.Random(0)
    values = [0.0, 1e-45, 1.1754944e-38, 1e-12, 0.03, 0.03, 0.03, 1.0, 3.4e38] + [rng.random() for _ in range(200)]
    values += [values[-1]] * 5 + [np.float32(0.1)] * 4
    items = [(float(np.float32(v)), i) for i, v in enumerate(rng.sample(values, len(values)))]
    items += [(float(np.float32(0.03)), 0xFFFFFFFE), (float(np.float32(0.03)), 0xFFFFFFFF)]   # the largest ids of a tied value
    items = list({(s, i) for s, i in items})
    by_key = sorted(items, key=lambda t: yard.pack_key(t[0], t[1]))
    by_rule = sorted(items, key=lambda t: (t[0], -t[1]))
    assert by_key == by_rule
    keys = [yard.pack_key(s, i) for s, i in items]
    assert all(0 <= k < 2 ** 63 for k in keys)          # non-negative as int64: finite, non-negative sparsity
    assert len(set(keys)) == len(keys)
    assert yard.pack_key(0.0, 0) == 0xFFFFFFFF and yard.pack_key(1.0, 5) == (0x3F800000 << 32) | (0xFFFFFFFF - 5)
