"""Generates tests/golden/ref_live.npz: the inputs and the outputs of the UNMODIFIED reference CPU rasterizer (oracle/_ref,
splat_points bin_size=0) for the scenes of tests/test_oracle_pinning.py::test_live_reference_if_built and
::test_cpu_bbox_variant_on_clamped_radii, so that both tests also run where oracle/_ref has not been built.

    python tests/golden/make_golden_live.py        (needs oracle/_ref: `make -C oracle ref`)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import oracle  # noqa: E402
import scenes  # noqa: E402

KEYS = ("points", "ellipse", "cutoff", "radii", "first_idx", "num_pts")
OUTS = ("idx", "zbuf", "qvalue", "occ")


def live_cases():
    """(name, scene, S, K) of test_live_reference_if_built"""
    for seed, (P, S, N, K) in enumerate([(700, 40, 1, 5), (300, 33, 2, 8), (50, 16, 1, 1)]):
        yield "live%d" % seed, scenes.random_splats(P, S, N, seed=10 + seed), S, K


def bbox_case():
    """the scene of test_cpu_bbox_variant_on_clamped_radii (radii halved below the true ellipse bbox)"""
    sc = scenes.random_splats(400, 32, 1, seed=5)
    sc["radii"] = (sc["radii"] * 0.5).astype(np.float32)
    return sc


def main():
    R = oracle.ref()
    if R is None:
        raise SystemExit("oracle/_ref not built (make -C oracle ref)")
    out = {}
    cases = [(n, sc, S, K) for n, sc, S, K in live_cases()] + [("bbox", bbox_case(), 32, 5)]
    for name, sc, S, K in cases:
        t = lambda k: torch.from_numpy(sc[k])
        ref = R.splat_points(t("points"), t("ellipse"), t("cutoff"), t("radii"), t("first_idx"), t("num_pts"),
                             0.05, S, K, 0, 0)
        for k in KEYS:
            out["%s_%s" % (name, k)] = sc[k]
        for k, v in zip(OUTS, ref):
            out["%s_ref_%s" % (name, k)] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "ref_live.npz"), **out)


if __name__ == "__main__":
    main()
