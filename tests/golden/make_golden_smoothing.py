"""Generates tests/golden/ref_smoothing.npz.

The filter: the REFERENCE's own `denoise_normals` (DSS/core/cloud.py:515-552), unmodified, imported in place with the stubs
of make_golden_setup.py, for N = 1 and K = 16.  On top of those it needs stand-ins for the two `frnn` calls it makes:
  - `frnn.frnn_grid_points(p1, p2, lengths1, lengths2, K, r, ...)` -> (squared distances, ids, None, None): the K nearest
    (the brute-force kNN of make_golden_setup.py) with d < r^2, else id -1 and distance -1;
  - `frnn.frnn_gather(x, idx, lengths)` -> x gathered at idx, ZEROS where idx is -1.
Scenes: the two patches of tests/smoothing_reference.py ("plane", "paraboloid", 1500 points) and its sphere scene (1000
points, where the radius of 0.2 and the 32 / P cut both remove neighbours).

The projection has NO reference run: `project_to_latent_surface` (:442-513) does not run on a current torch --
``not_converged[not_converged] = mask`` (:508) and ``not_converged_1[not_converged_1] = ...`` (:482) raise "unsupported
operation: some elements of the input tensor and the written-to tensor refer to a single memory location".  Its expected
outputs in the fixture are the float64 yardstick's (tests/smoothing_reference.py `project`, at the defaults, on the
yardstick's filtered normals rounded to fp32).  Arrays only.

    python tests/golden/make_golden_smoothing.py
"""
import os

import numpy as np
import torch

import make_golden_setup as base   # installs the stubs and imports the reference package from where it lies

import importlib  # noqa: E402
import frnn  # noqa: E402  (the stub)
import pytorch3d.ops.knn as ops3d_knn  # noqa: E402  (the stub)
import smoothing_reference as yard  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
K = 16


def _frnn_grid_points(p1, p2, lengths1=None, lengths2=None, K=1, r=0.2, grid=None, return_nn=False, **kw):
    knn = base._knn_points(p1, p2, lengths1, lengths2, K, False)
    inside = knn.dists < float(r) ** 2
    idx = torch.where(inside, knn.idx, torch.full_like(knn.idx, -1))
    dists = torch.where(inside, knn.dists, torch.full_like(knn.dists, -1.0))
    return dists, idx, None, None


def _frnn_gather(x, idx, lengths=None):
    out = torch.stack([x[b][idx[b].clamp(min=0)] for b in range(x.shape[0])], 0)
    return out * (idx >= 0)[..., None].to(out.dtype)


def main():
    frnn.frnn_grid_points, frnn.frnn_gather = _frnn_grid_points, _frnn_gather
    ops3d_knn._KNN = base._KNN
    ref_cloud = importlib.import_module("DSS.core.cloud")   # the UNMODIFIED reference module
    ref_cloud._KNN = base._KNN
    ref_cloud.frnn = frnn
    out = {"K": np.int32(K)}
    scenes = {name: yard.scene(name)[:2] for name in yard.SCENES}
    scenes["sphere"] = yard.sphere_scene()
    for name, (x, n) in scenes.items():
        P = x.shape[0]
        with torch.no_grad():
            got = ref_cloud.denoise_normals(torch.from_numpy(x)[None].clone(), torch.from_numpy(n)[None].clone(),
                                            torch.tensor([P]), neighborhood_size=K)
        assert got.shape == (1, P, 3)
        out[name + "_points"], out[name + "_normals"] = x, n
        out[name + "_filtered"] = got[0].numpy().astype(np.float32)
    for name in yard.SCENES:
        x, n = scenes[name]
        nf = yard.denoise(x, n, K=K)["normals"].astype(np.float32)
        p = yard.project(x, nf)
        out[name + "_projected"] = p["points"]          # float64
        out[name + "_converged"] = p["converged"]
    np.savez_compressed(os.path.join(HERE, "ref_smoothing.npz"), **out)
    for k, v in out.items():
        print(k, getattr(v, "shape", v), getattr(v, "dtype", ""))


if __name__ == "__main__":
    main()
