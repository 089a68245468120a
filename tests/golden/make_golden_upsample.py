"""Generates tests/golden/ref_upsample.npz by running the REFERENCE's own `upsample` (DSS/core/cloud.py:555-632), imported
in place with the stubs of make_golden_setup.py.  On top of those it needs
  - `pytorch3d.ops.knn_points` / `_KNN` bound INSIDE the imported module (cloud.py takes them from pytorch3d.ops.knn)
    -> the brute-force stand-in of make_golden_setup.py, which returns the neighbours' positions for return_nn;
  - `padded_to_list` / `list_to_padded` (pytorch3d.structures.utils)       -> trivial stand-ins.
Scenes: the unit sphere with 2 % radial noise of tests/upsample_reference.py `sphere_scene`, seeds 0 / 1 / 2:
257 -> 300 points (one round), 600 -> 900 (five rounds), 1000 -> 2000 (eight rounds), K = 16.  Arrays only: the input and the
reference's output of every scene.

    python tests/golden/make_golden_upsample.py
"""
import os

import numpy as np
import torch

import make_golden_setup as base   # installs the stubs and imports the reference package from where it lies

import importlib  # noqa: E402
import pytorch3d.ops.knn as ops3d_knn  # noqa: E402  (the stub)
import upsample_reference as yard  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ((1, 257, 300), (0, 600, 900), (2, 1000, 2000))   # seed, points, target


def _knn_points(p1, p2, lengths1=None, lengths2=None, K=1, return_nn=False, **kw):
    return base._knn_points(p1, p2, lengths1, lengths2, K, return_nn)


def _padded_to_list(x, sizes=None):
    return [x[b, :(sizes[b] if sizes is not None else x.shape[1])] for b in range(x.shape[0])]


def _list_to_padded(lst):
    out = lst[0].new_zeros(len(lst), max(t.shape[0] for t in lst), lst[0].shape[1])
    for b, t in enumerate(lst):
        out[b, :t.shape[0]] = t
    return out


def main():
    base.ops3d.knn_points = _knn_points
    ops3d_knn._KNN = base._KNN
    ref_cloud = importlib.import_module("DSS.core.cloud")   # the UNMODIFIED reference module
    ref_cloud._KNN, ref_cloud.knn_points = base._KNN, _knn_points
    ref_cloud.padded_to_list, ref_cloud.list_to_padded = _padded_to_list, _list_to_padded
    out = {"K": np.int32(16)}
    for seed, P, target in SCENES:
        x = yard.sphere_scene(seed, P)
        with torch.no_grad():
            grown, num = ref_cloud.upsample(torch.from_numpy(x)[None].clone(), target, neighborhood_size=16)
        assert int(num[0]) == target and grown.shape[1] == target
        out["s%d_in" % seed] = x
        out["s%d_out" % seed] = grown[0].numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "ref_upsample.npz"), **out)
    for k, v in out.items():
        print(k, getattr(v, "shape", v))


if __name__ == "__main__":
    main()
