"""Generates tests/golden/ref_losses_f64.npz: the REFERENCE's own `ProjectionLoss` and `RepulsionLoss`
(/root/reference/DSS/training/losses.py:148-495), unmodified, run end to end in FLOAT64 on the CPU under the stubs of
make_golden_losses.py, with autograd and a random upstream gradient providing the gradients.  It ties the float64
yardstick of tests/regularizer_reference.py to the reference (tests/test_regularizers_cpu.py: 1e-12 of the entry
magnitude, NaN in the same places).

The inputs are the float32 values of tests/regularizer_cases.py (FIXTURE_CASES) widened to float64.  The neighbour
search stand-in is `regularizer_reference.brute_knn` (float64 brute force, the point itself first, squared distances
rounded to float32 as the kernels receive them), padded like pytorch3d pads.  As in make_golden_losses.py the repulsion
loss runs cloud by cloud: get_spatial_w multiplies (N,P,K) by an (N,) factor, which only broadcasts for one cloud.

    python tests/golden/make_golden_losses_f64.py
"""
import os
import types

import numpy as np
import torch

import make_golden_losses as g32  # noqa: F401  (installs the stubs, imports the unmodified reference module)
import pytorch3d.ops as ops3d

import regularizer_cases as rc  # noqa: E402
import regularizer_reference as rr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ref_losses = g32.ref_losses


def _knn_points_f64(p1, p2, lengths1=None, lengths2=None, K=1, return_nn=False, **kw):
    """Self query of padded float64 clouds through brute_knn; rows and columns beyond a cloud's size are zero."""
    assert p1 is p2 or torch.equal(p1, p2)
    N, Pmax = p1.shape[:2]
    dists, idx = torch.zeros(N, Pmax, K, dtype=p1.dtype), torch.zeros(N, Pmax, K, dtype=torch.int64)
    for b in range(N):
        l = int(lengths1[b]) if lengths1 is not None else Pmax
        d2, ix = rr.brute_knn(p1[b, :l].detach().numpy(), [0], [l], K)
        dists[b, :l], idx[b, :l] = torch.from_numpy(d2.astype(np.float64)), torch.from_numpy(ix)
    nn = torch.stack([p2[b][idx[b]] for b in range(N)], 0) if return_nn else None
    return g32.base._KNN(dists, idx, nn)


ops3d.knn_points = _knn_points_f64


def run(case):
    first, num = case["first"], case["num"]
    live = [b for b in range(len(num)) if num[b] > 0]          # pytorch3d has no empty cloud inside a batch
    lengths = torch.tensor([int(num[b]) for b in live])
    maxp = int(lengths.max())

    def padded(a, dtype):
        out = torch.zeros((len(live), maxp) + a.shape[1:], dtype=dtype)
        for r, b in enumerate(live):
            out[r, : num[b]] = torch.from_numpy(a[first[b]: first[b] + num[b]]).to(dtype)
        return out

    def packed(x):
        out = np.zeros((len(case["points"]),) + tuple(x.shape[2:]))
        for r, b in enumerate(live):
            out[first[b]: first[b] + num[b]] = x[r, : num[b]].detach().numpy()
        return out

    P_pad, N_pad = padded(case["points"], torch.float64), padded(case["normals"], torch.float64)
    vis, inm = padded(case["visible"], torch.bool), padded(case["inmask"], torch.bool)
    flt = types.SimpleNamespace(visibility=vis, inmask=inm)
    kw = dict(reduction="none", knn_k=case["K"], filter_scale=case["filter_scale"], sharpness_sigma=case["sigma"])

    Pp = P_pad.clone().requires_grad_(True)
    pl = ref_losses.ProjectionLoss(**kw)
    loss = pl(g32._Clouds(Pp, N_pad, lengths), rebuild_knn=True, points_filter=flt)      # rows of the live clouds, packed
    assert loss.dtype == torch.float64
    rows = np.concatenate([np.arange(first[b], first[b] + num[b]) for b in live])
    (loss * torch.from_numpy(case["gl1"][rows]).double()).sum().backward()
    out = {"proj_loss": np.zeros(len(case["points"])), "proj_grad": packed(Pp.grad)}
    out["proj_loss"][rows] = loss.detach().numpy()
    with torch.no_grad():
        clouds = g32._Clouds(P_pad, N_pad, lengths)
        out["mollified"] = packed(pl._denoise_normals(clouds, pl.get_phi(clouds), flt).normals_padded())
    out["rep_loss"], out["rep_grad"] = np.zeros((len(case["points"]), 3)), np.zeros((len(case["points"]), 3))
    for r, b in enumerate(live):
        L, f = int(num[b]), int(first[b])
        Pr = P_pad[r: r + 1, :L].clone().requires_grad_(True)
        fb = types.SimpleNamespace(visibility=vis[r: r + 1, :L], inmask=inm[r: r + 1, :L])
        lossr = ref_losses.RepulsionLoss(**kw)(g32._Clouds(Pr, N_pad[r: r + 1, :L], lengths[r: r + 1]), rebuild_knn=True,
                                               points_filter=fb)                       # (L,3)
        assert lossr.dtype == torch.float64
        (lossr * torch.from_numpy(case["gl3"][f: f + L]).double()).sum().backward()
        out["rep_loss"][f: f + L], out["rep_grad"][f: f + L] = lossr.detach().numpy(), Pr.grad[0].numpy()
    return out


def main():
    out = {}
    for name in rc.FIXTURE_CASES:
        case = rc.case(name)
        for k in ("points", "normals", "first", "num", "visible", "inmask", "gl1", "gl3"):
            out["%s/%s" % (name, k)] = case[k]
        out[name + "/params"] = np.array([case["K"], case["sigma"], case["filter_scale"]], np.float64)
        with np.errstate(all="ignore"):
            res = run(case)
        for k, v in res.items():
            out["%s/%s" % (name, k)] = v
        print(name, {k: (float(np.nanmean(v)), int(np.isnan(v).sum())) for k, v in res.items()})
    path = os.path.join(HERE, "ref_losses_f64.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
