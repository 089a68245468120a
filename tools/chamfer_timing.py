#!/usr/bin/env python3
"""Developer tool (GPU box): `dss_amd.losses.chamfer_distance` forward + backward against the pure-torch stand-in
compat/pytorch3d/loss/chamfer.py (what a loop runs without it) on the same inputs and device, event-timed, the two
alternating; and the A/B behind the query order of dss_nearest_points -- the same search with the queries in input order
(a random permutation: what a caller hands over) and with the queries pre-sorted along the target's cells, i.e. the most
a binning pass could gain before its own cost.

Sizes: 99,790 x 100,000 (the trained cloud of BASELINE configs[2] against an n_eval_points-sized synthetic target) and
8,171 x 8,171 (bunny-8000 against a jittered copy).  -> JSON (stdout, and the file given as argv[1])"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "compat")):
    sys.path.insert(0, p)
import chamfer_reference as cr  # noqa: E402
import scenes  # noqa: E402
from dss_amd import losses, ops  # noqa: E402
from pytorch3d.loss import chamfer_distance as stand_in  # noqa: E402

dev = torch.device("cuda:0")


def event_ms(fn, reps):
    """median and spread of `reps` event-timed calls"""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4), "reps": reps}


def fwd_bwd(fn, x, y):
    def run():
        xg, yg = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        fn(xg, yg)[0].backward()
    return run


def cell_order(x, y):
    """x sorted by the cell of the target's grid it starts in (the arithmetic of knn_grid_kernel, on the host side)"""
    lo, hi = y.min(0).values, y.max(0).values
    res = int(np.ceil(np.sqrt(y.shape[0] / 24.0)))
    cell = (hi - lo).max() / res * 1.0001
    c = ((x - lo) / cell).floor().clamp(0, res - 1).long()
    return x[torch.argsort((c[:, 2] * res + c[:, 1]) * res + c[:, 0])].contiguous()


def measure(name, x_np, y_np, reps, reps_stand_in):
    x, y = torch.from_numpy(x_np).to(dev)[None], torch.from_numpy(y_np).to(dev)[None]
    row = {"scene": name, "Px": x.shape[1], "Py": y.shape[1]}
    hip, ref = fwd_bwd(losses.chamfer_distance, x, y), fwd_bwd(stand_in, x, y)
    a, b = losses.chamfer_distance(x, y)[0].item(), stand_in(x, y)[0].item()
    row["loss_hip"], row["loss_stand_in"] = a, b
    for _ in range(3):
        hip()
    ref()
    torch.cuda.synchronize()
    # alternate the two, as two halves each
    h1, s1 = event_ms(hip, reps), event_ms(ref, reps_stand_in)
    h2, s2 = event_ms(hip, reps), event_ms(ref, reps_stand_in)
    row["chamfer_fwd_bwd_hip"], row["chamfer_fwd_bwd_stand_in"] = [h1, h2], [s1, s2]
    row["chamfer_fwd_hip"] = event_ms(lambda: losses.chamfer_distance(x, y), reps)
    # query order A/B: one search x -> y, whole call (grid build of y included)
    xf, xn = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), x.shape[1], dtype=torch.int64, device=dev)
    yf, yn = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), y.shape[1], dtype=torch.int64, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(0)
    orders = {"as_given": x[0].contiguous(), "shuffled": x[0][torch.randperm(x.shape[1], generator=gen).to(dev)].contiguous()}
    orders["sorted_by_target_cell"] = cell_order(x[0], y[0])
    search = {}
    for rnd in range(2):
        for key, q in orders.items():
            run = lambda q=q: ops.nearest_points(q, xf, xn, y[0], yf, yn)  # noqa: E731
            run()
            search.setdefault(key, []).append(event_ms(run, reps))
    row["nearest_points_x_in_y"] = search
    d_a, _ = ops.nearest_points(orders["as_given"], xf, xn, y[0], yf, yn)
    d_s, _ = ops.nearest_points(orders["sorted_by_target_cell"], xf, xn, y[0], yf, yn)
    assert torch.equal(d_a.sort().values, d_s.sort().values), "the query order changed a result"
    return row


def main():
    trained = np.load(os.path.join(ROOT, "tests", "golden", "trained_cloud_cfg3.npz"))["points"]
    target, _, _ = scenes.synthetic_cloud(100000, seed=3)
    bunny = scenes.normalize_unit_sphere(cr.read_ply_points(os.path.join(ROOT, "tests", "golden", "bunny-8000.ply")))
    rng = np.random.default_rng(4)
    jittered = (bunny + rng.normal(0, 0.01, bunny.shape)).astype(np.float32)
    out = {"device": torch.cuda.get_device_name(0),
           "rows": [measure("trained_cfg3_vs_synthetic_100k", trained, target.astype(np.float32), 30, 3),
                    measure("bunny_8171_vs_jittered", bunny, jittered, 100, 10)]}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
