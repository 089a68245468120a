#!/usr/bin/env python3
"""Developer tool (GPU box): cost of the camera reduction (`ops.camera_backward`: two launches) next to the projection
backward (`ops.project_backward`: one launch) on the same inputs in the same process -- the yardstick, because it reads the
same bytes per (camera, point) pair and writes more.  Median and spread of 30 event-timed calls after warm-up, the two ops
alternating, for 1 x 32,684, 8 x 99,790 shared and 8 x 1,000,000 shared -> profiles/camera_backward_timing.json."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dss_amd import ops  # noqa: E402
from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform  # noqa: E402

dev = torch.device("cuda:0")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "camera_backward_timing.json")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


res = {}
for name, N, Pw, shared in (("1x32684", 1, 32684, False), ("8x99790_shared", 8, 99790, True), ("8x1000000_shared", 8, 1000000, True)):
    g = torch.Generator().manual_seed(0)
    R, T = look_at_view_transform(2.2, [10.0 + 17 * k for k in range(N)], [30.0 + 47 * k for k in range(N)])
    cams = FoVPerspectiveCameras(znear=0.1, R=R, T=T)
    M = cams.get_full_projection_transform().get_matrix().contiguous().to(dev)
    V = cams.get_world_to_view_transform().get_matrix().contiguous().to(dev)
    world = (torch.rand(Pw, 3, generator=g) - 0.5).to(dev)
    P = N * Pw
    num = torch.full((N,), Pw, dtype=torch.int64, device=dev)
    first = torch.arange(N, dtype=torch.int64, device=dev) * Pw
    grad = (torch.randn(P, 3, generator=g) * 0.05).to(dev)
    valid = (torch.rand(P, generator=g) > 0.33).to(dev)
    ops_ = {"project_backward": lambda: ops.project_backward(world, M, V, first, num, grad, valid, shared, 0.05),
            "camera_backward": lambda: ops.camera_backward(world, M, V, first, num, grad, valid, shared, 0.05)}
    for fn in ops_.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ops_}
    for _ in range(30):
        for k, fn in ops_.items():
            t[k].append(timed(fn))
    res[name] = {"pairs": P}
    for k, v in t.items():
        v.sort()
        res[name][k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(v[0], 2), "p90": round(v[26], 2),
                                "max": round(v[-1], 2)}
    res[name]["ratio_of_medians"] = round(res[name]["camera_backward_us"]["median"] / res[name]["project_backward_us"]["median"], 3)
    print(name, json.dumps(res[name]), flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
