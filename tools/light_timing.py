#!/usr/bin/env python3
"""Developer tool (GPU box): cost of the light reduction (`ops.phong_backward_lights`: two launches) next to the camera-centre
reduction of the same shading (`ops.phong_backward_camera`: two launches) on the same inputs in the same process -- the
yardstick, because it makes the same pass over the same pairs with 4 floats of partial per workgroup against 16 per light,
and one pass whatever L is where the light reduction makes one per light.  Median and spread of 30 event-timed calls after
warm-up, the two ops alternating, for 1 x 32,684, 8 x 99,790 shared and 8 x 1,000,000 shared with L = 1 and 2, point
lights, shininess 64 -> profiles/light_backward_timing.json."""
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
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "light_backward_timing.json")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


res = {}
for name, N, Pw, shared in (("1x32684", 1, 32684, False), ("8x99790_shared", 8, 99790, True), ("8x1000000_shared", 8, 1000000, True)):
    for L in (1, 2):
        g = torch.Generator().manual_seed(0)
        R, T = look_at_view_transform(2.2, [10.0 + 17 * k for k in range(N)], [30.0 + 47 * k for k in range(N)])
        cam = FoVPerspectiveCameras(R=R, T=T).get_camera_center().contiguous()
        world = torch.rand(Pw, 3, generator=g) - 0.5
        normals = torch.nn.functional.normalize(world + 0.3 * torch.randn(Pw, 3, generator=g), dim=1)
        P = N * Pw
        num = torch.full((N,), Pw, dtype=torch.int64)
        first = torch.arange(N, dtype=torch.int64) * Pw
        rgb, grad = torch.rand(P, 3, generator=g), torch.randn(P, 3, generator=g)
        amb, kd, ks = torch.rand(N, 3, generator=g), torch.rand(N, L, 3, generator=g), torch.rand(N, L, 3, generator=g)
        lvec = cam[:, None, :] * 1.1 + 0.5 * torch.randn(N, L, 3, generator=g)
        a = [t.to(dev) for t in (grad, world, normals, rgb, first, num, amb, kd, ks, lvec)] + [True, cam.to(dev), 64.0, shared]
        ops_ = {"phong_backward_camera": lambda: ops.phong_backward_camera(*a),
                "phong_backward_lights": lambda: ops.phong_backward_lights(*a)}
        for fn in ops_.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in ops_}
        for _ in range(30):
            for k, fn in ops_.items():
                t[k].append(timed(fn))
        key = "%s_L%d" % (name, L)
        res[key] = {"pairs": P, "lights": L}
        for k, v in t.items():
            v.sort()
            res[key][k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(v[0], 2), "p90": round(v[26], 2),
                                   "max": round(v[-1], 2)}
        res[key]["ratio_of_medians"] = round(res[key]["phong_backward_lights_us"]["median"]
                                             / res[key]["phong_backward_camera_us"]["median"], 3)
        print(key, json.dumps(res[key]), flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
