#!/usr/bin/env python3
"""Developer tool (GPU box): the normal filter (`ops.denoise_normals`, K = 16) and the 10 x 5 RIMLS projection (ten
`ops.rimls_step`, K = 31) against the same arithmetic in eager torch, fp32, on the same device: the yardstick's own code
(tests/smoothing_reference.py `denoise_from_lists`, `rimls_step_from_lists`) -- dense (P,K,3) tensors, no host decision, the
form a user has today.  Event-timed on the stream after a warm-up, the two forms alternating; the neighbour lists are built
once, outside every timed region, and shared by both.

Sizes: tests/golden/bunny-8000.ply (8,171 points, unit sphere) and a cloud of ~1M points: 125 copies of it on a 5 x 5 x 5
lattice of pitch 2.5, each jittered by 0.2 % (the density, and so the neighbourhoods, stay those of the bunny).
-> JSON (stdout, and the file given as argv[1])"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenes  # noqa: E402
import smoothing_reference as yard  # noqa: E402
from dss_amd import ops  # noqa: E402

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


def big_cloud(pts, nrm, side=5, pitch=2.5, jitter=0.002):
    rng = np.random.default_rng(0)
    offs = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) * pitch
    x = np.concatenate([pts + o + rng.normal(0, jitter, pts.shape) for o in offs], 0).astype(np.float32)
    return x, np.tile(nrm, (len(offs), 1)).astype(np.float32)


def measure(tag, x, n, reps_hip, reps_eager):
    pts, nrm = torch.from_numpy(x).to(dev), torch.from_numpy(n).to(dev)
    P = pts.shape[0]
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    num = torch.full((1,), P, dtype=torch.int64, device=dev)
    out = {"tag": tag, "P": P}
    for tool, K, c in (("filter_K16", 16, 4.0), ("projection_10x5_K31", 31, 16.0)):
        r = float(yard.default_radius(x, K, c))
        radius = torch.full((1,), r, dtype=torch.float32, device=dev)
        d, idx = ops.knn_points(pts, first, num, K + 1)          # outside the timed regions, shared by both forms
        nb, dl = idx[:, 1:].contiguous(), d[:, 1:].contiguous()
        live = dl < radius * radius
        if tool.startswith("filter"):
            hip = lambda: ops.denoise_normals(pts, nrm, d, idx, first, num, radius, K, 30.0)           # noqa: E731
            eager = lambda: yard.denoise_from_lists(pts, nrm, nb, live, 30.0)                          # noqa: E731
        else:
            n_unit, inv, can = yard.rimls_setup(nrm, dl, live)

            def hip():
                state, alive = pts, None
                for _ in range(10):
                    state, alive = ops.rimls_step(state, nrm, d, idx, first, num, radius, K, alive, 5)
                return state, alive

            def eager():
                state, alive = pts, can
                for _ in range(10):
                    state, alive, _ = yard.rimls_step_from_lists(state, n_unit, nb, live, inv, alive, 5)
                return state, alive
        a, b = hip(), eager()
        torch.cuda.synchronize()
        a, b = (a[0], b[0]) if isinstance(a, tuple) else (a, b)
        res = {"radius": r, "live_share": round(float(live.float().mean()), 4),
               "max_abs_difference_hip_eager": float((a - b).abs().max())}
        t = [event_ms(hip, reps_hip), event_ms(eager, reps_eager), event_ms(hip, reps_hip), event_ms(eager, reps_eager)]
        res["hip"], res["eager_torch_fp32"] = [t[0], t[2]], [t[1], t[3]]
        res["ratio_eager_over_hip"] = round(min(t[1]["median_ms"], t[3]["median_ms"]) / max(t[0]["median_ms"], t[2]["median_ms"]), 2)
        out[tool] = res
        del d, idx, nb, dl, live
        torch.cuda.empty_cache()
    return out


def main():
    pts, nrm = scenes.load_cloud("bunny")
    pts = scenes.normalize_unit_sphere(pts).astype(np.float32)
    nrm = np.asarray(nrm, np.float32)
    big = big_cloud(pts, nrm)
    out = {"device": torch.cuda.get_device_name(0),
           "sizes": [measure("bunny_8171", pts, nrm, 100, 20), measure("bunny_x125_jittered", big[0], big[1], 20, 3)]}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
