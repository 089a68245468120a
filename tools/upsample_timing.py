#!/usr/bin/env python3
"""Developer tool (GPU box): `dss_amd.cloud_ops.upsample` against the same operation written in dense torch on the same
device, event-timed, the two alternating; and one round split into its four stages (kNN / candidates / sort / insert).

The baseline is the reference's formulation (DSS/core/cloud.py:599-625: all K x K distances of every point as one tensor,
norm, min, max, sort, gather, cat) with `ops.knn_points` for the neighbours, chunked over P because the reference's own
form allocates the (P,K,K,3) tensor at once (0.3 GB at 99,790 points, K = 16).

Sizes: the trained cloud of BASELINE configs[2], 99,790 points -> 2 x 99,790 (eight rounds), and its first round alone,
K = 16.  -> JSON (stdout, and the file given as argv[1])"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dss_amd import cloud_ops, ops  # noqa: E402

dev = torch.device("cuda:0")
K = 16


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


def i64(v):
    return torch.tensor([v], dtype=torch.int64, device=dev)


def dense_round(pts, n_new, chunk=16384):
    """one round of one cloud in dense torch: the reference's tensors, P in chunks"""
    P = pts.shape[0]
    _, idx = ops.knn_points(pts, i64(0), i64(P), K + 1)
    idx = idx[:, 1:]
    sparsity = torch.empty(P, device=dev)
    cand = torch.empty(P, 3, device=dev)
    for s in range(0, P, chunk):
        p = pts[s:s + chunk]
        q = pts[idx[s:s + chunk]]                                   # (c,K,3)
        mid = (q + 2 * p[:, None, :]) / 3
        d = torch.norm(mid.unsqueeze(-2) - q.unsqueeze(-3), dim=-1)  # (c,K,K)
        sp, nb = d.min(dim=-1)[0].max(dim=-1)
        sparsity[s:s + chunk] = sp
        cand[s:s + chunk] = mid[torch.arange(mid.shape[0], device=dev), nb]
    order = sparsity.sort().indices[P - n_new:]
    return torch.cat([cand[order], pts], 0)


def dense_upsample(pts, target):
    while pts.shape[0] < target:
        pts = dense_round(pts, min(target - pts.shape[0], pts.shape[0] // 10))
    return pts


def stages(pts, n_new, reps):
    """the HIP side of one round, stage by stage, each on the previous one's outputs"""
    P = pts.shape[0]
    first, num = i64(0), i64(P)
    _, idx = ops.knn_points(pts, first, num, K + 1)
    _, father, key = ops.upsample_candidates(pts, idx, first, num, K)
    sel = torch.sort(key).indices[P - n_new:]
    new_num, nn = i64(P + n_new), i64(n_new)
    return {"knn_points_K17": event_ms(lambda: ops.knn_points(pts, first, num, K + 1), reps),
            "upsample_candidates": event_ms(lambda: ops.upsample_candidates(pts, idx, first, num, K), reps),
            "sort_keys": event_ms(lambda: torch.sort(key).indices[P - n_new:], reps),
            "upsample_insert": event_ms(lambda: ops.upsample_insert(pts, None, idx, father, sel, first, num, first, new_num, nn, K), reps)}


def main():
    x = np.load(os.path.join(ROOT, "tests", "golden", "trained_cloud_cfg3.npz"))["points"]
    pts = torch.from_numpy(x).to(dev)
    P = pts.shape[0]
    hip_round = lambda: cloud_ops.upsample(pts[None], P + P // 10, neighborhood_size=K)   # noqa: E731
    hip_full = lambda: cloud_ops.upsample(pts[None], 2 * P, neighborhood_size=K)           # noqa: E731
    ref_round = lambda: dense_round(pts, P // 10)                                          # noqa: E731
    ref_full = lambda: dense_upsample(pts, 2 * P)                                          # noqa: E731
    for fn in (hip_round, hip_full, ref_round, ref_full):
        fn()
    torch.cuda.synchronize()
    out = {"device": torch.cuda.get_device_name(0), "P": P, "K": K, "rounds_to_double": 8}
    # alternate the two forms, as two halves each
    r = [event_ms(hip_round, 20), event_ms(ref_round, 5), event_ms(hip_round, 20), event_ms(ref_round, 5)]
    out["one_round_hip"], out["one_round_dense_torch"] = [r[0], r[2]], [r[1], r[3]]
    f = [event_ms(hip_full, 5), event_ms(ref_full, 2), event_ms(hip_full, 5), event_ms(ref_full, 2)]
    out["double_hip"], out["double_dense_torch"] = [f[0], f[2]], [f[1], f[3]]
    out["one_round_stages_hip"] = stages(pts, P // 10, 20)
    a, b = hip_full()[0][0], ref_full()
    out["double_rows_equal_dense_torch"] = int((a == b).all(dim=1).sum().item())
    out["double_rows"] = int(a.shape[0])
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
