#!/usr/bin/env python3
"""Developer tool (GPU box): farthest point sampling by the persistent kernel (`ops.farthest_points`) against the loop a user
writes without it: the same algorithm in eager torch on the same device, per selected point a gather of the centre, `sub`,
square-sum, `minimum`, `argmax` and the store of the id -- no host decision, no synchronisation inside the loop.  (The torch
loop does not mark selected points; on clouds without duplicate points it selects the same ids, which is reported.)

Event-timed on the stream after a warm-up, the two forms alternating (two rounds each); medians with their spread.
Sizes: tests/golden/bunny-8000.ply (8,171 points, unit sphere) at 512 and 2,048 samples, a 100,000-point random cloud at 4,096
samples (streaming path), and for the cost of a step on every path one random cloud that fills each instantiation, and one
behind the last, at 1,024 samples (kernel alone).
-> text (stdout, and the file given as argv[1])"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenes  # noqa: E402
from dss_amd import ops, sampling_ops  # noqa: E402

dev = torch.device("cuda:0")


def event_ms(fn, reps):
    """sorted times of `reps` event-timed calls"""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)


def stats(times):
    return "median %9.3f ms  (min %9.3f, max %9.3f, %d reps)" % (times[len(times) // 2], times[0], times[-1], len(times))


def torch_loop(x, k):
    d = torch.full((x.shape[0],), float("inf"), device=x.device)
    idx = torch.empty((k,), dtype=torch.int64, device=x.device)
    c = torch.zeros((), dtype=torch.int64, device=x.device)
    for t in range(k):
        idx[t] = c
        diff = x - x.index_select(0, c.reshape(1))
        d = torch.minimum(d, diff.square().sum(-1))
        c = torch.argmax(d)
    return idx


def hip_call(x, k):
    P = x.shape[0]
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    num = torch.full((1,), P, dtype=torch.int64, device=dev)
    ks = torch.full((1,), k, dtype=torch.int64, device=dev)
    return lambda: ops.farthest_points(x, first, num, ks, None, k)


def compare(lines, tag, x, k, reps_hip, reps_torch):
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    hip = hip_call(x, k)
    eager = lambda: torch_loop(x, k)   # noqa: E731
    a, b = hip()[0], eager()           # warm-up of both forms at this shape
    torch.cuda.synchronize()
    same = bool(torch.equal(a, b))
    t = [event_ms(hip, reps_hip), event_ms(eager, reps_torch), event_ms(hip, reps_hip), event_ms(eager, reps_torch)]
    med = lambda s: s[len(s) // 2]     # noqa: E731
    h, e = max(med(t[0]), med(t[2])), min(med(t[1]), med(t[3]))
    lines.append("%s: %d points, %d samples; ids of the two forms equal: %s" % (tag, x.shape[0], k, same))
    for name, s in (("kernel     round 1", t[0]), ("torch loop round 1", t[1]), ("kernel     round 2", t[2]), ("torch loop round 2", t[3])):
        lines.append("    %s  %s" % (name, stats(s)))
    lines.append("    per selected point: kernel %.3f us (slower round), torch loop %.3f us (faster round); torch loop / kernel = %.1f"
                 % (1e3 * h / k, 1e3 * e / k, e / h))


def step_cost(lines, P, k, reps):
    x = torch.from_numpy(np.random.default_rng(P).uniform(-1, 1, (P, 3)).astype(np.float32)).to(dev)
    hip = hip_call(x, k)
    hip()
    torch.cuda.synchronize()
    t = event_ms(hip, reps)
    path = next((("registers, capacity %d" % c) for c in sampling_ops.REGISTER_CAPACITIES if P <= c), "streaming")
    lines.append("    %6d points (%s): %s = %.3f us per selected point" % (P, path, stats(t), 1e3 * t[len(t) // 2] / k))


def main():
    lines = ["device: %s" % torch.cuda.get_device_name(0), ""]
    pts, _ = scenes.load_cloud("bunny")
    pts = scenes.normalize_unit_sphere(pts).astype(np.float32)
    compare(lines, "bunny", pts, 512, 30, 5)
    compare(lines, "bunny", pts, 2048, 30, 5)
    big = np.random.default_rng(0).uniform(-1, 1, (100000, 3)).astype(np.float32)
    compare(lines, "random cloud (streaming path)", big, 4096, 5, 3)
    lines += ["", "cost of a step on every path, 1,024 samples, kernel alone (launch and row padding included):"]
    for cap in sampling_ops.REGISTER_CAPACITIES:
        step_cost(lines, cap, 1024, 20)
    step_cost(lines, sampling_ops.MAX_REGISTER_POINTS + 1, 1024, 10)
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
