#!/usr/bin/env python3
"""Developer tool (GPU box): the propagation of a consistent sign by the persistent kernel (`ops.orient_normals`) against the
loop a user writes without it: the same rounds in eager torch on the same device -- per iteration a gather of the neighbours'
stamps and normals, the dot products, the threshold, an argmax with the tie rule, the masked stores, and ONE host read of
"was anybody oriented" that decides between the next round, a level drop and a new seed (the decision the kernel takes inside
the workgroup).  The torch loop computes the same normals, stamps and parents, which is reported.

Event-timed on the stream after a warm-up, the two forms alternating (two rounds each); medians with their spread.
Clouds: tests/golden/clouds.npz bunny (8,171 points; PCA directions of 16 neighbours from `ops.local_frames`, propagation over
8) and 100,000 random points on a sphere (analytic normals of random sign, above the LDS capacity: stamps in the workspace).
-> text (stdout, and the file given as argv[1])"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenes  # noqa: E402
from dss_amd import normals_ops, ops  # noqa: E402

dev = torch.device("cuda:0")
BIG = torch.iinfo(torch.int64).max


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


def torch_loop(n, pts, idx, KP):
    """the contract of dss_orient_normals for ONE cloud in eager torch -> (normals, stamp, parent, iterations)"""
    P = n.shape[0]
    nb = idx[:, 1:min(KP, idx.shape[1], P)]
    valid = nb != torch.arange(P, device=n.device)[:, None]
    out, stamp = n.clone(), torch.zeros(P, dtype=torch.int32, device=n.device)
    parent = torch.full((P,), -1, dtype=torch.int64, device=n.device)
    z = torch.nan_to_num(pts[:, 2], nan=-float("inf"))
    tau, level, it, left = normals_ops.THRESHOLDS, 0, 0, P
    while left > 0 and it < 5 * P:
        it += 1
        o = out[nb]
        d = (n[:, None, 0] * o[..., 0] + n[:, None, 1] * o[..., 1]) + n[:, None, 2] * o[..., 2]
        a = d.abs()
        ok = valid & (stamp[nb] > 0) & (stamp[:, None] == 0) & (a >= tau[level])
        am = torch.where(ok, a, torch.full_like(a, -1.0))
        best = ok & (am == am.max(1, keepdim=True).values)
        jj = torch.where(best, nb, torch.full_like(nb, BIG)).min(1).values
        cand = jj != BIG
        dsel = torch.gather(d, 1, (best & (nb == jj[:, None])).to(torch.int8).argmax(1, keepdim=True))[:, 0]
        count = int(cand.sum())                                   # the host decision of the iteration
        if count:
            out = torch.where(cand[:, None], torch.where((dsel < 0)[:, None], -n, n), out)
            stamp = torch.where(cand, torch.full_like(stamp, it), stamp)
            parent = torch.where(cand, jj, parent)
            left -= count
            level = 0
        elif level < 3:
            level += 1
        else:
            s = torch.argmax(torch.where(stamp == 0, z, torch.full_like(z, -float("inf"))))   # the first of the largest
            v = n[s]
            sign = torch.where(v[2] != 0, v[2], torch.where(v[1] != 0, v[1], v[0]))
            out[s] = torch.where(sign < 0, -v, v)
            stamp[s] = it
            left -= 1
            level = 0
    return out, stamp, parent, it


def compare(lines, tag, n, pts, idx, KP, reps_hip, reps_torch):
    P = n.shape[0]
    first, num = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), P, dtype=torch.int64, device=dev)
    hip = lambda: ops.orient_normals(n, pts, idx, first, num, KP, return_stamps=True, return_parents=True)   # noqa: E731
    eager = lambda: torch_loop(n, pts, idx, KP)   # noqa: E731
    a, b = hip(), eager()                        # warm-up of both forms at this shape
    torch.cuda.synchronize()
    same = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]))
    its, seeds = b[3], int((a[2] == -1).sum())
    t = [event_ms(hip, reps_hip), event_ms(eager, reps_torch), event_ms(hip, reps_hip), event_ms(eager, reps_torch)]
    med = lambda s: s[len(s) // 2]               # noqa: E731
    h, e = max(med(t[0]), med(t[2])), min(med(t[1]), med(t[3]))
    path = "stamps in LDS" if P <= normals_ops.LDS_CAPACITY else "stamps in the workspace"
    lines.append("%s: %d points (%s), %d neighbours, %d iterations, %d seed(s); results of the two forms equal: %s"
                 % (tag, P, path, KP - 1, its, seeds, same))
    for name, s in (("kernel     round 1", t[0]), ("torch loop round 1", t[1]), ("kernel     round 2", t[2]), ("torch loop round 2", t[3])):
        lines.append("    %s  %s" % (name, stats(s)))
    lines.append("    per iteration: kernel %.3f us (slower round), torch loop %.3f us (faster round); torch loop / kernel = %.1f"
                 % (1e3 * h / its, 1e3 * e / its, e / h))


def main():
    lines = ["device: %s" % torch.cuda.get_device_name(0), ""]
    pts, _ = scenes.load_cloud("bunny")
    x = torch.from_numpy(pts).to(dev)
    first, num = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), x.shape[0], dtype=torch.int64, device=dev)
    _, idx = ops.knn_points(x, first, num, 16)
    _, pca = ops.local_frames(x, idx, first, num)
    compare(lines, "bunny", pca, x, idx, 8, 30, 5)
    rng = np.random.default_rng(0)
    big = rng.standard_normal((100000, 3))
    big /= np.linalg.norm(big, axis=1, keepdims=True)
    signs = np.where(rng.random(100000) < 0.5, -1.0, 1.0)[:, None]
    y = torch.from_numpy(big.astype(np.float32)).to(dev)
    n = torch.from_numpy((big * signs).astype(np.float32)).to(dev)
    first, num = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), 100000, dtype=torch.int64, device=dev)
    _, idx = ops.knn_points(y, first, num, 8)
    compare(lines, "random sphere", n, y, idx, 8, 10, 3)
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
