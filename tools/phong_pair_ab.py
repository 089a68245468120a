#!/usr/bin/env python3
"""Developer tool (GPU box): do two builds of the library (DSS_HIP_LIBRARY, as tools/ab_libs.py) compute the same bits in
the same time for the shading's four operators and the camera reduction next to them?  One library per process:

    python tools/phong_pair_ab.py hash OUT.json      one SHA-256 per (case, operator, output) of phong_forward,
        phong_backward, phong_backward_camera, phong_backward_lights and camera_backward on seeded inputs: every layout of
        tests/shading_reference.py x both light kinds x shininess 12 and 64, its IDENTITY_CASES, and the three shapes of
        tools/light_timing.py with L = 1 and 2.  Two builds agree when their files are equal (`cmp`).
    python tools/phong_pair_ab.py time OUT.json      median of 30 event-timed calls after warm-up of the four Phong
        operators at the three shapes of tools/light_timing.py (L = 2, point lights, shininess 64), in us
    python tools/phong_pair_ab.py compare OUT.json A1.json B1.json A2.json B2.json
        the `time` files of one run that alternated yardstick A and candidate B.  B passes at an (operator, shape) when its
        slower median exceeds A's slower median by no more than the distance between A's own two medians: that distance is
        the noise of the comparison, measured where it is used."""
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("1x32684", 1, 32684, False), ("8x99790_shared", 8, 99790, True), ("8x1000000_shared", 8, 1000000, True))
PHONG = ("phong_forward", "phong_backward", "phong_backward_camera", "phong_backward_lights")


def compare(out_path, a1, b1, a2, b2):
    A, B = [json.load(open(p)) for p in (a1, a2)], [json.load(open(p)) for p in (b1, b2)]
    res, ok = {}, True
    for shape in A[0]:
        for op in PHONG:
            a, b = [x[shape][op] for x in A], [x[shape][op] for x in B]
            row = {"yardstick_us": a, "candidate_us": b, "noise_us": round(abs(a[0] - a[1]), 2),
                   "excess_us": round(max(b) - max(a), 2)}
            row["pass"] = row["excess_us"] <= row["noise_us"]
            ok = ok and row["pass"]
            res["%s %s" % (shape, op)] = row
            print(shape, op, json.dumps(row))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if sys.argv[1] == "compare":
    sys.exit(compare(*sys.argv[2:7]))

import torch  # noqa: E402

sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import shading_reference as sr  # noqa: E402
from dss_amd import _lib, ops  # noqa: E402
from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform  # noqa: E402

dev = torch.device("cuda:0")


def cameras(N):
    R, T = look_at_view_transform(2.2, [10.0 + 17 * k for k in range(N)], [30.0 + 47 * k for k in range(N)])
    return FoVPerspectiveCameras(znear=0.1, R=R, T=T)


def shape_case(N, Pw, L):
    """the inputs of tools/light_timing.py, in the order of `sr.layout_case`"""
    g = torch.Generator().manual_seed(0)
    cam = cameras(N).get_camera_center().contiguous()
    world = torch.rand(Pw, 3, generator=g) - 0.5
    normals = torch.nn.functional.normalize(world + 0.3 * torch.randn(Pw, 3, generator=g), dim=1)
    P = N * Pw
    num, first = torch.full((N,), Pw, dtype=torch.int64), torch.arange(N, dtype=torch.int64) * Pw
    rgb, grad = torch.rand(P, 3, generator=g), torch.randn(P, 3, generator=g)
    amb, kd, ks = torch.rand(N, 3, generator=g), torch.rand(N, L, 3, generator=g), torch.rand(N, L, 3, generator=g)
    lvec = cam[:, None, :] * 1.1 + 0.5 * torch.randn(N, L, 3, generator=g)
    return world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad


def operators(case, shared, point, shin):
    """-> {operator: callable -> tuple of output tensors}"""
    world, normals, rgb, first, num, amb, kd, ks, lvec, cam, grad = [t.to(dev) for t in case]
    fwd = (world, normals, rgb, first, num, amb, kd, ks, lvec, point, cam, float(shin), shared)
    N, P = len(num), rgb.shape[0]
    g = torch.Generator().manual_seed(1)
    cams = cameras(N)
    M = cams.get_full_projection_transform().get_matrix().contiguous().to(dev)
    V = cams.get_world_to_view_transform().get_matrix().contiguous().to(dev)
    grad_screen, valid = (torch.randn(P, 3, generator=g) * 0.05).to(dev), (torch.rand(P, generator=g) > 0.33).to(dev)
    return {"phong_forward": lambda: (ops.phong_forward(*fwd),),
            "phong_backward": lambda: ops.phong_backward(grad, *fwd),
            "phong_backward_camera": lambda: (ops.phong_backward_camera(grad, *fwd),),
            "phong_backward_lights": lambda: ops.phong_backward_lights(grad, *fwd),
            "camera_backward": lambda: ops.camera_backward(world, M, V, first, num, grad_screen, valid, shared, 0.05)}


def hash_cases():
    for name in sr.LAYOUTS:
        for kind in sr.KINDS:
            for shin in (12, 64):
                yield "%s %s s=%d" % (name, kind, shin), sr.layout_case(name), kind, shin
    for name, kind, shin in sr.IDENTITY_CASES:
        yield "identity %s %s s=%d" % (name, kind, shin), sr.identity_case(name), kind, shin
    for name, N, Pw, shared in SHAPES:
        for L in (1, 2):
            yield "%s L=%d" % (name, L), (shape_case(N, Pw, L), shared), "point", 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


mode, out_path = sys.argv[1], sys.argv[2]
res = {}
if mode == "hash":
    for tag, (case, shared), kind, shin in hash_cases():
        own = sr.owned_rows(case, shared).to(dev)
        for op, fn in operators(case, shared, kind == "point", shin).items():
            for i, t in enumerate(fn()):
                if shared and (op, i) in (("phong_forward", 0), ("phong_backward", 2)):
                    t = t[own]   # a camera that owns fewer than Pw points leaves the rows of its missing pairs unspecified
                res["%s | %s | %d" % (tag, op, i)] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    print("%s: %d digests of %s" % (out_path, len(res), _lib.LIB_PATH))
elif mode == "time":
    for name, N, Pw, shared in SHAPES:
        fns = {k: v for k, v in operators(shape_case(N, Pw, 2), shared, True, 64).items() if k in PHONG}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(30):
            for k, fn in fns.items():
                t[k].append(timed(fn))
        res[name] = {k: round(statistics.median(v), 2) for k, v in t.items()}
        print(name, _lib.LIB_PATH, json.dumps(res[name]), flush=True)
else:
    sys.exit("unknown mode %r" % mode)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
