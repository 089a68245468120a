#!/usr/bin/env python3
"""Developer tool (GPU box): `ops.rasterize_meshes` + `ops.shade_mesh_flat` on an icosphere level 6 (81,920 faces) at 512^2
for N = 1 and N = 8 cameras.
   tools/mesh_raster_timing.py events [out.json]   device-event time per call, 5 windows of 200 calls after 20 warm-up calls
   tools/mesh_raster_timing.py trace N             50 calls, to be run under a kernel trace in a run of its own"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_raster_reference as mr  # noqa: E402
from dss_amd import ops  # noqa: E402
from dss_amd.cameras import FoVPerspectiveCameras, look_at_view_transform  # noqa: E402

dev = torch.device("cuda:0")
verts, faces = mr.icosphere(6)
assert len(faces) == 81920
tv, tf = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
first = torch.zeros(1, dtype=torch.int64, device=dev)
num = first + len(faces)
S = 512


def scene(N):
    rng = np.random.default_rng(N)
    R, T = look_at_view_transform(2.0, rng.uniform(-60, 60, N).tolist(), rng.uniform(-180, 180, N).tolist())
    cams = FoVPerspectiveCameras(znear=0.1, zfar=10.0, fov=60.0, R=R, T=T, device=dev)
    M = cams.get_full_projection_transform().get_matrix().contiguous()
    V = cams.get_world_to_view_transform().get_matrix().contiguous()
    c = cams.get_camera_center().contiguous()
    amb, kd, ks, d = mr.tri_color_lights(True)
    rep = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (N,) + a.shape))).to(dev)
    lights = (rep(amb), rep(kd), rep(ks), rep(d))
    zn, zf = cams.znear.contiguous(), cams.zfar.contiguous()

    def call():
        p, z, b, sv = ops.rasterize_meshes(tv, tf, first, num, M, V, zn, zf, c, S)
        return ops.shade_mesh_flat(p, b, tv, tf, first, num, c, *lights, False, 64.0), p
    return call


mode = sys.argv[1]
if mode == "events":
    out = {}
    for N in (1, 8):
        call = scene(N)
        for _ in range(20):
            rgba, p = call()
        torch.cuda.synchronize()
        cover = float((p >= 0).float().mean())
        windows = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(200):
                call()
            b.record()
            torch.cuda.synchronize()
            windows.append(a.elapsed_time(b) / 200 * 1e3)
        out["N=%d" % N] = dict(us_per_call=windows, us_per_view=[w / N for w in windows], covered=cover)
        print(N, ["%.1f" % w for w in windows], "us per call; covered %.3f" % cover, flush=True)
    if len(sys.argv) > 2:
        json.dump(out, open(sys.argv[2], "w"), indent=1)
else:
    call = scene(int(sys.argv[2]))
    for _ in range(50):
        call()
    torch.cuda.synchronize()
    print("trace run done", flush=True)
