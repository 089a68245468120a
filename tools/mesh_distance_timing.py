#!/usr/bin/env python3
"""Developer tool (GPU box): the two point-to-mesh searches (`ops.point_face_distance`, `ops.face_point_distance`) and
`losses.point_mesh_face_distance` forward + backward, each against a chunked brute-force torch evaluation of the same
definition (include/dss_hip.h) on the same inputs and device -- event-timed, warmed up, the two alternating; and the A/B of
the large-list multiple (DSS_OPT_MESH_LARGE, quarters of a cell) on the point -> face search.

Sizes: 100,000 points x a 99,904-face height-field sheet; 8,171 points (tests/golden/bunny-8000.ply) x a 1,280-face
icosphere; and, for the A/B, 20,000 points x a mesh of two triangle sizes (20,480 fine + 80 coarse faces), the only one of
the three that puts anything on the large list.  -> JSON (stdout, and the file given as argv[1], e.g. profiles/mesh_distance_timing.json)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import chamfer_reference as cr  # noqa: E402
import mesh_distance_reference as mr  # noqa: E402
from dss_amd import _lib, losses, ops  # noqa: E402

dev = torch.device("cuda:0")
INF = float("inf")


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


# ---- the definition in torch: q (Q,1,3) against A, B, C (1,F,3), or row by row on (M,3) pairs
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _seg(q, P, R):
    sw = (R[..., 0] < P[..., 0]) | ((R[..., 0] == P[..., 0]) & ((R[..., 1] < P[..., 1]) | ((R[..., 1] == P[..., 1]) & (R[..., 2] < P[..., 2]))))
    p0, p1 = torch.where(sw[..., None], R, P), torch.where(sw[..., None], P, R)
    e, w = p1 - p0, q - p0
    ee, we = _dot(e, e), _dot(w, e)
    first = (we <= 0) | (ee == 0)
    second = ~first & (we >= ee)
    t = we / torch.where(ee == 0, torch.ones_like(ee), ee)
    r = torch.where(first[..., None], w, torch.where(second[..., None], q - p1, w - t[..., None] * e))
    return _dot(r, r)


def d2_torch(q, A, B, C):
    n = torch.linalg.cross(B - A, C - A)
    nn = _dot(n, n)
    sides = [_dot(torch.linalg.cross(R - P, q - P), n) for P, R in ((A, B), (B, C), (C, A))]
    inside = (nn > 0) & (sides[0] > 0) & (sides[1] > 0) & (sides[2] > 0)
    h = _dot(q - A, n)
    plane = torch.where(inside, (h * h) / torch.where(nn > 0, nn, torch.ones_like(nn)), torch.full_like(h, INF))
    best = torch.full_like(h, INF)
    for cand in (_seg(q, A, B), _seg(q, B, C), _seg(q, C, A), plane):
        best = torch.where(cand < best, cand, best)
    return best


def brute_force(points, verts, faces, chunk):
    """both searches, chunked over the queries: (d2 (P,), idx (P,)), (d2 (F,), idx (F,))"""
    A, B, C = (verts[faces[:, k]][None] for k in range(3))
    dp, ip = [], []
    df = torch.full((faces.shape[0],), INF, device=dev)
    jf = torch.full((faces.shape[0],), -1, dtype=torch.int64, device=dev)
    for s in range(0, points.shape[0], chunk):
        D = d2_torch(points[s:s + chunk, None, :], A, B, C)
        d, i = D.min(1)
        dp.append(d), ip.append(i)
        m, j = D.min(0)
        better = m < df
        df, jf = torch.where(better, m, df), torch.where(better, j + s, jf)
    return (torch.cat(dp), torch.cat(ip)), (df, jf)


def brute_loss(points, verts, faces, chunk):
    """what a loop runs without the kernels: the search without a graph, then the pairs' distances with one"""
    with torch.no_grad():
        (_, ip), (_, jf) = brute_force(points, verts, faces, chunk)
    tri = verts[faces]
    d_p = d2_torch(points, tri[ip, 0], tri[ip, 1], tri[ip, 2])
    d_f = d2_torch(points[jf], tri[:, 0], tri[:, 1], tri[:, 2])
    return d_p.mean() + d_f.mean()


def sheet(nx, ny):
    v, f = mr.lattice_sheet(nx, ny)
    v = v.astype(np.float64)
    v[:, 0], v[:, 1] = v[:, 0] / nx * 2 - 1, v[:, 1] / ny * 2 - 1
    v[:, 2] = 0.3 * np.sin(3 * v[:, 0]) * np.cos(2 * v[:, 1])
    return v.astype(np.float32), f


def measure(name, pts_np, verts_np, faces_np, reps, reps_brute, chunk):
    pts, verts, faces = (torch.from_numpy(a).to(dev) for a in (pts_np, verts_np, faces_np))
    P, F = pts.shape[0], faces.shape[0]
    one = torch.zeros(1, dtype=torch.int64, device=dev)
    pn, fn = torch.full((1,), P, dtype=torch.int64, device=dev), torch.full((1,), F, dtype=torch.int64, device=dev)
    row = {"scene": name, "P": P, "F": F, "V": verts.shape[0], "brute_force_chunk": chunk}
    pf = lambda: ops.point_face_distance(pts, one, pn, verts, faces, one, fn)  # noqa: E731
    fp = lambda: ops.face_point_distance(pts, one, pn, verts, faces, one, fn)  # noqa: E731
    bf = lambda: brute_force(pts, verts, faces, chunk)  # noqa: E731

    def loss_hip():
        p, v = pts.detach().requires_grad_(True), verts.detach().requires_grad_(True)
        losses.point_mesh_face_distance(([v], [faces]), p[None]).backward()

    def loss_brute():
        p, v = pts.detach().requires_grad_(True), verts.detach().requires_grad_(True)
        brute_loss(p, v, faces, chunk).backward()

    (d_b, i_b), (df_b, jf_b) = bf()
    d_h, i_h = pf()
    df_h, jf_h = fp()
    # (torch.min names any of several equal minima, so the ids are compared only as a count)
    row["point_face_d2_equal_to_brute_force"] = bool(torch.equal(d_h, d_b))
    row["face_point_d2_equal_to_brute_force"] = bool(torch.equal(df_h, df_b))
    row["point_face_ids_differing_from_torch_min"] = int((i_h != i_b).sum())
    row["face_point_ids_differing_from_torch_min"] = int((jf_h != jf_b).sum())
    row["loss_hip"] = float(losses.point_mesh_face_distance(([verts], [faces]), pts[None]))
    row["loss_brute_force"] = float(brute_loss(pts, verts, faces, chunk))
    for _ in range(3):
        pf(), fp(), loss_hip()
    loss_brute()
    torch.cuda.synchronize()
    # alternate the two sides, two halves each
    for half in range(2):
        row.setdefault("point_face_hip", []).append(event_ms(pf, reps))
        row.setdefault("face_point_hip", []).append(event_ms(fp, reps))
        row.setdefault("both_searches_brute_force", []).append(event_ms(bf, reps_brute))
        row.setdefault("loss_fwd_bwd_hip", []).append(event_ms(loss_hip, reps))
        row.setdefault("loss_fwd_bwd_brute_force", []).append(event_ms(loss_brute, reps_brute))
    # the large-list multiple, in quarters of a cell (0 = the default), two rounds
    ab = {}
    for rnd in range(2):
        for quarters in (0, 2, 4, 8, 16, 32, 128):
            old = _lib.set_option(_lib.OPT_MESH_LARGE, quarters)
            try:
                d_q, i_q = pf()
                assert torch.equal(d_q, d_h) and torch.equal(i_q, i_h), "the multiple changed a result"
                ab.setdefault(str(quarters), []).append(event_ms(pf, reps))
            finally:
                _lib.set_option(_lib.OPT_MESH_LARGE, old)
    row["point_face_by_large_multiple_quarters"] = ab
    return row


def main():
    rng = np.random.default_rng(5)
    sv, sf = sheet(224, 223)
    on = sv[rng.integers(0, len(sv), 100000)]
    cloud = (on + rng.normal(0, 0.01, on.shape)).astype(np.float32)
    bunny = cr.read_ply_points(os.path.join(ROOT, "tests", "golden", "bunny-8000.ply")).astype(np.float32)
    bunny = ((bunny - bunny.mean(0)) / np.abs(bunny - bunny.mean(0)).max()).astype(np.float32)
    iv, if_ = mr.icosphere(3)
    # triangles of two sizes in one mesh (the uniform meshes above put nothing on the large list at any multiple): a fine
    # sphere inside a coarse one whose triangles span ~4 cells of the centroid grid
    fv, ff = mr.icosphere(5)
    cv, cf = mr.icosphere(1, radius=1.5)
    mixed_v, mixed_f = np.concatenate([fv, cv]), np.concatenate([ff, cf + len(fv)])
    around = rng.uniform(-1.6, 1.6, (20000, 3)).astype(np.float32)
    out = {"device": torch.cuda.get_device_name(0),
           "rows": [measure("cloud_100k_vs_sheet_99904_faces", cloud, sv, sf, 20, 1, 128),
                    measure("bunny_8171_vs_icosphere_1280_faces", bunny, iv, if_, 50, 5, 2048),
                    measure("mixed_sizes_20k_vs_20480_fine_plus_80_coarse_faces", around, mixed_v, mixed_f, 30, 3, 512)]}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
