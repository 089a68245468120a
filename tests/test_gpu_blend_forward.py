"""GPU: the forward image and the weight sums -- `ops.blend_forward` (`blend_forward_kernel<3>` / `<0>`, `csrc/blend.hip`),
the C entry `dss_splat_fine_blend` (the per-point-array epilogue of the fine pass at every `KMAX` and at runtime C, with
and without a tile workspace) and `ops.render_forward` (the packed-record epilogue at K <= 8, C = 3; the per-point-array one
elsewhere and in the lean mode) -- against the fp64 reference of `tests/blend_reference.py`, entry by entry.

Every comparison is ``|got - ref| <= bar A + UNDERFLOW`` per entry with ``A`` the sum of the entry's absolute terms and the
bar of the case from `blend_reference.BARS` (4 x what the documented arithmetic loses in plain fp32 on the CPU); entries
without a term must be exact zeros; no entry is left out.  Every "same bits" is `torch.equal`.  The fused epilogues claim
the arithmetic and the summation order of `blend_forward_kernel`: their `image` and `wsum` must be its bits, at every K and C.
Each test prints the largest observed |err| / A relative to the bar.

Measured on an MI355X, the worst entry of any case as a fraction of its bar (image / weight sum); the bars are 5e-7 ... 4e-6:

    ops.blend_forward                              0.27 (frag_k3_c5)     0.27 (frag_k5_c3)
    dss_splat_fine_blend, whole-cloud scan         0.25 (splat_k4_c3)    0.22 (splat_k3_c3)
    dss_splat_fine_blend, behind dss_splat_bin     0.25 (splat_k4_c3)    0.22 (splat_k3_c3)
    ops.render_forward, packed records             0.32 (teapot_k1_c3)   0.23 (teapot_k3_c3)
    ops.render_forward, per-point arrays           0.26 (teapot_k5_c5)   0.22 (teapot_k5_c5)
    ops.render_forward, lean workspace             0.24 (teapot_k5_c3)   0.22 (teapot_k5_c3)

(the smallest worst entry of a case is 0.08 of its bar), and every bit identity held: both epilogues against
`blend_forward_kernel` at every K and C, the lean mode, both cloud layouts, the bands and the strided output.
Measured once against two side builds of the library: with -0.7213 for -0.72134752 in `ewa_weight` every test here fails
but the four refusals; with a floor of 1e-5 in the per-point-array epilogue alone exactly the tests that run it fail (all 64
of `dss_splat_fine_blend`, the seven non-packed (K, C) of both camera scenes and the lean variant at K = 5), the rest pass.
"""
import numpy as np
import pytest
import torch

import blend_reference as br
from dss_amd import _lib, ops
from dss_amd.distributed import RowPartition

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEV_T = torch.device(DEV)
SENTINEL = -777.0


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the arrays of a case are read-only)


def _hold(tag, name, img, wsum, r):
    """image and weight sum against a reference of the case's bars -> the two violation ratios (<= 1 asserted)"""
    bars = br.BARS[name]
    v_img, v_wsum = br.violation(img, r.img, r.img_A, bars["img"]), br.violation(wsum, r.wsum, r.wsum_A, bars["wsum"])
    print("blend %-28s %-16s worst entry / bar: img %.3f  wsum %.3f" % (tag, name, v_img, v_wsum))
    assert v_img <= 1 and v_wsum <= 1, (tag, name, v_img, v_wsum)
    return v_img, v_wsum


def _reference_of_fragments(c, idx, qv, occ, scaler):
    """the fp64 reference of the fragments a call returned (pinned elsewhere): this isolates the blend"""
    return br.reference(idx.cpu().numpy(), qv.cpu().numpy(), occ.cpu().numpy(), scaler.cpu().numpy(), c.feat)


@pytest.mark.parametrize("name", br.FRAGMENT_CASES + br.GOLDEN_CASES)
def test_blend_forward_against_fp64(name):
    c, r = br.case(name), br.ref(name)
    idx, qv, occ, scaler, feat = _t(c.idx), _t(c.qv), _t(c.occ), _t(c.scaler), _t(c.feat)
    img, wsum = ops.blend_forward(idx, qv, occ, scaler, feat, return_wsum=True)
    _hold("blend_forward", name, img, wsum, r)
    assert torch.equal(img[..., c.C], occ)
    empty = ~(idx >= 0).any(-1)
    assert int(empty.sum()) > 0 or c.kind == "golden"
    assert not bool(img[empty][:, :c.C].any()) and bool((wsum[empty] == float(br.FLOOR)).all())
    assert torch.equal(ops.blend_forward(idx, qv, occ, scaler, feat), img)
    img2, wsum2 = ops.blend_forward(idx, qv, occ, scaler, feat, return_wsum=True)
    assert torch.equal(img2, img) and torch.equal(wsum2, wsum)


# ---- dss_splat_fine_blend ------------------------------------------------------------------------------------------------
def _fine_blend(d, K, C, rows=None, workspace=False, scaler="scaler", feat="feat", K_lists=None):
    """`dss_splat_fine_blend` (include/dss_hip.h) on the device tensors ``d`` of a splat scene -> idx, zbuf, qvalue, occupancy,
    visible, image, wsum; ``workspace``: behind `dss_splat_bin` on a tile workspace, else the whole-cloud scan per tile"""
    N, P, S = d["first"].shape[0], d["points"].shape[0], d["S"]
    row0, row1 = (0, S) if rows is None else rows
    nr, Kl = row1 - row0, K if K_lists is None else K_lists
    e = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=DEV)
    idx, zbuf, qv, occ = e(N, nr, S, Kl, dtype=torch.int32), e(N, nr, S, Kl), e(N, nr, S, Kl), e(N, nr, S)
    vis = torch.zeros(P, dtype=torch.uint8, device=DEV)
    image, wsum = e(N, nr, S, max(C, 1) + 1), e(N, nr, S)
    ws, nbytes = None, 0
    if workspace:
        nbytes = _lib.load().dss_splat_forward_workspace(N, P, S, K, 1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.call("dss_splat_bin", DEV_T, d["points"], d["radii"], d["first"], d["num"], N, P, S, row0, row1, ws, nbytes)
    _lib.call("dss_splat_fine_blend", DEV_T, d["points"], d["ellipse"], d["cutoff"], d["radii"], d["first"], d["num"], N, P,
              float(d["thr"]), S, K, row0, row1, idx, zbuf, qv, occ, vis, d[scaler], d[feat], C, image, wsum, ws, nbytes)
    return idx, zbuf, qv, occ, vis.view(torch.bool), image, wsum


def _splat_dev(c):
    sc = c.scene
    d = {k: _t(sc[k]) for k in ("points", "ellipse", "cutoff", "radii", "scaler")}
    d.update(first=_t(sc["first_idx"]), num=_t(sc["num_pts"]), feat=_t(c.feat), S=c.S, thr=sc["thr"], none=None)
    return d


@pytest.mark.parametrize("workspace", [False, True], ids=["scan", "binned"])
@pytest.mark.parametrize("name", br.SPLAT_CASES)
def test_splat_fine_blend_against_fp64(name, workspace):
    c = br.case(name)
    d = _splat_dev(c)
    idx, zbuf, qv, occ, vis, image, wsum = _fine_blend(d, c.K, c.C, workspace=workspace)
    want = ops.splat_points(d["points"], d["ellipse"], d["cutoff"], d["radii"], d["first"], d["num"], d["thr"], c.S, c.K,
                            None if workspace else 0, None, return_visible=True)
    for k, got, w_ in zip(("idx", "zbuf", "qvalue", "occupancy", "visible"), (idx, zbuf, qv, occ, vis), want):
        assert torch.equal(got, w_), (name, k)
    assert int((idx >= 0).all(-1).sum()) >= 100             # lists that are full: every slot of this KMAX sums
    _hold("fine_blend " + ("binned" if workspace else "scan"), name, image, wsum, _reference_of_fragments(c, idx, qv, occ, d["scaler"]))
    img, ws_ = ops.blend_forward(idx, qv, occ, d["scaler"], d["feat"], return_wsum=True)
    assert torch.equal(image, img) and torch.equal(wsum, ws_), "the fused epilogue must give blend_forward_kernel's bits"
    band = _fine_blend(d, c.K, c.C, rows=(8, 32), workspace=workspace)
    for k, got, full in zip(("idx", "zbuf", "qvalue", "occupancy"), band[:4], (idx, zbuf, qv, occ)):
        assert torch.equal(got, full[:, 8:32]), (name, k)
    assert torch.equal(band[5], image[:, 8:32]) and torch.equal(band[6], wsum[:, 8:32])


@pytest.mark.parametrize("what", ["K=33", "C=0", "C=9", "NULL scaler"])
def test_splat_fine_blend_refusals(what):
    c = br.case("splat_k8_c3")
    d = _splat_dev(c)
    d["feat9"] = torch.zeros((c.P, 9), device=DEV)
    kw = {"K=33": dict(K=33, C=3), "C=0": dict(K=8, C=0), "C=9": dict(K=8, C=9, feat="feat9"),
          "NULL scaler": dict(K=8, C=3, scaler="none")}[what]
    with pytest.raises(RuntimeError, match="dss_splat_fine_blend"):
        _fine_blend(d, K_lists=33, **kw)
    torch.cuda.synchronize()


# ---- ops.render_forward -------------------------------------------------------------------------------------------------
def _render(c, shared=True, **kw):
    w = c.scene
    N, Pw = c.N, w["world"].shape[0]
    world, normals = (w["world"], w["normals"]) if shared else (np.tile(w["world"], (N, 1)), np.tile(w["normals"], (N, 1)))
    first = torch.arange(N, device=DEV) * Pw
    num = torch.full((N,), Pw, device=DEV, dtype=torch.int64)
    full = lambda v: torch.full((N,), float(v), device=DEV)
    return ops.render_forward(_t(world), _t(normals), full(w["h"]), _t(w["M"]), _t(w["V"]), full(w["znear"]), full(w["zfar"]), first, num,
                              _t(c.feat), c.S, c.K, w["cutoff"], w["thr"], 1.0, False, shared, **kw)


def _same_image(a, b, what):
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["wsum"], b["wsum"]), what


@pytest.mark.parametrize("K,C", br.CAMERA_KC)
@pytest.mark.parametrize("which", ["teapot", "grazing"])
def test_render_forward_against_fp64(which, K, C):
    name = br.camera_name(which, K, C)
    c = br.case(name)
    f = _render(c)
    assert int(f["occupancy"].sum()) >= 100
    if which == "grazing":
        below = int(((f["wsum"] == float(br.FLOOR)) & (f["occupancy"] > 0)).sum())
        assert below >= 10 and int((f["wsum"] > float(br.FLOOR)).sum()) >= 10
    packed = K <= 8 and C == 3
    _hold("render_forward " + ("packed" if packed else "non-packed"), name, f["image"], f["wsum"],
          _reference_of_fragments(c, f["idx"], f["qvalue"], f["occupancy"], f["scaler"]))
    assert torch.equal(f["image"][..., C], f["occupancy"])
    img, wsum = ops.blend_forward(f["idx"], f["qvalue"], f["occupancy"], f["scaler"], _t(c.feat), return_wsum=True)
    assert torch.equal(f["image"], img) and torch.equal(f["wsum"], wsum), "the fused epilogue must give blend_forward_kernel's bits"
    if (K, C) not in ((5, 3), (12, 3)):
        return
    # the variants of the call: the same image and weight sum, bit for bit
    ref0 = _render(c, workspace_state=0)
    _same_image(ref0, f, "workspace_state 0")
    _lib.set_option(_lib.OPT_LEAN_WORKSPACE, 1)
    try:
        lean = _render(c, workspace_state=0)
    finally:
        _lib.set_option(_lib.OPT_LEAN_WORKSPACE, 0)
    _hold("render_forward lean", name, lean["image"], lean["wsum"],
          _reference_of_fragments(c, lean["idx"], lean["qvalue"], lean["occupancy"], lean["scaler"]))
    _same_image(lean, f, "DSS_OPT_LEAN_WORKSPACE")
    _same_image(_render(c, shared=False), f, "shared_cloud=False")
    S = c.S
    for part in (RowPartition(S, 4, 1), RowPartition(S, 4, 2, cyclic=True)):
        own = torch.tensor(part.row_indices(), device=DEV, dtype=torch.int64)
        fb = _render(c, rows=part.rows)
        assert torch.equal(fb["image"], f["image"][:, own]) and torch.equal(fb["wsum"], f["wsum"][:, own]), part.describe()
        _same_image(_render(c, rows=part.rows, band_outputs_only=True), fb, "band_outputs_only " + part.describe())
    # out_image: a strided view of a larger caller-owned buffer
    for rows, dense in ((None, f), (RowPartition(S, 4, 1).rows, _render(c, rows=RowPartition(S, 4, 1).rows))):
        nr = dense["image"].shape[1]
        buf = torch.full((nr + 3, c.N, S, C + 1), SENTINEL, device=DEV)
        view = buf[:nr].permute(1, 0, 2, 3)
        got = _render(c, rows=rows, out_image=view)
        assert got["image"].data_ptr() == buf.data_ptr()
        assert torch.equal(view, dense["image"]) and torch.equal(got["wsum"], dense["wsum"])
        assert bool((buf[nr:] == SENTINEL).all())
