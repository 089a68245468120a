"""CPU: the two things tests/test_gpu_forward_workspace.py leans on, checked without a GPU.

1. The layout mirror of tests/forward_workspace.py against the library's size queries (they run on the CPU): the zero region
   equals dss_splat_forward_clean_bytes, the total without records dss_splat_forward_workspace(bin_size=1), the total with
   records dss_render_forward_workspace -- exactly, over a grid of (N, P, S) that holds every shape of the GPU module, sides
   that are no multiple of 8, P at either side of 65,536 / 8 (the pool's floor) and of 2,000,000 (the cell-ordered binning's
   arrays), and both values of DSS_OPT_LEAN_WORKSPACE.  The lists (tiles x 8 x cap words) dominate the total and cap is a power
   of two, so an exact match pins cap.
2. The scenes: every scene of the GPU module, run through the oracle's point setup and the class prover, reaches the class its
   test names as the widest one, cannot reach a wider one, and shows the minimum counts (8 over-full sub-lists of the class's
   splat width, a tile that mixes a full and a partly filled sub-list, 64 empty tiles, 64 occupied tiles without overflow)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref_loop"))
import forward_workspace as fw  # noqa: E402
import oracle_ops  # noqa: E402
from dss_amd import _lib  # noqa: E402

GRID_N = (1, 2, 4, 16, 17)
GRID_S = (64, 100, 128, 129, 250, 512)
GRID_P = (1, 255, 3000, 3490, 6178, 6365, 8191, 8192, 8193, 99_790, 1_999_999, 2_000_000, 2_000_001, 2_000_101)


@pytest.mark.parametrize("lean", [0, 1])
def test_layout_mirror_equals_the_size_queries(lean):
    lib = _lib.load()
    old = _lib.set_option(_lib.OPT_LEAN_WORKSPACE, lean)
    try:
        for N in GRID_N:
            for S in GRID_S:
                for P in GRID_P:
                    plain, rec = fw.layout(N, P, S, lean), fw.layout(N, P, S, lean, with_records=True)
                    assert plain.clean_bytes == rec.clean_bytes == lib.dss_splat_forward_clean_bytes(N, P, S), (N, P, S)
                    assert plain.total == lib.dss_splat_forward_workspace(N, P, S, 5, 1), (N, P, S)
                    assert rec.total == lib.dss_render_forward_workspace(N, P, S, 5), (N, P, S)
    finally:
        _lib.set_option(_lib.OPT_LEAN_WORKSPACE, old)


def test_layout_regions_are_in_the_order_of_the_contract():
    lay = fw.layout(1, 3000, 128, with_records=True)
    names = list(lay.regions)
    assert names[:7] == ["counts", "cursor", "offset", "flag", "tail+ctrl", "queue.list", "mask"]
    assert lay.regions["lists"][0] == lay.clean_bytes and all(off % 256 == 0 for off, _ in lay.regions.values())
    assert (lay.cap, lay.spill_cap, lay.giant_cap, lay.capq) == (64, 65536, 1024, 16)
    assert "sort_id" not in lay.regions and "sort_id" in fw.layout(3, 2_000_101, 128, with_records=True).regions
    lean = fw.layout(1, 3000, 128, lean=True, with_records=True)
    assert lean.cap == 32 and "big" not in lean.regions and "rec" not in lean.regions and lean.clean_bytes == lay.clean_bytes


def _setup(s):
    t = s.tensors("cpu")
    return oracle_ops.point_setup(t["world"], t["normals"], t["h"], t["M"], t["V"], t["znear"], t["zfar"], t["first"], t["num"],
                                  s.S, fw.CUTOFF, fw.SIGMA)


@pytest.mark.parametrize("shape", list(fw.SHAPES))
@pytest.mark.parametrize("cls", fw.CLASSES)
def test_every_scene_reaches_its_class(cls, shape):
    s = fw.scene(cls, shape)
    o = _setup(s)
    pr = fw.prove(o["pts_screen"].numpy(), o["radii"].numpy(), o["valid"].numpy(), s.first, s.num, s.S, lean=cls == "e3")
    print(fw.check_minimum(pr, cls, shape))
    if s.N > 2:      # ragged clouds: one empty, one all culled, points that belong to no cloud
        v = o["valid"].numpy()
        assert s.num[1] == 0 and not v[s.first[-1]: s.first[-1] + s.num[-1]].any() and s.P > int(s.num.sum())
    assert len({fw.scene(c, shape).P for c in fw.CLASSES}) == 1          # the sequences keep (N, P, S)


@pytest.mark.parametrize("cls", ["b", "c", "d"])
def test_moved_cluster_keeps_its_class(cls):
    s = fw.scene(cls, "S128-N1", move=2)
    o = _setup(s)
    fw.check_minimum(fw.prove(o["pts_screen"].numpy(), o["radii"].numpy(), o["valid"].numpy(), s.first, s.num, s.S), cls)
