"""GPU: the render backward's gather -- `ops.render_backward` (`render_backward_kernel`, `csrc/raster_backward.hip`) on
every launch form, addressing, dealing and band path, and the unfused entries `ops.splat_backward`, `ops.occ_backward` and
`ops.blend_backward` -- against the fp64 reference of `tests/gather_reference.py`, entry by entry.

Error bookkeeping: every entry of `grad_pts` and `grad_features` is compared with its fp64 value RELATIVE TO ``A`` = the sum
of the absolute terms of that entry (`gather_reference`'s header), ``|got - ref| <= bar * A + UNDERFLOW``; entries without a
term (invisible points, rows between the clouds and beyond them, off-screen points in `grad_pts`, a cloud with rs = 0, the z
column) must be exact zeros.  No entry is left out: the pairs that take part are decided in fp32 exactly as the reference
method decides them, so a kernel decision that differs shows as an error of a whole term, four orders of magnitude beyond a
bar (`tests/test_gather_reference_cpu.py`: nineteen wrong formulas, each at least 10 x beyond).  rs must be the reference's
bits.  Each test prints the largest observed ratio per output.

The bars (`gather_reference.BARS`): for every case the same formulas ran in plain fp32 on the CPU, every operation rounded
and the sums sequential, against fp64; a bar is 4 x that figure rounded up to one significant digit (the kernels' summation
order, their reciprocal, their exp2 and their fused multiply-adds differ from numpy's by a few ulp per term).  The inputs of
a case (fragments, weight sums, visible flags, image gradient) are made on the CPU, the same for both tests.  Measured once
on an MI355X against two side builds of the gather: with `>=` for `>` at the radius exactly the `tie` and `bench512` tests
fail, on every path; with -0.7213 for -0.72134752 every test of the fused entry fails.

fp32 restatement on the CPU / bar / kernel on an MI355X, largest |err| / A per output (grad_pts: the largest of the runs with
the forward's weight sums, with wsum = None and, on the default path, without features):

    case           path                         grad_pts                 grad_features            grad_features, wsum = None
    pow2           default                      3.7e-07/2e-06/2.0e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    pow2_loss      default                      4.0e-07/2e-06/1.6e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    tie            default                      1.5e-07/7e-07/1.7e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    odd37          default                      2.5e-07/1e-06/1.5e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd37_whole    default                      6.2e-07/3e-06/1.0e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         default                      2.7e-07/2e-06/1.5e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    wide           default                      2.9e-07/2e-06/4.0e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    tiny           default                      1.5e-07/7e-07/1.7e-07    2.3e-07/1e-06/1.9e-07    1.8e-07/8e-07/1.8e-07
    depth_k1c1     default                      1.7e-07/7e-07/1.4e-07    1.5e-07/6e-07/1.5e-07    1.2e-07/5e-07/1.2e-07
    depth_k8c5     default                      2.1e-07/9e-07/1.3e-07    2.0e-07/9e-07/1.9e-07    2.3e-07/1e-06/2.1e-07
    depth_k9c8     default                      1.9e-07/8e-07/1.1e-07    2.4e-07/1e-06/1.7e-07    2.4e-07/1e-06/1.9e-07
    depth_k12c3    default                      2.3e-07/1e-06/1.2e-07    2.3e-07/1e-06/1.6e-07    2.3e-07/1e-06/1.7e-07
    nowsum         default                      3.1e-07/2e-06/1.8e-07    4.1e-07/2e-06/2.1e-07    3.7e-07/2e-06/2.1e-07
    ragged         default                      3.6e-07/2e-06/8.9e-08    2.0e-07/9e-07/1.5e-07    2.0e-07/8e-07/2.0e-07
    ragged_flags   default                      3.2e-07/2e-06/8.9e-08    2.0e-07/9e-07/1.5e-07    1.8e-07/8e-07/1.7e-07
    clip_all       default                      7.0e-08/3e-07/7.4e-08    2.1e-07/9e-07/1.5e-07    2.3e-07/1e-06/1.9e-07
    clip_none      default                      1.0e-07/5e-07/9.5e-08    2.1e-07/9e-07/1.5e-07    2.3e-07/1e-06/1.9e-07
    clip_median    default                      1.0e-07/5e-07/9.2e-08    2.1e-07/9e-07/1.5e-07    2.3e-07/1e-06/1.9e-07
    band96         default                      2.6e-07/2e-06/1.2e-07    2.5e-07/2e-06/2.1e-07    2.5e-07/2e-06/2.1e-07
    band100        default                      2.8e-07/2e-06/1.2e-07    2.4e-07/1e-06/2.0e-07    2.3e-07/1e-06/1.8e-07
    long           default                      2.9e-07/2e-06/1.5e-07    2.0e-07/9e-07/1.4e-07    2.0e-07/8e-07/1.4e-07
    bench512       default                      2.2e-07/9e-07/6.4e-08    2.3e-07/1e-06/2.1e-07    2.8e-07/2e-06/2.9e-07
    pow2           tpw0                         3.7e-07/2e-06/2.0e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           tpw0                         2.9e-07/2e-06/4.0e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          tpw0                         2.5e-07/1e-06/1.5e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         tpw0                         2.7e-07/2e-06/1.5e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            tpw0                         1.5e-07/7e-07/1.7e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    pow2           tpw1                         3.7e-07/2e-06/2.0e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           tpw1                         2.9e-07/2e-06/4.0e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          tpw1                         2.5e-07/1e-06/1.5e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         tpw1                         2.7e-07/2e-06/1.5e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            tpw1                         1.5e-07/7e-07/1.7e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    pow2           tpw2                         3.7e-07/2e-06/1.9e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           tpw2                         2.9e-07/2e-06/9.9e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          tpw2                         2.5e-07/1e-06/2.5e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         tpw2                         2.7e-07/2e-06/2.2e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            tpw2                         1.5e-07/7e-07/1.7e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    pow2           tpw4                         3.7e-07/2e-06/1.6e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           tpw4                         2.9e-07/2e-06/5.7e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          tpw4                         2.5e-07/1e-06/1.7e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         tpw4                         2.7e-07/2e-06/1.9e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            tpw4                         1.5e-07/7e-07/1.6e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    pow2           fused5                       3.7e-07/2e-06/2.0e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           fused5                       2.9e-07/2e-06/4.0e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          fused5                       2.5e-07/1e-06/1.5e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         fused5                       2.7e-07/2e-06/1.5e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            fused5                       1.5e-07/7e-07/1.7e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    pow2           fused1                       3.7e-07/2e-06/2.0e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           fused1                       2.9e-07/2e-06/4.0e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          fused1                       2.5e-07/1e-06/1.5e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         fused1                       2.7e-07/2e-06/1.5e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            fused1                       1.5e-07/7e-07/1.7e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    pow2           addr64                       3.7e-07/2e-06/1.6e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           addr64                       2.9e-07/2e-06/5.7e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          addr64                       2.5e-07/1e-06/1.7e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         addr64                       2.7e-07/2e-06/1.9e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            addr64                       1.5e-07/7e-07/1.6e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    pow2           grid                         3.7e-07/2e-06/2.0e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           grid                         2.9e-07/2e-06/4.0e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          grid                         2.5e-07/1e-06/1.5e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         grid                         2.7e-07/2e-06/1.5e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            grid                         1.5e-07/7e-07/1.7e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    pow2           grid_tpw1                    3.7e-07/2e-06/2.0e-07    2.1e-07/9e-07/2.2e-07    2.1e-07/9e-07/1.9e-07
    wide           grid_tpw1                    2.9e-07/2e-06/4.0e-08    1.2e-07/5e-07/9.5e-08    1.2e-07/5e-07/8.8e-08
    odd37          grid_tpw1                    2.5e-07/1e-06/1.5e-07    1.8e-07/8e-07/1.6e-07    1.9e-07/8e-07/1.6e-07
    odd100         grid_tpw1                    2.7e-07/2e-06/1.5e-07    1.8e-07/8e-07/1.8e-07    1.9e-07/8e-07/1.8e-07
    tie            grid_tpw1                    1.5e-07/7e-07/1.7e-07    1.5e-07/7e-07/1.9e-07    1.6e-07/7e-07/1.7e-07
    band96         band, 2 contiguous           2.6e-07/2e-06/1.2e-07    2.5e-07/2e-06/2.1e-07    -
    band96         band, 12 contiguous          2.6e-07/2e-06/1.5e-07    2.5e-07/2e-06/2.1e-07    -
    band96         band, 4 tile-row-cyclic      2.6e-07/2e-06/1.6e-07    2.5e-07/2e-06/2.1e-07    -
    band100        band, 2 contiguous           2.8e-07/2e-06/1.2e-07    2.4e-07/1e-06/2.0e-07    -
    band100        band, 12 contiguous          2.8e-07/2e-06/1.5e-07    2.4e-07/1e-06/2.0e-07    -
    band100        band, 4 tile-row-cyclic      2.8e-07/2e-06/1.6e-07    2.4e-07/1e-06/2.0e-07    -
    band96         owner mode contiguous image  2.6e-07/2e-06/1.2e-07    -                        -
    band96         owner mode contiguous plane  2.6e-07/2e-06/1.2e-07    -                        -
    band96         owner mode cyclic image      2.6e-07/2e-06/1.2e-07    -                        -
    band96         owner mode cyclic plane      2.6e-07/2e-06/1.2e-07    -                        -
    band100        owner mode contiguous image  2.8e-07/2e-06/1.2e-07    -                        -
    band100        owner mode contiguous plane  2.8e-07/2e-06/1.2e-07    -                        -
    band100        owner mode cyclic image      2.8e-07/2e-06/1.2e-07    -                        -
    band100        owner mode cyclic plane      2.8e-07/2e-06/1.2e-07    -                        -
    the other two band filters (`band_filter_kernel` with DSS_OPT_BACKWARD_FUSED = 1; `cell_hist_kernel` on `long`, bands
    (0, 104, 256) and cyclic of 4, the case's whole-image bars), largest figure over the bands:
    band96         fused1, 2 + 12 contiguous    2.6e-07/2e-06/1.5e-07    2.5e-07/2e-06/2.1e-07    -
    band96         fused1, 4 tile-row-cyclic    2.6e-07/2e-06/1.5e-07    2.5e-07/2e-06/2.1e-07    -
    band100        fused1, 2 + 12 contiguous    2.8e-07/2e-06/1.5e-07    2.4e-07/1e-06/2.0e-07    -
    band100        fused1, 4 tile-row-cyclic    2.8e-07/2e-06/1.5e-07    2.4e-07/1e-06/2.0e-07    -
    band96/100     fused1, owner mode (all 8)   2.8e-07/2e-06/1.2e-07    -                        -
    long           band, 2 contiguous           2.9e-07/2e-06/1.5e-07    2.0e-07/9e-07/1.6e-07    -
    long           band, 4 tile-row-cyclic      2.9e-07/2e-06/2.1e-07    2.0e-07/9e-07/1.8e-07    -
    long           owner mode (all 4)           2.9e-07/2e-06/1.5e-07    -                        -
    (`ops.backward_radius` on `long`, the only user of `median_hist_kernel<0>`: the reference's bits.)

    the unfused entries (test_unfused_entries_against_fp64): fp32 / bar / kernel
    case           splat_backward           + grad_zbuf: xy          + grad_zbuf: z           + grad_zbuf + clip 0.05
    pow2           3.7e-07/2e-06/2.0e-07    3.7e-07/2e-06/2.0e-07    1.5e-07/7e-07/1.3e-07    8.6e-08/4e-07/6.6e-08
    odd37          2.5e-07/1e-06/1.5e-07    2.5e-07/1e-06/1.5e-07    1.1e-07/5e-07/7.4e-08    8.6e-08/4e-07/6.2e-08
    odd100         2.7e-07/2e-06/1.9e-07    2.7e-07/2e-06/1.9e-07    1.2e-07/5e-07/1.7e-07    7.6e-08/4e-07/7.6e-08
    wide           2.9e-07/2e-06/4.6e-08    2.9e-07/2e-06/4.6e-08    7.9e-08/4e-07/6.0e-08    9.2e-08/4e-07/1.5e-08
    depth_k1c1     1.7e-07/7e-07/1.4e-07    1.7e-07/7e-07/1.4e-07    8.0e-08/4e-07/1.1e-07    8.1e-08/4e-07/4.6e-08
    depth_k8c5     2.1e-07/9e-07/1.4e-07    2.1e-07/9e-07/1.4e-07    1.2e-07/5e-07/1.1e-07    9.0e-08/4e-07/4.2e-08
    depth_k9c8     1.9e-07/8e-07/1.2e-07    1.9e-07/8e-07/1.2e-07    1.1e-07/5e-07/1.2e-07    6.6e-08/3e-07/4.0e-08
    depth_k12c3    2.3e-07/1e-06/1.2e-07    2.3e-07/1e-06/1.2e-07    1.3e-07/6e-07/1.1e-07    5.8e-08/3e-07/4.9e-08
    bench512       2.2e-07/9e-07/1.4e-07    2.2e-07/9e-07/1.4e-07    1.4e-07/6e-07/1.6e-07    2.2e-07/9e-07/6.8e-08
    case           occ_backward             blend scatter            blend gather             blend gather + wsum
    pow2           3.7e-07/2e-06/2.0e-07    2.1e-07/9e-07/1.9e-07    2.1e-07/9e-07/1.9e-07    2.1e-07/9e-07/2.2e-07
    odd37          2.5e-07/1e-06/1.5e-07    1.9e-07/8e-07/1.4e-07    1.9e-07/8e-07/1.6e-07    1.8e-07/8e-07/1.6e-07
    odd100         2.7e-07/2e-06/1.9e-07    1.9e-07/8e-07/2.0e-07    1.9e-07/8e-07/1.8e-07    1.8e-07/8e-07/1.8e-07
    wide           2.9e-07/2e-06/4.6e-08    1.2e-07/5e-07/1.6e-07    1.2e-07/5e-07/7.8e-08    1.2e-07/5e-07/9.5e-08
    depth_k1c1     1.7e-07/7e-07/1.4e-07    1.2e-07/5e-07/1.2e-07    1.2e-07/5e-07/1.2e-07    1.5e-07/6e-07/1.5e-07
    depth_k8c5     2.1e-07/9e-07/1.4e-07    2.3e-07/1e-06/1.9e-07    2.3e-07/1e-06/2.1e-07    2.0e-07/9e-07/1.9e-07
    depth_k9c8     1.9e-07/8e-07/1.2e-07    2.4e-07/1e-06/2.3e-07    2.4e-07/1e-06/1.9e-07    2.4e-07/1e-06/1.9e-07
    depth_k12c3    2.3e-07/1e-06/1.2e-07    2.3e-07/1e-06/2.1e-07    2.3e-07/1e-06/1.7e-07    2.3e-07/1e-06/1.6e-07
    bench512       2.2e-07/9e-07/1.4e-07    2.8e-07/2e-06/2.4e-07    2.8e-07/2e-06/2.9e-07    2.3e-07/1e-06/2.1e-07

The kernel figure nearest its bar: the z column of `ops.splat_backward` on odd100, 1.7e-07 against 5e-07 (0.34 of the bar);
the kernel figures span 1.5e-08 ... 2.9e-07.
No decision of a kernel differed from the reference's on any case or path, and rs had the reference's bits everywhere.
"""
import contextlib

import numpy as np
import pytest
import torch

import gather_reference as gr
from dss_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_CASES = ("pow2", "wide", "odd37", "odd100", "tie")
UNFUSED_CASES = ("pow2", "odd37", "odd100", "wide", "depth_k1c1", "depth_k8c5", "depth_k9c8", "depth_k12c3", "bench512")
_OPTIONS = dict(tpw=_lib.OPT_BACKWARD_TPW, fused=_lib.OPT_BACKWARD_FUSED, addr64=_lib.OPT_BACKWARD_ADDR64, grid=_lib.OPT_BACKWARD_GRID)
PATHS = {
    "tpw0": dict(tpw=0), "tpw1": dict(tpw=1), "tpw2": dict(tpw=2), "tpw4": dict(tpw=4),
    "fused5": dict(fused=5),          # medians in a launch of their own
    "fused1": dict(fused=1),          # the round-3 launch sequence
    "addr64": dict(addr64=1),
    "grid": dict(grid=8),             # N + 8 workgroups: the groups are dealt over several rounds, the last one is claimed
    "grid_tpw1": dict(grid=8, tpw=1),
}
_DEVICE = {}


@contextlib.contextmanager
def _options(N, **kw):
    try:
        for k, v in kw.items():
            _lib.set_option(_OPTIONS[k], N + v if k == "grid" else v)
        yield
    finally:
        for k in _OPTIONS:
            _lib.set_option(_OPTIONS[k], 0)


def _dev(name):
    """the case's tensors on the device, uploaded once"""
    if name not in _DEVICE:
        c = gr.case(name)
        t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
        _DEVICE[name] = dict(go=t(c.grad_out), idx=t(c.idx), qv=t(c.qv), wsum=t(c.wsum), scaler=t(c.scaler), pts=t(c.pts),
                             radii=t(c.radii), vis=t(c.vis.astype(np.uint8)), first=t(c.first), num=t(c.num), gz=t(c.grad_zbuf))
    return _DEVICE[name]


def _render(name, band=None, use_wsum=True, clip=None, **kw):
    """`ops.render_backward` of a case; ``band`` = (`rows` argument, image rows): the band's tensors are cut from the whole"""
    c, d = gr.case(name), _dev(name)
    cut = (lambda t: t) if band is None else (lambda t: t[:, torch.tensor(band[1], device=DEV)].contiguous())
    return ops.render_backward(cut(d["go"]), cut(d["idx"]), cut(d["qv"]), cut(d["wsum"]) if use_wsum else None, d["scaler"],
                               d["pts"], d["radii"], d["vis"], d["first"], d["num"], c.radii_s, c.clip if clip is None else clip,
                               image_size=c.S, rows=None if band is None else band[0], **kw)


def _ratio(tag, out_name, got, ref, A, bar):
    """the per-entry check of every comparison here -> the largest (|got - ref| - UNDERFLOW) / A"""
    worst, zeros_ok = gr.ratio(got, ref, A)
    assert zeros_ok, "%s %s: entries without a term must be exact zeros" % (tag, out_name)
    assert worst <= bar, (tag, out_name, worst, bar)
    return worst


def _check(tag, name, gf, gp, ref, feat_key="feat"):
    bars = gr.BARS[name]
    line = "pts %.1e (bar %.0e)" % (_ratio(tag, "grad_pts", gp, ref.pts, ref.pts_A, bars["pts"]), bars["pts"])
    if gf is not None:
        line += "  %s %.1e (bar %.0e)" % (feat_key, _ratio(tag, "grad_features", gf, ref.feat, ref.feat_A, bars[feat_key]), bars[feat_key])
    print("gather %-44s max |err| / A: %s" % (tag, line))


@pytest.mark.parametrize("name", gr.CASES)
def test_cases_against_fp64(name):
    """the default launch of every case, with the forward's weight sums and with wsum = None (recomputed and clamped), and
    without features"""
    c = gr.case(name)
    ref = gr.reference(name)
    gf, gp, rs = _render(name, return_rs=True)
    assert np.array_equal(rs.cpu().numpy(), ref.rs), "the search radius must have the reference's bits"
    _check(name, name, gf, gp, ref)
    gf, gp = _render(name, use_wsum=False)
    _check(name + " wsum=None", name, gf, gp, gr.reference(name, use_wsum=False), "feat_nowsum")
    gf, gp = _render(name, with_features=False)
    assert gf is None
    _check(name + " no features", name, None, gp, ref)
    owned = np.zeros(c.P, bool)
    for lo, n in zip(c.first, c.num):
        owned[lo:lo + n] = True
    assert not bool(gp[torch.from_numpy(~owned | ~c.vis.astype(bool)).to(DEV)].any())


@pytest.mark.parametrize("name", PATH_CASES)
@pytest.mark.parametrize("path", list(PATHS))
def test_paths_against_fp64(path, name):
    """tasks per wavefront, launch form, 64-bit addressing and a capped persistent grid: the same reference, the same bars"""
    c = gr.case(name)
    with _options(c.N, **PATHS[path]):
        gf, gp = _render(name)
        gf2, gp2 = _render(name, use_wsum=False)
    _check("%s %s" % (name, path), name, gf, gp, gr.reference(name))
    _check("%s %s wsum=None" % (name, path), name, gf2, gp2, gr.reference(name, use_wsum=False), "feat_nowsum")


@pytest.mark.parametrize("name", UNFUSED_CASES)
def test_unfused_entries_against_fp64(name):
    """`ops.splat_backward` without and with grad_zbuf (the z column is the sum over the point's fragments, A = sum |grad_zbuf|;
    the clip then acts on the 3-vector), `ops.backward_radius` + `ops.occ_backward`, and `ops.blend_backward` in its scatter,
    gather and gather + wsum forms"""
    c, d, bars = gr.case(name), _dev(name), gr.BARS[name]
    geom = (d["pts"], d["radii"], d["vis"], d["first"], d["num"])
    gocc = d["go"][..., c.C]

    def hold(entry, got, ref, A, key):
        print("unfused %-12s %-18s max |err| / A: %.1e (bar %.0e)" % (name, entry, _ratio(name, entry, got, ref, A, bars[key]), bars[key]))

    def splat(grad_zbuf, clip):
        return ops.splat_backward(d["pts"], d["radii"], d["vis"], d["idx"], gocc, grad_zbuf, d["first"], d["num"], c.radii_s, clip)
    ref = gr.reference(name, clip=-1.0)
    hold("splat", splat(None, -1.0), ref.pts, ref.pts_A, "pts")
    rz, g = gr.reference(name, with_z=True, clip=-1.0), splat(d["gz"], -1.0)
    hold("splat+z xy", g[:, :2], rz.pts[:, :2], rz.pts_A[:, :2], "pts")
    hold("splat+z z", g[:, 2], rz.pts[:, 2], rz.pts_A[:, 2], "z")
    rc = gr.reference(name, with_z=True, clip=gr.CLIP3)
    hold("splat+z clip", splat(d["gz"], gr.CLIP3), rc.pts, rc.pts_A, "pts3_clip")
    rs = ops.backward_radius(d["radii"], d["vis"], d["first"], d["num"], c.radii_s)
    assert np.array_equal(rs.cpu().numpy(), ref.rs)
    hold("occ", ops.occ_backward(d["pts"], d["radii"], d["vis"], rs, gocc, d["first"], d["num"]), ref.pts, ref.pts_A, "pts")
    rn = gr.reference(name, use_wsum=False)
    blend = lambda **kw: ops.blend_backward(d["go"], d["idx"], d["qv"], d["scaler"], c.P, **kw)[0]
    hold("blend scatter", blend(), rn.feat, rn.feat_A, "feat_nowsum")
    hold("blend gather", blend(geometry=geom), rn.feat, rn.feat_A, "feat_nowsum")
    hold("blend gather+wsum", blend(geometry=geom, wsum=d["wsum"]), ref.feat, ref.feat_A, "feat")


def _row_bands(name, tag, **options):
    """every band of `gr.band_rows`: the band's partial gradients against the reference restricted to the band's rows"""
    c = gr.case(name)
    for label, rows_arg, rows in gr.band_rows(name):
        with _options(c.N, **options):
            gf, gp = _render(name, band=(rows_arg, rows))
        _check("%s %s%s" % (name, label, tag), name, gf, gp, gr.reference(name, tuple(rows)))


def _owner_mode(name, layout, plane, tag, **options):
    """owner mode of the two contiguous bands, or of the cyclic partition of 4 (the last four entries of `gr.band_rows`)"""
    c, d, whole = gr.case(name), _dev(name), gr.reference(name)
    bands = gr.band_rows(name)
    owners, total = torch.zeros(c.P, device=DEV), torch.zeros((c.P, 3), device=DEV)
    for label, rows_arg, rows in (bands[:2] if layout == "contiguous" else bands[-4:]):
        kw = dict(grad_occ_full=d["go"][..., c.C].contiguous()) if plane else dict(grad_out_full=d["go"])
        with _options(c.N, **options):
            gf, gp = _render(name, band=(rows_arg, rows), **kw)
        part = gr.reference(name, tuple(rows))
        _ratio("%s owner %s%s" % (name, label, tag), "grad_features", gf, part.feat, part.feat_A, gr.BARS[name]["feat"])
        owners += (gp != 0).any(dim=1).float()
        total += gp            # (zeros on every rank but the owner: the sum IS the owner's entry)
    has_term = torch.from_numpy((whole.pts_A > 0).any(1)).to(DEV)
    assert float(owners.max()) <= 1.0 and bool((owners[has_term] == 1).all())
    _check("%s owner mode %s %s%s" % (name, layout, "plane" if plane else "image", tag), name, None, total, whole)


@pytest.mark.parametrize("name", ["band96", "band100"])
def test_row_bands_against_fp64(name):
    """contiguous bands (0, 40, S), twelve bands of 8 rows and a tile-row-cyclic partition of 4: every band's partial
    gradients against the reference restricted to the band's rows, with the scale of those rows"""
    _row_bands(name, "")


@pytest.mark.parametrize("plane", [False, True], ids=["grad_out_full", "grad_occ_full"])
@pytest.mark.parametrize("layout", ["contiguous", "cyclic"])
@pytest.mark.parametrize("name", ["band96", "band100"])
def test_owner_mode_against_fp64(name, layout, plane):
    """owner mode of a band: every point has a non-zero position gradient on at most one rank, every point with A > 0 on
    exactly one, and that rank's entry is the WHOLE-image reference's at the whole-image bar; the feature gradients are the
    band's partial sums"""
    _owner_mode(name, layout, plane, "")


@pytest.mark.parametrize("name", ["band96", "band100"])
def test_row_bands_on_the_round3_filter_against_fp64(name):
    """the same bands, references and bars with DSS_OPT_BACKWARD_FUSED = 1: the list is filtered by `band_filter_kernel`
    behind `median_visible_kernel`, not inside the gather launch"""
    _row_bands(name, " fused1", fused=1)


@pytest.mark.parametrize("plane", [False, True], ids=["grad_out_full", "grad_occ_full"])
@pytest.mark.parametrize("layout", ["contiguous", "cyclic"])
@pytest.mark.parametrize("name", ["band96", "band100"])
def test_owner_mode_on_the_round3_filter_against_fp64(name, layout, plane):
    """owner mode with DSS_OPT_BACKWARD_FUSED = 1: `band_filter_kernel` keeps by the own box, the gather tests the owner"""
    _owner_mode(name, layout, plane, " fused1", fused=1)


def test_row_bands_on_the_long_list_filter_against_fp64():
    """`long` (P > 262,144, fewer than 5,000 visible points) in two contiguous bands and in a tile-row-cyclic partition of 4:
    the filter sits in `cell_hist_kernel`; the whole-image bars of the case.  (`tests/test_gather_reference_cpu.py`: every band
    drops visible points and keeps others, and the band references add up to the whole image.)"""
    _row_bands("long", "")


@pytest.mark.parametrize("plane", [False, True], ids=["grad_out_full", "grad_occ_full"])
@pytest.mark.parametrize("layout", ["contiguous", "cyclic"])
def test_owner_mode_on_the_long_list_filter_against_fp64(layout, plane):
    _owner_mode("long", layout, plane, "")


def test_long_list_radius_has_the_reference_bits():
    """`ops.backward_radius` above 262,144 points: the only user of `median_hist_kernel<0>`"""
    c, d = gr.case("long"), _dev("long")
    assert c.P > 262144
    rs = ops.backward_radius(d["radii"], d["vis"], d["first"], d["num"], c.radii_s)
    assert np.array_equal(rs.cpu().numpy(), gr.reference("long").rs)
