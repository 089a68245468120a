"""GPU: the per-point setup forward -- `setup_point_arith` (`csrc/setup_body.h`) through `ops.point_setup`
(`point_setup_kernel`, the per-lane camera lookup) and through `ops.render_forward` (`setup_bin_kernel`: the wave-uniform
lookup; above 2M points `setup_cell_kernel`, whose reuse form stores through `setup_wave_store`) -- against the fp64
reference of `tests/setup_reference.py`, entry by entry, off the teapot: normals of every length, zero and edge-on ones
among them, an orthographic-style and a mirrored camera, exact depth boundaries, every h mode, anisotropic frames whose
normal is not the cloud's.

Error bookkeeping: every entry of the screen position, the ellipse, the radii and the scaler is compared with its fp64 value
RELATIVE TO THE SCALE of that entry (`setup_reference`'s header: first-order propagation, so that the cancellation of detG
raises the scale instead of hiding behind an array maximum), ``|got - ref| <= bar * scale`` (+ `UNDERFLOW` = 1e-30
absolute); decisions are exact apart from the pairs the reference lists as within rounding of a threshold (none on these
cases); culled and unowned rows hold the defaults exactly.  The bars (`setup_reference.BARS`): 4 x what the same formula
loses in plain fp32 torch on the CPU, rounded up (`tests/test_setup_reference_cpu.py` re-measures them and shows that
fourteen wrong formulas lie beyond them).

fp32 torch on the CPU / bar / kernel on an MI355X, largest |err| / scale per output:

    case                                     screen                   ellipse                  radii                    scaler
    packed-h_cloud-nocull-S64                7.2e-08/3e-07/7.2e-08   5.2e-08/3e-07/5.2e-08   3.0e-08/2e-07/2.9e-08   5.0e-08/3e-07/4.4e-08
    packed-h_cloud-nocull-S1024              7.2e-08/3e-07/7.2e-08   5.5e-08/3e-07/5.5e-08   1.0e-08/4e-08/1.0e-08   4.2e-08/2e-07/4.6e-08
    packed-h_cloud-backface-S64              6.8e-08/3e-07/6.8e-08   5.2e-08/3e-07/5.2e-08   3.0e-08/2e-07/2.9e-08   5.0e-08/3e-07/4.4e-08
    packed-h_cloud-backface-S1024            6.8e-08/3e-07/6.8e-08   5.5e-08/3e-07/5.5e-08   1.0e-08/4e-08/1.0e-08   4.2e-08/2e-07/4.6e-08
    packed-h_point-nocull-S64                7.2e-08/3e-07/7.2e-08   5.1e-08/3e-07/5.1e-08   2.5e-08/1e-07/2.5e-08   4.6e-08/2e-07/3.6e-08
    packed-h_point-nocull-S1024              7.2e-08/3e-07/7.2e-08   5.3e-08/3e-07/5.3e-08   9.7e-09/4e-08/9.7e-09   5.2e-08/3e-07/5.2e-08
    packed-h_point-backface-S64              6.8e-08/3e-07/6.8e-08   5.1e-08/3e-07/5.1e-08   2.5e-08/1e-07/2.5e-08   4.6e-08/2e-07/3.6e-08
    packed-h_point-backface-S1024            6.8e-08/3e-07/6.8e-08   5.3e-08/3e-07/5.3e-08   9.7e-09/4e-08/9.7e-09   5.2e-08/3e-07/5.2e-08
    packed-aniso-nocull-S64                  7.2e-08/3e-07/7.2e-08   4.9e-08/2e-07/4.9e-08   2.9e-08/2e-07/2.9e-08   5.4e-08/3e-07/5.2e-08
    packed-aniso-nocull-S1024                7.2e-08/3e-07/7.2e-08   3.6e-08/2e-07/3.6e-08   1.6e-08/7e-08/1.6e-08   4.0e-08/2e-07/4.0e-08
    packed-aniso-backface-S64                6.8e-08/3e-07/6.8e-08   4.5e-08/2e-07/4.5e-08   2.9e-08/2e-07/2.9e-08   4.5e-08/2e-07/4.4e-08
    packed-aniso-backface-S1024              6.8e-08/3e-07/6.8e-08   3.3e-08/2e-07/3.3e-08   9.6e-09/4e-08/9.6e-09   3.3e-08/2e-07/3.1e-08
    shared-h_cloud-nocull-S64                9.7e-08/4e-07/9.7e-08   6.1e-08/3e-07/6.1e-08   3.2e-08/2e-07/3.2e-08   9.0e-08/4e-07/7.5e-08
    shared-h_cloud-nocull-S1024              9.7e-08/4e-07/9.7e-08   5.4e-08/3e-07/5.4e-08   1.5e-08/7e-08/1.5e-08   7.2e-08/3e-07/5.1e-08
    shared-h_cloud-backface-S64              8.3e-08/4e-07/8.3e-08   6.1e-08/3e-07/6.1e-08   3.2e-08/2e-07/3.2e-08   9.0e-08/4e-07/7.5e-08
    shared-h_cloud-backface-S1024            8.3e-08/4e-07/8.3e-08   5.4e-08/3e-07/5.4e-08   1.5e-08/7e-08/1.5e-08   7.2e-08/3e-07/5.1e-08
    shared-h_point-nocull-S64                9.7e-08/4e-07/9.7e-08   6.2e-08/3e-07/6.2e-08   3.1e-08/2e-07/3.1e-08   8.4e-08/4e-07/8.0e-08
    shared-h_point-nocull-S1024              9.7e-08/4e-07/9.7e-08   4.5e-08/2e-07/4.5e-08   2.5e-08/1e-07/2.5e-08   7.7e-08/4e-07/6.7e-08
    shared-h_point-backface-S64              8.3e-08/4e-07/8.3e-08   5.6e-08/3e-07/5.6e-08   3.1e-08/2e-07/3.1e-08   7.9e-08/4e-07/8.0e-08
    shared-h_point-backface-S1024            8.3e-08/4e-07/8.3e-08   4.4e-08/2e-07/4.2e-08   2.5e-08/1e-07/2.5e-08   7.7e-08/4e-07/5.7e-08
    shared-h_packed-nocull-S64               9.7e-08/4e-07/9.7e-08   5.9e-08/3e-07/5.9e-08   3.2e-08/2e-07/3.2e-08   1.0e-07/4e-07/8.3e-08
    shared-h_packed-nocull-S1024             9.7e-08/4e-07/9.7e-08   5.2e-08/3e-07/5.2e-08   2.5e-08/1e-07/2.5e-08   8.1e-08/4e-07/6.7e-08
    shared-h_packed-backface-S64             8.3e-08/4e-07/8.3e-08   5.0e-08/3e-07/5.0e-08   3.0e-08/2e-07/3.2e-08   1.0e-07/4e-07/7.6e-08
    shared-h_packed-backface-S1024           8.3e-08/4e-07/8.3e-08   5.1e-08/3e-07/5.1e-08   2.5e-08/1e-07/2.5e-08   8.1e-08/4e-07/6.7e-08
    shared-aniso-nocull-S64                  9.7e-08/4e-07/9.7e-08   7.6e-08/4e-07/7.6e-08   3.1e-08/2e-07/3.1e-08   9.5e-08/4e-07/7.3e-08
    shared-aniso-nocull-S1024                9.7e-08/4e-07/9.7e-08   7.8e-08/4e-07/7.8e-08   3.1e-08/2e-07/3.1e-08   7.1e-08/3e-07/6.4e-08
    shared-aniso-backface-S64                8.3e-08/4e-07/8.3e-08   7.6e-08/4e-07/7.6e-08   3.1e-08/2e-07/3.1e-08   9.5e-08/4e-07/7.3e-08
    shared-aniso-backface-S1024              8.3e-08/4e-07/8.3e-08   6.5e-08/3e-07/6.5e-08   3.1e-08/2e-07/3.1e-08   7.1e-08/3e-07/5.9e-08
    ragged-h_cloud-nocull-S64                5.0e-08/2e-07/5.0e-08   4.1e-08/2e-07/4.1e-08   8.3e-09/4e-08/8.3e-09   2.5e-08/2e-07/2.5e-08
    ragged-h_cloud-nocull-S1024              5.0e-08/2e-07/5.0e-08   4.2e-08/2e-07/4.2e-08   8.4e-09/4e-08/8.4e-09   4.0e-08/2e-07/4.0e-08
    ragged-h_cloud-backface-S64              5.0e-08/2e-07/5.0e-08   4.1e-08/2e-07/4.1e-08   8.3e-09/4e-08/8.3e-09   2.3e-08/1e-07/2.3e-08
    ragged-h_cloud-backface-S1024            5.0e-08/2e-07/5.0e-08   4.2e-08/2e-07/4.2e-08   8.4e-09/4e-08/8.4e-09   4.0e-08/2e-07/4.0e-08
    ragged-h_point-nocull-S64                5.0e-08/2e-07/5.0e-08   4.1e-08/2e-07/4.1e-08   9.2e-09/4e-08/9.2e-09   2.4e-08/1e-07/2.4e-08
    ragged-h_point-nocull-S1024              5.0e-08/2e-07/5.0e-08   4.2e-08/2e-07/4.2e-08   8.3e-09/4e-08/8.3e-09   3.9e-08/2e-07/3.9e-08
    ragged-h_point-backface-S64              5.0e-08/2e-07/5.0e-08   4.1e-08/2e-07/4.1e-08   9.2e-09/4e-08/9.2e-09   2.2e-08/9e-08/2.3e-08
    ragged-h_point-backface-S1024            5.0e-08/2e-07/5.0e-08   4.2e-08/2e-07/4.2e-08   8.3e-09/4e-08/8.3e-09   3.9e-08/2e-07/3.9e-08
    ragged-aniso-nocull-S64                  5.0e-08/2e-07/5.0e-08   4.2e-08/2e-07/4.2e-08   1.7e-08/7e-08/1.7e-08   3.5e-08/2e-07/2.3e-08
    ragged-aniso-nocull-S1024                5.0e-08/2e-07/5.0e-08   2.5e-08/1e-07/2.5e-08   6.9e-09/3e-08/6.9e-09   3.5e-08/2e-07/2.3e-08
    ragged-aniso-backface-S64                5.0e-08/2e-07/5.0e-08   4.2e-08/2e-07/4.2e-08   1.7e-08/7e-08/1.7e-08   3.5e-08/2e-07/2.3e-08
    ragged-aniso-backface-S1024              5.0e-08/2e-07/5.0e-08   2.5e-08/1e-07/2.5e-08   6.9e-09/3e-08/6.9e-09   3.5e-08/2e-07/2.3e-08
    shared_partial-h_cloud-nocull-S64        8.9e-08/4e-07/8.9e-08   4.7e-08/2e-07/4.7e-08   3.0e-08/2e-07/3.0e-08   5.0e-08/2e-07/6.7e-08
    shared_partial-h_cloud-nocull-S1024      8.9e-08/4e-07/8.9e-08   4.7e-08/2e-07/4.7e-08   1.1e-08/5e-08/1.1e-08   4.0e-08/2e-07/4.4e-08
    shared_partial-h_cloud-backface-S64      7.8e-08/4e-07/7.8e-08   4.3e-08/2e-07/4.3e-08   3.0e-08/2e-07/3.0e-08   4.4e-08/2e-07/6.7e-08
    shared_partial-h_cloud-backface-S1024    7.8e-08/4e-07/7.8e-08   4.7e-08/2e-07/4.7e-08   1.1e-08/5e-08/1.1e-08   3.8e-08/2e-07/3.8e-08
    shared_partial-h_point-nocull-S64        8.9e-08/4e-07/8.9e-08   4.9e-08/2e-07/4.9e-08   3.1e-08/2e-07/3.1e-08   5.4e-08/3e-07/5.3e-08
    shared_partial-h_point-nocull-S1024      8.9e-08/4e-07/8.9e-08   4.1e-08/2e-07/4.1e-08   1.4e-08/6e-08/1.4e-08   4.4e-08/2e-07/3.8e-08
    shared_partial-h_point-backface-S64      7.8e-08/4e-07/7.8e-08   4.8e-08/2e-07/4.8e-08   3.1e-08/2e-07/3.1e-08   5.4e-08/3e-07/5.1e-08
    shared_partial-h_point-backface-S1024    7.8e-08/4e-07/7.8e-08   4.0e-08/2e-07/4.0e-08   1.0e-08/5e-08/1.0e-08   3.4e-08/2e-07/3.8e-08
    shared_partial-h_packed-nocull-S64       8.9e-08/4e-07/8.9e-08   5.0e-08/3e-07/5.0e-08   2.9e-08/2e-07/2.9e-08   6.9e-08/3e-07/8.8e-08
    shared_partial-h_packed-nocull-S1024     8.9e-08/4e-07/8.9e-08   4.1e-08/2e-07/4.1e-08   1.1e-08/5e-08/1.2e-08   4.3e-08/2e-07/4.3e-08
    shared_partial-h_packed-backface-S64     7.8e-08/4e-07/7.8e-08   4.4e-08/2e-07/4.4e-08   2.9e-08/2e-07/2.9e-08   4.8e-08/2e-07/6.0e-08
    shared_partial-h_packed-backface-S1024   7.8e-08/4e-07/7.8e-08   4.1e-08/2e-07/4.1e-08   1.0e-08/5e-08/1.2e-08   4.3e-08/2e-07/4.3e-08
    shared_partial-aniso-nocull-S64          8.9e-08/4e-07/8.9e-08   5.0e-08/3e-07/5.0e-08   2.9e-08/2e-07/2.9e-08   5.3e-08/3e-07/5.8e-08
    shared_partial-aniso-nocull-S1024        8.9e-08/4e-07/8.9e-08   4.2e-08/2e-07/4.2e-08   1.4e-08/6e-08/1.4e-08   4.6e-08/2e-07/3.9e-08
    shared_partial-aniso-backface-S64        7.8e-08/4e-07/7.8e-08   5.0e-08/3e-07/5.0e-08   2.6e-08/2e-07/2.6e-08   4.8e-08/2e-07/5.5e-08
    shared_partial-aniso-backface-S1024      7.8e-08/4e-07/7.8e-08   4.2e-08/2e-07/4.2e-08   1.4e-08/6e-08/1.4e-08   4.3e-08/2e-07/3.4e-08

No kernel figure exceeds 0.34 of its bar or 1.53 x the fp32-torch figure of its case (the torch figures: the CPU the table
was made on; the square root of another CPU moves them in the last bit); the kernel's bits are the oracle's on every case.
"""
import pytest
import torch

import setup_reference as sr
from dss_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, THR = 5, 0.05
_ids = [sr.case_id(k) for k in sr.CASES]
RENDER_CASES = [k for k in sr.CASES if k[3] == 64]          # what goes through render_forward: S <= 128
BAND = (16, 40)
KEYS = {"screen": "pts_screen", "ellipse": "ellipse_params", "radii": "radii", "scaler": "scaler"}
SIX = ("pts_screen", "ellipse_params", "radii", "scaler", "cutoff_threshold", "valid")


def _args(c):
    d = lambda t: t.to(DEV)
    return [d(c.world), d(c.normals), d(c.h), d(c.M), d(c.V), d(c.znear), d(c.zfar), d(c.first), d(c.num)]


def _aniso(c):
    return dict(vr6=None if c.vr6 is None else c.vr6.to(DEV), frame_normals=None if c.fn is None else c.fn.to(DEV))


def _point_setup(c):
    return ops.point_setup(*_args(c), c.S, sr.CUTOFF, sr.SIGMA, c.backface, c.shared, **_aniso(c))


def _features(c):
    return torch.rand(sr.packed_rows(c), 3, generator=torch.Generator().manual_seed(11)).to(DEV)


def _render(c, **kw):
    return ops.render_forward(*_args(c), _features(c), c.S, K, sr.CUTOFF, THR, sr.SIGMA, c.backface, c.shared, **_aniso(c), **kw)


def _got(out):
    got = {name: out[key].cpu().reshape(out[key].shape[0], -1) for name, key in KEYS.items()}
    got["valid"] = out["valid"].cpu()
    return got


@pytest.mark.parametrize("key", sr.CASES, ids=_ids)
def test_point_setup_against_the_reference(key):
    c, ref, bars = sr.case(*key), sr.reference(*key), sr.BARS[key]
    out = _point_setup(c)
    got = _got(out)
    worst, wrong = sr.ratios(got, ref)
    print("point_setup %-40s max |err| / scale: %s" % (sr.case_id(key), "  ".join(
        "%s %.1e (bar %.0e)" % (n, w, b) for n, w, b in zip(sr.OUTPUTS, worst, bars))))
    assert not wrong, wrong
    for name, w, b in zip(sr.OUTPUTS, worst, bars):
        assert w <= b, (name, w, b)
    assert bool((out["cutoff_threshold"] == sr.CUTOFF).all())          # the full mode writes the constant on every row
    # the contract at the top of setup.hip, where the branches are: the oracle's bits on every pair the kernel keeps
    want = sr.oracle_outputs(c, got["valid"])
    for name in sr.OUTPUTS:
        assert torch.equal(got[name], want[name]), name


@pytest.mark.parametrize("key", RENDER_CASES, ids=[sr.case_id(k) for k in RENDER_CASES])
def test_render_forward_gives_the_bits_of_point_setup(key):
    """`setup_bin_kernel` (one camera per wavefront where its 64 points lie in one cloud, per lane where they straddle two)
    against `point_setup_kernel`: all six point outputs, on the whole image and on a row band"""
    c = sr.case(*key)
    want = _point_setup(c)
    for rows in (None, BAND):
        f = _render(c, rows=rows)
        for k in SIX:
            assert torch.equal(f[k], want[k]), (k, rows)


@pytest.mark.parametrize("key", RENDER_CASES, ids=[sr.case_id(k) for k in RENDER_CASES])
def test_band_outputs_only(key):
    """`band_outputs_only=True` with `rows`: position, radii and validity are the full call's bits on every row; ellipse, scaler
    and cutoff are the full call's bits for every splat that can reach the band (decided from the fp64 reference, the splats
    within rounding of the band's edge left out: at most 1 % of the owned pairs) and the zero fill for every splat that cannot"""
    c, ref = sr.case(*key), sr.reference(*key)
    reach, miss, unsure = (t.to(DEV) for t in sr.reference_reach(ref, sr.BARS[key], c.S, BAND))
    assert int(unsure.sum()) <= 0.01 * int(ref.owned.sum()) and bool(reach.any()) and bool((miss & ref.valid.to(DEV)).any())
    full, band = _render(c, rows=BAND), _render(c, rows=BAND, band_outputs_only=True)
    for k in ("pts_screen", "radii", "valid"):
        assert torch.equal(band[k], full[k]), k
    for k in ("ellipse_params", "scaler", "cutoff_threshold"):
        assert torch.equal(band[k][reach], full[k][reach]), k
        assert bool((band[k][miss] == 0).all()), k
    for k in ("idx", "qvalue", "occupancy", "image", "visible"):
        assert torch.equal(band[k], full[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# Above 2M points (SORT_MIN_P, raster_forward.hip) the forward bins in screen-cell order and the setup runs in
# `setup_cell_kernel`; with a saved order (DSS_WS_ORDER_REUSE) that kernel is nothing but the setup, and full wavefronts store
# through `setup_wave_store` (16-byte runs through LDS) -- or, where a buffer is not aligned for that, per lane.
BIG_SIZES = (700_001, 900_037, 400_063)         # 2,000,101 points: no cloud boundary and no end on a multiple of 64
BIG_S = 128


def _big_inputs(backface=True):
    g = torch.Generator(DEV).manual_seed(5)
    u = lambda *s: torch.rand(*s, generator=g, device=DEV)
    P = sum(BIG_SIZES)
    pool = sr.camera_pool()
    cams = ("p1", "p2", "p3")
    M, V = (torch.stack([pool[k][i] for k in cams]).to(DEV) for i in (0, 1))
    zn, zf = (torch.tensor([pool[k][i] for k in cams], device=DEV) for i in (2, 3))
    world = u(P, 3) - 0.5
    normals = torch.nn.functional.normalize(u(P, 3) * 2.0 - 1.0, dim=1) * torch.ldexp(1.0 + u(P), torch.randint(
        -10, 10, (P,), generator=g, device=DEV))[:, None]
    h = torch.tensor([5e-5, 1e-4, 2e-4], device=DEV)
    num = torch.tensor(BIG_SIZES, device=DEV, dtype=torch.int64)
    first = torch.cumsum(num, 0) - num
    return [world, normals, h, M, V, zn, zf, first, num], u(P, 3), backface


def _big_render(inp, state, **kw):
    args, feat, backface = inp
    return ops.render_forward(*args, feat, BIG_S, K, sr.CUTOFF, THR, sr.SIGMA, backface, False, workspace_state=state, **kw)


def _offset_view(P, mark):
    """a dense (P,3) view 4 bytes into a larger allocation filled with ``mark``: `setup_wide_ok` is false for it"""
    buf = torch.full((3 * P + 8,), mark, device=DEV)
    view = buf[1:1 + 3 * P].view(P, 3)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return buf, view


def test_two_million_points_every_store_path_gives_the_bits_of_point_setup():
    inp = _big_inputs()
    args, _feat, backface = inp
    P = sum(BIG_SIZES)
    assert P > 2_000_000 and P % 64 and all(int(f) % 64 for f in args[7][1:])
    want = ops.point_setup(*args, BIG_S, sr.CUTOFF, sr.SIGMA, backface, False)
    frac = float(want["valid"].float().mean())
    assert 0.1 < frac < 0.6          # the near planes cut the cube, back faces are culled
    save, reuse = 0 | _lib.WS_ORDER_SAVE, 0 | _lib.WS_ORDER_REUSE
    for rows in (None, (32, 64)):
        for state in (0, save, reuse):              # sorts for itself / sorts and keeps the order / the setup alone, wave stores
            f = _big_render(inp, state, rows=rows)
            for k in SIX:
                assert torch.equal(f[k], want[k]), (k, rows, state)
    # the misaligned fallback: an ellipse buffer that is not 16-byte aligned -> per-lane stores, same bits, nothing beyond it
    mark = 7.25
    buf, ell = _offset_view(P, mark)
    sca, cut = torch.empty(P, device=DEV), torch.empty(P, device=DEV)
    f = _big_render(inp, reuse, point_outputs=(ell, sca, cut))
    assert f["ellipse_params"].data_ptr() == ell.data_ptr()
    for k in SIX:
        assert torch.equal(f[k], want[k]), k
    assert float(buf[0]) == mark and bool((buf[1 + 3 * P:] == mark).all()) and not bool((ell == mark).any())


def test_two_million_points_band_outputs_only():
    """the band form of every store path: the splats that reach the band -- decided in fp64 from the positions and radii that
    the test above pins to `point_setup`, those within a few ulps of the band's edge left out -- hold the full call's ellipse,
    scaler and cutoff; the others keep what the buffer held (the zero fill, or the caller's sentinel)"""
    inp = _big_inputs()
    args, _feat, backface = inp
    P, rows = sum(BIG_SIZES), (32, 64)
    want = ops.point_setup(*args, BIG_S, sr.CUTOFF, sr.SIGMA, backface, False)
    scr, rad = want["pts_screen"].double(), want["radii"].double()
    slack = [2.0 ** -21 * (1.0 + scr[:, k].abs() + rad[:, k]) for k in range(2)]
    reach, miss = sr.band_reach(scr[:, 0], scr[:, 1], rad[:, 0], rad[:, 1], want["valid"], BIG_S, rows, slack[0], slack[1])
    assert int((~reach & ~miss).sum()) <= 0.01 * P and 0.02 * P < int(reach.sum()) < 0.5 * P
    save, reuse = 0 | _lib.WS_ORDER_SAVE, 0 | _lib.WS_ORDER_REUSE
    full = _big_render(inp, 0, rows=rows)
    mark = 7.25
    for state in (0, save, reuse, "reuse, misaligned"):
        if state == "reuse, misaligned":
            buf, ell = _offset_view(P, mark)
            outs = (ell, torch.full((P,), mark, device=DEV), torch.full((P,), mark, device=DEV))
            band = _big_render(inp, reuse, rows=rows, band_outputs_only=True, point_outputs=outs)
            rest = mark
            assert float(buf[0]) == mark and bool((buf[1 + 3 * P:] == mark).all())
        else:
            band = _big_render(inp, state, rows=rows, band_outputs_only=True)
            rest = 0.0
        for k in ("pts_screen", "radii", "valid", "idx", "qvalue", "occupancy", "image", "visible"):
            assert torch.equal(band[k], full[k]), (k, state)
        for k in ("ellipse_params", "scaler", "cutoff_threshold"):
            assert torch.equal(band[k][reach], want[k][reach]), (k, state)
            assert bool((band[k][miss] == rest).all()), (k, state)
