"""fp64 reference of the image loss of the training iteration and of its gradient w.r.t. the rendered RGBA image
(dss_amd/csrc/image_loss.hip), for the entry-by-entry tests (tests/test_image_loss_reference_cpu.py,
tests/test_gpu_image_loss_reference.py).  Test infrastructure: numpy, no product code in the formulas.  Written from the
method's definition, `Trainer.calc_dr_loss` (trainer.py:332-372) with `BaseLoss` / `L1Loss` / `IouLoss`
(losses.py:24-61, 130-137, 498-513) and `eps_denom` (mathHelper.py:10-14):

    inside = t != 0 and a != 0                                  a = predicted alpha, t = target mask
    rgb    = sum_inside sum_c |img_c - pred_c| / #inside        (0 without a pixel inside)
    sil    = mean |t - a| + 0.01 mean_n (1 - I_n / eps_denom(U_n)),   I = sum a t,  U = sum (a + t - a t)
    total  = lambda_rgb rgb + lambda_sil sil

Five sums per image -- inside count, sum_inside sum_c |img - pred|, sum |t - a|, I, U -- carry the whole forward, for the
image or for any set of its rows (a band's partial sums come from the same code).  The gradient takes the sums as an
input, as the kernels' backward takes the forward's fp64 sums.

Every value carries `A`, the sum of the absolute values of the terms added to form it; the error of an entry is
``|got - want| / A`` (floor 1e-30), and an entry with A == 0 is expected exactly.  The inside count is exact (A = 0).
Decisions are taken on the fp32 inputs as the method takes them -- `inside`, the three-valued sign by comparing the two
operands, `cnt > 0`, the clamp of `eps_denom` with the gradient ``-t / eps`` on the clamped branch, the reference's
``lambda > 0`` gates -- and everything after a decision is fp64.  lambda and `grad_total` reach the kernels as fp32:
callers pass values that are fp32 already (`LAMBDAS`, `GRAD_TOTALS`).

``dtype=np.float32`` restates the kernels' documented arithmetic in fp32: every per-pixel term in fp32, fp32 partial sums
per thread over the reduce kernel's pixel-to-thread partition (thread `i % (nb 1024)` of an image's `nb` blocks takes pixel
i, its pixels in order), the 64 partials of a wavefront added in fp32 (`order`: lane order, reversed lane order, or the
adjacent-pairs tree; `case_figures` takes the worst of the three, the kernel's shuffle tree is one more order), doubles
after that; `w_rgb`, `w_l1` and the IoU part of the alpha gradient rounded to fp32, their sum and the product with
`grad_total` in fp32; the four losses rounded to fp32.  It shows what the number format alone costs: a bar is 4x its figure.

``mut=`` names one wrong formula (`MUTATIONS`).  `inside_half` thresholds both masks at one half; `iou_no_one_minus_t` takes
the I-term of the IoU gradient only where t == 0 (a factor ``t == 0`` for ``1 - t``): neither shows on binary data."""
import functools
import types
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
THREADS, MAX_BLOCKS, TERMS = 1024, 64, 5      # reduce kernel: threads per block, blocks per image, sums per image
EPS = 1e-17                                   # eps_denom
FLOOR = 1e-30
OUTPUTS = ("sums", "losses", "grad")
LAMBDAS = ((1.0, 1.0), (float(F32(0.7)), 2.0))
GRAD_TOTALS = (None, float(F32(0.37)))
ORDERS = ("lanes", "reversed", "tree")

SHAPES = [(1, 1, 1), (1, 1, 5), (2, 3, 1021), (1, 64, 64), (1, 17, 241), (3, 37, 53), (5, 8, 8), (65, 3, 5), (1, 512, 512),
          (1, 513, 512), (1, 641, 512)]        # 641 x 512: the second trip's slot u = 1 ends after 512 threads, u = 2, 3 are past the end
BAND_SHAPES = [(3, 128, 20), (2, 72, 20), (64, 2, 3)]
CASES = ["%s_%dx%dx%d" % ((kind,) + s) for s in SHAPES for kind in ("soft", "bin")] + ["soft_%dx%dx%d" % s for s in BAND_SHAPES]
TINY_U = {"soft_3x37x53": 2, "soft_5x8x8": 4, "soft_3x128x20": 2}     # case: the image with 0 < U < 1e-17
EMPTY = {"soft_5x8x8": 3}                                             # case: the all-empty image (U == 0)
NO_TARGET = {"soft_2x3x1021": 1, "soft_3x128x20": 1}                  # case: the image without any target silhouette


def image_blocks(rows, W):
    return int(min(max((rows * W + 4 * THREADS - 1) // (4 * THREADS), 1), MAX_BLOCKS))


def soft_images(rng, N, H, W):
    """soft masks and alphas in [0, 1] with exact zeros and ones mixed in, colours with exact ties, alpha ties"""
    def soft():
        v = rng.random((N, H, W)).astype(F32)
        u = rng.random((N, H, W))
        v[u < 0.25] = 0.0
        v[u > 0.85] = 1.0
        return v
    img = rng.random((N, H, W, 3)).astype(F32)
    rgba = rng.random((N, H, W, 4)).astype(F32)
    rgba[..., 3], mask = soft(), soft()
    tie = rng.random((N, H, W, 3)) < 0.1
    rgba[..., :3][tie] = img[tie]
    tie = rng.random((N, H, W)) < 0.05
    rgba[..., 3][tie] = mask[tie]
    return rgba, img, mask


def tiny_union(rgba, mask, n):
    """image n: masks of order 1e-18 on a few pixels, exact zeros elsewhere: 0 < U < 1e-17 with t > 0"""
    a, t = rgba[n, ..., 3].reshape(-1), mask[n].reshape(-1)        # views
    a[:], t[:] = 0.0, 0.0
    P = a.size
    for j, i in enumerate(range(0, P, max(P // 3, 1))):            # at most four pixels: sum t <= 4.6e-18
        t[i] = F32((1.0 + 0.1 * j) * 1e-18)
    for j, i in enumerate(range(0, P, max(P // 2, 1))):            # at most three: sum a <= 2.7e-18; pixel 0 is inside
        a[i] = F32((0.7 + 0.2 * j) * 1e-18)


def _plant(rgba, img, mask, nonfinite=True):
    """image 0 (64 pixels at least): the entries at which an fp32 kernel can decide wrongly, at fixed pixels"""
    a, t = rgba[0, ..., 3].reshape(-1), mask[0].reshape(-1)
    p, c = rgba[0, ..., :3].reshape(-1, 3), img[0].reshape(-1, 3)
    tiny, sub = F32(1.5e-38), np.nextafter(F32(1.5e-38), F32(1))
    a[0], t[0], p[0, 0], c[0, 0] = tiny, sub, sub, tiny            # normal values one ulp (a subnormal amount) apart
    a[1], t[1], p[1, 1], c[1, 1] = F32(3e-39), F32(2e-39), F32(2e-39), F32(3e-39)   # subnormal operands
    a[2], t[2] = F32(1e-30), F32(1e-30)                            # a t underflows, both non-zero: inside
    a[3], t[3] = F32(1e-20), F32(1e-30)
    a[4], t[4] = F32(1e-30), F32(0.75)
    if nonfinite:
        a[5], t[5], p[5], c[5, 0] = 0.0, F32(0.5), np.nan, np.inf  # NaN / Inf colours outside `inside`
        a[6], t[6], p[6, 1], c[6] = F32(0.5), 0.0, -np.inf, np.nan
        a[7], t[7], p[7], c[7] = 0.0, 0.0, np.inf, np.inf
    a[8], t[8] = F32(0.625), F32(0.625)                            # alpha tie inside, with a colour tie
    p[8] = c[8]
    a[9], t[9] = F32(1.0), F32(1.0)
    a[10], t[10] = F32(1.0), F32(0.25)                             # the two terms of the alpha gradient meet (t < a = 1)
    a[11], t[11] = F32(0.75), F32(1.0)


@functools.lru_cache(maxsize=None)
def case(name):
    kind, shape = name.split("_")
    N, H, W = (int(v) for v in shape.split("x"))
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if kind == "bin":                                              # today's data: every mask and alpha exactly 0 or 1
        img = rng.random((N, H, W, 3)).astype(F32)
        rgba = rng.random((N, H, W, 4)).astype(F32)
        rgba[..., 3] = rng.random((N, H, W)) < 0.4
        mask = (rng.random((N, H, W)) < 0.5).astype(F32)
        if H * W < 8:
            rgba[0, 0, 0, 3], mask[0, 0, 0] = 1.0, 1.0
    else:
        rgba, img, mask = soft_images(rng, N, H, W)
        if H * W < 8:
            rgba[0, 0, 0, 3], mask[0, 0, 0] = F32(0.3), F32(0.6)
        if H * W >= 64:
            _plant(rgba, img, mask)
        if H * W % 4096 == 1:                                      # the lone pixel beyond the last full 4096: soft and inside
            rgba[0, -1, -1, 3], mask[0, -1, -1] = F32(0.4), F32(0.9)
        if name in NO_TARGET:
            mask[NO_TARGET[name]] = 0.0
        if name in EMPTY:
            mask[EMPTY[name]], rgba[EMPTY[name], ..., 3] = 0.0, 0.0
        if name in TINY_U:
            tiny_union(rgba, mask, TINY_U[name])
    for a in (rgba, img, mask):
        a.setflags(write=False)
    return types.SimpleNamespace(name=name, N=N, H=H, W=W, rgba=rgba, img=img, mask=mask)


def golden_case():
    """The inputs of tests/golden/ref_image_loss_f64.npz (the reference's own `Trainer.calc_dr_loss` run in float64 on them):
    four soft 24 x 20 images -- planted ties, subnormal differences and underflowing products in image 0 (finite colours:
    autograd's |x|' turns a NaN outside the mask into a NaN gradient), image 1 without a target silhouette, image 2 all
    empty (U == 0), image 3 with 0 < U < 1e-17"""
    N, H, W = 4, 24, 20
    rgba, img, mask = soft_images(np.random.default_rng(20), N, H, W)
    _plant(rgba, img, mask, nonfinite=False)
    mask[1] = 0.0
    mask[2], rgba[2, ..., 3] = 0.0, 0.0
    tiny_union(rgba, mask, 3)
    return types.SimpleNamespace(name="golden", N=N, H=H, W=W, rgba=rgba, img=img, mask=mask)


# ------------------------------------------------------------------------------------------------------------------------
# the five sums of a set of rows
# ------------------------------------------------------------------------------------------------------------------------
def band_arrays(c, rows=None, mut=None):
    """(N, r, W, .) rows `rows` (image row indices, None = all) of the render and of the targets"""
    rows = np.arange(c.H) if rows is None else np.asarray(rows, np.int64)
    N, r, W = c.N, len(rows), c.W
    rgba, img, mask = c.rgba[:, rows], c.img[:, rows], c.mask[:, rows]
    if mut == "mask_stride_band" and r:             # image n of the band's mask taken r W floats after image n - 1, not H W
        flat = c.mask.reshape(-1)
        idx = rows[0] * W + np.arange(N)[:, None] * (r * W) + np.arange(r * W)[None]
        mask = flat[idx % flat.size].reshape(N, r, W)
    if mut == "target_strides_swapped" and r:       # pixel (y, x) read at y * (stride of x) + x * (stride of y)
        y, x = np.meshgrid(rows, np.arange(W), indexing="ij")
        img = c.img.reshape(N, c.H * W, 3)[:, (y + x * W) % (c.H * W)]
    return rgba, img, mask


def inside_of(a32, t32, mut=None):
    if mut == "inside_half":
        return (t32 > 0.5) & (a32 > 0.5)
    if mut == "inside_product":
        with np.errstate(under="ignore"):
            return (a32 * t32) != 0                 # the fp32 product underflows
    return (t32 != 0) & (a32 != 0)


def pixel_terms(rgba, img, mask, dtype=F64, mut=None):
    """-> (terms, magnitudes), each (N, P, 5) in `dtype`: the per-pixel contributions to the five sums"""
    N = rgba.shape[0]
    a32, t32 = rgba[..., 3].reshape(N, -1), mask.reshape(N, -1)
    inside = inside_of(a32, t32, mut)
    a, t = a32.astype(dtype), t32.astype(dtype)
    p, c = rgba[..., :3].reshape(N, -1, 3).astype(dtype), img.reshape(N, -1, 3).astype(dtype)
    with np.errstate(all="ignore"):
        d = np.abs(c[..., 0] - p[..., 0]) + np.abs(c[..., 1] - p[..., 1]) + np.abs(c[..., 2] - p[..., 2])
        at = a * t
        inter = np.minimum(a, t) if mut == "inter_min" else at
        uni = np.maximum(a, t) if mut == "union_max" else (a + t) - at
        uni_A = np.maximum(a, t) if mut == "union_max" else (np.abs(a) + np.abs(t)) + np.abs(at)
    srgb = np.where(inside, d, dtype(0))            # a colour outside `inside` never reaches a sum, NaN or not
    smask = np.abs(t - a)
    terms = np.stack([inside.astype(dtype), srgb, smask, inter, uni], -1)
    mags = np.stack([np.zeros_like(srgb), srgb, smask, np.abs(inter), uni_A], -1)
    return terms, mags


def _kept(P, nb, mut):
    """pixels of one image that a wrong reduce loop still adds: pixel i belongs to thread i % (nb 1024), block
    (i % (nb 1024)) // 1024, and is that thread's k-th pixel, k = i // (nb 1024) = 4 trip + slot"""
    i = np.arange(P)
    stride = nb * THREADS
    thread, k = i % stride, i // stride
    if mut == "second_trip_dropped":
        return k < 4
    if mut == "last_block_dropped":
        return thread // THREADS != nb - 1
    if mut == "tail_slot_dropped":                 # a thread whose last trip is not full adds only that trip's slot 0
        n_k = -(-(P - thread) // stride)
        last = (n_k - 1) // 4
        return ~((k // 4 == last) & (n_k - 4 * last < 4) & (k % 4 >= 1))
    return np.ones(P, bool)


def _wave_add(x, order):
    """(..., 64, 5) fp32 -> (..., 5): the 64 lanes added in fp32"""
    if order == "tree":
        while x.shape[-2] > 1:
            x = x[..., 0::2, :] + x[..., 1::2, :]
        return x[..., 0, :]
    lanes = range(64) if order == "lanes" else range(63, -1, -1)
    acc = np.zeros(x.shape[:-2] + x.shape[-1:], F32)
    for l in lanes:
        acc = acc + x[..., l, :]
    return acc


def band_sums(c, rows=None, dtype=F64, mut=None, nb=None, order="lanes"):
    """The five sums of every image over the rows `rows` -> (sums, A), each (N, 5) float64.  ``nb``: blocks per image of the
    reduce launch (default: the unfused forward's; the fused band form always launches 64)."""
    rgba, img, mask = band_arrays(c, rows, mut)
    N, P = c.N, rgba.shape[1] * c.W
    nb = image_blocks(rgba.shape[1], c.W) if nb is None else nb
    terms, mags = pixel_terms(rgba, img, mask, dtype, mut)
    keep = _kept(P, nb, mut)
    terms, mags = terms * keep[None, :, None].astype(dtype), mags * keep[None, :, None].astype(dtype)
    A = mags.astype(F64).sum(1)
    if dtype == F64:
        return terms.sum(1), A
    stride = nb * THREADS
    K = max(-(-P // stride), 1)
    pad = np.zeros((N, K * stride, TERMS), F32)
    pad[:, :P] = terms
    pad = pad.reshape(N, K, stride, TERMS)
    acc = np.zeros((N, stride, TERMS), F32)
    for k in range(K):                              # a thread's pixels in order (adding the padding's +0 changes no bit)
        acc = acc + pad[:, k]
    waves = _wave_add(acc.reshape(N, stride // 64, 64, TERMS), order)
    return waves.astype(F64).sum(1), A


def finalize(per_image, per_image_A, mut=None):
    """(N, 5) -> (N + 1, 5): the totals over the batch in the last row"""
    s, A = per_image.copy(), per_image_A.copy()
    if mut == "images_from_4_dropped":
        s[4:], A[4:] = 0.0, 0.0
    return np.concatenate([s, s.sum(0, keepdims=True)]), np.concatenate([A, A.sum(0, keepdims=True)])


def _denominator(U):
    return np.where(U < 0, -1.0, 1.0) * np.maximum(np.abs(U), EPS)


def losses_of(sums, pix, lam, mut=None, gate=True):
    """sums (N + 1, 5), pix = pixels of one FULL image -> (losses, A), each (4,) float64: total, weighted rgb term, weighted
    silhouette term, IoU term.  ``gate=False``: a term is multiplied by its lambda whatever its sign (the kernels)."""
    N = sums.shape[0] - 1
    lam_rgb, lam_sil = (float(v) for v in lam)
    cnt, srgb, smask = sums[N, 0], sums[N, 1], sums[N, 2]
    ratio = sums[:N, 3] / _denominator(sums[:N, 4])
    iou, iou_A = (1.0 - ratio).sum(), (1.0 + np.abs(ratio)).sum()
    if mut != "iou_no_over_n":
        iou, iou_A = iou / N, iou_A / N
    rgb = srgb / cnt if cnt > 0 else 0.0
    if mut == "rgb_mean_over_3cnt":
        rgb /= 3.0
    k = 1.0 if mut == "no_001" else 0.01
    sil, sil_A = smask / (N * pix) + k * iou, np.abs(smask) / (N * pix) + k * iou_A
    w_rgb = lam_rgb if (lam_rgb > 0 or not gate) else 0.0
    w_sil = lam_sil if (lam_sil > 0 or not gate) else 0.0
    val = np.array([w_rgb * rgb + w_sil * sil, w_rgb * rgb, w_sil * sil, iou])
    A = np.array([abs(w_rgb * rgb) + abs(w_sil) * sil_A, abs(w_rgb * rgb), abs(w_sil) * sil_A, iou_A])
    return val, A


def sign3(x, y):
    """the sign of x - y decided on the two fp32 operands (no difference is formed: it could round to zero)"""
    return (x > y).astype(F64) - (x < y).astype(F64)


def grad_of(c, sums, lam, grad_total=None, rows=None, dtype=F64, mut=None, gate=True):
    """d total / d rgba on the rows `rows` from given `sums` (N + 1, 5) -> (grad, A), each (N, r, W, 4) float64"""
    rgba, img, mask = band_arrays(c, rows, mut)
    N, r, W = c.N, rgba.shape[1], c.W
    lam_rgb, lam_sil = (float(v) for v in lam)
    pix = (r * W) if mut == "l1_mean_over_band" else c.H * W
    up = 1.0 if (grad_total is None or mut == "grad_total_ignored") else float(grad_total)
    cnt = sums[N, 0]
    I, U = sums[:N, 3].reshape(N, 1, 1), sums[:N, 4].reshape(N, 1, 1)
    a32, t32 = rgba[..., 3], mask
    inside = inside_of(a32, t32, mut)
    w_rgb = lam_rgb / cnt if (cnt > 0 and (lam_rgb > 0 or not gate)) else 0.0
    if mut == "rgb_mean_over_3cnt":
        w_rgb /= 3.0
    on = lam_sil > 0 or not gate
    w_l1 = lam_sil / (N * pix) if on else 0.0
    flip = -1.0 if mut == "sign_flipped" else 1.0
    s_rgb = np.where(inside[..., None], flip * sign3(rgba[..., :3], img), 0.0)
    s_a = flip * sign3(a32, t32)
    t = t32.astype(F64)
    Ue = _denominator(U)
    one_minus_t = (t32 == 0).astype(F64) if mut == "iou_no_one_minus_t" else 1.0 - t
    full = -(t * Ue - I * one_minus_t) / (Ue * Ue)
    diou = full if mut == "clamp_branch_full_formula" else np.where(np.abs(U) > EPS, full, -t / Ue)
    t2 = lam_sil * (1.0 if mut == "no_001" else 0.01) * diou
    t2 = (t2 if mut == "iou_no_over_n" else t2 / N) if on else np.zeros_like(t2)
    g, A = np.empty((N, r, W, 4)), np.empty((N, r, W, 4))
    A[..., :3], A[..., 3] = np.abs(w_rgb * s_rgb * up), (np.abs(w_l1 * s_a) + np.abs(t2)) * abs(up)
    if dtype == F64:
        g[..., :3], g[..., 3] = w_rgb * s_rgb * up, (w_l1 * s_a + t2) * up
    else:
        up32 = F32(up)
        g[..., :3] = (F32(w_rgb) * s_rgb.astype(F32)) * up32
        g[..., 3] = (F32(w_l1) * s_a.astype(F32) + t2.astype(F32)) * up32
    return g, A


def contiguous(bounds):
    return [np.arange(bounds[g], bounds[g + 1]) for g in range(len(bounds) - 1)]


def cyclic(H, G):
    """tile-row-cyclic bands: rank g owns the 8-row tile rows g, g + G, ..."""
    return [np.array([t * 8 + i for t in range(g, -(-H // 8), G) for i in range(8) if t * 8 + i < H], np.int64) for g in range(G)]


def reference_of(c, lam=(1.0, 1.0), grad_total=None, dtype=F64, mut=None, bands=None, order="lanes", gate=True, grad_sums=None):
    """The whole operation on case `c` -> sums / losses / grad with their `_A`.  ``bands``: lists of image rows; their sums are
    added in fp64 as the all-reduce adds them, and the gradient is evaluated band by band.  ``grad_sums``: the sums that the
    gradient is given (default: the ones computed here)."""
    bands = [np.arange(c.H)] if bands is None else bands
    nb = None if len(bands) == 1 else MAX_BLOCKS
    parts = [band_sums(c, rows, dtype, mut, nb, order) for rows in bands]
    sums, sums_A = finalize(sum(p[0] for p in parts), sum(p[1] for p in parts), mut)
    losses, losses_A = losses_of(sums, c.H * c.W, lam, mut, gate)
    if dtype != F64:
        losses = losses.astype(F32).astype(F64)
    grad, grad_A = np.zeros((c.N, c.H, c.W, 4)), np.zeros((c.N, c.H, c.W, 4))
    for rows in bands:
        if len(rows):
            grad[:, rows], grad_A[:, rows] = grad_of(c, sums if grad_sums is None else grad_sums, lam, grad_total, rows, dtype,
                                                     mut, gate)
    return types.SimpleNamespace(sums=sums, sums_A=sums_A, losses=losses, losses_A=losses_A, grad=grad, grad_A=grad_A)


@functools.lru_cache(maxsize=None)
def ref(name, lam=LAMBDAS[0], grad_total=None):
    return reference_of(case(name), lam, grad_total)


def alpha_plane(alpha, mut=None):
    """The alpha channel (N, r, W) of a band gradient written a second time into the (row, camera, col) send buffer of r + 3
    rows prefilled with 7 -> the buffer.  `alpha_out_dense_strides` writes it with the dense strides (r W, W)."""
    N, r, W = alpha.shape
    buf = np.full((r + 3, N, W), 7.0)
    if mut == "alpha_out_dense_strides":
        buf.reshape(-1)[: alpha.size] = alpha.reshape(-1)
    else:
        buf[:r] = alpha.transpose(1, 0, 2)
    return buf


# ------------------------------------------------------------------------------------------------------------------------
# error measure, figures, bars
# ------------------------------------------------------------------------------------------------------------------------
def rel_err(got, want, A):
    """per entry |got - want| / A (floor 1e-30); where A == 0 the entry is expected exactly: 0 or inf"""
    got, want, A = np.asarray(got, F64), np.asarray(want, F64), np.asarray(A, F64)
    with np.errstate(all="ignore"):
        err = np.abs(got - want) / np.maximum(A, FLOOR)
    err = np.where(A == 0, np.where(got == want, 0.0, np.inf), err)
    return np.where(np.isnan(err), np.inf, err)


def violation(got, want, A, bar):
    """the largest per-entry error in units of the bar (a bar of 0 asks for the exact value)"""
    err = rel_err(got, want, A)
    worst = float(err.max()) if err.size else 0.0
    if bar == 0:
        return 0.0 if worst == 0 else np.inf
    return worst / bar


def variants():
    return [(lam, gt) for lam in LAMBDAS for gt in GRAD_TOTALS]


@functools.lru_cache(maxsize=None)
def case_figures(name):
    """{output: the largest per-entry error of the fp32 restatement on the case}, over both lambda pairs, both `grad_total`
    and the three orders of the wavefront's additions.  The gradient is restated from the reference's sums: it is a function of
    given fp64 sums, and the IoU part -(t U - I (1 - t)) / U^2 would magnify a change of its input where t U meets I (1 - t)."""
    c, figs = case(name), dict.fromkeys(OUTPUTS, 0.0)
    for order in ORDERS:
        for lam, gt in variants():
            r = ref(name, lam, gt)
            f = reference_of(c, lam, gt, dtype=F32, order=order, grad_sums=r.sums)
            for o in OUTPUTS:
                figs[o] = max(figs[o], float(rel_err(getattr(f, o), getattr(r, o), getattr(r, o + "_A")).max()))
    return figs


# mutation: (the output it must show in, the cases on which it must lie 10x beyond the bar, bands of those cases or None)
_SOFT_BIG = ["soft_1x64x64", "soft_3x37x53", "soft_1x512x512"]
BANDS_3x128 = (0, 40, 41, 128)
MUTATIONS = {
    "inside_half": ("sums", _SOFT_BIG, None),
    "inside_product": ("sums", _SOFT_BIG, None),
    "union_max": ("sums", _SOFT_BIG + ["soft_1x1x5"], None),
    "inter_min": ("sums", _SOFT_BIG + ["soft_1x1x5"], None),
    "iou_no_one_minus_t": ("grad", _SOFT_BIG, None),
    "iou_no_over_n": ("grad", ["soft_3x37x53", "soft_2x3x1021", "bin_5x8x8"], None),
    "no_001": ("grad", _SOFT_BIG + ["bin_3x37x53"], None),
    "l1_mean_over_band": ("grad", ["soft_3x128x20"], BANDS_3x128),
    "rgb_mean_over_3cnt": ("grad", _SOFT_BIG + ["bin_3x37x53"], None),
    "sign_flipped": ("grad", _SOFT_BIG + ["bin_1x1x1"], None),
    "grad_total_ignored": ("grad", _SOFT_BIG + ["bin_1x1x5"], None),
    "mask_stride_band": ("sums", ["soft_3x128x20"], BANDS_3x128),
    "target_strides_swapped": ("sums", ["soft_3x37x53", "soft_1x17x241", "bin_2x3x1021"], None),
    "second_trip_dropped": ("sums", ["soft_1x513x512", "soft_1x641x512", "bin_1x513x512"], None),
    "tail_slot_dropped": ("sums", ["soft_1x641x512", "soft_1x17x241", "bin_1x641x512"], None),
    "last_block_dropped": ("sums", ["soft_1x17x241", "soft_1x512x512", "bin_1x513x512"], None),
    "images_from_4_dropped": ("sums", ["soft_5x8x8", "soft_65x3x5", "bin_65x3x5"], None),
    "clamp_branch_full_formula": ("grad", ["soft_3x37x53", "soft_5x8x8"], None),
    "alpha_out_dense_strides": ("alpha_out", ["soft_2x72x20"], None),
}
BINARY_BLIND = ["inside_half", "inside_product", "union_max", "inter_min", "iou_no_one_minus_t"]   # what binary data cannot see
