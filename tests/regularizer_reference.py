"""Float64 yardstick of the point-cloud regularisers and of the in-mask filter (dss_amd/csrc/regularizers.hip), with the
magnitude of every output entry, plus a restatement of the same formulas in a chosen dtype.

The formulas are those of the reference (DSS/training/losses.py:148-495, DSS/models/point_modeling.py:188-212), on the
PACKED layout: `first` / `num` give the row range of every cloud, `knn_idx` holds cloud-local ids with the point itself
in column 0 (losses.py:177-179 drops that column), lists of a cloud shorter than K are zero-padded (idx 0, distance 0)
as pytorch3d pads them and are used as they stand (the reference builds `knn_mask` and never applies it).

    phi_k      = max(0, 1 - d_k / (4 mean_k d_k))^4                                   get_phi          :261-276
    mollified  = sum_k phi_k n_j / eps_denom(sum_k phi_k), own normal where keep      _denoise_normals :182-220
    normal_w_k = exp(-|u_j - u_i|^2 / sigma^2), u = F.normalize(mollified)            get_normal_w     :222-245
    projection   w_k = phi_k normal_w_k (visible_j ? 1 : 0.1f)                                         :324-346
                 sdf_k = (x_j - p_i) . m_j ;  loss_i = sum_k w_k sdf_k^2 / eps_denom(sum_k w_k)        :372-389
    repulsion    s_k = exp(-|x_j - p_i|^2 (num_n / diag_n^2) filter_scale);  w_k = s_k normal_w_k      :247-259, :467-472
                 r = sum_k w_k (I - m_j m_j^T)(p_i - x_j) / eps_denom(sum_k w_k) * (1 + sum_k s_k)     :436-485
                 loss_ic = exp(-|r_c|)                                                                 :487
Every weight is a constant for autograd (no_grad blocks, .detach() on the neighbour positions), so only p_i carries a
gradient: d loss_i / d p_i = -2 sum_k w_k sdf_k m_j / den, and d r_c / d p_e = sum_k w_k (delta_ce - m_jc m_je) * density / den.

Error measure (as tests/shading_reference.py): |got - want| / magnitude with a 1e-30 floor, where the magnitude of an
entry is the sum of the absolute values of every product added to form it -- down to the three products of `sdf` and
of the dot product inside the projector.  For exp(-|r|) the error of r is carried over: magnitude = loss (1 + mag r),
and the repulsion gradient uses that magnitude for its factor loss_c.  A magnitude of 0 marks an entry the formula
has no term for (a kept normal, a row no cloud owns): the expectation there is exact.

The yardstick takes the kernel's inputs (float32 values) and computes in float64.  `restate_*` are the same formulas
with every operation in `dtype`; they size the bars of tests/test_gpu_regularizers.py and carry the one-line mutations
of tests/test_regularizers_cpu.py.  Neither is the code under test.
"""
import numpy as np

F64 = np.float64
VIS_W = np.float32(0.1)   # visibility_w is a float32 tensor in the reference whatever the points' dtype (:339-340)
MUTATIONS = ("drop_last", "include_self", "h_mean_over_K", "normal_w_raw", "sdf_unit_normals", "visible_of_point",
             "invisible_is_zero", "ignore_keep", "no_first_idx", "cloud0_spatial", "no_filter_scale", "density_no_plus1",
             "flip_negative_sign", "ignore_grad_loss", "eps_denom0_is_0", "no_normalize_clamp")


def cloud_of(P, first, num):
    """(P,) cloud of every packed row, -1 for a row no cloud owns."""
    c = np.full(P, -1, np.int64)
    for n, (f, l) in enumerate(zip(first, num)):
        c[int(f): int(f) + int(l)] = n
    return c


def brute_knn(points, first, num, K):
    """Self query by float64 brute force -> (d2 float32 (P,K), idx int64 (P,K) cloud-local).  The point itself is column
    0 whatever coincides with it; ties keep the lower id; a cloud shorter than K is zero-padded; unowned rows are 0."""
    P = points.shape[0]
    d2, idx = np.zeros((P, K), np.float32), np.zeros((P, K), np.int64)
    for f, l in zip(first, num):
        f, l = int(f), int(l)
        if l == 0:
            continue
        x = points[f: f + l].astype(F64)
        d = ((x[:, None] - x[None]) ** 2).sum(-1)
        d[np.arange(l), np.arange(l)] = -1.0
        order = np.argsort(d, axis=1, kind="stable")[:, :K]
        k = order.shape[1]
        idx[f: f + l, :k] = order
        d2[f: f + l, :k] = np.take_along_axis(d, order, 1)
        d2[f: f + l, 0] = 0
    return d2, idx


def eps_denom(d, eps=1e-17):   # utils/mathHelper.py:10-14
    return (np.sign(d) + (d == 0)) * np.maximum(np.abs(d), eps)


def _unit(v):                  # F.normalize(dim=-1), eps 1e-12
    return v / np.maximum(np.sqrt((v * v).sum(-1, keepdims=True)), 1e-12)


def _neighbours(P, knn_idx, first, num):
    c = cloud_of(P, first, num)
    owned = c >= 0
    base = np.where(owned, np.asarray(first, np.int64)[np.maximum(c, 0)], 0)
    j = base[:, None] + knn_idx[:, 1:]
    j[~owned] = 0
    return c, owned, j


def _phi(d):
    h = d.mean(-1, keepdims=True) * 4
    w = 1 - d / h
    w = np.where(w < 0, 0.0, w)   # NaN (h == 0) stays NaN, like w[w < 0] = 0
    w = w * w
    return w * w


def mollify_normals(normals, knn_d2, knn_idx, keep, first, num):
    """-> (mollified (P,3), magnitude (P,3))"""
    with np.errstate(all="ignore"):
        n = np.asarray(normals, F64)
        _, owned, j = _neighbours(len(n), knn_idx, first, num)
        w = _phi(np.asarray(knn_d2, F64)[:, 1:])
        terms = w[:, :, None] * n[j]
        den = eps_denom(w.sum(1))[:, None]
        out, mag = terms.sum(1) / den, np.abs(terms).sum(1) / np.abs(den)
        kept = ~owned if keep is None else (~owned | np.asarray(keep, bool))
        out[kept], mag[kept] = n[kept], 0.0
    return out, mag


def _normal_w(m, j, sigma):
    u = _unit(m)
    diff = u[j] - u[:, None]
    return np.exp(-(diff * diff).sum(-1) * (1 / (sigma * sigma)))


def projection_loss(points, mollified, knn_d2, knn_idx, visible, first, num, sigma, grad_loss=None):
    """-> (loss (P,), its magnitude, grad_points (P,3), its magnitude); grad_loss None = ones"""
    with np.errstate(all="ignore"):
        x, m = np.asarray(points, F64), np.asarray(mollified, F64)
        P = len(x)
        _, owned, j = _neighbours(P, knn_idx, first, num)
        vis_w = np.ones(P) if visible is None else np.where(np.asarray(visible, bool), 1.0, F64(VIS_W))
        w = _phi(np.asarray(knn_d2, F64)[:, 1:]) * _normal_w(m, j, sigma) * vis_w[j]
        a = (x[j] - x[:, None]) * m[j]                       # the three products of sdf
        sdf, sabs = a.sum(-1), np.abs(a).sum(-1)
        den = eps_denom(w.sum(1))
        loss, loss_mag = (w * sdf * sdf).sum(1) / den, (w * sabs * sabs).sum(1) / np.abs(den)
        gl = np.ones(P) if grad_loss is None else np.asarray(grad_loss, F64)
        grad = gl[:, None] * (-2 * (w * sdf)[:, :, None] * m[j]).sum(1) / den[:, None]
        grad_mag = np.abs(gl)[:, None] * (2 * (w * sabs)[:, :, None] * np.abs(m[j])).sum(1) / np.abs(den)[:, None]
        loss[~owned], loss_mag[~owned], grad[~owned], grad_mag[~owned] = 0.0, 0.0, 0.0, 0.0
    return loss, loss_mag, grad, grad_mag


def spatial_inv_sigma(points, first, num):
    """(N,) num_points / |bounding-box diagonal|^2 (get_spatial_w, :251-253); NaN for an empty cloud"""
    out = np.full(len(first), np.nan)
    with np.errstate(all="ignore"):
        for n, (f, l) in enumerate(zip(first, num)):
            if l > 0:
                x = np.asarray(points[int(f): int(f) + int(l)], F64)
                out[n] = F64(np.float32(l)) / ((x.max(0) - x.min(0)) ** 2).sum()
    return out


def repulsion_loss(points, mollified, knn_idx, first, num, sigma, filter_scale, grad_loss=None, inv_sigma=None):
    """-> (loss (P,3), its magnitude, grad_points (P,3), its magnitude).  A row no cloud owns holds loss 1, gradient 0:
    what the kernel writes there (every sum empty, r = 0).  ``inv_sigma`` (N,) replaces num / diag^2 (the oracle's
    interface takes that factor, rounded to float32, from its caller)."""
    with np.errstate(all="ignore"):
        x, m = np.asarray(points, F64), np.asarray(mollified, F64)
        P = len(x)
        c, owned, j = _neighbours(P, knn_idx, first, num)
        inv_sigma = (spatial_inv_sigma(x, first, num) if inv_sigma is None else np.asarray(inv_sigma, F64))[np.maximum(c, 0)]
        df, mj = x[:, None] - x[j], m[j]
        s = np.exp(-(df * df).sum(-1) * inv_sigma[:, None] * filter_scale)
        w = s * _normal_w(m, j, sigma)
        dotp = df * mj                                        # the three products of the projector's dot product
        proj = df - dotp.sum(-1, keepdims=True) * mj
        proj_mag = np.abs(df) + np.abs(dotp).sum(-1, keepdims=True) * np.abs(mj)
        den = eps_denom(w.sum(1))[:, None]
        density = (s.sum(1) + 1.0)[:, None]
        r = (proj * w[:, :, None]).sum(1) / den * density
        r_mag = (proj_mag * w[:, :, None]).sum(1) / np.abs(den) * density
        loss = np.exp(-np.abs(r))
        loss_mag = loss * (1 + r_mag)
        gl = np.ones((P, 3)) if grad_loss is None else np.asarray(grad_loss, F64)
        eye = np.eye(3)
        A = (w[:, :, None, None] * (eye - mj[:, :, :, None] * mj[:, :, None, :])).sum(1)               # (P,c,e)
        A_mag = (w[:, :, None, None] * (eye + np.abs(mj[:, :, :, None] * mj[:, :, None, :]))).sum(1)
        scale = density / den
        grad = ((gl * -np.sign(r) * loss)[:, :, None] * A).sum(1) * scale
        grad_mag = ((np.abs(gl) * loss_mag)[:, :, None] * A_mag).sum(1) * np.abs(scale)
        loss[~owned], loss_mag[~owned], grad[~owned], grad_mag[~owned] = 1.0, 0.0, 0.0, 0.0
    return loss, loss_mag, grad, grad_mag


def rel_err(got, want, mag):
    """Per-entry |got - want| / max(magnitude, 1e-30); inf where exactly one of the two is NaN, 0 where both are."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    with np.errstate(all="ignore"):
        e = np.abs(got - want) / np.maximum(np.nan_to_num(np.asarray(mag, F64), nan=0.0, posinf=np.inf), 1e-30)
    both, one = np.isnan(got) & np.isnan(want), np.isnan(got) != np.isnan(want)
    e[both] = 0.0
    e[one] = np.inf
    return e


# ---------------------------------------------------------------------------------------------------------------------
# The same formulas with every operation in `dtype`.  `mut` names one deliberate one-line defect (MUTATIONS).
# ---------------------------------------------------------------------------------------------------------------------
def _r_eps_denom(d, T, mut):
    zero = T(0) if mut == "eps_denom0_is_0" else T(1)
    return (np.sign(d) + (d == 0) * zero).astype(T) * np.maximum(np.abs(d), T(1e-17))


def _r_unit(v, T, mut):
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    return v / (n if mut == "no_normalize_clamp" else np.maximum(n, T(1e-12)))


def _r_cols(K, mut):
    return slice(0, K) if mut == "include_self" else slice(1, K - 1) if mut == "drop_last" else slice(1, K)


def _r_neighbours(P, knn_idx, first, num, mut):
    c = cloud_of(P, first, num)
    owned = c >= 0
    base = np.where(owned, np.asarray(first, np.int64)[np.maximum(c, 0)], 0)
    if mut == "no_first_idx":
        base = np.zeros_like(base)
    j = base[:, None] + knn_idx[:, _r_cols(knn_idx.shape[1], mut)]
    j[~owned] = 0
    return c, owned, j


def _r_phi(knn_d2, T, mut):
    K = knn_d2.shape[1]
    d = knn_d2.astype(T)[:, _r_cols(K, mut)]
    h = d.sum(-1, keepdims=True) / T(K if mut == "h_mean_over_K" else d.shape[1]) * T(4)
    w = T(1) - d / h
    w = np.where(w < 0, T(0), w)
    w = w * w
    return w * w


def _r_normal_w(m, j, sigma, T, mut):
    u = m if mut == "normal_w_raw" else _r_unit(m, T, mut)
    diff = u[j] - u[:, None]
    return np.exp(-(diff * diff).sum(-1) * (T(1) / (T(sigma) * T(sigma))))


def restate_mollify(normals, knn_d2, knn_idx, keep, first, num, dtype=np.float32, mut=None):
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        n = np.asarray(normals).astype(T)
        _, owned, j = _r_neighbours(len(n), knn_idx, first, num, mut)
        w = _r_phi(np.asarray(knn_d2), T, mut)
        out = (w[:, :, None] * n[j]).sum(1) / _r_eps_denom(w.sum(1), T, mut)[:, None]
        kept = ~owned if (keep is None or mut == "ignore_keep") else (~owned | np.asarray(keep, bool))
        out[kept] = n[kept]
    assert out.dtype == T
    return out


def restate_projection(points, mollified, knn_d2, knn_idx, visible, first, num, sigma, grad_loss=None, dtype=np.float32,
                       mut=None):
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        x, m = np.asarray(points).astype(T), np.asarray(mollified).astype(T)
        P = len(x)
        _, owned, j = _r_neighbours(P, knn_idx, first, num, mut)
        low = T(0) if mut == "invisible_is_zero" else T(VIS_W)
        vis_w = np.ones(P, T) if visible is None else np.where(np.asarray(visible, bool), T(1), low)
        vis_nb = np.broadcast_to(vis_w[:, None], j.shape) if mut == "visible_of_point" else vis_w[j]
        w = _r_phi(np.asarray(knn_d2), T, mut) * _r_normal_w(m, j, sigma, T, mut) * vis_nb
        mj = m[j]
        sdf = ((x[j] - x[:, None]) * (_r_unit(m, T, mut)[j] if mut == "sdf_unit_normals" else mj)).sum(-1)
        den = _r_eps_denom(w.sum(1), T, mut)
        loss = (w * sdf * sdf).sum(1) / den
        gl = np.ones(P, T) if (grad_loss is None or mut == "ignore_grad_loss") else np.asarray(grad_loss).astype(T)
        grad = gl[:, None] * (T(-2) * (w * sdf)[:, :, None] * mj).sum(1) / den[:, None]
        loss[~owned], grad[~owned] = 0, 0
    assert loss.dtype == T and grad.dtype == T
    return loss, grad


def restate_repulsion(points, mollified, knn_idx, first, num, sigma, filter_scale, grad_loss=None, dtype=np.float32,
                      mut=None):
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        x, m = np.asarray(points).astype(T), np.asarray(mollified).astype(T)
        P = len(x)
        c, owned, j = _r_neighbours(P, knn_idx, first, num, mut)
        inv = np.full(len(first), np.nan, T)
        for n, (f, l) in enumerate(zip(first, num)):
            if l > 0:
                box = x[int(f): int(f) + int(l)]
                inv[n] = T(l) / ((box.max(0) - box.min(0)) ** 2).sum()
        inv_sigma = inv[np.zeros_like(c) if mut == "cloud0_spatial" else np.maximum(c, 0)]
        df, mj = x[:, None] - x[j], m[j]
        s = np.exp(-(df * df).sum(-1) * inv_sigma[:, None] * T(1 if mut == "no_filter_scale" else filter_scale))
        w = s * _r_normal_w(m, j, sigma, T, mut)
        proj = df - (df * mj).sum(-1, keepdims=True) * mj
        den = _r_eps_denom(w.sum(1), T, mut)[:, None]
        density = (s.sum(1) + T(0 if mut == "density_no_plus1" else 1))[:, None]
        r = (proj * w[:, :, None]).sum(1) / den * density
        loss = np.exp(-np.abs(r))
        gl = np.ones((P, 3), T) if (grad_loss is None or mut == "ignore_grad_loss") else np.asarray(grad_loss).astype(T)
        A = (w[:, :, None, None] * (np.eye(3, dtype=T) - mj[:, :, :, None] * mj[:, :, None, :])).sum(1)
        sign = np.abs(np.sign(r)) if mut == "flip_negative_sign" else np.sign(r)   # -l for r > 0, +l for r < 0
        grad = ((gl * -sign * loss)[:, :, None] * A).sum(1) * (density / den)
        loss[~owned], grad[~owned] = 1, 0
    assert loss.dtype == T and grad.dtype == T
    return loss, grad


# ---------------------------------------------------------------------------------------------------------------------
# In-mask filter (point_modeling.py:188-212, utils/__init__.py get_tensor_values): float64 projection p_h @ M, the
# position clamp(-ndc_xy, -1, 1), F.grid_sample(bilinear, reflection, align_corners=False) != 0, any over the views,
# & visible.  Inside [-1, 1] the reflection is the identity, so the unnormalised coordinate is only clipped to
# [0, size - 1].  A NaN position (NaN coordinate, 0/0 projection) is NEVER in mask: the documented decision of the
# kernel (torch's CPU grid_sample returns the value of its clipped corner pixel for a NaN position instead).
# ---------------------------------------------------------------------------------------------------------------------
def sample_positions(points, M):
    """-> (gx, gy) (N,P) float64: clamp(-ndc, -1, 1), NaN kept"""
    with np.errstate(all="ignore"):
        ph = np.concatenate([np.asarray(points, F64), np.ones((len(points), 1))], 1)
        c = np.einsum("pi,nij->npj", ph, np.asarray(M, F64))
        g = -c[..., :2] / c[..., 3:4]
        g = np.where(np.isnan(g), np.nan, np.clip(g, -1.0, 1.0))
    return g[..., 0], g[..., 1]


def bilinear_sample(img, gx, gy):
    """grid_sample(bilinear, reflection, align_corners=False) of one (H,W) image at positions inside [-1,1] ->
    (value, margin): margin = distance in pixels of the position to the nearest place where a tap's weight reaches 0."""
    H, W = img.shape
    img = np.asarray(img, F64)
    ux, uy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    ix, iy = np.clip(ux, 0, W - 1), np.clip(uy, 0, H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    fx, fy = ix - x0, iy - y0
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    inx, iny = (x0 + 1 < W), (y0 + 1 < H)
    v = img[y0, x0] * ((1 - fx) * (1 - fy)) + inx * img[y0, x1] * (fx * (1 - fy)) + iny * img[y1, x0] * ((1 - fx) * fy) \
        + (inx & iny) * img[y1, x1] * (fx * fy)

    def margin(u, size):   # outside [0, size-1] the clip holds the coordinate: the nearest boundary is the clip's edge
        return np.where(u < 0, -u, np.where(u > size - 1, u - (size - 1), np.abs(u - np.round(u))))
    return v, np.minimum(margin(ux, W), margin(uy, H))


def points_inmask(points, M, mask, visible=None):
    """-> (inmask bool (P,), margin (P,) pixels: the smallest distance over the views to a decision boundary)"""
    gx, gy = sample_positions(points, M)
    P = len(points)
    flag, margin = np.zeros(P, bool), np.full(P, np.inf)
    for n in range(len(M)):
        ok = ~(np.isnan(gx[n]) | np.isnan(gy[n]))
        v, mg = bilinear_sample(mask[n], np.where(ok, gx[n], 0.0), np.where(ok, gy[n], 0.0))
        flag |= ok & (v != 0)
        margin = np.minimum(margin, np.where(ok, mg, np.inf))
    if visible is not None:
        flag &= np.asarray(visible, bool)
    return flag, margin
