"""Float64 yardstick of the two tools that clean a cloud (the reference: `denoise_normals` and
`project_to_latent_surface`, DSS/core/cloud.py:515-552 and :442-513), brute force, written from the contract and stated once
for the CPU tests, the GPU tests and the timing script.  Everything after the lists is torch in the dtype of the inputs:
float64 is the yardstick, float32 is the eager form a user would run on the GPU (and shows what fp32 can hold).

Neighbourhood of a point (both tools): entries 1 .. K of its (distance, id) ordered list, self dropped.  The LIST is the
contract of `dss_knn_points`: fp32 distances in the form (dx dx + dy dy) + dz dz on the fp32 positions, ordered by a stable
sort (`lists`, the arithmetic of upsample_reference.knn_lists).  Entry j is LIVE iff it is a real point (j < P - 1) and its
list distance d_j < r^2, both sides fp32; r = `search_radius` or min(c K sqrt(diag / P), 0.2), diag the length of the
bounding-box diagonal, c = 4 (filter) or 16 (projection).  A dead entry contributes nothing.

Filter      n = normalize(normal), wn_j = exp(-((1 - n_j.n) / sigma)^2), inv = P / 2, dp_j = |q_j - p|^2,
            wp_j = exp(-dp_j inv) if dp_j <= 16 / inv else 0, out = normalize(sum wn_j wp_j n_j); a point whose weights sum
            to 0 keeps n.  F.normalize with eps 1e-12.
Projection  lists, the neighbours' normalised normals and inv = 1 / (16 d_0) (d_0 the list distance of the nearest live
            neighbour) are fixed from the input; a point without live neighbour or with d_0 = 0 is never live.  An outer
            iteration, for every live point, from the positions of the iteration before: diff_j = p - q_j, fx_j = diff_j.n_j,
            alpha_j = 1, f = 0, g = 0; `max_est_iter` times: [from the second pass on alpha_j = exp(-(|n_j - g| / 0.5)^2)
            exp(-(fx_j - f)^2 inv / 4)]; phi_j = exp(-|diff_j|^2 inv), w_j = phi_j alpha_j, gw_j = 2 diff_j inv phi_j w_j,
            f = sum w_j fx_j / eps_denom(sum w_j), g = (sum gw_j fx_j - f sum gw_j + sum w_j n_j) / eps_denom(sum w_j).
            Then move = f g, p <- p - move, live iff |move| > 5e-4.
It also reports how close every decision was: the convergence margin min | |move| / 5e-4 - 1 | and the radius margin
min | d_j / r^2 - 1 |.
"""
import numpy as np
import torch
import torch.nn.functional as F

MOVE_EPS = 5e-4
SCENES = {"plane": (0.0, 3), "paraboloid": (0.3, 2)}   # name -> (c of z = c (x^2 + y^2), seed)
P_SCENE = 1500


def scene(name, P=P_SCENE):
    """Noisy patch of z = c (x^2 + y^2) over [-0.5, 0.5]^2 -> (points (P,3), normals (P,3), true normals (P,3)): fp32
    roundings of 0.4 % position noise along the true normal and 10 % normal noise; the true normals in float64."""
    c, seed = SCENES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(P, 3, dtype=torch.float64, generator=g) - 0.5
    n_true = F.normalize(torch.stack([-2 * c * x[:, 0], -2 * c * x[:, 1], torch.ones(P, dtype=torch.float64)], dim=1), dim=1)
    x[:, 2] = c * (x[:, 0] ** 2 + x[:, 1] ** 2)
    x = x + n_true * 0.004 * torch.randn(P, 1, dtype=torch.float64, generator=g)
    normals = F.normalize(n_true + 0.1 * torch.randn(P, 3, dtype=torch.float64, generator=g), dim=1)
    return x.numpy().astype(np.float32), normals.numpy().astype(np.float32), n_true.numpy()


def sphere_scene(seed=0, P=1000):
    """upsample_reference.sphere_scene with normals: the radial direction with 10 % noise -> (points, normals) float32.  At
    this density the default radius of 0.2 and the filter's 32 / P cut both remove neighbours."""
    import upsample_reference
    x = upsample_reference.sphere_scene(seed, P)
    g = torch.Generator().manual_seed(seed + 100)
    xt = torch.from_numpy(x).double()
    n = F.normalize(F.normalize(xt, dim=1) + 0.1 * torch.randn(P, 3, dtype=torch.float64, generator=g), dim=1)
    return x, n.numpy().astype(np.float32)


def surface_distance(name, pts):
    """rms of z - c (x^2 + y^2) (the vertical distance; the patches are flat or nearly so)"""
    c, _ = SCENES[name]
    p = np.asarray(pts, np.float64)
    return float(np.sqrt(np.mean((p[:, 2] - c * (p[:, 0] ** 2 + p[:, 1] ** 2)) ** 2)))


def normal_error(normals, n_true):
    n = np.asarray(normals, np.float64)
    return float(np.mean(1.0 - (n * n_true).sum(-1)))


def lists(pts, K):
    """-> (nb (P,K) int64, d (P,K) float32): ids and fp32 list distances of the K nearest OTHER points in (distance, id)
    order; a cloud of fewer than K + 1 points gets id 0 / distance 0 behind its P - 1 entries, like the zero padding of
    `dss_knn_points`."""
    p = np.asarray(pts).astype(np.float32)
    P = p.shape[0]
    nb = np.zeros((P, K), np.int64)
    dd = np.zeros((P, K), np.float32)
    k = min(K, P - 1)
    for s in range(0, P, 1024):
        d = p[s:s + 1024, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        order = np.argsort(d2, axis=1, kind="stable")[:, 1:k + 1]
        nb[s:s + 1024, :k] = order
        dd[s:s + 1024, :k] = np.take_along_axis(d2, order, axis=1)
    return nb, dd


def default_radius(pts, K, c):
    """min(c K sqrt(diag / P), 0.2) as float"""
    p = np.asarray(pts, np.float64)
    diag = float(np.linalg.norm(p.max(0) - p.min(0))) if p.shape[0] else 0.0
    return min(c * K * np.sqrt(diag / max(p.shape[0], 1)), 0.2)


def live_entries(d, P, radius):
    """(P,K) bool from the fp32 list distances: a real point and d_j < r^2 with r and r^2 rounded to fp32"""
    K = d.shape[1]
    r = np.float32(radius)
    r2 = r * r
    assert r2.dtype == np.float32 and d.dtype == np.float32
    return (np.arange(K)[None, :] < P - 1) & (d < r2)


def radius_margin(d, P, radius):
    """min | d_j / r^2 - 1 | over the real entries (1.0 when there is none)"""
    K = d.shape[1]
    real = np.broadcast_to(np.arange(K)[None, :] < P - 1, d.shape)
    if not real.any():
        return 1.0
    return float(np.abs(d[real].astype(np.float64) / float(radius) ** 2 - 1.0).min())


def eps_denom(d, eps=1e-17):   # DSS/utils/mathHelper.py:10-14
    return (d.sign() + (d == 0).to(d.dtype)) * d.abs().clamp(min=eps)


def denoise_from_lists(pts, normals, nb, live, sigma=30.0):
    """The filter on given lists, torch, in the dtype and on the device of `pts`.  nb (P,K) int64, live (P,K) bool."""
    P = pts.shape[0]
    n = F.normalize(normals, dim=-1, eps=1e-12)
    nj, q = n[nb], pts[nb]
    wn = torch.exp(-((1.0 - (nj * n[:, None, :]).sum(-1)) / sigma) ** 2)
    inv = P / 2.0
    dp = ((q - pts[:, None, :]) ** 2).sum(-1)
    wp = torch.exp(-dp * inv) * (dp <= 16.0 / inv)
    w = wn * wp * live
    out = F.normalize((w[..., None] * nj).sum(-2), dim=-1, eps=1e-12)
    return torch.where((w.sum(-1) > 0)[:, None], out, n)


def rimls_setup(normals, d, live):
    """what is fixed before the first step -> (normalised normals, inv (P,), can_move (P,) bool)"""
    n = F.normalize(normals, dim=-1, eps=1e-12)
    d0 = d[:, 0].to(normals.dtype)   # the list is ascending: the nearest live neighbour is its first entry, or there is none
    can = live[:, 0] & (d0 > 0)
    inv = torch.where(can, 1.0 / (16.0 * torch.where(can, d0, torch.ones_like(d0))), torch.zeros_like(d0))
    return n, inv, can


def rimls_step_from_lists(pts, n, nb, live, inv, alive, max_est_iter=5):
    """One outer iteration on ALL points (dense, no host decision; the result of a point that is not `alive` is dropped)
    -> (points, alive, |move| (P,))."""
    q, nj = pts[nb], n[nb]
    diff = pts[:, None, :] - q
    fx = (diff * nj).sum(-1)
    iv = inv[:, None]
    phi = torch.exp(-(diff * diff).sum(-1) * iv) * live
    f = torch.zeros_like(inv)
    g = torch.zeros_like(pts)
    alpha = torch.ones_like(fx)
    for it in range(max_est_iter):
        if it > 0:
            a = (nj - g[:, None, :]).norm(dim=-1) / 0.5
            alpha = torch.exp(-a ** 2) * torch.exp(-(fx - f[:, None]) ** 2 * iv / 4.0)
        w = phi * alpha
        gw = 2.0 * diff * (iv * phi * w)[..., None]
        den = eps_denom(w.sum(-1))
        f = (w * fx).sum(-1) / den
        g = ((gw * fx[..., None]).sum(-2) - f[:, None] * gw.sum(-2) + (w[..., None] * nj).sum(-2)) / den[:, None]
    move = f[:, None] * g
    size = move.norm(dim=-1)
    new = torch.where(alive[:, None], pts - move, pts)
    return new, alive & (size > MOVE_EPS), size


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def denoise(pts, normals, K=16, sigma=30.0, search_radius=None, dtype=torch.float64):
    """-> dict(normals (P,3) numpy, nb, d, live, radius, radius_margin)"""
    pts, normals = np.asarray(pts, np.float32), np.asarray(normals, np.float32)
    P = pts.shape[0]
    nb, d = lists(pts, K)
    r = default_radius(pts, K, 4.0) if search_radius is None else float(search_radius)
    live = live_entries(d, P, r)
    out = denoise_from_lists(_t(pts, dtype), _t(normals, dtype), torch.from_numpy(nb), torch.from_numpy(live), sigma)
    return dict(normals=out.numpy(), nb=nb, d=d, live=live, radius=r, radius_margin=radius_margin(d, P, r))


def project(pts, normals, K=31, max_proj_iters=10, max_est_iter=5, search_radius=None, dtype=torch.float64):
    """-> dict(points (P,3) numpy, converged (P,) bool, alive: list of (P,) bool after every step, states: list of (P,3)
    after every step, margin = the convergence margin, radius, radius_margin, nb, d, live)"""
    pts, normals = np.asarray(pts, np.float32), np.asarray(normals, np.float32)
    P = pts.shape[0]
    nb, d = lists(pts, K)
    r = default_radius(pts, K, 16.0) if search_radius is None else float(search_radius)
    live = live_entries(d, P, r)
    x, nbt, lt = _t(pts, dtype), torch.from_numpy(nb), torch.from_numpy(live)
    n, inv, alive = rimls_setup(_t(normals, dtype), torch.from_numpy(d), lt)
    margin, history, states = float("inf"), [], []
    for _ in range(max_proj_iters):
        was = alive
        x, alive, size = rimls_step_from_lists(x, n, nbt, lt, inv, alive, max_est_iter)
        if bool(was.any()):
            margin = min(margin, float((size[was].double() / MOVE_EPS - 1.0).abs().min()))
        history.append(alive.numpy().copy())
        states.append(x.numpy().copy())
    return dict(points=x.numpy(), converged=~alive.numpy(), alive=history, states=states, margin=margin, radius=r,
                radius_margin=radius_margin(d, P, r), nb=nb, d=d, live=live)
