"""Shared test helpers: seeded small scenes, camera construction for the oracles, comparison metrics."""
import math

import numpy as np

from oracle import OracleCamera


def look_at(center, target=(0, 0, 0), up=(0, 1.0, 0)):
    c = np.asarray(center, np.float64)
    f = np.asarray(target, np.float64) - c
    f /= np.linalg.norm(f)
    r = np.cross(np.asarray(up, np.float64), f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    R = np.stack([r, u, f])
    w2c = np.eye(4)
    w2c[:3, :3] = R
    w2c[:3, 3] = -R @ c
    return w2c


def oracle_camera(W, H, w2c, fx=None, fy=None, cx=None, cy=None, near=0.01, far=100.0, bg=(0, 0, 0), sh_degree=0):
    """Same arithmetic as the reference's setup_camera (/root/reference/src/tracking/helpers.py:10-33), numpy fp32."""
    fx = float(W) if fx is None else fx
    fy = float(W) if fy is None else fy
    cx = W / 2.0 if cx is None else cx
    cy = H / 2.0 if cy is None else cy
    w2c32 = np.asarray(w2c, np.float32)
    proj = np.array([[2 * fx / W, 0, -(W - 2 * cx) / W, 0], [0, 2 * fy / H, -(H - 2 * cy) / H, 0],
                     [0, 0, far / (far - near), -(far * near) / (far - near)], [0, 0, 1, 0]], np.float32)
    vm = np.ascontiguousarray(w2c32.T)
    full = (vm @ proj.T).astype(np.float32)
    campos = np.linalg.inv(w2c32.astype(np.float64))[:3, 3].astype(np.float32)
    return OracleCamera(H, W, W / (2 * fx), H / (2 * fy), np.asarray(bg, np.float32), 1.0, vm, full, sh_degree, campos)


def ring_camera(W, H, v=0, V=4, radius=4.0, height=0.8, **kw):
    th = 2 * math.pi * v / V + 0.3
    return oracle_camera(W, H, look_at((radius * math.cos(th), height, radius * math.sin(th))), **kw)


def random_gaussians(P, seed=0, scale_lo=0.02, scale_hi=0.3, spread=1.0, sh_M=0):
    rng = np.random.default_rng(seed)
    means = rng.uniform(-spread, spread, (P, 3)).astype(np.float32)
    scales = np.exp(rng.uniform(np.log(scale_lo), np.log(scale_hi), (P, 3))).astype(np.float32)
    rot = rng.normal(size=(P, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    op = (1 / (1 + np.exp(-rng.uniform(-2, 4, (P, 1))))).astype(np.float32)
    col = rng.uniform(0, 1, (P, 3)).astype(np.float32)
    out = dict(means3D=means, scales=scales, rotations=rot, opacities=op, colors_precomp=col)
    if sh_M:
        out["shs"] = (rng.normal(size=(P, sh_M, 3)) * 0.4).astype(np.float32)
    return out


def rel_err(a, b):
    """Norm-wise relative error: max|a-b| / max|b| (the metric behind every '<= 1e-4 rel' claim for
    tensors whose entries are sums with cancellation -- gradients)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def mixed_err(a, b, atol_frac=1e-4):
    """Element-wise |a-b| / (|b| + atol_frac * max|b|): max over elements."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / (np.abs(b) + atol_frac * (np.abs(b).max() + 1e-30))).max())


def row_err(a, b, floor_frac=1e-3):
    """Row-wise (per-Gaussian) relative error: for every row i,  max_j |a_ij - b_ij| / (max_j |b_ij| + floor_frac * max|b|).
    Returns (worst value, its row).  Tighter than ``rel_err``: a Gaussian whose gradient is 1e-3 of the tensor maximum must
    still be right to the stated relative tolerance, not to 1e-4 of the LARGEST gradient in the tensor."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0, -1
    a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    num = np.abs(a2 - b2).max(1)
    den = np.abs(b2).max(1) + floor_frac * (np.abs(b2).max() + 1e-300)
    r = num / den
    i = int(np.argmax(r))
    return float(r[i]), i


def row_err_quantiles(a, b, floor_frac=1e-3, qs=(0.5, 0.99, 0.9999)):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    r = np.abs(a2 - b2).max(1) / (np.abs(b2).max(1) + floor_frac * (np.abs(b2).max() + 1e-300))
    return [float(np.quantile(r, q)) for q in qs]


# ---- the frustum clamp edge (A.1-4): Gaussians whose fp32 txtz / tytz sits within a few ulp of +-1.3 tanfov ----

def frustum_decisions_fp32(cam, means3D):
    """The forward's clamp decision, replicated on the host: view-space position, txtz / tytz and the limit in fp32 with every
    operation separately rounded, in the forward's order (gsr_preprocess_fwd.hip, contraction off).  Returns (clamped [P,2] bool,
    (txtz, tytz) [P,2] float32, (limx, limy))."""
    v = np.asarray(cam.viewmatrix, np.float32).reshape(-1)
    p = np.asarray(means3D, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    pv = [((v[r] * x + v[4 + r] * y) + v[8 + r] * z) + v[12 + r] for r in range(3)]
    t = np.stack([pv[0] / pv[2], pv[1] / pv[2]], 1).astype(np.float32)
    lim = np.array([np.float32(1.3) * np.float32(cam.tanfovx), np.float32(1.3) * np.float32(cam.tanfovy)], np.float32)
    return (t < -lim) | (t > lim), t, lim


def frustum_decisions_mixed(cam, means3D):
    """The clamp decision of the per-Gaussian backward before it took the forward's: only the first product of each view-space
    coordinate widened to fp64 (``(real)view[0] * p.x + view[4] * p.y + ...``: the other two are fp32 products, rounded, then added in
    fp64), the division and the limit ``1.3f * (real)tanfovx`` in fp64.  Returns clamped [P,2] bool."""
    v = np.asarray(cam.viewmatrix, np.float32).reshape(-1)
    p = np.asarray(means3D, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    d = np.float64
    pv = [((d(v[r]) * x.astype(d) + (v[4 + r] * y).astype(d)) + (v[8 + r] * z).astype(d)) + d(v[12 + r]) for r in range(3)]
    t = np.stack([pv[0] / pv[2], pv[1] / pv[2]], 1)
    lim = np.array([d(np.float32(1.3)) * d(np.float32(cam.tanfovx)), d(np.float32(1.3)) * d(np.float32(cam.tanfovy))])
    return (t < -lim) | (t > lim)


def clamp_edge_camera(W=96, H=80, sh_degree=0):
    """The clamp-edge scenes' camera: a general orientation (every view-matrix entry nonzero) and an off-centre principal point."""
    return oracle_camera(W, H, look_at((3.1, 0.9, 1.7), target=(0.05, -0.1, 0.02)), fx=float(W), fy=float(W), cx=0.42 * W, cy=0.57 * H,
                         sh_degree=sh_degree)


def clamp_edge_scene(cam, n_edge=200, n_plain=300, seed=0, ulps=8, walk=64):
    """Seeded scene of ``n_edge`` Gaussians whose fp32 txtz (or tytz) lies within +-``ulps`` ulp of +-limx (limy) -- both axes, both
    signs, both sides of the limit -- among ``n_plain`` ordinary ones in front of the camera.

    Random placement in that band rarely lands where the two arithmetics of the old backward disagree, so each edge candidate is walked:
    its world x moves in 1-ulp steps (np.nextafter; 0, +1, -1, +2, ... up to ``walk`` steps) until ``frustum_decisions_fp32`` and
    ``frustum_decisions_mixed`` disagree on its axis while txtz stays in the band; a candidate with no such step keeps its first position in the band.  The
    edge Gaussians are large enough to reach into the image, so they receive gradient.  Returns (Gaussians dict, edge indices)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(cam.viewmatrix, np.float64).reshape(4, 4)      # view[c*4 + r] = w2c[r, c]
    R, tr = v[:3, :3].T, v[3, :3]
    _, _, lim = frustum_decisions_fp32(cam, np.zeros((1, 3), np.float32))
    pts = np.zeros((n_edge, 3), np.float32)
    for k in range(n_edge):
        ax, sgn = k % 2, (1.0 if (k // 2) % 2 == 0 else -1.0)
        L = np.float32(sgn) * lim[ax]
        tz = rng.uniform(2.5, 4.5)
        off = int(rng.integers(-ulps, ulps + 1))
        t_ax = float(L) + off * float(np.spacing(lim[ax]))
        t_other = rng.uniform(-0.8, 0.8) * float(lim[1 - ax]) / 1.3
        pvw = np.zeros(3)
        pvw[ax], pvw[1 - ax], pvw[2] = t_ax * tz, t_other * tz, tz
        w = (R.T @ (pvw - tr)).astype(np.float32)
        best = in_band = None
        for step in range(walk + 1):
            for s in ((step,) if step == 0 else (step, -step)):
                cand = w.copy()
                xs = cand[0]
                for _ in range(abs(s)):
                    xs = np.nextafter(xs, np.float32(np.inf) if s > 0 else np.float32(-np.inf))
                cand[0] = xs
                c32, t32, _ = frustum_decisions_fp32(cam, cand[None])
                if abs(float(t32[0, ax]) - float(L)) > ulps * float(np.spacing(lim[ax])):
                    continue
                in_band = cand if in_band is None else in_band
                if c32[0, ax] != frustum_decisions_mixed(cam, cand[None])[0, ax]:
                    best = cand
                    break
            else:
                continue
            break
        pts[k] = best if best is not None else (in_band if in_band is not None else w)
    g = random_gaussians(n_plain + n_edge, seed=seed + 1, scale_lo=0.03, scale_hi=0.2, spread=0.8)
    edge = np.arange(n_plain, n_plain + n_edge)
    g["means3D"][edge] = pts
    g["scales"][edge] = np.exp(rng.uniform(np.log(0.25), np.log(0.6), (n_edge, 3))).astype(np.float32)
    g["opacities"][edge] = rng.uniform(0.3, 0.9, (n_edge, 1)).astype(np.float32)
    return g, edge
