"""References of the anti-aliasing tests (test_antialias_cpu.py, test_antialias_gpu.py).

With A, B, C the projected 2D covariance before the 0.3 px^2 dilation h, the staged opacity is o' = o c with
    r = (A C - B^2) / ((A + h)(C + h) - B^2),   c = sqrt(max(r, 2.5e-5)).
  * ``aa_factor``: c(theta) in fp64 torch (autograd gives dc/dtheta; a floored Gaussian's c is a constant);
  * ``ratio_closed_grad``: the closed-form dr/d{A, B, C} the kernel uses;
  * ``aa_ratio32``: the forward's fp32 r, replicated on the host with the forward's operations in its order (its side of the floor);
  * ``aa_term`` / ``compose``: dL/do = c dL/do' and the covariance / position term dL/do' o dc/dtheta that turn the oracle's gradients
    (oracle fed o') into the anti-aliased render's.
"""
import numpy as np
import torch

H_DIL = 0.3
FLOOR = float(np.float32(2.5e-5))       # the kernels' 2.5e-5f


def cov2d_undilated(cam, means3D, scales=None, rotations=None, cov3D_precomp=None):
    """(A, B, C) [P] fp64 torch, the EWA projection of oracle/dense_oracle.py (frustum clamp: the clamped tx / ty are constants)."""
    f64 = torch.float64
    V = torch.as_tensor(np.asarray(cam.viewmatrix, np.float32).reshape(4, 4)).to(f64)
    P = means3D.shape[0]
    pv = (torch.cat([means3D, torch.ones(P, 1, dtype=f64)], 1) @ V)[:, :3]
    if cov3D_precomp is not None:
        c6 = cov3D_precomp
        Sig = torch.stack([torch.stack([c6[:, 0], c6[:, 1], c6[:, 2]], 1), torch.stack([c6[:, 1], c6[:, 3], c6[:, 4]], 1),
                           torch.stack([c6[:, 2], c6[:, 4], c6[:, 5]], 1)], 1)
    else:
        r, x, y, z = rotations[:, 0], rotations[:, 1], rotations[:, 2], rotations[:, 3]
        R = torch.stack([
            torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
            torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
            torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
        M = R * (scales * float(cam.scale_modifier))[:, None, :]
        Sig = M @ M.transpose(1, 2)
    W, H = cam.image_width, cam.image_height
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
    limx, limy = 1.3 * cam.tanfovx, 1.3 * cam.tanfovy
    tz = pv[:, 2]
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    xcl = (txtz < -limx) | (txtz > limx)
    ycl = (tytz < -limy) | (tytz > limy)
    tx = torch.where(xcl, (txtz.clamp(-limx, limx) * tz).detach(), pv[:, 0])
    ty = torch.where(ycl, (tytz.clamp(-limy, limy) * tz).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], 1),
                     torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], 1)], 1)
    T = J @ V[:3, :3].t()[None]
    cov2 = T @ Sig @ T.transpose(1, 2)
    return cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]


def ratio(A, B, C, h=H_DIL):
    return (A * C - B * B) / ((A + h) * (C + h) - B * B)


def ratio_closed_grad(A, B, C, h=H_DIL):
    """dr/dA, dr/dB, dr/dC in the cancellation-free forms of the kernel (B: the off-diagonal entry, det = A C - B^2)."""
    D = (A + h) * (C + h) - B * B
    D2 = D * D
    return h * (C * C + h * C + B * B) / D2, -2.0 * h * B * (A + C + h) / D2, h * (A * A + h * A + B * B) / D2


def aa_factor(cam, means3D, scales=None, rotations=None, cov3D_precomp=None, floored=None):
    """c(theta) [P] fp64 torch.  ``floored`` ([P] bool, e.g. the forward's decision from ``aa_ratio32``): which Gaussians take the floor
    (a constant c); the others are sqrt(r), derivative included, even where the fp64 r lies a rounding below the floor.  Default: the fp64
    r's own decision."""
    A, B, C = cov2d_undilated(cam, means3D, scales, rotations, cov3D_precomp)
    r = ratio(A, B, C)
    if floored is None:
        floored = r.detach() < FLOOR
    floored = torch.as_tensor(floored, dtype=torch.bool)
    return torch.sqrt(torch.where(floored, torch.full_like(r, FLOOR), r))


def aa_term(cam, g, dL_do_staged, floored=None):
    """fp64 numpy: dL/do = c dL/do' (key 'opacities') and the term sum_i dL/do'_i o_i dc_i/dtheta for theta in means3D and scales /
    rotations or cov3D_precomp.  ``g``: the Gaussians (numpy; o = g['opacities'])."""
    f64 = torch.float64
    keys = ("means3D",) + (("cov3D_precomp",) if g.get("cov3D_precomp") is not None else ("scales", "rotations"))
    t = {k: torch.tensor(np.asarray(g[k], np.float64), dtype=f64, requires_grad=True) for k in keys}
    c = aa_factor(cam, t["means3D"], t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"), floored)
    go = torch.tensor(np.asarray(dL_do_staged, np.float64).reshape(-1), dtype=f64)
    o = torch.tensor(np.asarray(g["opacities"], np.float64).reshape(-1), dtype=f64)
    (go * o * c).sum().backward()
    out = {k: t[k].grad.numpy() for k in keys}
    out["opacities"] = (c.detach() * go).numpy().reshape(-1, 1)
    out["_c"] = c.detach().numpy()
    return out


def compose(ref, term):
    """The oracle's gradients (fed o') with the anti-aliasing term: opacities replaced by c dL/do', the covariance / position term added."""
    out = dict(ref)
    for k, v in term.items():
        if k.startswith("_"):
            continue
        out[k] = v if k == "opacities" else np.asarray(ref[k], np.float64) + v
    return out


def aa_ratio32(cam, means3D, scales=None, rotations=None, cov3D_precomp=None):
    """The forward's fp32 r [P] (gsr_preprocess_fwd.hip + gsr_aa_ratio, contraction off): every operation separately rounded, in its
    order; det0 = A C - B^2 as Kahan's fma product difference (the two fmas evaluated exactly in fp64, then rounded once)."""
    f = np.float32
    v = np.asarray(cam.viewmatrix, f).reshape(-1)
    p = np.asarray(means3D, f)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    pv = [((v[r] * x + v[4 + r] * y) + v[8 + r] * z) + v[12 + r] for r in range(3)]
    if cov3D_precomp is not None:
        c = [np.asarray(cov3D_precomp, f)[:, k] for k in range(6)]
    else:
        q = np.asarray(rotations, f)
        r, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        one, two = f(1.0), f(2.0)
        R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - r * qz), two * (qx * qz + r * qy)],
             [two * (qx * qy + r * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - r * qx)],
             [two * (qx * qz - r * qy), two * (qy * qz + r * qx), one - two * (qx * qx + qy * qy)]]
        s = f(cam.scale_modifier) * np.asarray(scales, f)
        M = [[R[a][b] * s[:, b] for b in range(3)] for a in range(3)]

        def dot(a, b):
            return (M[a][0] * M[b][0] + M[a][1] * M[b][1]) + M[a][2] * M[b][2]
        c = [dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)]
    W, H = f(cam.image_width), f(cam.image_height)
    tfx, tfy = f(cam.tanfovx), f(cam.tanfovy)
    fx, fy = W / (f(2.0) * tfx), H / (f(2.0) * tfy)
    limx, limy = f(1.3) * tfx, f(1.3) * tfy
    tz = pv[2]
    tx = np.clip(pv[0] / tz, -limx, limx) * tz
    ty = np.clip(pv[1] / tz, -limy, limy) * tz
    J00, J02 = fx / tz, -(fx * tx) / (tz * tz)
    J11, J12 = fy / tz, -(fy * ty) / (tz * tz)
    T0 = [J00 * v[0] + J02 * v[2], J00 * v[4] + J02 * v[6], J00 * v[8] + J02 * v[10]]
    T1 = [J11 * v[1] + J12 * v[2], J11 * v[5] + J12 * v[6], J11 * v[9] + J12 * v[10]]
    c0, c1, c2, c3, c4, c5 = c
    U0 = [(T0[0] * c0 + T0[1] * c1) + T0[2] * c2, (T0[0] * c1 + T0[1] * c3) + T0[2] * c4, (T0[0] * c2 + T0[1] * c4) + T0[2] * c5]
    U1 = [(T1[0] * c0 + T1[1] * c1) + T1[2] * c2, (T1[0] * c1 + T1[1] * c3) + T1[2] * c4, (T1[0] * c2 + T1[1] * c4) + T1[2] * c5]
    a = (U0[0] * T0[0] + U0[1] * T0[1]) + U0[2] * T0[2]
    b = (U0[0] * T1[0] + U0[1] * T1[1]) + U0[2] * T1[2]
    cc = (U1[0] * T1[0] + U1[1] * T1[1]) + U1[2] * T1[2]
    h = f(0.3)
    det = (a + h) * (cc + h) - b * b
    w = b * b
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    e = (w64 - b64 * b64).astype(f)                                    # fmaf(-B, B, w): exact
    fm = (a.astype(np.float64) * cc.astype(np.float64) - w64).astype(f)  # fmaf(A, C, -w)
    return (fm + e) / det


def staged_opacity32(cam, g):
    """The forward's staged o' = fl(o * sqrtf(max(r32, floor))) [P] float32, and r32."""
    r32 = aa_ratio32(cam, g["means3D"], g.get("scales"), g.get("rotations"), g.get("cov3D_precomp"))
    c32 = np.sqrt(np.maximum(r32, np.float32(FLOOR)))
    return np.asarray(g["opacities"], np.float32).reshape(-1) * c32, r32
