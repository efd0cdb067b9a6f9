"""Camera gradients (GaussianRasterizer(..., camera_gradients=True), rasterize_gaussians(..., camera_gradients=True),
rasterize_gaussians_views(..., camera_gradients=True)): dL/d(viewmatrix, projmatrix, campos, bg).

References: the dense fp64 oracle with leaf camera tensors (tests/camera_ref.py; test_camera_grad_cpu.py checks it against finite
differences of a pose), and the rigid-motion identity -- moving the scene by E equals moving the camera by E -- whose scene side comes from
the existing per-Gaussian gradients.  Pixels whose fp32 blend decisions the oracle marks ambiguous get no incoming gradient."""
import math

import numpy as np
import pytest
import torch

from camera_ref import CAMERA_KEYS, F64, compose_camera, dense_camera_grads, dense_render, se3
from hipcheck import _settings
from oracle import TiledOracle
from util import clamp_edge_camera, clamp_edge_scene, look_at, oracle_camera, random_gaussians, rel_err, ring_camera

pytestmark = pytest.mark.gpu

BAR = 1e-3   # against the fp64 oracle: the kernels' fp32 inputs / outputs and fp32 blend, ambiguous pixels masked (no bar looser than 1e-3)


def _scene(kind, P, seed, spread=0.8):
    deg = int(kind[2:]) if kind.startswith("sh") else 0
    g = random_gaussians(P, seed=seed, scale_lo=0.03, scale_hi=0.25, spread=spread, sh_M=(deg + 1) ** 2 if kind.startswith("sh") else 0)
    if kind.startswith("sh"):
        del g["colors_precomp"]
    if kind == "cov3d":
        g["cov3D_precomp"] = _cov3d(g["scales"], g["rotations"])
        del g["scales"], g["rotations"]
    return g, deg


def _cov3d(scales, rotations):
    q = rotations.astype(np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * scales.astype(np.float64)[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def _masked_dL(cam, g, seed, deg=0):
    """A random colour gradient, zero on the pixels the fp32 oracle marks ambiguous (one flipped 1/255 decision away)."""
    H, W = cam.image_height, cam.image_width
    dL = np.random.default_rng(seed).uniform(-1, 1, (3, H, W)).astype(np.float32)
    o = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g.get("colors_precomp"), scales=g.get("scales"),
                    rotations=g.get("rotations"), shs=g.get("shs"), cov3D_precomp=g.get("cov3D_precomp"))
    dL[:, o.ambiguous] = 0.0
    return dL


def _leaf_settings(rs):
    """The settings with fresh leaf camera tensors that require a gradient."""
    return rs._replace(**{k: getattr(rs, k).detach().clone().requires_grad_(True) for k in CAMERA_KEYS})


def _render(rs, g, dev, dL, camera=True, frozen=False, depth=False, alpha=False, aa=False, dD=None, dA=None):
    """One GaussianRasterizer call and its backward: (outputs, camera grads dict, Gaussian grads dict)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = {k: torch.tensor(v, device=dev, requires_grad=not frozen) for k, v in g.items()}
    m2 = torch.zeros((g["means3D"].shape[0], 3), device=dev, requires_grad=not frozen)
    kw = {k: t[k] for k in ("shs", "colors_precomp", "scales", "rotations", "cov3D_precomp") if k in t}
    out = GaussianRasterizer(rs, differentiable_depth=depth, return_alpha=alpha, antialiasing=aa, camera_gradients=camera)(
        means3D=t["means3D"], means2D=m2, opacities=t["opacities"], **kw)
    loss = (out[0] * torch.as_tensor(dL, device=dev)).sum()
    if dD is not None:
        loss = loss + (out[2] * torch.as_tensor(dD, device=dev)).sum()
    if dA is not None:
        loss = loss + (out[3] * torch.as_tensor(dA, device=dev)).sum()
    loss.backward()
    cg = {k: None if getattr(rs, k).grad is None else getattr(rs, k).grad.detach().cpu().numpy().reshape(-1) for k in CAMERA_KEYS}
    gg = {k: None if v.grad is None else v.grad.detach().cpu().numpy() for k, v in t.items()}
    gg["means2D"] = None if m2.grad is None else m2.grad.cpu().numpy()
    return out, cg, gg


# ---------------------------------------------------------------------------------------------------------------- 1. dense fp64 oracle
@pytest.mark.parametrize("pynode", [False, True])
@pytest.mark.parametrize("kind,P", [("precomp", 200), ("sh0", 120), ("sh1", 150), ("sh2", 80), ("sh3", 300), ("cov3d", 50)])
def test_against_the_dense_fp64_oracle(dev, monkeypatch, kind, P, pynode):
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_PY_NODE", pynode)
    W, H = 96, 80
    g, deg = _scene(kind, P, seed=11 + P)
    cam = ring_camera(W, H, v=1, radius=3.2, bg=(0.3, 0.2, 0.1), sh_degree=deg)
    dL = _masked_dL(cam, g, seed=P)
    _, got, _ = _render(_leaf_settings(_settings(cam, dev)), g, dev, dL)
    ref = dict(zip(CAMERA_KEYS, dense_camera_grads(cam, g, dL, deg)))
    for k in CAMERA_KEYS:
        if k == "campos" and not kind.startswith("sh"):
            assert np.all(got[k] == 0), "precomputed colours: campos is never read"
            continue
        e = rel_err(got[k], ref[k])
        assert e < BAR, f"{kind} {k}: {e:.3e}"
    # what the forward never reads
    assert np.all(got["viewmatrix"].reshape(4, 4)[:, 3] == 0) and np.all(got["projmatrix"].reshape(4, 4)[:, 2] == 0)


# ---------------------------------------------------------------------------------------------------------------- 2. pose only
@pytest.mark.parametrize("kind", ["precomp", "sh2"])
def test_pose_only_matches_the_oracle(dev, kind):
    """Frozen Gaussians, a trainable 6-DoF pose composed as setup_camera composes it (torch.inverse for campos): the forward must not take
    GSR_FORWARD_ONLY (will_backward counts the camera tensors), and dL/dxi must be the oracle's."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    W, H = 96, 80
    g, deg = _scene(kind, 200, seed=3)
    w2c0 = look_at((0.8, 0.9, 3.3))
    xi = torch.zeros(6, device=dev, requires_grad=True)
    w2c = se3(xi) @ torch.tensor(w2c0, dtype=torch.float32, device=dev)
    view, proj, campos = compose_camera(w2c, W, H)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    rs = GaussianRasterizationSettings(H, W, 0.5, H / (2.0 * W), bg, 1.0, view, proj, deg, campos, False)
    t = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    kw = {k: t[k] for k in ("shs", "colors_precomp", "scales", "rotations") if k in t}
    out = GaussianRasterizer(rs, camera_gradients=True)(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]),
                                                       opacities=t["opacities"], **kw)
    cam = oracle_camera(W, H, w2c0, bg=(0.1, 0.2, 0.3), sh_degree=deg)
    dL = _masked_dL(cam, g, seed=7)
    (out[0] * torch.tensor(dL, device=dev)).sum().backward()
    xi64 = torch.zeros(6, dtype=F64, requires_grad=True)
    v64, p64, c64 = compose_camera(se3(xi64) @ torch.tensor(np.asarray(w2c0, np.float32), dtype=F64), W, H)
    img = dense_render(W, H, 0.5, H / (2.0 * W), torch.tensor([0.1, 0.2, 0.3], dtype=F64), v64.reshape(-1), p64.reshape(-1), c64, g, deg)
    (img * torch.tensor(dL, dtype=F64)).sum().backward()
    e = rel_err(xi.grad.cpu().numpy(), xi64.grad.numpy())
    assert e < BAR, f"{kind}: {e:.3e}"


# ---------------------------------------------------------------------------------------------------------------- 3. rigid motion
def _mm(A, B):
    """4x4 product as exact sums of products (identity factors give the other factor's bits, whatever the BLAS)."""
    return (A[:, :, None] * B[None, :, :]).sum(1)


def _scene_terms(g, d3, dcov):
    """Per-Gaussian terms of dL/d(omega, tau) of the scene moved by exp(xi) at xi = 0, in fp64: tau_k -> dL/dmeans3D_k, omega_k ->
    dL/dmeans3D . (e_k x p) + <dL/dSigma, G_k Sigma + Sigma G_k^T>.  Returns [P, 6]."""
    p = g["means3D"].astype(np.float64)
    d3 = d3.astype(np.float64)
    out = np.zeros((p.shape[0], 6))
    out[:, 3:] = d3
    G = [np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0.0]]), np.array([[0, 0, 1], [0, 0, 0], [-1, 0, 0.0]]),
         np.array([[0, -1, 0], [1, 0, 0], [0, 0, 0.0]])]
    for k in range(3):
        out[:, k] = (d3 * (p @ G[k].T)).sum(1)
    if dcov is not None:
        c = g["cov3D_precomp"].astype(np.float64)
        S = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1)
        dc = dcov.astype(np.float64)
        dS = np.stack([np.stack([dc[:, 0], 0.5 * dc[:, 1], 0.5 * dc[:, 2]], 1), np.stack([0.5 * dc[:, 1], dc[:, 3], 0.5 * dc[:, 4]], 1),
                       np.stack([0.5 * dc[:, 2], 0.5 * dc[:, 4], dc[:, 5]], 1)], 1)
        for k in range(3):
            Sd = G[k][None] @ S + S @ G[k].T[None]
            out[:, k] += (dS * Sd).sum((1, 2))
    return out


def _rigid_case(dev, kind, V, depth, alpha, aa, rotation, P=300, W=96, H=80, seed=0, scene=None, w2cs=None, intr=None):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_gaussians, rasterize_gaussians_views
    g, deg = _scene(kind, P, seed=seed) if scene is None else scene
    P = g["means3D"].shape[0]
    intr = {} if intr is None else intr
    rng = np.random.default_rng(seed + 1)
    w2c0 = [torch.tensor(look_at((3.6 * math.cos(2 * math.pi * v / V + 0.3), 0.8, 3.6 * math.sin(2 * math.pi * v / V + 0.3)))
                         if w2cs is None else w2cs[v], dtype=torch.float32, device=dev) for v in range(V)]
    bg = torch.tensor([0.2, 0.3, 0.4], device=dev)
    # what the forward must reproduce: the plain render of each view's w2c0
    dL = torch.tensor(rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32), device=dev)
    dD = torch.tensor(rng.uniform(-1, 1, (V, 1, H, W)).astype(np.float32), device=dev) if depth else None
    dA = torch.tensor(rng.uniform(-1, 1, (V, 1, H, W)).astype(np.float32), device=dev) if alpha else None
    mask = torch.tensor([0, 0, 0, 1, 1, 1.0], device=dev) if not rotation else torch.ones(6, device=dev)
    base = {k: torch.tensor(v, device=dev) for k, v in g.items()}

    def run(xi_scene, xi_cam):
        E = se3(xi_scene * mask)
        t = dict(base)
        x, y, z = base["means3D"][:, 0], base["means3D"][:, 1], base["means3D"][:, 2]
        t["means3D"] = torch.stack([E[r, 0] * x + E[r, 1] * y + E[r, 2] * z + E[r, 3] for r in range(3)], 1)
        if rotation:
            c = base["cov3D_precomp"]
            S = torch.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1)
            R = E[:3, :3]
            RS = (R[None, :, :, None] * S[:, None, :, :]).sum(2)
            RSR = (RS[:, :, :, None] * R.t()[None, None, :, :]).sum(2)
            t["cov3D_precomp"] = torch.stack([RSR[:, 0, 0], RSR[:, 0, 1], RSR[:, 0, 2], RSR[:, 1, 1], RSR[:, 1, 2], RSR[:, 2, 2]], 1)
        for k in t:
            if k != "means3D" and not (rotation and k == "cov3D_precomp"):
                t[k] = t[k].detach().requires_grad_(True)
        for k in ("means3D", "cov3D_precomp") if rotation else ("means3D",):   # the scene side reads their gradients
            if t[k].requires_grad:
                t[k].retain_grad()
            else:
                t[k] = t[k].detach().requires_grad_(True)
        Ec = se3(xi_cam * mask)
        rss = []
        for v in range(V):
            view, proj, campos = compose_camera(_mm(w2c0[v], Ec), W, H, **intr)
            rss.append(GaussianRasterizationSettings(H, W, 0.5, H / (2.0 * W), bg, 1.0, view, proj, deg, campos, False))
        kw = dict(shs=t.get("shs"), colors_precomp=t.get("colors_precomp"), scales=t.get("scales"), rotations=t.get("rotations"),
                  cov3D_precomp=t.get("cov3D_precomp"))
        flags = dict(differentiable_depth=depth, return_alpha=alpha, antialiasing=aa, camera_gradients=xi_cam.requires_grad)
        if V == 1:
            m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
            e = lambda a: torch.empty(0, device=dev) if a is None else a  # noqa: E731
            out = rasterize_gaussians(t["means3D"], m2, e(kw["shs"]), e(kw["colors_precomp"]), t["opacities"], e(kw["scales"]),
                                      e(kw["rotations"]), e(kw["cov3D_precomp"]), rss[0], **flags)
            out = tuple(o.unsqueeze(0) if k != 1 else o for k, o in enumerate(out))
        else:
            m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
            out = rasterize_gaussians_views(rss, t["means3D"], m2, t["opacities"], **kw, **flags)
        loss = (out[0] * dL).sum()
        if depth:
            loss = loss + (out[2] * dD).sum()
        if alpha:
            loss = loss + (out[3] * dA).sum()
        loss.backward()
        return out, t

    z = torch.zeros(6, device=dev)
    plain, _ = run(z, z)
    xs = torch.zeros(6, device=dev, requires_grad=True)
    out_s, ts = run(xs, z)
    xc = torch.zeros(6, device=dev, requires_grad=True)
    out_c, _ = run(z, xc)
    # at xi = 0 both transforms are exactly the identity: the same forward, bit for bit
    for k in (0, 2) + ((3,) if alpha else ()):
        assert torch.equal(out_s[k], plain[k]) and torch.equal(out_c[k], plain[k]), k
    terms = _scene_terms({k: v.cpu().numpy() for k, v in base.items()}, ts["means3D"].grad.cpu().numpy(),
                         ts["cov3D_precomp"].grad.cpu().numpy() if rotation else None)
    scene, scale = terms.sum(0), np.abs(terms).sum(0)
    cams = xc.grad.cpu().numpy().astype(np.float64)
    sel = slice(0, 6) if rotation else slice(3, 6)
    assert np.all(scale[sel] > 0)
    err = (np.abs(scene - cams) / scale)[sel]
    # fp32 rounding only: the per-Gaussian outputs (scene side) and the camera pass's fp32 outputs / the fp32 composition (camera side)
    assert err.max() < 1e-5, (kind, V, depth, alpha, aa, rotation, err, scene, cams)
    return err


@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("depth,alpha,aa", [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                                            (True, True, True)])
def test_translation_identity(dev, V, depth, alpha, aa):
    for kind in ("precomp", "sh3", "cov3d"):
        if V > 1 and kind.startswith("sh"):
            continue       # (SH multi-view: the single-view path per view, covered by V = 1 and test_views_equal_single_views)
        _rigid_case(dev, kind, V, depth, alpha, aa, rotation=False)


@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("depth,alpha,aa", [(False, False, False), (True, True, False), (False, False, True), (True, True, True)])
def test_rotation_identity(dev, V, depth, alpha, aa):
    _rigid_case(dev, "cov3d", V, depth, alpha, aa, rotation=True)


def test_rigid_identity_full_size(dev):
    """The configs[2] size: 100 k Gaussians, 800 x 800, four views, anti-aliasing with depth and alpha (the only check of the AA camera
    term at scale: tests/antialias_ref.py takes the camera as numpy)."""
    _rigid_case(dev, "cov3d", 4, True, True, True, rotation=True, P=100_000, W=800, H=800, seed=21)


# ---------------------------------------------------------------------------------------------------------------- 4, 5. multi-view
def _views_grads(dev, rss, g, dL, per_view_col=None):
    from diff_gaussian_rasterization import rasterize_gaussians_views
    V = len(rss)
    t = {k: torch.tensor(v, device=dev, requires_grad=k != "colors_precomp") for k, v in g.items()}
    col = t["colors_precomp"] if per_view_col is None else torch.tensor(per_view_col, device=dev)
    m2 = torch.zeros((V, g["means3D"].shape[0], 3), device=dev, requires_grad=True)
    out = rasterize_gaussians_views(rss, t["means3D"], m2, t["opacities"], colors_precomp=col, scales=t["scales"], rotations=t["rotations"],
                                    camera_gradients=True)
    (out[0] * torch.tensor(dL, device=dev)).sum().backward()
    return out


@pytest.mark.parametrize("V", [2, 4, 17])
def test_views_equal_single_views(dev, V):
    """rasterize_gaussians_views' camera gradients equal single-view calls' (V = 17: the split into two library calls)."""
    W, H = 64, 48
    g, _ = _scene("precomp", 300, seed=5)
    cams = [ring_camera(W, H, v=v, V=V, bg=(0.1, 0.5, 0.2)) for v in range(V)]
    rss = [_leaf_settings(_settings(c, dev)) for c in cams]
    dL = np.random.default_rng(2).uniform(-1, 1, (V, 3, H, W)).astype(np.float32)
    _views_grads(dev, rss, g, dL)
    for v in range(V):
        _, ref, _ = _render(_leaf_settings(_settings(cams[v], dev)), g, dev, dL[v])
        for k in ("bg", "viewmatrix", "projmatrix"):
            got = rss[v]._asdict()[k].grad.cpu().numpy().reshape(-1)
            assert rel_err(got, ref[k]) < 1e-5, (v, k)      # the same chain; another blend-backward reduction order
        assert np.all(rss[v].campos.grad.cpu().numpy() == 0)


def test_fused_pairs_run_unfused(dev, monkeypatch):
    """Two views with the same camera tensors and their own frozen colours: the forward fuses them, the camera-gradient backward goes
    through gsr_backward_batch_ex's camera records (unfused), and the shared camera tensors get the sum of two separately rendered views' gradients."""
    from diff_gaussian_rasterization import _hip
    W, H = 64, 48
    g, _ = _scene("precomp", 300, seed=6)
    cam = ring_camera(W, H, v=0, bg=(0.4, 0.1, 0.3))
    rs = _leaf_settings(_settings(cam, dev))
    cols = np.stack([g["colors_precomp"], np.ones_like(g["colors_precomp"])])
    dL = np.random.default_rng(4).uniform(-1, 1, (2, 3, H, W)).astype(np.float32)
    seen = []
    orig = _hip.rasterize_backward_batch

    def spy(*a, **k):
        seen.append((a[0][0].geometry_of is not None, k.get("camera_grads")))
        return orig(*a, **k)
    monkeypatch.setattr(_hip, "rasterize_backward_batch", spy)
    _views_grads(dev, [rs, rs], g, dL, per_view_col=cols)
    assert seen and seen[0][0] and seen[0][1] is not None, "the forward must have paired the views, and camera grads asked for"
    ref = {k: 0.0 for k in CAMERA_KEYS}
    for v in range(2):
        gv = dict(g)
        gv["colors_precomp"] = cols[v].astype(np.float32)
        _, r, _ = _render(_leaf_settings(_settings(cam, dev)), gv, dev, dL[v])
        for k in CAMERA_KEYS:
            ref[k] = ref[k] + r[k]
    for k in ("bg", "viewmatrix", "projmatrix"):
        assert rel_err(getattr(rs, k).grad.cpu().numpy().reshape(-1), ref[k]) < 1e-5, k


# ---------------------------------------------------------------------------------------------------------------- 6, 7. defaults, determinism
@pytest.mark.parametrize("pynode", [False, True])
def test_defaults_unchanged_and_gaussian_gradients_bit_identical(dev, monkeypatch, pynode):
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_PY_NODE", pynode)
    W, H = 96, 80
    for kind in ("precomp", "sh2"):
        g, deg = _scene(kind, 400, seed=8)
        cam = ring_camera(W, H, v=2, bg=(0.2, 0.2, 0.6), sh_degree=deg)
        dL = np.random.default_rng(9).uniform(-1, 1, (3, H, W)).astype(np.float32)
        rs0 = _leaf_settings(_settings(cam, dev))
        out0, cg0, gg0 = _render(rs0, g, dev, dL, camera=False)
        assert all(v is None for v in cg0.values()), "without the keyword a camera tensor gets no gradient"
        rs1 = _leaf_settings(_settings(cam, dev))
        out1, cg1, gg1 = _render(rs1, g, dev, dL, camera=True)
        for a, b in zip(out0, out1):
            assert torch.equal(a, b)
        for k in gg0:
            assert (gg0[k] is None and gg1[k] is None) or np.array_equal(gg0[k], gg1[k]), (kind, k)
        assert all(cg1[k] is not None for k in CAMERA_KEYS)


def test_determinism_and_retain_graph(dev):
    """Two backwards of one forward (retain_graph=True) give the same camera gradients, bit for bit (no atomics)."""
    from diff_gaussian_rasterization import rasterize_gaussians_views
    W, H, V = 96, 80, 4
    g, _ = _scene("precomp", 3000, seed=10)
    rss = [_leaf_settings(_settings(ring_camera(W, H, v=v, V=V), dev)) for v in range(V)]
    t = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in g.items()}
    out = rasterize_gaussians_views(rss, t["means3D"], torch.zeros((V, 3000, 3), device=dev, requires_grad=True), t["opacities"],
                                    colors_precomp=t["colors_precomp"], scales=t["scales"], rotations=t["rotations"], camera_gradients=True)
    loss = (out[0] * torch.rand(out[0].shape, device=dev, generator=torch.Generator(dev).manual_seed(1))).sum()
    loss.backward(retain_graph=True)
    first = [[getattr(rs, k).grad.clone() for k in CAMERA_KEYS] for rs in rss]
    for rs in rss:
        for k in CAMERA_KEYS:
            getattr(rs, k).grad = None
    loss.backward()
    for a, rs in zip(first, rss):
        for x, k in zip(a, CAMERA_KEYS):
            assert torch.equal(x, getattr(rs, k).grad), k


# ---------------------------------------------------------------------------------------------------------------- 8. frustum-clamp edge
@pytest.mark.parametrize("rotation", [False, True])
def test_clamp_edge_follows_the_forward(dev, rotation):
    """Gaussians within a few ulp of the frustum clamp, both sides (util.clamp_edge_scene).  The dense oracle decides the clamp in fp64
    and flips some of them (a whole dtx / dty term each), so the reference is the rigid-motion identity: the scene side is the
    per-Gaussian backward's, which takes the forward's fp32 decisions (tests/test_bwd_chain_edges_gpu.py checks it against fp64 with those
    decisions), and the camera side must agree with it to fp32 rounding -- it could not if the camera pass decided the clamp otherwise."""
    cam = clamp_edge_camera()
    g, edge = clamp_edge_scene(cam)
    g["cov3D_precomp"] = _cov3d(g.pop("scales"), g.pop("rotations"))
    W, H = cam.image_width, cam.image_height
    w2c = look_at((3.1, 0.9, 1.7), target=(0.05, -0.1, 0.02))
    _rigid_case(dev, "cov3d", 1, False, False, False, rotation, W=W, H=H, scene=(g, 0), w2cs=[w2c],
                intr=dict(fx=float(W), fy=float(W), cx=0.42 * W, cy=0.57 * H))


# ---------------------------------------------------------------------------------------------------------------- 9. edge cases
@pytest.mark.parametrize("pynode", [False, True])
def test_edge_cases(dev, monkeypatch, pynode):
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_PY_NODE", pynode)
    W, H = 64, 48
    cam = ring_camera(W, H, bg=(0.3, 0.6, 0.9))
    dL = np.random.default_rng(13).uniform(-1, 1, (3, H, W)).astype(np.float32)
    dsum = dL.astype(np.float64).sum((1, 2))
    # P = 0: the image is the background -- dL/dbg = the sum of dL/dC, the rest 0
    g0 = {k: v[:0] for k, v in random_gaussians(4, seed=1).items()}
    _, got, _ = _render(_leaf_settings(_settings(cam, dev)), g0, dev, dL)
    assert np.allclose(got["bg"], dsum, rtol=1e-6, atol=1e-4) and not got["viewmatrix"].any() and not got["projmatrix"].any()
    # every Gaussian behind the camera (culled; nothing covered): the same
    g1 = random_gaussians(50, seed=2, spread=0.3)
    w2c = np.asarray(look_at((0, 0, 4.0)), np.float64)
    g1["means3D"] = (g1["means3D"] + np.array([0, 0, 8.0], np.float32)).astype(np.float32)      # beyond the camera at z = 4, looking at 0
    cam1 = oracle_camera(W, H, w2c, bg=(0.3, 0.6, 0.9))
    _, got, _ = _render(_leaf_settings(_settings(cam1, dev)), g1, dev, dL)
    assert np.allclose(got["bg"], dsum, rtol=1e-6, atol=1e-4) and not got["viewmatrix"].any() and not got["projmatrix"].any()
    # every pixel covered by opaque Gaussians (a close camera): dL/dbg = sum T_final dL, against the oracle
    cam2 = ring_camera(W, H, radius=1.6, bg=(0.3, 0.6, 0.9))
    g2 = random_gaussians(400, seed=3, scale_lo=0.3, scale_hi=0.6, spread=0.4)
    g2["opacities"][:] = 0.98
    dL2 = _masked_dL(cam2, g2, seed=14)
    _, got, _ = _render(_leaf_settings(_settings(cam2, dev)), g2, dev, dL2)
    ref = dict(zip(CAMERA_KEYS, dense_camera_grads(cam2, g2, dL2)))
    assert np.abs(got["bg"]).max() < 1e-2 * np.abs(dL2).sum(axis=(1, 2)).min()    # T_final ~ 0 everywhere
    assert rel_err(got["viewmatrix"], ref["viewmatrix"]) < BAR and rel_err(got["projmatrix"], ref["projmatrix"]) < BAR
    assert np.abs(got["bg"] - ref["bg"]).max() < 1e-6 * np.abs(dL2).sum()    # bg: tiny sums of T_final dL
    # wrong-shaped camera tensors are rejected
    rs = _settings(cam, dev)
    for name, bad in (("bg", torch.zeros(4, device=dev)), ("viewmatrix", torch.zeros(3, 4, device=dev)),
                      ("campos", torch.zeros(2, device=dev))):
        with pytest.raises((ValueError, RuntimeError)):
            _render(rs._replace(**{name: bad}), random_gaussians(20, seed=4), dev, dL)
