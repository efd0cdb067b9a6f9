"""Anti-aliasing (GaussianRasterizer(..., antialiasing=True), rasterize_gaussians(..., antialiasing=True),
rasterize_gaussians_views(..., antialiasing=True)): the staged opacity o' = o c and its gradient.

References (tests/antialias_ref.py; test_antialias_cpu.py checks them against each other on the CPU):
  * forward: an anti-aliased forward IS a plain forward whose opacities are the staged o' -- bit for bit, lists included;
  * gradients: the unedited tiled oracle fed o' (its fp64 build as referee, with the rule of test_depth_grad_gpu._compare), composed
    with the fp64 torch term -- dL/do = c dL/do', plus dL/do' o dc/dtheta on means3D and scales / rotations or cov3D_precomp -- and the
    dense fp64 oracle fed o c(theta), c in fp64 torch, so that autograd gives the whole gradient.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from antialias_ref import FLOOR, aa_factor, aa_term, compose, cov2d_undilated, ratio, staged_opacity32
from hipcheck import ROW_TOL_WORST, TOL, _row_check, _settings
from oracle import TiledOracle
from oracle.dense_oracle import dense_rasterize
from util import look_at, mixed_err, oracle_camera, random_gaussians, rel_err, ring_camera, row_err

pytestmark = pytest.mark.gpu

KEYS = ("means3D", "means2D", "opacities", "scales", "rotations", "cov3D_precomp", "colors_precomp", "shs")


def _cov3d(g):
    q = g["rotations"].astype(np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * g["scales"].astype(np.float64)[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def _scene(kind, P=2000, seed=5):
    """Default scenes: sizes from sub-pixel to tens of pixels, so c spans the floor to ~1."""
    g = random_gaussians(P, seed=seed, scale_lo=0.002, scale_hi=0.15, sh_M=16 if kind == "sh" else 0)
    if kind == "sh":
        del g["colors_precomp"]
    if kind == "cov3d":
        g["cov3D_precomp"] = _cov3d(g)
        del g["scales"], g["rotations"]
    return g


def _geo(g):
    return dict(scales=g.get("scales"), rotations=g.get("rotations"), cov3D_precomp=g.get("cov3D_precomp"))


def _with_opacity(g, o):
    out = dict(g)
    out["opacities"] = np.asarray(o, np.float32).reshape(-1, 1)
    return out


def _staged(cam, g, dev, sh_degree=None):
    """The staged o' of an anti-aliased forward (record part 1, .y: debug_views(state)['rec'][:, 5]) and that forward's debug views."""
    from diff_gaussian_rasterization import _hip
    t = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    out = _hip.rasterize_forward(_settings(cam, dev, sh_degree=sh_degree), t["means3D"], t["opacities"], t.get("colors_precomp"),
                                 t.get("shs"), t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"), antialiasing=True)
    views = _hip.debug_views(out[3])
    torch.cuda.synchronize()
    return views["rec"][:, 5].cpu().numpy(), out, views


def _render(cam, g, dev, aa, dL=None, frozen=(), depth=False, alpha=False, dLd=None, dLa=None, sh_degree=None):
    """One GaussianRasterizer call (``aa`` None: the keyword omitted).  Returns (outputs as numpy, gradients or None)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = {k: torch.tensor(v, device=dev, requires_grad=dL is not None and k not in frozen) for k, v in g.items()}
    m2 = torch.zeros((g["means3D"].shape[0], 3), device=dev, requires_grad=dL is not None)
    kw = {} if aa is None else {"antialiasing": aa}
    r = GaussianRasterizer(raster_settings=_settings(cam, dev, sh_degree=sh_degree), differentiable_depth=depth, return_alpha=alpha, **kw)
    out = r(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], shs=t.get("shs"), colors_precomp=t.get("colors_precomp"),
            scales=t.get("scales"), rotations=t.get("rotations"), cov3D_precomp=t.get("cov3D_precomp"))
    grads = None
    if dL is not None:
        loss = (out[0] * torch.tensor(dL, device=dev)).sum()
        if dLd is not None:
            loss = loss + (out[2] * torch.tensor(dLd.reshape(out[2].shape), device=dev)).sum()
        if dLa is not None:
            loss = loss + (out[3] * torch.tensor(dLa.reshape(out[3].shape), device=dev)).sum()
        loss.backward()
        grads = {k: v.grad.detach().cpu().numpy() for k, v in t.items() if v.grad is not None}
        grads["means2D"] = m2.grad.detach().cpu().numpy()
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in out], grads


def _floored(cam, g):
    return staged_opacity32(cam, g)[1] < np.float32(FLOOR)


def _compare(tag, got, ref, keys=KEYS, referee=None, tol=TOL):
    """fp32 bars against ``ref``; a tensor that misses them goes to ``referee()`` (the fp64 composition) with the rule of
    test_depth_grad_gpu._compare: no further from fp64 than twice the fp32 reference + 2e-5 norm-wise, four times + 1e-4 in its worst row."""
    ref64 = None
    for k in keys:
        if got.get(k) is None or ref.get(k) is None:
            continue
        try:
            e = rel_err(got[k], ref[k])
            assert e < tol, f"{tag} grad {k}: rel err {e:.3e}"
            _row_check(f"antialias {tag} grad {k}", got[k], ref[k])
        except AssertionError:
            if referee is None:
                raise
            if ref64 is None:
                ref64 = referee()
            e_hip, e_o = rel_err(got[k], ref64[k]), rel_err(ref[k], ref64[k])
            r_hip, r_o = row_err(got[k], ref64[k])[0], row_err(ref[k], ref64[k])[0]
            note = f"{tag} grad {k} vs fp64: norm-wise HIP {e_hip:.2e} / fp32 {e_o:.2e}, worst row HIP {r_hip:.2e} / fp32 {r_o:.2e}"
            assert e_hip <= max(TOL, 2.0 * e_o + 2e-5), note
            assert r_hip <= max(ROW_TOL_WORST, 4.0 * r_o + 1e-4), note


def _oracle_composed(cam, g, o_s, dL, floored, decisions_of=None):
    """The tiled oracle fed o' (fp64 build with ``decisions_of``), composed with the fp64 term.  Returns (gradients, the oracle run)."""
    gs = _with_opacity(g, o_s)
    f64 = decisions_of is not None
    oc = TiledOracle(cam, gs["means3D"], gs["opacities"], colors_precomp=gs.get("colors_precomp"), shs=gs.get("shs"), nthreads=4,
                     f64=f64, decisions_of=decisions_of, **_geo(gs))
    ref = {k: (None if v is None else np.asarray(v, np.float64)) for k, v in oc.backward(dL).items()}
    return compose(ref, aa_term(cam, g, ref["opacities"], floored)), oc


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("kind", ["scales", "cov3d", "sh"])
def test_forward_staged_opacity_and_identity(dev, kind):
    """The staged o' equals the host replication of the forward's fp32 arithmetic bit for bit, and o c_fp64 within 1e-2 (default scenes;
    measured worst below); the anti-aliased forward equals a plain forward fed those o', bit for bit: colour, depth, radii, the records,
    the tile lists, n_contrib and final_T."""
    from diff_gaussian_rasterization import _hip
    W, H = 160, 120
    sh_degree = 3 if kind == "sh" else 0
    cam = ring_camera(W, H, v=1, bg=(0.2, 0.1, 0.3), sh_degree=sh_degree)
    g = _scene(kind)
    o_s, out_aa, v_aa = _staged(cam, g, dev, sh_degree)
    radii = out_aa[1].cpu().numpy()
    alive = radii > 0
    assert alive.sum() > 1000
    o_host, r32 = staged_opacity32(cam, g)
    assert np.array_equal(o_s[alive].view(np.uint32), o_host[alive].view(np.uint32))
    o = g["opacities"].reshape(-1).astype(np.float64)
    c64 = aa_factor(cam, torch.tensor(g["means3D"], dtype=torch.float64),
                    **{k: (None if v is None else torch.tensor(v, dtype=torch.float64)) for k, v in _geo(g).items()}).numpy()
    rel = np.abs(o_s[alive] - o[alive] * c64[alive]) / (o[alive] * c64[alive])
    print(f"staged o' vs o c_fp64 ({kind}): worst rel {rel.max():.2e}, median {np.median(rel):.2e}; c in [{c64[alive].min():.3g}, 1)")
    assert rel.max() < 1e-2
    assert (c64[alive] < 0.5).sum() > 100 and (c64[alive] > 0.9).sum() > 100     # the scenes span the factor
    t = {k: torch.tensor(v, device=dev) for k, v in _with_opacity(g, o_s).items()}
    out_p = _hip.rasterize_forward(_settings(cam, dev, sh_degree=sh_degree), t["means3D"], t["opacities"], t.get("colors_precomp"),
                                   t.get("shs"), t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"))
    v_p = _hip.debug_views(out_p[3])
    for i in range(3):
        assert torch.equal(out_aa[i], out_p[i]), i
    assert out_aa[3].num_rendered == out_p[3].num_rendered
    for k in ("rec", "point_list", "ranges", "n_contrib", "final_T", "offsets", "tiles_touched"):
        assert torch.equal(v_aa[k], v_p[k]), k
    # o' < o: the lists of the anti-aliased render are never longer
    out_0 = _hip.rasterize_forward(_settings(cam, dev, sh_degree=sh_degree), *[torch.tensor(g[k], device=dev) if g.get(k) is not None else None
                                   for k in ("means3D", "opacities", "colors_precomp", "shs", "scales", "rotations", "cov3D_precomp")])
    assert out_aa[3].num_rendered < out_0[3].num_rendered


@pytest.mark.parametrize("pynode", [False, True])
def test_forward_nodes_and_capacity_mode(dev, monkeypatch, pynode):
    """Through GaussianRasterizer (the C++ node: count-first, then capacity mode with the layer state; or the Python node): the
    anti-aliased outputs -- colour, radii, depth, alpha -- equal the plain node's fed o', bit for bit, call after call."""
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_PY_NODE", pynode)
    if not pynode:
        assert dgr._C is not None
        dgr.layer_state(dev).reset()
    cam = ring_camera(128, 96, v=2)
    g = _scene("scales", P=1500, seed=8)
    o_s = _staged(cam, g, dev)[0]
    calls0 = dgr.layer_state(dev).stats()["capacity_calls"] if not pynode else 0
    runs = [(_render(cam, g, dev, True, alpha=True)[0], _render(cam, _with_opacity(g, o_s), dev, False, alpha=True)[0]) for _ in range(3)]
    for aa_out, plain_out in runs:
        for a, b, ref in zip(aa_out, plain_out, runs[0][1]):
            assert np.array_equal(a, b) and np.array_equal(a, ref)
    if not pynode:
        assert dgr.layer_state(dev).stats()["capacity_calls"] >= calls0 + 4     # the repeats took the capacity path


def test_forward_batch_and_fused_pair(dev):
    """rasterize_gaussians_views(antialiasing=True): view v equals a single-view plain render fed view v's o' (the factor is per view),
    bit for bit; a pair of views with one camera and per-view colours (fused into one tile pass) likewise."""
    from diff_gaussian_rasterization import rasterize_gaussians_views
    V, W, H = 3, 128, 96
    cams = [ring_camera(W, H, v=v, V=V) for v in range(V)]
    g = _scene("scales", P=2500, seed=9)
    t = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    rs = [_settings(c, dev) for c in cams]
    m2 = torch.zeros((V, g["means3D"].shape[0], 3), device=dev)
    col, radii, depth = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                                                  rotations=t["rotations"], antialiasing=True)
    for v in range(V):
        single = _render(cams[v], _with_opacity(g, _staged(cams[v], g, dev)[0]), dev, False)[0]
        assert np.array_equal(col[v].cpu().numpy(), single[0]) and np.array_equal(radii[v].cpu().numpy(), single[1])
        assert np.array_equal(depth[v].cpu().numpy(), single[2])
    cols = np.stack([g["colors_precomp"], np.random.default_rng(3).uniform(0, 1, g["colors_precomp"].shape).astype(np.float32)])
    m2p = torch.zeros((2, g["means3D"].shape[0], 3), device=dev)
    colp = rasterize_gaussians_views([rs[0], rs[0]], t["means3D"], m2p, t["opacities"], colors_precomp=torch.tensor(cols, device=dev),
                                     scales=t["scales"], rotations=t["rotations"], antialiasing=True)[0]
    o_s = _staged(cams[0], g, dev)[0]
    for v in range(2):
        gv = _with_opacity(g, o_s)
        gv["colors_precomp"] = cols[v]
        assert np.array_equal(colp[v].cpu().numpy(), _render(cams[0], gv, dev, False)[0][0]), v


def test_forward_raw_parameters(dev):
    """The capacity-mode batch forward with the activations inside the preprocess (raw parameters): the same colours as the anti-aliased
    forward of the activated values, and its fused-activation backward: d logit = sigma' (c g), the anti-aliased opacity gradient."""
    from diff_gaussian_rasterization import _hip
    V, W, H, P = 2, 128, 96, 2000
    cams = [ring_camera(W, H, v=v, V=V) for v in range(V)]
    rs = [_settings(c, dev) for c in cams]
    rng = np.random.default_rng(12)
    g = _scene("scales", P=P, seed=12)
    m3 = torch.tensor(g["means3D"], device=dev)
    col = torch.tensor(g["colors_precomp"], device=dev)
    un = torch.tensor(rng.normal(size=(P, 4)).astype(np.float32), device=dev)
    lo = torch.tensor(rng.uniform(-2, 4, (P, 1)).astype(np.float32), device=dev)
    ls = torch.tensor(np.log(g["scales"]), device=dev)
    rot, op, sc = _hip.activate_forward(un, lo, ls)
    dL = torch.tensor(rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32), device=dev)
    ref = _hip.rasterize_forward_batch(rs, m3, op, col, None, sc, rot, None, prepare_backward=True, antialiasing=True)
    d_ref = _hip.rasterize_backward_batch(ref[3], dL, m3, ref[1], col, None, sc, rot, None, want_color_grad=False)
    got = _hip.rasterize_forward_batch(rs, m3, None, col, None, None, None, None, prepare_backward=True, no_host_sync=True,
                                       raw=(un, lo, ls), antialiasing=True)
    assert got[3][0].raw_fused is not None and _hip.forward_counts_ok(got[3])
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    act = got[3][0].act
    d_got = _hip.rasterize_backward_batch(got[3], dL, m3, got[1], col, None, act[2], act[0], None, want_color_grad=False)
    torch.cuda.synchronize()
    o = op.reshape(-1, 1)
    assert rel_err(d_got[3].cpu().numpy(), (d_ref[3] * o * (1 - o)).cpu().numpy()) < 1e-6
    assert rel_err(d_got[0].cpu().numpy(), d_ref[0].cpu().numpy()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("kind", ["scales", "cov3d", "sh", "scales_frozen_colours"])
def test_gradients_against_the_composed_oracle(dev, kind):
    """Colours / SH 0-3 / cov3D_precomp scenes: the anti-aliased gradients against the fp32 tiled oracle fed o' composed with the fp64 term
    (default bars; rows that miss them go to the fp64 build as referee); the image against the oracle's within 1e-4."""
    W, H = 160, 120
    sh_degree = 3 if kind == "sh" else 0
    cam = ring_camera(W, H, v=3, bg=(0.2, 0.1, 0.3), sh_degree=sh_degree)
    g = _scene("scales" if kind.startswith("scales") else kind, seed=21)
    o_s = _staged(cam, g, dev, sh_degree)[0]
    gs = _with_opacity(g, o_s)
    probe = TiledOracle(cam, gs["means3D"], gs["opacities"], colors_precomp=gs.get("colors_precomp"), shs=gs.get("shs"), nthreads=4, **_geo(gs))
    ok = ~probe.ambiguous
    dL = np.random.default_rng(4).uniform(-1, 1, (3, H, W)).astype(np.float32)
    dL[:, ~ok] = 0.0
    frozen = ("colors_precomp",) if kind == "scales_frozen_colours" else ()
    out, got = _render(cam, g, dev, True, dL, frozen=frozen, sh_degree=sh_degree)
    assert mixed_err(out[0][:, ok], probe.color[:, ok]) < 1e-4
    floored = _floored(cam, g)
    ref, oc = _oracle_composed(cam, g, o_s, dL, floored)
    _compare(kind, got, ref, referee=lambda: _oracle_composed(cam, g, o_s, dL, floored, decisions_of=oc)[0])


def test_gradients_against_the_dense_fp64_oracle(dev):
    """The dense fp64 oracle fed o c(theta), c in fp64 torch: autograd gives every gradient, the factor's included."""
    P, W, H = 60, 40, 32
    g = random_gaussians(P, seed=33, scale_lo=0.005, scale_hi=0.25, spread=0.6)
    cam = ring_camera(W, H, v=1, radius=3.0, bg=(0.3, 0.2, 0.1))
    o_s = _staged(cam, g, dev)[0]
    gs = _with_opacity(g, o_s)
    ok = ~TiledOracle(cam, gs["means3D"], gs["opacities"], colors_precomp=gs["colors_precomp"], **_geo(gs)).ambiguous
    dL = np.random.default_rng(6).uniform(-1, 1, (3, H, W)).astype(np.float32)
    dL[:, ~ok] = 0.0
    _, got = _render(cam, g, dev, True, dL)
    f64 = torch.float64
    t = {k: torch.tensor(v.astype(np.float64), dtype=f64, requires_grad=True) for k, v in g.items()}
    c = aa_factor(cam, t["means3D"], t["scales"], t["rotations"], floored=_floored(cam, g))
    img = dense_rasterize(H, W, cam.tanfovx, cam.tanfovy, torch.tensor(cam.bg, dtype=f64), 1.0, torch.tensor(cam.viewmatrix),
                          torch.tensor(cam.projmatrix), 0, torch.tensor(cam.campos), t["means3D"], t["opacities"] * c[:, None],
                          colors_precomp=t["colors_precomp"], scales=t["scales"], rotations=t["rotations"])[0]
    (img * torch.tensor(dL, dtype=f64)).sum().backward()
    assert c.min() < 0.3
    for k in ("means3D", "opacities", "scales", "rotations", "colors_precomp"):
        e = rel_err(got[k], t[k].grad.numpy())
        assert e < TOL, f"{k}: {e:.3e}"


# ---------------------------------------------------------------------------------------------------------------- multi-view
def _views(cams, g, dev, aa=True, frozen=(), depth=False, alpha=False, seed=0, colours=None):
    from diff_gaussian_rasterization import rasterize_gaussians_views
    V, H, W = len(cams), cams[0].image_height, cams[0].image_width
    rng = np.random.default_rng(seed)
    t = {k: torch.tensor(v, device=dev, requires_grad=k not in frozen) for k, v in g.items()}
    colt = t["colors_precomp"] if colours is None else torch.tensor(colours, device=dev, requires_grad="colors_precomp" not in frozen)
    m2 = torch.zeros((V, g["means3D"].shape[0], 3), device=dev, requires_grad=True)
    out = rasterize_gaussians_views([_settings(c, dev) for c in cams], t["means3D"], m2, t["opacities"], colors_precomp=colt,
                                    scales=t["scales"], rotations=t["rotations"], differentiable_depth=depth, return_alpha=alpha,
                                    antialiasing=aa)
    dLs = [rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32), rng.uniform(-1, 1, (V, 1, H, W)).astype(np.float32),
           rng.uniform(-1, 1, (V, 1, H, W)).astype(np.float32)]
    loss = (out[0] * torch.tensor(dLs[0], device=dev)).sum()
    if depth:
        loss = loss + (out[2] * torch.tensor(dLs[1], device=dev)).sum()
    if alpha:
        loss = loss + (out[3] * torch.tensor(dLs[2], device=dev)).sum()
    loss.backward()
    grads = {k: v.grad.cpu().numpy() for k, v in t.items() if v.grad is not None}
    if colours is not None and colt.grad is not None:
        grads["colors_precomp"] = colt.grad.cpu().numpy()
    grads["means2D"] = m2.grad.cpu().numpy()
    torch.cuda.synchronize()
    return grads, dLs


def _sum_of_singles(cams, g, dev, dLs, frozen=(), depth=False, alpha=False, colours=None):
    tot = {}
    m2 = []
    for v, cam in enumerate(cams):
        gv = dict(g)
        if colours is not None:
            gv["colors_precomp"] = colours[v]
        _, gr = _render(cam, gv, dev, True, dLs[0][v], frozen=frozen, depth=depth, alpha=alpha,
                        dLd=dLs[1][v] if depth else None, dLa=dLs[2][v] if alpha else None)
        m2.append(gr.pop("means2D"))
        for k, x in gr.items():
            if k == "colors_precomp" and colours is not None:
                tot.setdefault(k, []).append(x)
            else:
                tot[k] = tot.get(k, 0.0) + x.astype(np.float64)
    if colours is not None and "colors_precomp" in tot:
        tot["colors_precomp"] = np.stack(tot["colors_precomp"])
    tot["means2D"] = np.stack(m2)
    return tot


@pytest.mark.parametrize("V", [2, 5, 8])
def test_multiview_equals_sum_of_single_views(dev, V):
    """Every view's dL/do' is scaled by its own c before the views are summed (registers in the loop kernel, the LDS exchange of the
    one-wave-per-view kernel): a V-view call equals the sum of its single views."""
    cams = [ring_camera(128, 96, v=v, V=V) for v in range(V)]
    g = _scene("scales", P=3000, seed=40 + V)
    got, dLs = _views(cams, g, dev, seed=V)
    ref = _sum_of_singles(cams, g, dev, dLs)
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "colors_precomp"):
        assert rel_err(got[k], ref[k]) < 1e-5, k


def test_fused_pair_and_depth_alpha_multiview(dev):
    """A fused pair (one camera, per-view colours, frozen colours: one tile pass for both) and a 2-view call with depth and alpha
    gradients, each against the sum of its single views."""
    cam = ring_camera(128, 96, v=1)
    g = _scene("scales", P=2500, seed=50)
    cols = np.stack([g["colors_precomp"], np.random.default_rng(5).uniform(0, 1, g["colors_precomp"].shape).astype(np.float32)])
    got, dLs = _views([cam, cam], g, dev, frozen=("colors_precomp",), seed=1, colours=cols)
    ref = _sum_of_singles([cam, cam], g, dev, dLs, frozen=("colors_precomp",), colours=cols)
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        assert rel_err(got[k], ref[k]) < 1e-5, ("pair", k)
    cams = [ring_camera(128, 96, v=v) for v in range(2)]
    got, dLs = _views(cams, g, dev, depth=True, alpha=True, seed=2)
    ref = _sum_of_singles(cams, g, dev, dLs, depth=True, alpha=True)
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "colors_precomp"):
        assert rel_err(got[k], ref[k]) < 1e-5, ("depth+alpha", k)


def test_depth_and_alpha_with_antialiasing(dev):
    """Single view, depth and alpha gradients with anti-aliasing: the plain render fed o' (same forward, bit for bit) composed with the
    fp64 term of its own opacity gradient."""
    cam = ring_camera(128, 96, v=0)
    g = _scene("scales", P=2000, seed=60)
    o_s = _staged(cam, g, dev)[0]
    rng = np.random.default_rng(7)
    dL, dLd, dLa = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((3, 96, 128), (1, 96, 128), (1, 96, 128)))
    _, got = _render(cam, g, dev, True, dL, depth=True, alpha=True, dLd=dLd, dLa=dLa)
    _, plain = _render(cam, _with_opacity(g, o_s), dev, False, dL, depth=True, alpha=True, dLd=dLd, dLa=dLa)
    ref = compose({k: np.asarray(v, np.float64) for k, v in plain.items()}, aa_term(cam, g, plain["opacities"], _floored(cam, g)))
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "colors_precomp"):
        assert rel_err(got[k], ref[k]) < 1e-5, k
        _row_check(f"antialias depth+alpha {k}", got[k], ref[k])


def test_mixed_flags_and_unknown_bits_are_rejected(dev):
    """One launch serves all views of a batch call: views that disagree on GSR_SETTINGS_ANTIALIASING are rejected (-2), forward and
    backward; so is a settings word with a bit the ABI does not define."""
    from diff_gaussian_rasterization import _hip
    lib = _hip.load_library()
    rs = _settings(ring_camera(64, 48), dev)
    s0, k0 = _hip._make_settings(rs, dev, 0)
    s1, k1 = _hip._make_settings(rs, dev, 0, antialiasing=True)
    assert s0.prefiltered == 0 and s1.prefiltered == 2
    sarr = (_hip.GsrSettings * 2)(s0, s1)
    batch = torch.empty((4096,), dtype=torch.uint8, device=dev)
    rc = lib.gsr_forward_batch(2, sarr, 10, *([None] * 13), C.c_void_p(batch.data_ptr()), None, None, None, None, 0, None)
    assert rc == -2 and b"GSR_SETTINGS_ANTIALIASING" in lib.gsr_last_error()
    rc = lib.gsr_backward_batch_ex(2, sarr, 10, *([None] * 10), C.c_void_p(batch.data_ptr()), *([None] * 13))
    assert rc == -2 and b"GSR_SETTINGS_ANTIALIASING" in lib.gsr_last_error()
    s0.prefiltered = 4
    rc = lib.gsr_forward_preprocess(C.byref(s0), 10, *([None] * 11))
    assert rc == -2 and b"unknown bits" in lib.gsr_last_error()


# ---------------------------------------------------------------------------------------------------------------- edges
def _pixel_centred_scene(cam, targets, seed=0, opacity=0.99):
    """Isotropic Gaussians centred on pixel centres, 6 px apart, whose fp64 r is ``targets`` (bisection on the scale)."""
    rng = np.random.default_rng(seed)
    W, H = cam.image_width, cam.image_height
    v = np.asarray(cam.viewmatrix, np.float64).reshape(4, 4)
    R, tr = v[:3, :3].T, v[3, :3]
    fx = W / (2.0 * cam.tanfovx)
    pts, n = [], len(targets)
    cols = (W - 8) // 6
    for k in range(n):
        px, py = 4 + 6 * (k % cols), 4 + 6 * (k // cols)
        z = rng.uniform(3.0, 4.0)
        ndcx, ndcy = (2 * px + 1) / W - 1, (2 * py + 1) / H - 1
        pv = np.array([ndcx * z * W / (2 * fx), ndcy * z * H / (2 * fx), z])
        pts.append(R.T @ (pv - tr))
    m3 = torch.tensor(np.asarray(pts, np.float32).astype(np.float64))
    rot = torch.zeros((n, 4), dtype=torch.float64)
    rot[:, 0] = 1.0
    lo, hi = torch.full((n,), 1e-6, dtype=torch.float64), torch.full((n,), 1.0, dtype=torch.float64)
    tgt = torch.tensor(targets, dtype=torch.float64)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        r = ratio(*cov2d_undilated(cam, m3, mid[:, None].expand(n, 3), rot))
        lo, hi = torch.where(r < tgt, mid, lo), torch.where(r < tgt, hi, mid)
    s = (0.5 * (lo + hi)).numpy().astype(np.float32)
    g = dict(means3D=m3.numpy().astype(np.float32), scales=np.repeat(s[:, None], 3, 1), rotations=rot.numpy().astype(np.float32),
             opacities=np.full((n, 1), opacity, np.float32), colors_precomp=rng.uniform(0, 1, (n, 3)).astype(np.float32))
    return g


def test_floor_edge_takes_the_forwards_side(dev):
    """Gaussians walked to r ~ 2.5e-5 in 1-ulp steps of their scale: the backward takes the floor decision of the forward's fp32 r, also
    where the fp64 r falls on the other side.  Reference: the plain render fed o' composed with the fp64 term under the forward's decision."""
    W, H = 128, 96
    cam = oracle_camera(W, H, look_at((2.9, 0.7, 1.9)))
    n = 250
    g = _pixel_centred_scene(cam, FLOOR * (1.0 + np.linspace(-3e-6, 3e-6, n)), seed=1)
    f64 = torch.float64
    # walk each scale in ulps until the fp32 and fp64 decisions disagree (kept at its start when no step within 24 does)
    for i in range(n):
        s0 = g["scales"][i, 0]
        for step in range(25):
            s = s0
            for _ in range(step // 2 + (step % 2)):
                s = np.nextafter(s, np.float32(np.inf) if step % 2 else np.float32(0))
            gi = {k: v[i:i + 1].copy() for k, v in g.items()}
            gi["scales"][:] = s
            r64 = ratio(*cov2d_undilated(cam, torch.tensor(gi["means3D"], dtype=f64), torch.tensor(gi["scales"], dtype=f64),
                                         torch.tensor(gi["rotations"], dtype=f64))).item()
            if (staged_opacity32(cam, gi)[1][0] < np.float32(FLOOR)) != (r64 < FLOOR):
                g["scales"][i] = s
                break
    fl32 = _floored(cam, g)
    r64 = ratio(*cov2d_undilated(cam, torch.tensor(g["means3D"], dtype=f64), torch.tensor(g["scales"], dtype=f64),
                                 torch.tensor(g["rotations"], dtype=f64))).numpy()
    differ = fl32 != (r64 < FLOOR)
    print(f"floor edge: {fl32.sum()} of {n} floored by the forward, {differ.sum()} where the fp64 r disagrees")
    assert fl32.sum() > 20 and (~fl32).sum() > 20 and differ.sum() >= 1
    o_s = _staged(cam, g, dev)[0]
    assert np.array_equal(o_s, staged_opacity32(cam, g)[0])
    dL = np.random.default_rng(2).uniform(-1, 1, (3, H, W)).astype(np.float32)
    _, got = _render(cam, g, dev, True, dL)
    _, plain = _render(cam, _with_opacity(g, o_s), dev, False, dL)
    assert (np.abs(plain["opacities"]) > 0).sum() > 0.9 * n        # every Gaussian is seen, floored ones included
    ref = compose({k: np.asarray(v, np.float64) for k, v in plain.items()}, aa_term(cam, g, plain["opacities"], fl32))
    for k in ("means3D", "opacities", "scales"):
        assert rel_err(got[k], ref[k]) < 1e-5, k
        worst, row = row_err(got[k][differ], ref[k][differ])
        assert worst < 1e-4, (k, worst, row)
    # on the other side of the floor the covariance term would be large (c = 0.005: o g dc dominates the scale gradient)
    alt = compose({k: np.asarray(v, np.float64) for k, v in plain.items()}, aa_term(cam, g, plain["opacities"], ~fl32 & differ | fl32 & ~differ))
    assert row_err(got["scales"][differ], alt["scales"][differ])[0] > 1e-2


def test_thin_gaussians_against_fp64(dev):
    """Elongated Gaussians with r in [1e-4, 1e-2] (det0 = A C - B^2 a difference of nearly equal products, A C / det0 up to ~5e4): the
    forward's c and every gradient against fp64, bars from the measurement (printed):
      * c32 vs c64: worst 4.2e-3 (median 2.9e-5) -- what is left after the fma product difference comes from the fp32 A, B, C themselves;
      * gradients against the composed fp32 oracle, fp64 referee: means3D, means2D, opacities, scales, colours within the default bars;
      * rotations: 1.4e-4 norm-wise and 9.8e-3 in the worst row from fp64, where the composed fp32 reference is 8e-6 / 9e-5 (likely:
        the large o g dc term in dL/dcov3D, rounded to fp32 before the rotation step takes its small remainder).  Bars: 3e-4 norm-wise,
        2e-2 worst row."""
    W, H = 128, 96
    cam = ring_camera(W, H, v=0, bg=(0.1, 0.1, 0.1))
    P = 1500
    rng = np.random.default_rng(77)
    g = random_gaussians(P, seed=77, scale_lo=0.04, scale_hi=0.08, spread=0.8)
    tgt = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), P))
    f64 = torch.float64
    m3, rot = torch.tensor(g["means3D"], dtype=f64), torch.tensor(g["rotations"], dtype=f64)
    lo, hi = torch.full((P,), 1e-7, dtype=f64), torch.tensor(g["scales"][:, 0].astype(np.float64))
    for _ in range(60):      # shrink axes 1 and 2 until r hits the target: one long axis, two thin ones
        mid = 0.5 * (lo + hi)
        sc = torch.stack([hi.new_tensor(g["scales"][:, 0]), mid, mid], 1)
        r = ratio(*cov2d_undilated(cam, m3, sc, rot))
        lo, hi = torch.where(r < torch.tensor(tgt), mid, lo), torch.where(r < torch.tensor(tgt), hi, mid)
    g["scales"][:, 1] = g["scales"][:, 2] = (0.5 * (lo + hi)).numpy().astype(np.float32)
    A, B, C = cov2d_undilated(cam, m3, torch.tensor(g["scales"], dtype=f64), rot)
    r = ratio(A, B, C).numpy()
    o_s = _staged(cam, g, dev)[0]
    alive = o_s > 0
    assert alive.sum() > 1000 and r[alive].min() > 5e-5 and r[alive].max() < 2e-2
    c64 = np.sqrt(np.maximum(r, FLOOR))
    rel = np.abs(o_s[alive] / g["opacities"][alive, 0] - c64[alive]) / c64[alive]
    cancel = (A * C).numpy()[alive] / np.maximum((A * C - B * B).numpy()[alive], 1e-300)
    print(f"thin: c32 vs c64 worst rel {rel.max():.2e} (median {np.median(rel):.2e}); A C / det0 up to {cancel.max():.2e}")
    assert rel.max() < 1e-2
    gs = _with_opacity(g, o_s)
    ok = ~TiledOracle(cam, gs["means3D"], gs["opacities"], colors_precomp=gs["colors_precomp"], **_geo(gs)).ambiguous
    dL = np.random.default_rng(8).uniform(-1, 1, (3, H, W)).astype(np.float32)
    dL[:, ~ok] = 0.0
    _, got = _render(cam, g, dev, True, dL)
    floored = _floored(cam, g)
    ref, oc = _oracle_composed(cam, g, o_s, dL, floored)
    _compare("thin", got, ref, keys=tuple(k for k in KEYS if k != "rotations"),
             referee=lambda: _oracle_composed(cam, g, o_s, dL, floored, decisions_of=oc)[0])
    ref64 = _oracle_composed(cam, g, o_s, dL, floored, decisions_of=oc)[0]
    for k in ("means3D", "scales", "rotations"):
        print(f"thin {k} vs fp64: norm-wise HIP {rel_err(got[k], ref64[k]):.2e} / fp32 {rel_err(ref[k], ref64[k]):.2e}, "
              f"worst row HIP {row_err(got[k], ref64[k])[0]:.2e} / fp32 {row_err(ref[k], ref64[k])[0]:.2e}")
    assert rel_err(got["rotations"], ref64["rotations"]) < 3e-4 and row_err(got["rotations"], ref64["rotations"])[0] < 2e-2


# ---------------------------------------------------------------------------------------------------------------- defaults
def test_defaults_are_bit_identical(dev, monkeypatch):
    """antialiasing=False is the call without the keyword, bit for bit, for every output and gradient (C++ node, Python node, views)."""
    import diff_gaussian_rasterization as dgr
    cam = ring_camera(128, 96, v=1)
    g = _scene("scales", P=1500, seed=70)
    dL = np.random.default_rng(9).uniform(-1, 1, (3, 96, 128)).astype(np.float32)
    for pynode in (False, True):
        monkeypatch.setattr(dgr, "_PY_NODE", pynode)
        a_out, a_gr = _render(cam, g, dev, None, dL, alpha=True)
        b_out, b_gr = _render(cam, g, dev, False, dL, alpha=True)
        assert all(np.array_equal(x, y) for x, y in zip(a_out, b_out))
        assert a_gr.keys() == b_gr.keys() and all(np.array_equal(a_gr[k], b_gr[k]) for k in a_gr)
    cams = [ring_camera(128, 96, v=v) for v in range(2)]
    a, _ = _views(cams, g, dev, aa=False, seed=3)
    from diff_gaussian_rasterization import rasterize_gaussians_views
    t = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in g.items()}
    m2 = torch.zeros((2, 1500, 3), device=dev, requires_grad=True)
    out = rasterize_gaussians_views([_settings(c, dev) for c in cams], t["means3D"], m2, t["opacities"], colors_precomp=t["colors_precomp"],
                                    scales=t["scales"], rotations=t["rotations"])
    rng = np.random.default_rng(3)
    (out[0] * torch.tensor(rng.uniform(-1, 1, (2, 3, 96, 128)).astype(np.float32), device=dev)).sum().backward()
    for k in ("means3D", "opacities", "scales", "rotations", "colors_precomp"):
        assert np.array_equal(a[k], t[k].grad.cpu().numpy()), k
    assert np.array_equal(a["means2D"], m2.grad.cpu().numpy())


def test_alternating_modes_through_the_cpp_node(dev, monkeypatch):
    """Plain and anti-aliased calls of one scene alternate through the C++ node with its layer state (list reuse, capacity mode): each
    call gives its own mode's outputs and gradients -- those of the Python node, which remembers nothing -- so no stale list is reused."""
    import diff_gaussian_rasterization as dgr
    assert dgr._C is not None
    cam = ring_camera(128, 96, v=2)
    g = _scene("scales", P=1500, seed=71)
    dL = np.random.default_rng(10).uniform(-1, 1, (3, 96, 128)).astype(np.float32)
    monkeypatch.setattr(dgr, "_PY_NODE", True)
    ref = {aa: _render(cam, g, dev, aa, dL) for aa in (False, True)}
    monkeypatch.setattr(dgr, "_PY_NODE", False)
    st = dgr.layer_state(dev)
    st.reset()
    hits0 = st.stats()["list_reuse_hits"] + st.stats()["twins_seen_late"]
    for aa in (False, True, False, True, True, False, False, True):
        out, gr = _render(cam, g, dev, aa, dL)
        assert all(np.array_equal(x, y) for x, y in zip(out, ref[aa][0])), aa
        for k in gr:
            assert rel_err(gr[k], ref[aa][1][k]) < 1e-6, (aa, k)
    assert st.stats()["list_reuse_hits"] + st.stats()["twins_seen_late"] > hits0     # the repeats of one mode did look at the cache


# ---------------------------------------------------------------------------------------------------------------- full size
def test_full_size_step(dev, full_scene):
    """One 4 x 800^2 anti-aliased forward and backward of the benchmark scene: finite gradients, and no more list entries than the plain step."""
    from diff_gaussian_rasterization import _hip, rasterize_gaussians_views
    params, cams, p2r = full_scene
    rv = p2r(params)
    x = {k: rv[k].detach().contiguous() for k in ("means3D", "opacities", "colors_precomp", "scales", "rotations")}
    with torch.no_grad():
        n_plain = [s.num_rendered for s in _hip.rasterize_forward_batch(cams, x["means3D"], x["opacities"], x["colors_precomp"], None,
                                                                         x["scales"], x["rotations"], None)[3]]
        n_aa = [s.num_rendered for s in _hip.rasterize_forward_batch(cams, x["means3D"], x["opacities"], x["colors_precomp"], None,
                                                                      x["scales"], x["rotations"], None, antialiasing=True)[3]]
    print(f"full size: num_rendered plain {n_plain}, anti-aliased {n_aa}")
    assert all(a <= p for a, p in zip(n_aa, n_plain)) and sum(n_aa) < sum(n_plain)
    for p in params.values():
        p.grad = None
    m2 = torch.zeros((len(cams), rv["means3D"].shape[0], 3), device=dev, requires_grad=True)
    out = rasterize_gaussians_views(cams, rv["means3D"], m2, rv["opacities"], colors_precomp=rv["colors_precomp"], scales=rv["scales"],
                                    rotations=rv["rotations"], antialiasing=True)
    (out[0] * 0.5).sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    for k in ("means3D", "logit_opacities", "log_scales", "unnorm_rotations"):
        assert params[k].grad is not None and torch.isfinite(params[k].grad).all(), k
