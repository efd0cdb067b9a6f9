"""SH colours in the multi-view batch: ``rasterize_gaussians_views(shs=..., batched_sh=True)``.

The forward is the per-view forward bit for bit; the backward -- gsr_backward_batch_ex with per-view colour gradients, then
gsr_sh_backward_views (sh_bwd_views_kernel) -- is held to the fp64 build of the oracle, per view with the fp32 run's decisions and summed
over the views in fp64, at the project's bars: norm-wise ``rel_err < TOL`` and the row-wise ``_row_check``."""
import os

import numpy as np
import pytest
import torch

from hipcheck import *  # noqa: F401,F403
from hipcheck import _ROW_LOG, _row_check, _settings  # noqa: F401
from util import look_at, oracle_camera

pytestmark = pytest.mark.gpu

W, H = 112, 80
NAMES = ("means3D", "opacities", "shs", "scales", "rotations")
_LOG = os.path.join(os.path.dirname(_ROW_LOG), "sh_views_distance.log")      # next to hipcheck's row-margins log
_refs = {}


def _reference(tag, g, cams, seed):
    """Per view: TiledOracle in fp32, its fp64 build with the fp32 run's decisions, the gradient image zeroed where the fp32 run calls a
    pixel ambiguous.  Returns (dL [V,3,H,W] fp32, view-summed fp64 gradients, per-view fp64 means2D gradients, fp32 oracles).  Computed
    once per scene and left unchanged."""
    if tag in _refs:
        return _refs[tag]
    rng = np.random.default_rng(seed)
    kw = dict(shs=g["shs"], scales=g["scales"], rotations=g["rotations"], nthreads=4)
    dLs, m2, o32s = [], [], []
    total = {k: np.zeros(g[k].shape, np.float64) for k in NAMES}
    for cam in cams:
        o32 = TiledOracle(cam, g["means3D"], g["opacities"], **kw)
        o64 = TiledOracle(cam, g["means3D"], g["opacities"], f64=True, decisions_of=o32, **kw)
        dL = rng.uniform(-1, 1, (3, cam.image_height, cam.image_width)).astype(np.float32)
        dL[:, o32.ambiguous] = 0.0
        g64 = o64.backward(dL)
        for k in NAMES:
            total[k] += np.asarray(g64[k], np.float64).reshape(total[k].shape)
        dLs.append(dL); m2.append(np.asarray(g64["means2D"], np.float64)); o32s.append(o32)
    _refs[tag] = (np.stack(dLs), total, m2, o32s)
    return _refs[tag]


def _run(g, settings, dL, dev, backward=True, extra_loss=None, unaligned_shs=False, **kw):
    from diff_gaussian_rasterization import rasterize_gaussians_views
    V, P = len(settings), g["means3D"].shape[0]
    t = {k: torch.tensor(g[k], device=dev, requires_grad=True) for k in NAMES}
    leaves = dict(t)
    if unaligned_shs:      # the coefficients as rows 1.. of a larger leaf: contiguous, 12 M bytes past an aligned address
        big = torch.zeros((P + 1,) + g["shs"].shape[1:], device=dev)
        big[1:] = torch.as_tensor(g["shs"], device=dev)
        leaves["shs"] = big.requires_grad_(True)
        t["shs"] = leaves["shs"][1:]
        assert t["shs"].is_contiguous() and t["shs"].data_ptr() % 16 != 0
    m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
    out = rasterize_gaussians_views(settings, t["means3D"], m2, t["opacities"], shs=t["shs"], scales=t["scales"],
                                    rotations=t["rotations"], **kw)
    if backward:
        loss = (out[0] * torch.as_tensor(dL, device=dev)).sum()
        if extra_loss is not None:
            loss = loss + extra_loss(out)
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in leaves.items()}
    if unaligned_shs and grads["shs"] is not None:
        assert not grads["shs"][0].any()
        grads["shs"] = grads["shs"][1:]
    grads["means2D"] = m2.grad
    return out, grads


def _against_fp64(tag, g, cams, dev, seed, **kw):
    dL, total, m2, o32s = _reference(tag, g, cams, seed)
    out, grads = _run(g, [_settings(c, dev) for c in cams], dL, dev, batched_sh=True, **kw)
    n = lambda x: x.detach().cpu().numpy()  # noqa: E731
    for v, o in enumerate(o32s):
        assert np.array_equal(n(out[1][v]), o.radii), (tag, v)
    for k in NAMES:
        assert grads[k] is not None and torch.isfinite(grads[k]).all(), (tag, k)
        err = rel_err(n(grads[k]), total[k])
        print(f"{tag} grad {k}: norm-wise {err:.3e}")
        assert err < TOL, (tag, k, err)
        _row_check(f"sh views {tag} grad {k} (view sum, fp64)", n(grads[k]), total[k])
    for v in range(len(cams)):
        if np.abs(m2[v]).max() == 0.0:      # a view that sees nothing: exact zeros
            assert not n(grads["means2D"][v]).any(), (tag, v)
            continue
        err = rel_err(n(grads["means2D"][v]), m2[v])
        assert err < TOL, (tag, v, err)
        _row_check(f"sh views {tag} view {v} grad means2D (fp64)", n(grads["means2D"][v]), m2[v])
    # exact zeros: coefficients beyond the degree's, and the rows of Gaussians no view saw
    deg = cams[0].sh_degree
    gs = n(grads["shs"])
    assert not gs[:, (deg + 1) ** 2:, :].any(), tag
    unseen = np.all(np.stack([o.radii for o in o32s]) <= 0, axis=0)
    assert not gs[unseen].any(), tag
    return out, grads, o32s


def test_forward_is_the_per_view_forward(dev):
    """Two cameras and a repeat, M = 16 at degree 2: colour, radii and depth equal three GaussianRasterizer calls bit for bit (the same
    preprocess and blend kernel bodies, fed from the view table)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    P = 600
    g = random_gaussians(P, seed=71, scale_lo=0.03, scale_hi=0.25, sh_M=16)
    s0, s1 = (_settings(ring_camera(W, H, v=i, sh_degree=2, bg=(0.2, 0.3, 0.1)), dev) for i in (0, 1))
    settings = [s0, s1, s0]
    out, _ = _run(g, settings, None, dev, backward=False, batched_sh=True)
    t = {k: torch.tensor(g[k], device=dev) for k in NAMES}
    for v, rs in enumerate(settings):
        im, radii, depth = GaussianRasterizer(raster_settings=rs)(means3D=t["means3D"], means2D=torch.zeros((P, 3), device=dev),
                                                                 opacities=t["opacities"], shs=t["shs"], scales=t["scales"],
                                                                 rotations=t["rotations"])
        assert torch.equal(out[0][v], im) and torch.equal(out[1][v], radii) and torch.equal(out[2][v], depth), v


# a reduced cross: every tile edge of the 64-Gaussian wave tile at (16, 3) and two views; every coefficient count and every view count at
# P = 257; and M = 10 at degree 2, a count that is none of 1 / 4 / 9 / 16: the kernel build that takes M at run time
_EDGES = ([(P, 16, 3, 2) for P in (1, 63, 64, 65, 257)] + [(257, M, d, 2) for M, d in ((1, 0), (4, 1), (9, 2), (16, 1), (10, 2))]
          + [(257, 16, 3, V) for V in (1, 5)])


@pytest.mark.parametrize("P,M,deg,V", _EDGES)
def test_backward_against_fp64_at_the_shape_edges(dev, P, M, deg, V):
    g = random_gaussians(P, seed=100 + P + M, scale_lo=0.05, scale_hi=0.3, spread=1.0 if P == 1 else 2.2, sh_M=M)   # (some Gaussians outside every frustum)
    cams = [ring_camera(W, H, v=i, V=5, sh_degree=deg, bg=(0.1, 0.2, 0.3)) for i in range(V)]
    _against_fp64(f"edges P{P} M{M} deg{deg} V{V}", g, cams, dev, seed=P + 7 * V)


def test_coefficients_off_the_16_byte_grid(dev):
    """``shs`` as a contiguous slice that starts 12 bytes past an aligned address (M = 1): the coalesced phases cannot move 16 bytes at a
    time and take their 4-byte form.  Same scene, cameras and reference as the (257, 1, 0, 2) edge case."""
    P, M, deg, V = 257, 1, 0, 2
    g = random_gaussians(P, seed=100 + P + M, scale_lo=0.05, scale_hi=0.3, spread=2.2, sh_M=M)
    cams = [ring_camera(W, H, v=i, V=5, sh_degree=deg, bg=(0.1, 0.2, 0.3)) for i in range(V)]
    _against_fp64(f"edges P{P} M{M} deg{deg} V{V}", g, cams, dev, seed=P + 7 * V, unaligned_shs=True)


def test_the_cases_a_view_loop_gets_wrong(dev):
    """One scene with (a) a view that looks away (every radius <= 0), (b) Gaussians that only some views see, (c) SH colours clamped at 0
    in some (view, Gaussian, channel) and not in others -- each condition asserted on the oracle before anything is compared."""
    P = 300
    g = random_gaussians(P, seed=5, scale_lo=0.05, scale_hi=0.3, spread=2.5, sh_M=16)
    g["shs"][::3, 0, :] -= 1.4          # a third of the Gaussians sit near rgb = 0: some channels clamp in some views
    kw = dict(sh_degree=3, bg=(0.3, 0.1, 0.2))
    away = oracle_camera(W, H, look_at((4.0, 0.8, 0.0), target=(9.0, 0.8, 0.0)), **kw)
    cams = [ring_camera(W, H, v=0, **kw), away, ring_camera(W, H, v=1, **kw), ring_camera(W, H, v=2, **kw)]
    _, _, _, o32s = _reference("view loop", g, cams, 11)
    radii = np.stack([o.radii for o in o32s])
    assert (radii[1] <= 0).all(), "(a) the second camera must see nothing"
    seen = radii[[0, 2, 3]] > 0
    assert (seen.any(0) & ~seen.all(0)).sum() >= 10, "(b) Gaussians visible in some views only"
    rgb = np.stack([o.rgb for o in o32s])[[0, 2, 3]]
    vis = np.broadcast_to(seen[:, :, None], rgb.shape)
    assert ((rgb == 0) & vis).sum() >= 10 and ((rgb > 0) & vis).sum() >= 10, "(c) clamped and unclamped channels among the visible"
    both = ((rgb == 0) & vis).any(0) & ((rgb > 0) & vis).any(0)
    assert both.any(), "(c) a (Gaussian, channel) clamped in one view and not in another"
    _against_fp64("view loop", g, cams, dev, seed=11)


def test_seventeen_views_split_into_two_library_calls(dev):
    """V = 17 > GSR_MAX_BATCH: two library calls, autograd adds the two dL/dsh -- still the fp64 sum over all views."""
    P, V, w, h = 200, 17, 64, 48
    g = random_gaussians(P, seed=17, scale_lo=0.05, scale_hi=0.3, sh_M=16)
    cams = [ring_camera(w, h, v=i, V=V, sh_degree=3, bg=(0.0, 0.1, 0.2)) for i in range(V)]
    _against_fp64("17 views", g, cams, dev, seed=17)


def _scene(dev, P=400, V=3, seed=33):
    g = random_gaussians(P, seed=seed, scale_lo=0.04, scale_hi=0.3, spread=1.5, sh_M=16)
    cams = [ring_camera(W, H, v=i, sh_degree=3, bg=(0.2, 0.2, 0.4)) for i in range(V)]
    dL = np.random.default_rng(seed).uniform(-1, 1, (V, 3, H, W)).astype(np.float32)
    return g, [_settings(c, dev) for c in cams], dL


def test_same_call_twice_is_bit_identical(dev):
    g, settings, dL = _scene(dev)
    _, a = _run(g, settings, dL, dev, batched_sh=True)
    _, b = _run(g, settings, dL, dev, batched_sh=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("switches", [("differentiable_depth",), ("return_alpha",), ("antialiasing",),
                                      ("differentiable_depth", "return_alpha", "antialiasing")], ids="+".join)
def test_with_the_other_switches(dev, switches):
    """Depth, alpha and anti-aliasing, alone and together, with loss terms on depth and alpha: the outputs equal the ``batched_sh=False``
    call's (which existing tests hold to the oracle) bit for bit, every gradient within TOL norm-wise -- the project's bar between two
    fp32 evaluations; the observed distance goes to sh_views_distance.log, next to hipcheck's row-margins log."""
    g, settings, dL = _scene(dev)
    kw = {s: True for s in switches}
    rng = np.random.default_rng(2)
    dD = torch.tensor(rng.uniform(-1, 1, (len(settings), 1, H, W)).astype(np.float32), device=dev)
    dA = torch.tensor(rng.uniform(-1, 1, (len(settings), 1, H, W)).astype(np.float32), device=dev)

    def extra(out):
        loss = (out[2] * dD).sum() if "differentiable_depth" in switches else 0.0
        return loss + ((out[3] * dA).sum() if "return_alpha" in switches else 0.0)
    out_on, on = _run(g, settings, dL, dev, extra_loss=extra, batched_sh=True, **kw)
    out_off, off = _run(g, settings, dL, dev, extra_loss=extra, batched_sh=False, **kw)
    assert len(out_on) == len(out_off) == (4 if "return_alpha" in switches else 3)
    for a, b in zip(out_on, out_off):
        assert torch.equal(a, b)
    lines = []
    for k in off:
        d = rel_err(on[k].cpu().numpy(), off[k].cpu().numpy())
        lines.append(f"{'+'.join(switches)} grad {k}: on vs off norm-wise {d:.3e}")
        print(lines[-1])
        assert d < TOL, (k, d)
    try:
        os.makedirs(os.path.dirname(_LOG), exist_ok=True)
        with open(_LOG, "a") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass


def test_camera_gradients_take_the_per_view_path(dev):
    """``camera_gradients=True``: the batch camera pass has no SH term for campos, so the call runs per view whatever ``batched_sh`` says --
    images, gradients and camera gradients are the ``batched_sh=False`` call's bit for bit."""
    g, settings, dL = _scene(dev, V=2)
    res = []
    for flag in (True, False):
        ss = [rs._replace(**{f: getattr(rs, f).clone().requires_grad_(True) for f in ("bg", "viewmatrix", "projmatrix", "campos")})
              for rs in settings]
        out, grads = _run(g, ss, dL, dev, camera_gradients=True, batched_sh=flag)
        cam = [getattr(rs, f).grad for rs in ss for f in ("bg", "viewmatrix", "projmatrix", "campos")]
        assert all(c is not None for c in cam)
        res.append((out, grads, cam))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.equal(a, b)


def test_backward_twice_over_one_forward(dev):
    """retain_graph: the SH pass adds into dL_dmeans3D, so every backward must start from a freshly written buffer."""
    from diff_gaussian_rasterization import rasterize_gaussians_views
    g, settings, dL = _scene(dev)
    V, P = len(settings), g["means3D"].shape[0]
    t = {k: torch.tensor(g[k], device=dev, requires_grad=True) for k in NAMES}
    m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
    im = rasterize_gaussians_views(settings, t["means3D"], m2, t["opacities"], shs=t["shs"], scales=t["scales"],
                                   rotations=t["rotations"], batched_sh=True)[0]
    d = torch.tensor(dL, device=dev)
    im.backward(gradient=d, retain_graph=True)
    first = {k: v.grad.clone() for k, v in t.items()}
    for v in t.values():
        v.grad = None
    im.backward(gradient=d)
    torch.cuda.synchronize()
    for k, v in t.items():
        assert torch.isfinite(v.grad).all() and torch.equal(first[k], v.grad), k
