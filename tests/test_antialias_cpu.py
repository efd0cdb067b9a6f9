"""Anti-aliasing, the parts that need no GPU: the ABI bit, the keywords and the settings record, a finite-difference
check of the closed-form dr/d{A, B, C} and of the fp64 factor c(theta), and the composed references of test_antialias_gpu.py checked
against each other -- the tiled oracle fed o' plus the fp64 term, against the dense fp64 oracle fed o c(theta)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from antialias_ref import FLOOR, aa_factor, aa_term, compose, cov2d_undilated, ratio, ratio_closed_grad, staged_opacity32
from oracle import TiledOracle
from oracle.dense_oracle import dense_rasterize, finite_difference
from util import random_gaussians, rel_err, ring_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_bit_and_exports():
    from diff_gaussian_rasterization import _hip
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        h = f.read()
    assert re.search(r"^#define GSR_SETTINGS_ANTIALIASING 2\b", h, re.M)
    assert re.search(r"^#define GSR_VERSION 125\b", h, re.M)
    assert _hip.ANTIALIASING == 2
    lib = ctypes.CDLL(_hip.LIB_PATH)          # dlopen works without a GPU
    for sym in _hip.EXPORTS:
        getattr(lib, sym)
    # the switch rides in the existing settings word: the record keeps its layout
    assert [f[0] for f in _hip.GsrSettings._fields_][7] == "prefiltered" and ctypes.sizeof(_hip.GsrSettings) == 64


def test_keywords_default_false_and_settings_record():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians, rasterize_gaussians_views
    for f in (GaussianRasterizer.__init__, rasterize_gaussians, rasterize_gaussians_views):
        assert inspect.signature(f).parameters["antialiasing"].default is False
    assert GaussianRasterizer(raster_settings=None).antialiasing is False
    assert GaussianRasterizer(raster_settings=None, antialiasing=True).antialiasing is True
    assert len(GaussianRasterizationSettings._fields) == 11
    import diff_gaussian_rasterization as dgr
    if dgr._C is not None:
        assert "antialiasing: bool = False" in dgr._C.rasterize.__doc__
        assert "antialiasing: bool = False" in dgr._C.rasterize_gaussians_backward.__doc__
        assert "antialiasing: bool = False" in dgr._C.rasterize_gaussians.__doc__


def test_settings_word_carries_the_bit():
    from diff_gaussian_rasterization import _hip
    from hipcheck import _settings
    rs = _settings(ring_camera(32, 24), torch.device("cpu"))
    assert _hip._make_settings(rs, torch.device("cpu"), 0)[0].prefiltered == 0
    assert _hip._make_settings(rs, torch.device("cpu"), 0, antialiasing=True)[0].prefiltered == 2
    assert _hip._make_settings(rs._replace(prefiltered=True), torch.device("cpu"), 0, antialiasing=True)[0].prefiltered == 3


def test_closed_form_ratio_gradient():
    """dr/dA, dr/dB, dr/dC of the kernel's cancellation-free forms against central differences (fp64), thin Gaussians included."""
    rng = np.random.default_rng(3)
    n = 400
    A = np.exp(rng.uniform(np.log(1e-4), np.log(50.0), n))
    C = np.exp(rng.uniform(np.log(1e-4), np.log(50.0), n))
    B = rng.uniform(-0.999, 0.999, n) * np.sqrt(A * C)
    dA, dB, dC = ratio_closed_grad(A, B, C)
    for k, d in enumerate((dA, dB, dC)):
        x = [A.copy(), B.copy(), C.copy()]
        eps = 1e-7 * np.maximum(np.abs(x[k]), 1e-3)
        xp, xm = [v.copy() for v in x], [v.copy() for v in x]
        xp[k] += eps
        xm[k] -= eps
        fd = (ratio(*xp) - ratio(*xm)) / (2 * eps)
        assert np.abs(d - fd).max() / np.abs(fd).max() < 1e-6, k      # (thin Gaussians: r itself cancels, so the differences are norm-wise)
    # and the autograd of r itself
    t = [torch.tensor(v, requires_grad=True) for v in (A, B, C)]
    ratio(*t).sum().backward()
    for tt, d in zip(t, (dA, dB, dC)):
        assert np.allclose(tt.grad.numpy(), d, rtol=1e-9, atol=1e-15)


@pytest.mark.parametrize("cov", [False, True])
def test_factor_finite_difference(cov):
    """c(theta; camera) in fp64 torch: its autograd against central differences for means3D and scales / rotations or cov3D_precomp."""
    P = 12
    g = random_gaussians(P, seed=4, scale_lo=0.002, scale_hi=0.05, spread=0.6)
    cam = ring_camera(40, 30, v=1, radius=3.0)
    f64 = torch.float64
    base = {"means3D": g["means3D"], "scales": g["scales"], "rotations": g["rotations"]}
    if cov:
        from test_antialias_gpu import _cov3d
        base = {"means3D": g["means3D"], "cov3D_precomp": _cov3d(g)}
    w = torch.tensor(np.random.default_rng(1).uniform(0.5, 1.5, P), dtype=f64)

    def f(t):
        return (w * aa_factor(cam, t["means3D"], t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"))).sum()

    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in base.items()}
    c = aa_factor(cam, t["means3D"], t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"))
    assert (c.detach() < 0.5).any() and (c.detach() > FLOOR ** 0.5).all()
    f(t).backward()
    for k in base:
        def loss_of(x, k=k):
            tt = {kk: torch.tensor(v.astype(np.float64)) for kk, v in base.items()}
            tt[k] = x
            return f(tt)
        x0 = torch.tensor(base[k].astype(np.float64))
        fd = finite_difference(loss_of, x0, eps=1e-6 * float(x0.abs().max()))
        err = (t[k].grad - fd).abs().max() / fd.abs().max()
        assert err < 1e-5, f"{k}: {err:.3e}"


def test_host_ratio32_follows_fp64():
    """The host replication of the forward's fp32 r is close to fp64 r (the decision it gives is the forward's)."""
    g = random_gaussians(500, seed=6, scale_lo=0.002, scale_hi=0.15)
    cam = ring_camera(160, 120, v=1)
    f64 = torch.float64
    _, r32 = staged_opacity32(cam, g)
    r64 = ratio(*cov2d_undilated(cam, torch.tensor(g["means3D"], dtype=f64), torch.tensor(g["scales"], dtype=f64),
                                 torch.tensor(g["rotations"], dtype=f64))).numpy()
    front = (np.asarray(cam.viewmatrix, np.float32).reshape(4, 4)[:3, 2] @ g["means3D"].T.astype(np.float64)
             + np.asarray(cam.viewmatrix, np.float32).reshape(4, 4)[3, 2]) > 0.2
    assert r32.dtype == np.float32
    assert np.max(np.abs(r32[front] - r64[front]) / r64[front]) < 1e-2


def test_composed_oracles_agree():
    """The two references of the GPU tests, on the CPU at a small size: the fp32 tiled oracle fed o' (rounded o c_fp64), its gradients
    composed with the fp64 term, against the dense fp64 oracle fed o c(theta) through autograd."""
    P, W, H = 40, 36, 28
    g = random_gaussians(P, seed=11, scale_lo=0.004, scale_hi=0.25, spread=0.6)
    cam = ring_camera(W, H, v=2, radius=3.0, bg=(0.3, 0.2, 0.1))
    f64 = torch.float64
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in g.items()}
    c = aa_factor(cam, t["means3D"], t["scales"], t["rotations"])
    o_s = (g["opacities"].reshape(-1) * c.detach().numpy()).astype(np.float32)
    gs = dict(g, opacities=o_s.reshape(-1, 1))
    oc = TiledOracle(cam, gs["means3D"], gs["opacities"], colors_precomp=gs["colors_precomp"], scales=gs["scales"], rotations=gs["rotations"],
                     f64=True)
    dL = np.random.default_rng(2).uniform(-1, 1, (3, H, W)).astype(np.float32)
    dL[:, oc.ambiguous] = 0.0
    ref = compose({k: (None if v is None else np.asarray(v, np.float64)) for k, v in oc.backward(dL).items()},
                  aa_term(cam, g, oc.backward(dL)["opacities"]))
    img = dense_rasterize(H, W, cam.tanfovx, cam.tanfovy, torch.tensor(cam.bg, dtype=f64), 1.0, torch.tensor(cam.viewmatrix),
                          torch.tensor(cam.projmatrix), 0, torch.tensor(cam.campos), t["means3D"], t["opacities"] * c[:, None],
                          colors_precomp=t["colors_precomp"], scales=t["scales"], rotations=t["rotations"])[0]
    assert np.abs(img.detach().numpy() - oc.color)[:, ~oc.ambiguous].max() < 1e-5
    (img * torch.tensor(dL, dtype=f64)).sum().backward()
    assert c.min() < 0.3
    for k in ("means3D", "opacities", "scales", "rotations", "colors_precomp"):
        e = rel_err(ref[k], t[k].grad.numpy())
        assert e < 1e-5, f"{k}: {e:.3e}"
