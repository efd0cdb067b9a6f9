"""Rendered alpha, the parts that need no GPU: the ABI surface, the Python keyword and its documentation, and an fp64 check (dense oracle)
of the two identities the GPU tests (test_alpha_gpu.py) use as references:
  (I1) A = 1 - T_final is channel 0 of a render with colours 1 and background 0;
  (I2) A = 1 + channel 0 of a render with colours 0 and background (-1, 0, 0) -- the arithmetic of the blend backward's alpha term."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from oracle.dense_oracle import dense_rasterize, finite_difference
from util import random_gaussians, ring_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsr_alpha_views", "gsr_backward_ex", "gsr_backward_batch_ex")


def test_abi_exports():
    from diff_gaussian_rasterization import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)          # dlopen works without a GPU
    for sym in SYMBOLS:
        getattr(lib, sym)
        assert sym in _hip.EXPORTS
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        h = f.read()
    for sym in SYMBOLS:
        assert f"int {sym}(" in h


def test_keyword_defaults_and_docs():
    from diff_gaussian_rasterization import GaussianRasterizer, rasterize_gaussians, rasterize_gaussians_views
    for f in (GaussianRasterizer.__init__, rasterize_gaussians, rasterize_gaussians_views):
        assert inspect.signature(f).parameters["return_alpha"].default is False
    assert GaussianRasterizer(raster_settings=None).return_alpha is False
    assert GaussianRasterizer(raster_settings=None, return_alpha=True).return_alpha is True
    # the means2D note: a view's screen-space gradient includes its own alpha term
    for doc in (GaussianRasterizer.__doc__, rasterize_gaussians_views.__doc__):
        assert "means2D" in doc and "alpha term" in doc and "separate call" in doc


def test_torch_layer_takes_the_alpha_keywords():
    import diff_gaussian_rasterization as dgr
    if dgr._C is None:
        return
    assert "dL_dout_alpha" in dgr._C.rasterize_gaussians_backward.__doc__
    assert "return_alpha: bool = False" in dgr._C.rasterize.__doc__


def _cov3d(g):
    q = g["rotations"].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * g["scales"].astype(np.float64)[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


@pytest.mark.parametrize("cov", [False, True])
def test_identities_are_the_alpha_gradient(cov):
    """I1 and I2 through autograd agree with each other and with central finite differences of 1 - T_final (T_final read as channel 0
    of a third render: colours 0, background (1, 0, 0)), for means3D, opacities and scales / rotations or cov3D_precomp (fp64)."""
    P, W, H = 6, 14, 11
    g = random_gaussians(P, seed=78, scale_lo=0.2, scale_hi=0.5, spread=0.5)
    cam = ring_camera(W, H, v=1, radius=3.0)
    f64 = torch.float64
    dLa = torch.tensor(np.random.default_rng(1).uniform(-1, 1, (H, W)), dtype=f64)
    geo = ("cov3D_precomp",) if cov else ("scales", "rotations")
    base = {"means3D": g["means3D"], "opacities": g["opacities"]}
    if cov:
        base["cov3D_precomp"] = _cov3d(g)
    else:
        base.update(scales=g["scales"], rotations=g["rotations"])
    keys = ("means3D", "opacities") + geo

    def render(t, colour, bg):
        return dense_rasterize(H, W, cam.tanfovx, cam.tanfovy, torch.tensor(bg, dtype=f64), 1.0, torch.tensor(cam.viewmatrix),
                               torch.tensor(cam.projmatrix), 0, torch.tensor(cam.campos), t["means3D"], t["opacities"],
                               colors_precomp=torch.full((P, 3), float(colour), dtype=f64),
                               **{k: t[k] for k in geo})[0]

    grads, alphas = [], []
    for colour, bg, sign in ((1.0, (0.0, 0.0, 0.0), 1.0), (0.0, (-1.0, 0.0, 0.0), 1.0)):
        t = {k: torch.tensor(v, dtype=f64, requires_grad=True) for k, v in base.items()}
        c = render(t, colour, bg)
        a = c[0] if colour == 1.0 else 1.0 + c[0]
        (a * dLa).sum().backward()
        grads.append({k: t[k].grad.clone() for k in keys})
        alphas.append(a.detach())
    assert torch.allclose(alphas[0], alphas[1], rtol=0, atol=1e-12)
    assert alphas[0].max() > 0.3      # the scene covers the image
    for k in keys:
        assert torch.allclose(grads[0][k], grads[1][k], rtol=1e-10, atol=1e-12), k
    for k in keys:
        x0 = torch.tensor(base[k], dtype=f64)

        def loss_of(x, k=k):
            t = {kk: torch.tensor(v, dtype=f64) for kk, v in base.items()}
            t[k] = x
            with torch.no_grad():
                T = render(t, 0.0, (1.0, 0.0, 0.0))[0]       # the background term alone: T_final
            return ((1.0 - T) * dLa).sum()
        fd = finite_difference(loss_of, x0.clone(), eps=1e-6)
        err = (grads[0][k] - fd).abs().max() / fd.abs().max()
        assert fd.abs().max() > 1e-4 and err < 1e-5, f"{k}: {err:.3e}"
