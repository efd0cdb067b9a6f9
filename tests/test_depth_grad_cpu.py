"""Differentiable depth, the parts that need no GPU: the ABI surface, the Python keyword, and a finite-difference check (fp64, dense
oracle) of the colour-channel identity the GPU tests (test_depth_grad_gpu.py) use as their reference."""
import ctypes
import inspect
import os

import numpy as np
import torch

from oracle.dense_oracle import dense_rasterize, finite_difference
from util import random_gaussians, ring_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports():
    from diff_gaussian_rasterization import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)          # dlopen works without a GPU
    for sym in ("gsr_backward_ex", "gsr_backward_batch_ex", "gsr_backward_scratch_bytes_depth"):
        getattr(lib, sym)
        assert sym in _hip.EXPORTS
    sz, i32, u32 = ctypes.c_size_t, ctypes.c_int32, ctypes.c_uint32
    for f in (lib.gsr_backward_scratch_bytes, lib.gsr_backward_scratch_bytes_depth):
        f.restype, f.argtypes = sz, [i32, u32]
    for D in (0, 1, 1000, 123457):
        # the records keep their size; the depth scratch adds one float per entry behind them
        base = lib.gsr_backward_scratch_bytes(10, D)
        assert lib.gsr_backward_scratch_bytes_depth(10, D) >= base + 4 * max(D, 1)
    assert lib.gsr_backward_scratch_bytes(10, 1000) == -(-1000 * 9 * 4 // 256) * 256


def test_keyword_on_both_entry_points():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians_views
    assert len(GaussianRasterizationSettings._fields) == 11
    assert inspect.signature(rasterize_gaussians_views).parameters["differentiable_depth"].default is False
    assert inspect.signature(GaussianRasterizer.__init__).parameters["differentiable_depth"].default is False
    r = GaussianRasterizer(raster_settings=None, differentiable_depth=True)
    assert r.differentiable_depth is True
    assert GaussianRasterizer(raster_settings=None).differentiable_depth is False
    # fused pairs (views sharing a camera) are documented to run unfused in a depth backward
    assert "unfused" in rasterize_gaussians_views.__doc__
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        assert "differentiated unfused" in f.read()


def test_torch_layer_takes_the_depth_gradient_as_an_optional_argument():
    import diff_gaussian_rasterization as dgr
    if dgr._C is None:
        return
    doc = dgr._C.rasterize_gaussians_backward.__doc__
    assert "want_color_grad: bool = True" in doc and "dL_dout_depth" in doc and "= None" in doc
    assert "differentiable_depth: bool = False" in dgr._C.rasterize.__doc__


def _scene():
    P, W, H = 6, 14, 11
    g = random_gaussians(P, seed=77, scale_lo=0.2, scale_hi=0.5, spread=0.5)
    cam = ring_camera(W, H, v=1, radius=3.0)
    return g, cam, P, W, H


def _render(cam, g, m3, colors):
    f64 = torch.float64
    return dense_rasterize(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, torch.zeros(3, dtype=f64), 1.0,
                           torch.tensor(cam.viewmatrix), torch.tensor(cam.projmatrix), 0, torch.tensor(cam.campos), m3,
                           torch.tensor(g["opacities"], dtype=f64), colors_precomp=colors,
                           scales=torch.tensor(g["scales"], dtype=f64), rotations=torch.tensor(g["rotations"], dtype=f64))


def test_colour_channel_identity_is_the_depth_gradient():
    """D = sum_i alpha_i T_i z_i: the colour render with colour z(means3D) and background 0 has D as every channel, and autograd through
    it is the gradient of D itself (central finite differences of the forward's depth output, fp64)."""
    g, cam, P, W, H = _scene()
    f64 = torch.float64
    dLd = torch.tensor(np.random.default_rng(0).uniform(-1, 1, (H, W)), dtype=f64)
    vm = torch.tensor(cam.viewmatrix, dtype=f64).reshape(4, 4)   # column-major flat: z = p @ V[:3, 2] + V[3, 2]

    def z_of(m3):
        return m3 @ vm[:3, 2] + vm[3, 2]

    m3 = torch.tensor(g["means3D"], dtype=f64, requires_grad=True)
    color, _, depth, _ = _render(cam, g, m3, z_of(m3)[:, None].expand(P, 3))
    assert torch.allclose(color[0], depth[0], rtol=1e-12, atol=1e-12)     # the same image
    assert depth.abs().max() > 0.1
    (color[0] * dLd).sum().backward()
    dv = np.asarray(cam.viewmatrix, np.float64).reshape(-1)
    assert np.allclose(z_of(m3).detach().numpy(), g["means3D"].astype(np.float64) @ dv[[2, 6, 10]] + dv[14])

    def loss_of_depth(x):
        with torch.no_grad():
            _, _, d, _ = _render(cam, g, x, torch.zeros(P, 3, dtype=f64))
        return (d[0] * dLd).sum()
    fd = finite_difference(loss_of_depth, torch.tensor(g["means3D"], dtype=f64).clone(), eps=1e-6)
    err = (m3.grad - fd).abs().max() / fd.abs().max()
    assert fd.abs().max() > 1e-3 and err < 1e-5, f"{err:.3e}"
