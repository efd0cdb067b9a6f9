"""Camera gradients, the parts that need no GPU: the ABI additions, the keywords, and the dense fp64 oracle's
camera gradients against central finite differences of a 6-DoF pose -- the reference of test_camera_grad_gpu.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from camera_ref import F64, compose_camera, dense_camera_grads, dense_render, se3
from util import look_at, oracle_camera, random_gaussians

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_version_and_scratch():
    from diff_gaussian_rasterization import _hip
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        h = f.read()
    assert re.search(r"^#define GSR_VERSION 125\b", h, re.M)
    assert "typedef struct gsr_camera_grads" in h
    lib = ctypes.CDLL(_hip.LIB_PATH)          # dlopen works without a GPU
    for sym in ("gsr_backward_ex", "gsr_backward_batch_ex", "gsr_camera_scratch_bytes"):
        assert sym in _hip.EXPORTS
        getattr(lib, sym)
    assert lib.gsr_version() == 125
    lib = _hip.load_library()
    b = lib.gsr_camera_scratch_bytes
    assert b(1, 100, 96, 80) > 0 and b(1, 0, 96, 80) > 0
    assert b(4, 100_000, 800, 800) > b(1, 100_000, 800, 800) > b(1, 1000, 800, 800) > 0
    assert b(2, 300_000, 96, 80) > b(2, 100_000, 96, 80)
    # the record is four device pointers in the header's order
    assert [f[0] for f in _hip.GsrCameraGrads._fields_] == ["dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos", "dL_dbg"]


def test_keywords_default_false():
    from diff_gaussian_rasterization import GaussianRasterizer, rasterize_gaussians, rasterize_gaussians_views
    for f in (GaussianRasterizer.__init__, rasterize_gaussians, rasterize_gaussians_views):
        assert inspect.signature(f).parameters["camera_gradients"].default is False
    assert GaussianRasterizer(raster_settings=None).camera_gradients is False
    assert GaussianRasterizer(raster_settings=None, camera_gradients=True).camera_gradients is True
    from diff_gaussian_rasterization import _hip
    for f in (_hip.rasterize_backward, _hip.rasterize_backward_batch):
        assert inspect.signature(f).parameters["camera_grads"].default is None
    import diff_gaussian_rasterization as dgr
    if dgr._C is not None:
        assert "camera_gradients: bool = False" in dgr._C.rasterize.__doc__


def test_wrong_shaped_camera_tensors_rejected_before_any_launch():
    from diff_gaussian_rasterization import _camera_tensors
    from hipcheck import _settings
    rs = _settings(oracle_camera(32, 24, look_at((0, 0.5, 4.0))), torch.device("cpu"))
    assert len(_camera_tensors([rs, rs])) == 8
    for name, bad in (("bg", torch.zeros(4)), ("viewmatrix", torch.zeros(3, 4)), ("projmatrix", torch.zeros(1, 4, 3)),
                      ("campos", torch.zeros(2))):
        with pytest.raises(ValueError, match=name):
            _camera_tensors([rs._replace(**{name: bad})])


def _pose_loss(xi, w2c0, g, W, H, dL, sh_degree, bg):
    view, proj, campos = compose_camera(se3(xi) @ w2c0, W, H)
    img = dense_render(W, H, 0.5, H / (2.0 * W), bg, view.reshape(-1), proj.reshape(-1), campos, g, sh_degree)   # fx = fy = W
    return (img * dL).sum()


@pytest.mark.parametrize("sh", [0, 1])
def test_dense_oracle_camera_gradients_match_pose_finite_differences(sh):
    """d loss / d xi of a 6-DoF pose w2c(xi) = exp(xi) w2c0, composed as setup_camera composes it: autograd through the oracle's leaf-free
    graph against central differences (fp64), and the same number from the oracle's camera gradients chained by hand through the
    composition.  Small scenes, away from the decision boundaries (no Gaussian near the clamp, the alpha cut or the tile rects)."""
    W, H = 40, 32
    g = random_gaussians(30, seed=4, scale_lo=0.08, scale_hi=0.3, spread=0.5, sh_M=4 if sh else 0)
    if sh:
        del g["colors_precomp"]
    w2c0 = torch.tensor(look_at((0.4, 0.6, 3.2)), dtype=F64)
    bg = torch.tensor([0.2, 0.5, 0.7], dtype=F64)
    dL = torch.tensor(np.random.default_rng(1).uniform(-1, 1, (3, H, W)))
    xi = torch.zeros(6, dtype=F64, requires_grad=True)
    loss = _pose_loss(xi, w2c0, g, W, H, dL, sh, bg)
    loss.backward()
    ad = xi.grad.numpy().copy()
    eps = 1e-6
    fd = np.zeros(6)
    for k in range(6):
        e = torch.zeros(6, dtype=F64)
        e[k] = eps
        with torch.no_grad():
            fd[k] = (_pose_loss(e, w2c0, g, W, H, dL, sh, bg) - _pose_loss(-e, w2c0, g, W, H, dL, sh, bg)).item() / (2 * eps)
    # central differences of a smooth fp64 function: O(eps^2) truncation, 1e-10 / eps cancellation
    assert np.abs(ad - fd).max() / np.abs(fd).max() < 1e-5, (ad, fd)
    # the oracle's camera gradients (the GPU tests' reference), chained through the composition by autograd, give the same dL/dxi
    view, proj, campos = compose_camera(w2c0, W, H)
    cam = type("Cam", (), dict(image_width=W, image_height=H, tanfovx=0.5, tanfovy=H / (2.0 * W), bg=bg.numpy(),
                               viewmatrix=view.numpy(), projmatrix=proj.numpy(), campos=campos.numpy()))
    gb, gv, gp, gc = dense_camera_grads(cam, g, dL.numpy(), sh)
    xi2 = torch.zeros(6, dtype=F64, requires_grad=True)
    v2, p2, c2 = compose_camera(se3(xi2) @ w2c0, W, H)
    (torch.dot(v2.reshape(-1), torch.tensor(gv)) + torch.dot(p2.reshape(-1), torch.tensor(gp)) + torch.dot(c2, torch.tensor(gc))).backward()
    assert np.abs(xi2.grad.numpy() - ad).max() / np.abs(ad).max() < 1e-9
    # the entries the forward never reads get exactly zero, campos is zero for precomputed colours, bg = sum of T_final dL
    assert np.all(gv.reshape(4, 4)[:, 3] == 0) and np.all(gp.reshape(4, 4)[:, 2] == 0)
    assert (np.abs(gc).max() > 0) == bool(sh)
    assert np.abs(gb).max() > 0
