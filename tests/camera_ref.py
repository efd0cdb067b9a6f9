"""References of the camera-gradient tests: the camera composed from a world-to-camera matrix as
gsdyn.camera.setup_camera composes it (in torch, differentiable), a 6-DoF pose perturbation, and the dense fp64 oracle's camera gradients.

The dense oracle (oracle/dense_oracle.py) builds everything from viewmatrix, projmatrix, campos and bg as fp64 torch ops, so leaf camera
tensors that require a gradient give the exact fp64 camera gradient; its clamped tx / ty and radius are detached constants, as the
kernels treat them."""
import numpy as np
import torch

from oracle.dense_oracle import dense_rasterize

F64 = torch.float64
CAMERA_KEYS = ("bg", "viewmatrix", "projmatrix", "campos")


def twist(xi):
    """4 x 4 twist matrix of xi = (omega, tau) (any dtype / device)."""
    z = xi.new_zeros(())
    w0, w1, w2, t0, t1, t2 = xi[0], xi[1], xi[2], xi[3], xi[4], xi[5]
    return torch.stack([torch.stack([z, -w2, w1, t0]), torch.stack([w2, z, -w0, t1]), torch.stack([-w1, w0, z, t2]),
                        torch.stack([z, z, z, z])])


def se3(xi):
    """exp(twist(xi)): exactly the identity at xi = 0."""
    return torch.linalg.matrix_exp(twist(xi))


def compose_camera(w2c, W, H, fx=None, fy=None, cx=None, cy=None, near=0.01, far=100.0):
    """(viewmatrix [1,4,4], projmatrix [1,4,4], campos [3]) from a world-to-camera matrix, as gsdyn.camera.setup_camera composes them
    (the transposed w2c, w2c^T bmm opengl_proj^T, torch.inverse(w2c)[:3, 3]); differentiable, in w2c's dtype and device."""
    fx = float(W) if fx is None else fx
    fy = float(W) if fy is None else fy
    cx = W / 2.0 if cx is None else cx
    cy = H / 2.0 if cy is None else cy
    gl = torch.tensor([[2 * fx / W, 0.0, -(W - 2 * cx) / W, 0.0], [0.0, 2 * fy / H, -(H - 2 * cy) / H, 0.0],
                       [0.0, 0.0, far / (far - near), -(far * near) / (far - near)], [0.0, 0.0, 1.0, 0.0]],
                      dtype=w2c.dtype, device=w2c.device)
    view = w2c.unsqueeze(0).transpose(1, 2)
    proj = view.bmm(gl.unsqueeze(0).transpose(1, 2))
    campos = torch.inverse(w2c)[:3, 3]
    return view, proj, campos


def dense_render(W, H, tanfovx, tanfovy, bg, view, proj, campos, g, sh_degree=0):
    """The dense fp64 oracle's colour image of scene dict g (numpy or tensors) under the given camera tensors."""
    t = {k: (v if isinstance(v, torch.Tensor) else torch.tensor(np.asarray(v, np.float64))).to(F64) for k, v in g.items()}
    return dense_rasterize(H, W, tanfovx, tanfovy, bg, 1.0, view, proj, sh_degree, campos, t["means3D"], t["opacities"],
                           colors_precomp=t.get("colors_precomp"), scales=t.get("scales"), rotations=t.get("rotations"),
                           shs=t.get("shs"), cov3D_precomp=t.get("cov3D_precomp"))[0]


def dense_camera_grads(cam, g, dL, sh_degree=0):
    """dL/d(bg, viewmatrix, projmatrix, campos) of sum(dL * colour) from the dense fp64 oracle, flat numpy arrays of 3, 16, 16, 3
    (campos: zeros when the colours are precomputed -- the oracle never reads it then)."""
    leaves = [torch.tensor(np.asarray(a, np.float64).reshape(-1), dtype=F64, requires_grad=True)
              for a in (cam.bg, cam.viewmatrix, cam.projmatrix, cam.campos)]
    img = dense_render(cam.image_width, cam.image_height, cam.tanfovx, cam.tanfovy, leaves[0], leaves[1], leaves[2], leaves[3], g, sh_degree)
    (img * torch.tensor(np.asarray(dL, np.float64))).sum().backward()
    return [np.zeros(t.numel()) if t.grad is None else t.grad.numpy() for t in leaves]
