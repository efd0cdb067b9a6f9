"""The rigid alignment of the training loss: per sample the rotation and translation that take one point cloud onto another over a mask
(Umeyama's least-squares fit with the scale fixed at 1 -- the reference's ``umeyama_algorithm(..., fixed_scale=True)``, its
src/gnn/utils.py:7-40, as its ``rigid_loss`` calls it, src/train.py:32-40).

The rule set, for one sample with ``n`` masked rows:

* ``mu_x``, ``mu_y`` are the masked means and ``C = (1 / n) sum_masked (Y - mu_y)(X - mu_x)^T``; ``s1 >= s2 >= s3`` are C's singular
  values, ``u_i`` / ``v_i`` its left / right vectors.
* rank >= 2, meaning ``s2 > 3 * 2^-23 * s1`` (the threshold of the bones' rotation fit), and ``n >= 3``:
  ``R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T`` -- the reference's ``U diag(1, 1, det U det V^T) V^T`` written so that no sign convention
  of an SVD enters, and its answer for a planar cloud too (rank 2: rope or cloth on the table).  ``code = 0``.
* rank <= 1 or ``n < 3``: the rotation is not determined; ``R = I``, ``t = mu_y - mu_x``, ``code = 1``.  The sample still has its ``sse``.
* ``n = 0``: ``R = I``, ``t = 0``, ``sse = 0``, ``code = 1``; nothing divides by zero.
* a non-finite value in a masked row of X or Y: the sample's ``R``, ``t``, ``aligned``, the masked rows of ``residual`` and ``sse`` are
  NaN (``code = 1``); no other sample is affected.  An unmasked row never enters the fit.
* ``t = mu_y - mu_x R^T``.

Nothing here is differentiable: the reference detaches the alignment.  Out of scope: the scale ``c`` (``fixed_scale=False``; the reference
never asks for it)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

RANK_TOL = 3.0 * 2.0 ** -23


def _kernel_ok(X, Y, mask) -> bool:
    return (X.is_cuda and X.dtype == torch.float32 and Y.dtype == torch.float32 and mask.dtype == torch.bool and Y.device == X.device
            and mask.device == X.device and X.is_contiguous() and Y.is_contiguous() and mask.is_contiguous())


def _check_shapes(X, Y, mask):
    if X.dim() != 3 or X.shape[2] != 3 or tuple(Y.shape) != tuple(X.shape) or tuple(mask.shape) != tuple(X.shape[:2]):
        raise ValueError(f"umeyama_fit: X, Y [B, N, 3] and mask [B, N], please (got {tuple(X.shape)}, {tuple(Y.shape)}, {tuple(mask.shape)})")
    if mask.dtype != torch.bool:
        raise ValueError(f"umeyama_fit: a bool mask, please (got {mask.dtype})")
    if Y.dtype != X.dtype or not X.dtype.is_floating_point:
        raise ValueError(f"umeyama_fit: X and Y of one floating dtype, please (got {X.dtype}, {Y.dtype})")


def umeyama_fit_torch(X: torch.Tensor, Y: torch.Tensor, mask: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The rule set of this module in plain torch, in the dtype of X (the DEFINITION; ``torch.linalg.svd`` of the B 3x3 matrices)."""
    _check_shapes(X, Y, mask)
    X, Y = X.detach(), Y.detach()
    B, dt = X.shape[0], X.dtype
    m = mask[..., None]
    zero = X.new_zeros(())
    count = mask.sum(1)
    n = count.clamp(min=1).to(dt)[:, None, None]
    mu_x = torch.where(m, X, zero).sum(1, keepdim=True) / n
    mu_y = torch.where(m, Y, zero).sum(1, keepdim=True) / n
    C = torch.where(m, Y - mu_y, zero).transpose(1, 2) @ torch.where(m, X - mu_x, zero) / n
    finite = torch.isfinite(C).all(2).all(1) & torch.isfinite(mu_x).all(2).all(1) & torch.isfinite(mu_y).all(2).all(1)
    U, S, Vh = torch.linalg.svd(torch.where(finite[:, None, None], C, zero))      # (a NaN never reaches the library)
    u1, u2, v1, v2 = U[:, :, 0], U[:, :, 1], Vh[:, 0], Vh[:, 1]
    u3, v3 = torch.linalg.cross(u1, u2), torch.linalg.cross(v1, v2)
    fit = u1[:, :, None] * v1[:, None] + u2[:, :, None] * v2[:, None] + u3[:, :, None] * v3[:, None]
    ok = finite & (count >= 3) & (S[:, 1] > RANK_TOL * S[:, 0])
    R = torch.where(ok[:, None, None], fit, torch.eye(3, dtype=dt, device=X.device).expand(B, 3, 3))
    R = torch.where(finite[:, None, None], R, X.new_full((), float("nan")))
    t = mu_y - mu_x @ R.transpose(1, 2)
    aligned = X @ R.transpose(1, 2) + t
    residual = torch.where(m, Y - aligned, zero)
    return dict(R=R, t=t, aligned=aligned, residual=residual, sse=(residual * residual).sum((1, 2)), count=count.to(torch.int32),
                code=(~ok).to(torch.int32))


def umeyama_fit(X: torch.Tensor, Y: torch.Tensor, mask: torch.Tensor, kernel: Optional[bool] = None) -> Dict[str, torch.Tensor]:
    """Per sample the rigid transform taking the masked rows of ``X`` onto those of ``Y``: X, Y [B, N, 3], mask [B, N] bool ->
    dict(R [B, 3, 3], t [B, 1, 3], aligned [B, N, 3] = X R^T + t, residual [B, N, 3] = Y - aligned on the masked rows and exactly 0
    elsewhere, sse [B] = sum of residual^2, count [B] int32 = the masked rows, code [B] int32) under the rule set of the module docstring.
    Nothing is differentiable.

    Contiguous float32 tensors on a HIP device go to the kernel ``gsr_rigid_fit`` (one launch, fp64 inside, every output rounded to fp32
    once, bit-identical from run to run); CPU tensors, float64 and non-contiguous views take the torch statement ``umeyama_fit_torch``.
    ``kernel``: None routes as just said, False forces the torch statement, True demands the kernel (``ValueError`` if the tensors do not
    qualify)."""
    _check_shapes(X, Y, mask)
    use = _kernel_ok(X, Y, mask) if kernel is None else bool(kernel)
    if not use:
        return umeyama_fit_torch(X, Y, mask)
    from diff_gaussian_rasterization import _hip
    return _hip.rigid_fit(X.detach(), Y.detach(), mask)
