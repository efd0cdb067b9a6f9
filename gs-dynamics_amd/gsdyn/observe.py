"""Depth cameras to planner state: unprojection, crop, voxel grid, outlier filter, farthest-point thinning -- the
perception step in front of ``plan_actions`` (the reference's ``get_tabletop_points`` / ``get_state_cur`` / ``construct_state``).

The definition.  It has one right answer, bit for bit, on CPU and GPU; every operation is in the tensors' dtype, one at a time, unfused.

Unprojection of pixel (x, y) of view v with depth d, ``K[v] = (fx, fy, cx, cy)``, ``R[v]``, ``t[v]`` (camera to board)::

    xc = ((x - cx) * (1/fx)) * d        yc = ((y - cy) * (1/fy)) * d        zc = d
    w_i = ((R[i,0]*xc + R[i,1]*yc) + R[i,2]*zc) + t[i]

A pixel is kept if ``depth_range[0] < d < depth_range[1]`` (both strict, the bounds rounded to fp32: a NaN and a RealSense zero drop
out), its mask is non-zero, and ``lo <= w <= hi`` on every axis (inclusive, as Open3D's crop).  ``voxel_down_sample`` takes ``points`` in
place of ``w`` and keeps the finite rows inside ``bounds``.

Voxel of a kept point: ``inv_h = fl32(1 / fl32(voxel_size))``; per axis ``u = fl(fl(w - lo) * inv_h)``, the cell is ``c = floor(u)``, the
offset ``f = u - c`` (exact).  The origin is the box's lower corner (Open3D anchors at the cloud's minimum minus h/2, which moves with one
noisy point).  ``(hi - lo) * inv_h >= 2^21 - 1`` on some axis raises ``ValueError``: the key is three 21-bit cells.

Mean -- exact, not a running fp32 sum: ``q = int64(f * 2^32)`` (exact for every cell >= 1; in cell 0 it truncates below 2^-32 of a cell),
``S`` = the integer sum of q over the voxel's n members, ``mean = fl32((c + S / (n * 2^32)) * (1/inv_h) + lo)`` evaluated in fp64.  Colours
are ``fl32(sum of the uint8 channel / (255 n))``, evaluated in fp64.

Rows ascend in ``"first"``, the lowest input index among a voxel's members (for images the flat pixel index ``(v*H + y)*W + x``).

Consequences: the rows as a set do not depend on the order of the input; two runs give the same bits; the device kernels
(csrc/gsr_voxel.hip) and the plain-torch statement below give the same bits.  With fp64 ``points`` the same formulas run in fp64 (inv_h =
1 / voxel_size in fp64); the bit-for-bit promises are for fp32."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .dynamics import downsample_vertices, remove_statistical_outliers

KERNEL_MAX_N = 1 << 24        # csrc/gsr_voxel.hip VOX_MAX_N
MAX_CELLS = float(2 ** 21 - 1)


# ------------------------------------------------------------------------------------------ the grid of a call
def _grid(lo, hi, voxel_size: float, dtype) -> dict:
    """Host constants of a call: the box as numbers of ``dtype``, inv_h, its fp64 reciprocal, cells of the box."""
    npt = np.float32 if dtype == torch.float32 else np.float64
    lo, hi = np.asarray(lo, dtype=npt).reshape(3), np.asarray(hi, dtype=npt).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError(f"the box must be finite with lo <= hi on every axis; got lo = {lo.tolist()}, hi = {hi.tolist()}")
    h = npt(voxel_size)
    if not (np.isfinite(h) and h > 0):
        raise ValueError(f"voxel_size must be a positive finite number; got {voxel_size!r}")
    with np.errstate(over="ignore", divide="ignore"):
        inv_h = npt(1.0) / h
        ext = (hi - lo) * inv_h
    if not np.isfinite(inv_h) or not (ext < npt(MAX_CELLS)).all():
        raise ValueError(f"(hi - lo) / voxel_size must stay below 2^21 - 1 on every axis (the key is three 21-bit cells); got {ext.tolist()}")
    cells = 1
    for e in ext:
        cells *= int(np.floor(e)) + 1
    return dict(lo=[float(x) for x in lo], hi=[float(x) for x in hi], inv_h=float(inv_h), h64=1.0 / float(inv_h), cells=cells)


def _empty(dev, dtype, with_colors: bool) -> Dict[str, Optional[torch.Tensor]]:
    return {"points": torch.empty((0, 3), dtype=dtype, device=dev), "colors": torch.empty((0, 3), dtype=torch.float32, device=dev) if with_colors else None,
            "counts": torch.empty((0,), dtype=torch.int32, device=dev), "first": torch.empty((0,), dtype=torch.int64, device=dev)}


def _voxel_torch(w: torch.Tensor, keep: torch.Tensor, colors: Optional[torch.Tensor], g: dict) -> Dict[str, Optional[torch.Tensor]]:
    """The definition in plain torch: w [N, 3], keep [N] bool (range, mask and box tests done), colors [N, 3] uint8 or None.  Elementwise
    operations only; the integer sums are ``index_add_`` on int64, the order a ``scatter_reduce(amin)`` of the index."""
    dev, dtype = w.device, w.dtype
    idx = torch.nonzero(keep)[:, 0]
    if idx.numel() == 0:
        return _empty(dev, dtype, colors is not None)
    lo = torch.tensor(g["lo"], dtype=dtype, device=dev)
    u = (w[idx] - lo) * g["inv_h"]
    c = torch.floor(u)
    q = ((u - c) * 4294967296.0).to(torch.int64)
    ci = c.to(torch.int64)
    key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
    uniq, inv = torch.unique(key, return_inverse=True)
    M = int(uniq.numel())
    n = torch.zeros(M, dtype=torch.int64, device=dev).index_add_(0, inv, torch.ones_like(inv))
    S = torch.zeros((M, 3), dtype=torch.int64, device=dev).index_add_(0, inv, q)
    first = torch.full((M,), int(w.shape[0]), dtype=torch.int64, device=dev).scatter_reduce_(0, inv, idx, "amin")
    order = torch.argsort(first)
    uniq, n, S, first = uniq[order], n[order], S[order], first[order]
    cell = torch.stack([uniq >> 42, (uniq >> 21) & 0x1fffff, uniq & 0x1fffff], 1).to(torch.float64)
    nd = n.to(torch.float64)
    mean = (cell + S.to(torch.float64) / (nd * 4294967296.0)[:, None]) * g["h64"] + lo.to(torch.float64)
    col = None
    if colors is not None:
        C = torch.zeros((M, 3), dtype=torch.int64, device=dev).index_add_(0, inv, colors[idx].to(torch.int64))[order]
        col = (C.to(torch.float64) / (255.0 * nd)[:, None]).to(torch.float32)
    return {"points": mean.to(dtype), "colors": col, "counts": n.to(torch.int32), "first": first}


def _inside(w: torch.Tensor, g: dict) -> torch.Tensor:
    lo, hi = torch.tensor(g["lo"], dtype=w.dtype, device=w.device), torch.tensor(g["hi"], dtype=w.dtype, device=w.device)
    return ((w >= lo) & (w <= hi)).all(-1)


def _check_colors(colors, lead_shape, dev, who: str):
    if colors is None:
        return
    if not (torch.is_tensor(colors) and colors.dtype == torch.uint8 and tuple(colors.shape) == tuple(lead_shape) + (3,)):
        raise ValueError(f"{who}: colors must be a uint8 tensor {list(lead_shape) + [3]}")
    if colors.device != dev:
        raise ValueError(f"{who}: colors must live on the device of the points / depths")


# ------------------------------------------------------------------------------------------ voxel_down_sample
@torch.no_grad()
def voxel_down_sample(points: torch.Tensor, voxel_size: float, *, colors: Optional[torch.Tensor] = None, bounds=None) -> Dict[str, Optional[torch.Tensor]]:
    """One mean point per occupied voxel, by the definition of this module: points [N, 3] (fp32 or fp64), colors None or uint8 [N, 3], bounds
    ``(lo[3], hi[3])`` -> {"points" [M, 3] in the dtype of ``points``, "colors" [M, 3] float in [0, 1] or None, "counts" [M] int32, "first" [M]
    int64}, rows ascending in ``first``.  Rows with a non-finite coordinate or outside ``bounds`` are dropped.

    ``bounds=None`` takes the per-axis minimum and maximum of the finite rows; that costs one extra host read-back (six numbers).
    A contiguous fp32 tensor on a HIP device with N <= 2^24 takes the kernels (csrc/gsr_voxel.hip; one 4-byte read-back, for M); every other
    input -- CPU, fp64, a strided view, a larger N -- the plain-torch statement of the same definition, with the same bits in fp32."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype not in (torch.float32, torch.float64):
        raise ValueError("voxel_down_sample: points must be a float32 or float64 tensor [N, 3]")
    points = points.detach()
    N, dev = int(points.shape[0]), points.device
    _check_colors(colors, (N,), dev, "voxel_down_sample")
    if bounds is None:
        fin = torch.isfinite(points).all(1)
        if N == 0 or not bool(fin.any()):
            return _empty(dev, points.dtype, colors is not None)
        p = points[fin]
        b = torch.stack([p.amin(0), p.amax(0)]).cpu().numpy()
        lo, hi = b[0], b[1]
    else:
        lo, hi = (x.detach().cpu().numpy() if torch.is_tensor(x) else x for x in bounds)
    g = _grid(lo, hi, voxel_size, points.dtype)
    if N == 0:
        return _empty(dev, points.dtype, colors is not None)
    if points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and N <= KERNEL_MAX_N and (colors is None or colors.is_contiguous()):
        from diff_gaussian_rasterization import _hip
        pts, col, cnt, first = _hip.voxel_points(points, g["lo"], g["hi"], g["inv_h"], min(N, g["cells"]), colors=colors)
        return {"points": pts, "colors": col, "counts": cnt, "first": first}
    return _voxel_torch(points, _inside(points, g), colors, g)


# ------------------------------------------------------------------------------------------ depth_to_cloud
def _intrinsics(K, V: int, dev) -> torch.Tensor:
    """[V, 4] = (fx, fy, cx, cy) fp32 on ``dev``; a [V, 3, 3] matrix is accepted and must have zero skew (that check reads K on the host)."""
    K = torch.as_tensor(K)
    if tuple(K.shape) == (V, 3, 3):
        Kh = K.detach().to("cpu", torch.float64)
        off = Kh.clone()
        off[:, 0, 0] = off[:, 1, 1] = off[:, 0, 2] = off[:, 1, 2] = 0.0
        off[:, 2, 2] -= 1.0
        if bool((off != 0).any()):
            raise ValueError("depth_to_cloud: a [V, 3, 3] K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (zero skew)")
        K = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1)
    if tuple(K.shape) != (V, 4):
        raise ValueError(f"depth_to_cloud: K must be [V, 4] = (fx, fy, cx, cy) or [V, 3, 3]; got {list(K.shape)} for V = {V}")
    return K.detach().to(device=dev, dtype=torch.float32).contiguous()


def _world_torch(depths: torch.Tensor, K4: torch.Tensor, R: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """The unprojection of the definition, elementwise and unfused: [V, H, W, 3]."""
    V, H, W = depths.shape
    dev = depths.device
    x = torch.arange(W, dtype=torch.float32, device=dev)[None, None, :]
    y = torch.arange(H, dtype=torch.float32, device=dev)[None, :, None]
    k = K4[:, :, None, None]
    xc = ((x - k[:, 2]) * (1.0 / k[:, 0])) * depths
    yc = ((y - k[:, 3]) * (1.0 / k[:, 1])) * depths
    r = R[:, :, :, None, None]
    return torch.stack([((r[:, i, 0] * xc + r[:, i, 1] * yc) + r[:, i, 2] * depths) + t[:, i, None, None] for i in range(3)], -1)


@torch.no_grad()
def depth_to_cloud(depths: torch.Tensor, K, R, t, bbox, *, colors: Optional[torch.Tensor] = None, masks: Optional[torch.Tensor] = None,
                   depth_range=(0.0, 2.0), voxel_size: float = 0.005) -> Dict[str, Optional[torch.Tensor]]:
    """The depth images of the fixed cameras -> the voxel-averaged cloud of the workspace, in the board frame (the definition of this module).

    depths [V, H, W] float32 metres; K [V, 4] = (fx, fy, cx, cy) or a zero-skew [V, 3, 3]; R [V, 3, 3] and t [V, 3] camera to board; bbox [3, 2]
    (rows x, y, z; columns lo, hi -- the reference's layout; a tensor or numpy; read on the host, so pass it from there); colors [V, H, W, 3]
    uint8; masks [V, H, W] bool or uint8 (a caller's segmentation).  Returns the dict of ``voxel_down_sample``; ``"first"`` is the flat pixel
    index ``(v*H + y)*W + x``.

    Contiguous device tensors with V*H*W <= 2^24 take one fused kernel over the pixels (csrc/gsr_voxel.hip: the world cloud is never
    written; one 4-byte read-back, for M); everything else the plain-torch statement, with the same bits."""
    if not torch.is_tensor(depths) or depths.dim() != 3 or depths.dtype != torch.float32:
        raise ValueError("depth_to_cloud: depths must be a float32 tensor [V, H, W]")
    depths = depths.detach()
    V, H, W = (int(s) for s in depths.shape)
    dev = depths.device
    K4 = _intrinsics(K, V, dev)
    R, t = torch.as_tensor(R), torch.as_tensor(t)
    if tuple(R.shape) != (V, 3, 3) or tuple(t.shape) != (V, 3):
        raise ValueError(f"depth_to_cloud: R must be [V, 3, 3] and t [V, 3]; got {list(R.shape)} and {list(t.shape)} for V = {V}")
    R, t = R.detach().to(device=dev, dtype=torch.float32).contiguous(), t.detach().to(device=dev, dtype=torch.float32).contiguous()
    box = np.asarray(bbox.detach().cpu().numpy() if torch.is_tensor(bbox) else bbox)
    if box.shape != (3, 2):
        raise ValueError(f"depth_to_cloud: bbox must be [3, 2] (rows x, y, z; columns lo, hi); got {list(box.shape)}")
    _check_colors(colors, (V, H, W), dev, "depth_to_cloud")
    if masks is not None and not (torch.is_tensor(masks) and masks.dtype in (torch.bool, torch.uint8) and tuple(masks.shape) == (V, H, W) and masks.device == dev):
        raise ValueError("depth_to_cloud: masks must be a bool or uint8 tensor [V, H, W] on the depths' device")
    if len(depth_range) != 2:
        raise ValueError("depth_to_cloud: depth_range = (lo, hi)")
    g = _grid(box[:, 0], box[:, 1], voxel_size, torch.float32)
    d_lo, d_hi = float(np.float32(depth_range[0])), float(np.float32(depth_range[1]))
    N = V * H * W
    if N == 0:
        return _empty(dev, torch.float32, colors is not None)
    if (depths.is_cuda and depths.is_contiguous() and N <= KERNEL_MAX_N and (colors is None or colors.is_contiguous())
            and (masks is None or masks.is_contiguous())):
        from diff_gaussian_rasterization import _hip
        pts, col, cnt, first = _hip.voxel_depth_views(depths, K4, R, t, g["lo"], g["hi"], d_lo, d_hi, g["inv_h"], min(N, g["cells"]), colors=colors, masks=masks)
        return {"points": pts, "colors": col, "counts": cnt, "first": first}
    w = _world_torch(depths, K4, R, t).reshape(N, 3)
    d = depths.reshape(N)
    keep = (d > d_lo) & (d < d_hi) & _inside(w, g)
    if masks is not None:
        keep = keep & (masks.reshape(N) != 0)
    return _voxel_torch(w, keep, None if colors is None else colors.reshape(N, 3), g)


# ------------------------------------------------------------------------------------------ observe_state
@torch.no_grad()
def observe_state(depths: torch.Tensor, K, R, t, bbox, *, colors: Optional[torch.Tensor] = None, masks: Optional[torch.Tensor] = None, depth_range=(0.0, 2.0),
                  voxel_size: float = 0.005, nb_neighbors: int = 25, std_ratio0: float = 1.5, fps_radius: float = 0.02, max_nobj: int = 100,
                  start_idx: int = 0) -> Dict[str, Optional[torch.Tensor]]:
    """The perception step in front of ``plan_actions``: ``depth_to_cloud``, then ``remove_statistical_outliers(points, nb_neighbors,
    std_ratio0, 0.5, knn="grid")``, then ``downsample_vertices(inliers, max_nobj, fps_radius, start_idx)``.

    Returns {"state" [n, 3]: what ``plan_actions(model, state, ...)`` takes; "points" [M, 3] and "colors" (or None): the voxel cloud;
    "inlier_idx" [m]: rows of ``points`` the outlier loop kept; "state_idx" [n]: rows of ``points`` the state was taken from}.  Segmentation
    models and the table-plane fit of the reference are not part of this: ``masks`` is where a caller's segmentation comes in."""
    cloud = depth_to_cloud(depths, K, R, t, bbox, colors=colors, masks=masks, depth_range=depth_range, voxel_size=voxel_size)
    pts = cloud["points"]
    if pts.shape[0] == 0:
        e = torch.empty((0,), dtype=torch.int64, device=pts.device)
        return {"state": pts, "points": pts, "colors": cloud["colors"], "inlier_idx": e, "state_idx": e}
    inl = remove_statistical_outliers(pts, nb_neighbors, std_ratio0, 0.5, knn="grid")
    state, idx = downsample_vertices(pts[inl].contiguous(), max_nobj, fps_radius, start_idx)
    return {"state": state, "points": pts, "colors": cloud["colors"], "inlier_idx": inl, "state_idx": inl[idx.to(inl.device)]}
