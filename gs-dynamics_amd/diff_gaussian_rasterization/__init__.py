"""``diff_gaussian_rasterization`` -- MI355X-native drop-in for the rasterizer package gs-dynamics imports.

Same import surface the reference uses:

    from diff_gaussian_rasterization import GaussianRasterizer                          # render/renderer.py:3
    from diff_gaussian_rasterization import GaussianRasterizationSettings as Camera     # tracking/helpers.py:5
    im, radius, depth = GaussianRasterizer(raster_settings=cam)(**rendervar)            # tracking/train_utils.py:178

(paths relative to /root/reference/src).  The compute path is ``libgsr_hip.so`` (hand-written gfx950
kernels behind the C-ABI of ``include/gsr.h``); this module is the thin host mirror: argument checks,
allocation through torch's caching allocator, and the autograd glue.  There is no CPU implementation.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import nn

import os

from . import _hip

# The torch C++ layer (csrc/gsr_torch.cpp -> _C.so, built by __graft_entry__.build()): a single-view call is ONE native call,
# _C.rasterize, whose autograd node is in C++.  Absent (not built) or switched off (GSR_NO_TORCH_EXT=1, or GSR_HIP_LIB pointing at
# another library build, which _C is not linked against): the Python node _RasterizeGaussians over the ctypes binding in _hip.py
# does the same work call by call.  Multi-view calls always take the ctypes binding.
_C = None
if os.environ.get("GSR_NO_TORCH_EXT") != "1" and "GSR_HIP_LIB" not in os.environ:
    try:
        import importlib
        _C = importlib.import_module(__name__ + "._C")
    except ImportError:
        _C = None
_CTYPES_FORWARD, _CTYPES_BACKWARD = _hip.rasterize_forward, _hip.rasterize_backward
_PY_NODE = os.environ.get("GSR_PY_AUTOGRAD") == "1"   # A/B: the Python node over the ctypes binding instead of _C.rasterize


_LAYER_STATES = {}     # device index -> _C.LayerState: what the torch C++ layer remembers between GaussianRasterizer calls on that device


def layer_state(device=None):
    """The torch C++ layer's state for ``device`` (default: the current HIP device), created on first use: the last forward's tile lists
    (the reference renders every camera twice with the same geometry), the entry capacities per (P, H, W) of the capacity-mode forward and
    the twin predictor.  Owned HERE, not by the extension (no global state in the library or its torch layer):
    ``layer_state().stats()`` inspects it, ``.reset()`` forgets everything learned, ``.list_reuse`` / ``.capacity_mode`` are the switches,
    ``reset_layer_states()`` drops every device's.  None when the C++ layer is not loaded."""
    if _C is None:
        return None
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = torch.cuda.current_device() if dev.index is None else dev.index
    st = _LAYER_STATES.get(idx)
    if st is None:
        st = _LAYER_STATES[idx] = _C.LayerState()
    return st


def reset_layer_states():
    _LAYER_STATES.clear()


def _native():
    """The torch C++ layer, unless a test double / spy has replaced the ctypes entry points (then those must be the ones called)."""
    if _C is not None and _hip.rasterize_forward is _CTYPES_FORWARD and _hip.rasterize_backward is _CTYPES_BACKWARD:
        return _C
    return None


__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "rasterize_gaussians_views", "layer_state",
           "reset_layer_states"]


class GaussianRasterizationSettings(NamedTuple):
    """Per-view camera record; the 11 fields (names and order) the reference constructs at
    /root/reference/src/tracking/helpers.py:20-32."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool


def _prep(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """None for absent/empty inputs, else a contiguous fp32 tensor (no copy when already so)."""
    if t is None or t.numel() == 0:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _save_inputs(ctx, m3, radii, col_, sh_, sc_, rot_, cov_):
    """Which optional inputs the call had (``ctx.has``), and the inputs the backward needs (absent ones as empty placeholders)."""
    ctx.has = (sh_ is not None, col_ is not None, sc_ is not None, cov_ is not None)
    empty = m3.new_empty(0)
    ctx.save_for_backward(m3, radii, *(empty if t is None else t for t in (col_, sh_, sc_, rot_, cov_)))
    ctx.mark_non_differentiable(radii)


def _input_grads(ctx, d_means3D, d_means2D, d_sh, d_colors, d_opacity, d_scales, d_rot, d_cov):
    """One gradient slot per apply() argument: None for the inputs the call did not have and for the settings and the switches."""
    has_sh, has_col, has_sc, has_cov = ctx.has
    return (d_means3D, d_means2D, d_sh if has_sh else None, d_colors if has_col else None, d_opacity, d_scales if has_sc else None,
            d_rot if has_sc else None, d_cov if has_cov else None, None, None, None, None, None)


_CAMERA_FIELDS = ("bg", "viewmatrix", "projmatrix", "campos")   # the settings tensors camera_gradients differentiates, in apply() order
_CAMERA_NUMEL = (3, 16, 16, 3)


def _camera_tensors(settings_list):
    """The trailing apply() arguments of a camera_gradients call: (bg, viewmatrix, projmatrix, campos) of every view, checked."""
    out = []
    for rs in settings_list:
        for name, n in zip(_CAMERA_FIELDS, _CAMERA_NUMEL):
            t = getattr(rs, name)
            if not isinstance(t, torch.Tensor) or t.numel() != n:
                raise ValueError(f"camera_gradients=True: raster_settings.{name} must be a tensor of {n} elements, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            out.append(t)
    return out


def _camera_grads(ctx, cam_out, v, first=13):
    """The gradients of view v's four camera arguments (apply() slots first + 4 v ...): each in the shape, dtype and device the caller
    passed; None where none is needed."""
    grads = []
    for k in range(4):
        shape, dtype, device = ctx.cam_meta[4 * v + k]
        g = cam_out[k] if cam_out is not None else None
        need = ctx.needs_input_grad[first + 4 * v + k]
        grads.append(g.reshape(shape).to(dtype=dtype, device=device) if (need and g is not None) else None)
    return grads


class _RasterizeGaussians(torch.autograd.Function):
    """One view over the ctypes binding: forward -> (color, radii, depth[, alpha]); backward -> grads for the 8 tensor inputs, None for
    settings."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, differentiable_depth=False, return_alpha=False, antialiasing=False, camera_gradients=False, *camera):
        # grad_depth is ignored unless differentiable_depth: do not let autograd fill a zero image for it (or for an unused colour / alpha)
        ctx.set_materialize_grads(False)
        ctx.depth = bool(differentiable_depth)
        ctx.alpha = bool(return_alpha)
        # camera_gradients: `camera` = (bg, viewmatrix, projmatrix, campos) of raster_settings, the trailing apply() arguments
        ctx.camera = bool(camera_gradients)
        ctx.cam_meta = [(t.shape, t.dtype, t.device) for t in camera]
        m3 = _prep(means3D)
        if m3 is None:
            if means3D is not None and means3D.dim() == 2 and means3D.shape[1] == 3:
                # P = 0: zero-filled outputs without launching anything
                dev = means3D.device
                H, W = int(raster_settings.image_height), int(raster_settings.image_width)
                ctx.empty = True
                if ctx.camera:    # the backward's dL/dbg needs the settings (nothing was blended: the sum of dL/dC)
                    ctx.state = _hip.empty_state(raster_settings, dev)
                return (torch.zeros((3, H, W), device=dev), torch.zeros((0,), dtype=torch.int32, device=dev),
                        torch.zeros((1, H, W), device=dev)) + ((torch.zeros((1, H, W), device=dev),) if ctx.alpha else ())
            raise RuntimeError("means3D must have dimensions (num_points, 3)")
        if m3.dim() != 2 or m3.shape[1] != 3:
            raise RuntimeError("means3D must have dimensions (num_points, 3)")
        ctx.empty = False
        sh_, col_, op_ = _prep(sh), _prep(colors_precomp), _prep(opacities)
        sc_, rot_, cov_ = _prep(scales), _prep(rotations), _prep(cov3Ds_precomp)
        # (the state's settings carry the anti-aliasing bit: the backward takes it from there)
        color, radii, depth, state = _hip.rasterize_forward(raster_settings, m3, op_, col_, sh_, sc_, rot_, cov_,
                                                            **({"antialiasing": True} if antialiasing else {}))
        ctx.state = state
        _save_inputs(ctx, m3, radii, col_, sh_, sc_, rot_, cov_)
        if ctx.alpha:
            return color, radii, depth, _hip.rendered_alpha([state])[0]
        return color, radii, depth

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha=None):
        # grad_radii: accepted, ignored; grad_depth: used with differentiable_depth; grad_alpha: used whenever autograd delivers one
        want = tuple(ctx.needs_input_grad[13 + k] for k in range(4)) if ctx.camera else None
        if want is not None and not any(want):
            want = None
        cam = {} if want is None else {"camera_grads": want}
        if ctx.empty:
            if want is None:
                return (None,) * (13 + len(ctx.cam_meta))
            H, W = ctx.state.H, ctx.state.W
            g = grad_color if grad_color is not None else torch.zeros((3, H, W), device=ctx.state.keep[0].device)
            cam_out = _hip.rasterize_backward(ctx.state, g, ctx.state.keep[0].new_empty((0, 3)), None, None, None, None, None, None,
                                              **cam)[8]
            return (None,) * 13 + tuple(_camera_grads(ctx, cam_out, 0))
        m3, radii, col_, sh_, sc_, rot_, cov_ = ctx.saved_tensors
        has_sh, has_col, has_sc, has_cov = ctx.has
        if grad_color is None:
            grad_color = torch.zeros((3, ctx.state.H, ctx.state.W), device=m3.device)
        r = _hip.rasterize_backward(
            ctx.state, grad_color, m3, radii, col_ if has_col else None, sh_ if has_sh else None,
            sc_ if has_sc else None, rot_ if has_sc else None, cov_ if has_cov else None,
            want_color_grad=bool(has_col and ctx.needs_input_grad[3]),
            **({"grad_depth": grad_depth} if (ctx.depth and grad_depth is not None) else {}),
            **({} if grad_alpha is None else {"grad_alpha": grad_alpha}), **cam)
        d_means3D, d_means2D, d_colors, d_opacity, d_scales, d_rot, d_cov, d_sh = r[:8]
        return _input_grads(ctx, d_means3D, d_means2D, d_sh, d_colors, d_opacity, d_scales, d_rot, d_cov) + \
            tuple(_camera_grads(ctx, r[8] if want is not None else None, 0) if ctx.camera else ())


class _RasterizeGaussiansViews(torch.autograd.Function):
    """V views of the same Gaussians in one call (extension of the reference API, which renders one view
    per call): forward -> (color[V,3,H,W], radii[V,P], depth[V,1,H,W][, alpha[V,1,H,W]]); backward sums the per-view input
    gradients.  ``means2D`` is a [V,P,3] holder so each view's screen-space gradient stays separate
    (densification accumulates their norms per view, /root/reference/src/tracking/external.py:138-142)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings_list,
                differentiable_depth=False, return_alpha=False, antialiasing=False, camera_gradients=False, batched_sh=False, *camera):
        ctx.set_materialize_grads(False)
        ctx.depth = bool(differentiable_depth)
        ctx.alpha = bool(return_alpha)
        # camera_gradients: `camera` = (bg, viewmatrix, projmatrix, campos) of every view in turn, the trailing apply() arguments
        # (slots 14 ...: batched_sh sits between the switch and them)
        ctx.camera = bool(camera_gradients)
        ctx.cam_meta = [(t.shape, t.dtype, t.device) for t in camera]
        m3 = _prep(means3D)
        if m3 is None or m3.dim() != 2 or m3.shape[1] != 3:
            raise RuntimeError("means3D must have dimensions (num_points, 3)")
        sh_, col_, op_ = _prep(sh), _prep(colors_precomp), _prep(opacities)
        sc_, rot_, cov_ = _prep(scales), _prep(rotations), _prep(cov3Ds_precomp)
        wants_grad = any(ctx.needs_input_grad)
        color, radii, depth, states = _hip.rasterize_forward_batch(list(settings_list), m3, op_, col_, sh_, sc_, rot_, cov_,
                                                                   prepare_backward=wants_grad, **({} if wants_grad else {"forward_only": True}),
                                                                   **({"depth_scratch": True} if (ctx.depth and wants_grad) else {}),
                                                                   **({"antialiasing": True} if antialiasing else {}),
                                                                   # (the batch camera pass has no SH term for campos: per view then)
                                                                   **({"batched_sh": True} if (batched_sh and sh_ is not None and not camera_gradients) else {}))
        ctx.states = states
        _save_inputs(ctx, m3, radii, col_, sh_, sc_, rot_, cov_)
        if ctx.alpha:
            return color, radii, depth, _hip.rendered_alpha(states)
        return color, radii, depth

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha=None):
        m3, radii, col_, sh_, sc_, rot_, cov_ = ctx.saved_tensors
        has_sh, has_col, has_sc, has_cov = ctx.has
        V = len(ctx.states)
        if grad_color is None:
            grad_color = torch.zeros((V, 3, ctx.states[0].H, ctx.states[0].W), device=m3.device)
        want = None
        if ctx.camera:     # one flag per settings field: any view's tensor of that field needs a gradient
            want = tuple(any(ctx.needs_input_grad[14 + 4 * v + k] for v in range(V)) for k in range(4))
            if not any(want):
                want = None
        r = _hip.rasterize_backward_batch(
            ctx.states, grad_color, m3, radii, col_ if has_col else None, sh_ if has_sh else None,
            sc_ if has_sc else None, rot_ if has_sc else None, cov_ if has_cov else None,
            want_color_grad=bool(has_col and ctx.needs_input_grad[3]),
            **({"grad_depth": grad_depth} if (ctx.depth and grad_depth is not None) else {}),
            **({"grad_alpha": grad_alpha} if grad_alpha is not None else {}),
            **({} if want is None else {"camera_grads": want}))
        d3, d2, dc, do, ds, dr, dcov, dsh = r[:8]
        cam = []
        for v in range(len(ctx.cam_meta) // 4):
            cam += _camera_grads(ctx, r[8][v] if want is not None else None, v, 14)
        # gradients arrive already summed over views (means2D stays per view); the state stays on ctx so that a
        # second backward (retain_graph=True) works, and is released with the graph
        return _input_grads(ctx, d3, d2, dsh, dc, do, ds, dr, dcov) + (None,) + tuple(cam)


def rasterize_gaussians_views(settings_list, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                              rotations=None, cov3D_precomp=None, differentiable_depth=False, return_alpha=False, antialiasing=False,
                              camera_gradients=False, batched_sh=False):
    """Render ``len(settings_list)`` views of one set of Gaussians.  ``means2D``: [V,P,3] gradient holder.
    ``differentiable_depth``: the depth output [V,1,H,W] is differentiated too (see GaussianRasterizer); views that share a camera,
    which the backward otherwise fuses into one pass, are then differentiated unfused.
    ``return_alpha``: a fourth output, the rendered alpha [V,1,H,W] = 1 - final_T, always differentiable (see GaussianRasterizer); views
    that share a camera stay fused.  A view's ``means2D`` gradient then includes its own alpha term: a caller that wants a colour-only
    densification statistic must render alpha with a separate call (its own means2D holder).
    ``antialiasing``: every view is rendered with the opacity compensation (see GaussianRasterizer).
    ``camera_gradients``: every view's bg, viewmatrix, projmatrix and campos get their gradients (see GaussianRasterizer); views that
    share a camera, which the backward otherwise fuses into one pass, are then differentiated unfused.
    ``batched_sh`` (with ``shs``; a performance switch, not a semantic one): the views take the batch path that precomputed colours
    take -- one launch per stage for all views, one host sync -- and one SH pass sums dL/dsh over the views, instead of one single-view
    forward and backward per view and a stack-and-sum of V gradient sets.  The forward outputs are the per-view path's bit for bit; the
    gradients agree with it to fp32 rounding (the multi-view per-Gaussian kernel sums in another order).  Where the batch cannot serve,
    the per-view path runs silently: today that is ``camera_gradients=True`` (the batch camera pass has no SH term for campos).
    Ignored with precomputed colours."""
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    empty = torch.Tensor([])
    settings_list = tuple(settings_list)
    V = len(settings_list)
    if V == 0:
        raise ValueError("rasterize_gaussians_views: no views")
    per_view_col = colors_precomp is not None and colors_precomp.dim() == 3

    def call(lo, hi):
        whole = lo == 0 and hi == V          # no slice nodes in the graph (their backward is a zero-fill + copy each)
        return _RasterizeGaussiansViews.apply(
            means3D, means2D if whole else means2D[lo:hi], empty if shs is None else shs,
            empty if colors_precomp is None else (colors_precomp[lo:hi] if (per_view_col and not whole) else colors_precomp), opacities,
            empty if scales is None else scales, empty if rotations is None else rotations,
            empty if cov3D_precomp is None else cov3D_precomp, settings_list[lo:hi], bool(differentiable_depth), bool(return_alpha),
            bool(antialiasing), bool(camera_gradients), bool(batched_sh),
            *(_camera_tensors(settings_list[lo:hi]) if camera_gradients else ()))
    if V <= _hip.MAX_BATCH:
        return call(0, V)
    # more views than one library call takes: several calls, outputs concatenated (autograd sums the shared inputs)
    parts = [call(lo, min(V, lo + _hip.MAX_BATCH)) for lo in range(0, V, _hip.MAX_BATCH)]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(len(parts[0])))


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, differentiable_depth=False, return_alpha=False, antialiasing=False, camera_gradients=False):
    """One view (upstream's entry point).  ``return_alpha``: a fourth output, the rendered alpha [1,H,W] (see GaussianRasterizer).
    ``antialiasing``: the opacity compensation (see GaussianRasterizer).  ``camera_gradients``: gradients for the settings' bg,
    viewmatrix, projmatrix and campos (see GaussianRasterizer)."""
    native = _native() if (means3D is not None and means3D.is_cuda) else None
    if native is not None and not _PY_NODE:
        # one crossing into the torch C++ layer: forward and the autograd node live there (csrc/gsr_torch.cpp: RasterizeFn)
        rs = raster_settings
        return native.rasterize(layer_state(means3D.device), means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs.bg, rs.viewmatrix,
                                rs.projmatrix, rs.campos, float(rs.tanfovx), float(rs.tanfovy), int(rs.image_height), int(rs.image_width),
                                float(rs.scale_modifier), int(rs.sh_degree), bool(rs.prefiltered),
                                differentiable_depth=bool(differentiable_depth), return_alpha=bool(return_alpha),
                                antialiasing=bool(antialiasing), camera_gradients=bool(camera_gradients))
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, bool(differentiable_depth), bool(return_alpha), bool(antialiasing),
                                     bool(camera_gradients), *(_camera_tensors([raster_settings]) if camera_gradients else ()))


class GaussianRasterizer(nn.Module):
    """Constructed per call by the reference (``Renderer(raster_settings=cam)(**rendervar)``,
    /root/reference/src/tracking/train_utils.py:178): construction does no work.

    ``differentiable_depth`` (extension, default False): the depth output is differentiated too.  D = sum_i alpha_i T_i z_i (z_i: the
    Gaussian's view-space depth, no background term) is treated as a fourth colour channel with colour z_i and background 0, plus
    z_i -> means3D; the depth term reaches every input gradient through dL/dalpha.  False: the depth gradient is ignored, as upstream.

    ``return_alpha`` (extension, default False): forward returns a fourth tensor, the rendered alpha [1,H,W] = 1 - final_T (the forward's
    own transmittance after the last blended entry; 0 where nothing was blended) -- the mask the reference renders a second time with
    colours = 1 on black.  It is always differentiable: its gradient reaches means2D, opacities, the covariance (scales / rotations or
    cov3D_precomp) and means3D, never the colours or SHs.  ``means2D.grad`` then includes the alpha term, as autograd requires: a caller
    that wants a colour-only densification statistic must render alpha with a separate call (its own means2D holder).  False: upstream's
    three outputs.

    ``antialiasing`` (extension, default False; upstream's ``antialiasing`` rasterizer setting, Mip-Splatting's 2D filter): each Gaussian's
    opacity is scaled by c = sqrt(max(det0 / det1, 2.5e-5)), det0 / det1 the determinants of its screen-space covariance before / after
    the fixed 0.3 px^2 dilation, so a Gaussian smaller than a pixel keeps the energy of its undilated footprint instead of being drawn too
    fat and too bright.  The opacity gradient is dL/do = c dL/d(o c), and the term through c reaches the covariance (scales / rotations or
    cov3D_precomp) and means3D.  Conic, radii, depth and the tile rects are unchanged.  Combines with ``differentiable_depth`` and
    ``return_alpha``.  False: every output and gradient is bit for bit the plain render's.  

    ``camera_gradients`` (extension, default False): the settings' ``bg``, ``viewmatrix``, ``projmatrix`` and ``campos`` are
    differentiated too, each gradient in the shape the caller passed (a [1,4,4] transposed view included), for pose refinement or camera
    tracking against a frozen scene.  viewmatrix[3, 7, 11, 15] and projmatrix[2, 6, 10, 14] (column-major as stored) are never read by the
    forward and get 0; campos reaches the render only through the SH view direction and gets 0 with precomputed colours.  ``tanfovx`` /
    ``tanfovy`` are Python floats: no focal-length or field-of-view gradient is provided, although J depends on them.  Combines with the
    three switches above.  False: a camera tensor that requires a gradient gets None, as upstream, and every output and gradient is bit
    for bit the plain render's.  """

    def __init__(self, raster_settings: GaussianRasterizationSettings, differentiable_depth: bool = False, return_alpha: bool = False,
                 antialiasing: bool = False, camera_gradients: bool = False):
        super().__init__()
        self.raster_settings = raster_settings
        self.differentiable_depth = bool(differentiable_depth)
        self.return_alpha = bool(return_alpha)
        self.antialiasing = bool(antialiasing)
        self.camera_gradients = bool(camera_gradients)

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            native = _native() if positions.is_cuda else None
            if native is not None:
                return native.mark_visible(positions, self.raster_settings.viewmatrix, self.raster_settings.projmatrix)
            return _hip.mark_visible(positions, self.raster_settings.viewmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        empty = torch.Tensor([])
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, rs, differentiable_depth=self.differentiable_depth, return_alpha=self.return_alpha,
                                   antialiasing=self.antialiasing, camera_gradients=self.camera_gradients)
