"""The image-loss kernels (gsr_loss.hip: the fused L1 + SSIM forward in its three builds, its backward, the two finishing kernels), each
against the plain fp64 reference of tests/loss_ref.py at the shapes chosen against the kernels' geometry -- a 32 x 54 output tile with a
halo of 5, 8 row segments of 7, workgroups permuted over 8 slots, finishing sums with loop boundaries at 64 / 192 / 256 partials and
16 waves, a view table of at most 32 images x 4 channels, plain batches chunked by 32 channels.

Bounds (none taken from the kernels): values 1e-5 relative (test_fused_image_loss_matches_torch_formula) or the soak's 2e-5 |ref| + 1e-7
(test_random_shapes_of_the_fused_image_loss), whichever is wider for the value at hand; gradients and moments TOL = 1e-4 of the
per-image maximum, POINTWISE.  Only the ill-conditioned contents of group H may go to the referee rule of test_bwd_chain_edges_gpu._referee
(HIP no further from fp64 than twice the fp32 CPU evaluation of the same statements + 2e-5), at most three of them (the last test counts);
tests/test_loss_ref_cpu.py shows that the fp32 evaluation meets the plain bounds on every other case.  Margins go to
loss_kernels_parity.txt next to hipcheck's row-margin log."""
import os

import numpy as np
import pytest
import torch

import loss_ref as R
from hipcheck import _ROW_LOG, TOL

pytestmark = pytest.mark.gpu
_LOG = os.path.join(os.path.dirname(_ROW_LOG), "loss_kernels_parity.txt")
_REFEREED = []
UP = 0.7             # upstream gradient of the total


def _log(line):
    try:
        os.makedirs(os.path.dirname(_LOG), exist_ok=True)
        with open(_LOG, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass
    if os.environ.get("GSR_TEST_VERBOSE"):
        print(line)


@pytest.fixture(autouse=True)
def _fresh_target_cache():
    """No test depends on another's cached target moments."""
    from diff_gaussian_rasterization import _hip
    _hip._target_moments.clear()
    yield
    _hip._target_moments.clear()


class _Builds:
    """Records, per views-loss call, whether the table carried cached target moments (MODE 1) or not (MODE 0)."""

    def __enter__(self):
        from diff_gaussian_rasterization import _hip
        self.hip, self.orig, self.seen = _hip, _hip._loss_table, []

        def spy(*a, **k):
            self.seen.append((a[4] if len(a) > 4 else k.get("moments")) is not None)
            return self.orig(*a, **k)
        _hip._loss_table = spy
        return self

    def __exit__(self, *exc):
        self.hip._loss_table = self.orig
        return False


def _device_scene(s, dev):
    d = dict(s)
    d["targets"] = [t.to(dev) for t in s["targets"]]
    return d


def _run_views(dev, s, upstream=UP, w_l1=R.W_L1, w_ssim=R.W_SSIM, cam_grads=True):
    """One views_image_loss call + backward on the device.  ``s['targets']`` must already live there (the cache is keyed on the objects)."""
    from gsdyn import losses as L
    r = s["renders"].to(dev).requires_grad_(True)
    m, c = s["cam_m"].to(dev).requires_grad_(cam_grads), s["cam_c"].to(dev).requires_grad_(cam_grads)
    total, per = L.views_image_loss(r, s["targets"], s["rows"], s["weights"], m, c, w_l1, w_ssim)
    leaves = (r, m, c) if cam_grads else (r,)
    g = torch.autograd.grad(total * upstream, leaves, allow_unused=True)
    g = [torch.zeros_like(l) if x is None else x for x, l in zip(g, leaves)]
    out = dict(total=total.detach(), per=per.detach(), d_renders=g[0])
    out["d_cam_m"], out["d_cam_c"] = (g[1], g[2]) if cam_grads else (None, None)
    return out


def _same_bits(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


def _items(got, ref, grad_scale=None, cam_scale=None):
    """Every comparison of one result as (name, error, bound, denominator): values as absolute errors against the wider of the two
    existing value bounds, gradients as max error / max |fp64 gradient| (of the renders: per image, i.e. pointwise) against TOL."""
    items = []
    vals = [("total", float(got["total"]), float(ref["total"]))] + [(f"per[{i}]", float(a), float(b)) for i, (a, b) in enumerate(zip(got["per"], ref["per"]))]
    for name, a, b in vals:
        items.append((name, abs(a - b), max(1e-5 * abs(b), 2e-5 * abs(b) + 1e-7), abs(b)))
    d, dr = got["d_renders"].detach().cpu().double(), ref["d_renders"]
    assert d.shape == dr.shape
    for i in range(d.shape[0]):
        scale = float(dr[i].abs().max()) if grad_scale is None else grad_scale
        e = float((d[i] - dr[i]).abs().max())
        if scale == 0.0:                                           # weight 0: the gradient is exactly 0
            assert e == 0.0, f"d_renders[{i}]: the fp64 gradient is exactly 0"
            continue
        q = np.unravel_index(int((d[i] - dr[i]).abs().argmax()), tuple(d[i].shape))
        items.append((f"d_renders[{i}] worst at {tuple(int(v) for v in q)}", e / scale, TOL, 1.0))
    for k in ("d_cam_m", "d_cam_c"):
        if got[k] is None:
            continue
        a, b = got[k].detach().cpu().double(), ref[k]
        assert a.shape == b.shape, k
        used = b.abs().amax(dim=1) > 0
        if cam_scale is None and bool((~used).any()):
            assert float(a[~used].abs().max()) == 0.0, f"{k}: a camera row that no image uses has a gradient"
        if cam_scale is not None:
            items.append((k, float((a - b).abs().max()) / cam_scale, TOL, 1.0))
        elif bool(used.any()):
            items.append((k, float((a - b).abs().max()) / float(b.abs().max()), TOL, 1.0))
    return items


def _worst(items):
    return max((e / bd for n, e, bd, _ in items if n == "total" or n.startswith("per[")), default=0.0), \
        max((e / bd for n, e, bd, _ in items if not (n == "total" or n.startswith("per["))), default=0.0)


def _check(tag, got, ref, grad_scale=None):
    items = _items(got, ref, grad_scale)
    ev, eg = _worst(items)
    _log(f"{tag}: value {ev:.3f} of its bound, gradient {eg:.3f} of TOL")
    missed = [(n, f"{e:.3e} > {bd:.3e}") for n, e, bd, _ in items if e > bd]
    assert not missed, (tag, missed)


# ------------------------------------------------------------------------------------------------------- A: tile and halo edges
@pytest.mark.parametrize("H,W", R.EDGE_SHAPES)
def test_tile_and_halo_edges(dev, H, W):
    """Every H x W around the tile, the halo and the window: the 5-moment build, the cached 3-moment build (bit-identical) and the plain
    batch path, all pointwise against fp64."""
    from gsdyn import losses as L
    s = _device_scene(R.views_scene(H, W), dev)
    ref = R.reference_of(s, upstream=UP)
    with _Builds() as b:
        first, second = _run_views(dev, s), _run_views(dev, s)
    assert b.seen == [False, True]                      # MODE 0, then MODE 1 on the same target objects
    _check(f"A/{H}x{W}/views", first, ref)
    assert _same_bits(first, second), f"A/{H}x{W}: the cached-moments build differs from the five-moment build"
    x = s["renders"][1:2].to(dev).requires_grad_(True)  # the plain path: image 1 (no camera row) as a batch of one
    lb = L.image_loss(x, s["targets"][1][None])
    (g,) = torch.autograd.grad(lb[0] * (UP * s["weights"][1]), x)
    plain = dict(total=lb[0].detach() * s["weights"][1], per=lb.detach(), d_renders=g, d_cam_m=None, d_cam_c=None)
    pref = dict(total=ref["per"][1] * s["weights"][1], per=ref["per"][1:2], d_renders=ref["d_renders"][1:2])
    _check(f"A/{H}x{W}/plain", plain, pref)


# ------------------------------------------------------------------------------------------------- B: target moments against fp64
@pytest.mark.parametrize("H,W", R.EDGE_SHAPES)
def test_target_moments_against_fp64(dev, H, W):
    """blur(y), blur(y*y) of the target-moments build, pointwise, with 1 to 4 channels."""
    from diff_gaussian_rasterization import _hip
    from gsdyn.losses import _window_1d
    y4 = R.noise_ramp(np.random.default_rng([H, W, 4]), 1, 4, H, W)[0]
    B, D = R.target_moments(y4)
    win = _hip._window(_window_1d())
    worst = 0.0
    for c in range(1, 5):
        _hip._target_moments.clear()
        t = y4[:c].contiguous().to(dev)
        with _hip._on(dev):
            img0, m0 = _hip._moments_of(win, t)
            img1, m1 = _hip._moments_of(win, t)
        assert m0 is None and img0 is t and img1 is t and tuple(m1.shape) == (2, c, H, W)
        got = m1.cpu().double()
        for name, a, b in (("blur(y)", got[0], B[:c]), ("blur(y*y)", got[1], D[:c])):
            for p in range(c):
                e = float((a[p] - b[p]).abs().max()) / float(b[p].abs().max())
                worst = max(worst, e)
                assert e <= TOL, (f"B/{H}x{W}/c{c}", name, p, e)
    _log(f"B/{H}x{W}: moments {worst / TOL:.3f} of TOL")


# ------------------------------------------------------------------------------------------------------------------ C: slot map
@pytest.mark.parametrize("N", sorted(R.SLOT_CASES))
def test_workgroup_slot_map(dev, N):
    """tiles x planes below, at and above the 8 slots and not a multiple of 8; every plane distinct, so a tile computed for another plane
    or written to another partial slot changes a per-image loss."""
    s = _device_scene(R.slot_scene(N), dev)
    ref = R.reference_of(s, upstream=UP)
    first, second = _run_views(dev, s), _run_views(dev, s)
    _check(f"C/N{N}", first, ref)
    assert _same_bits(first, second)


# ------------------------------------------------------------------------------------------------------------ D: finishing sums
@pytest.mark.parametrize("k,C", [(k, 1) for k in R.FINISH_K1] + [(k, 3) for k in R.FINISH_K3])
def test_finishing_sums(dev, k, C):
    """k partials per channel (backward) and k * C per image (forward) around the strided sum's loop boundaries."""
    s = _device_scene(R.finish_scene(k, C), dev)
    _check(f"D/k{k}-c{C}", _run_views(dev, s), R.reference_of(s, upstream=UP))


# --------------------------------------------------------------------------------------------------------- E: view-table shapes
@pytest.mark.parametrize("name", sorted(R.table_cases()))
def test_view_tables(dev, name):
    """Image counts around the 16 waves of the finishing kernels, the full 32 x 4 table, one shared camera row, descending rows, no
    rows; mixed-sign and zero weights, a negative upstream gradient; an unused camera row keeps gradient exactly 0 (_errors)."""
    s = _device_scene(R.table_scene(name), dev)
    ref = R.reference_of(s, upstream=-UP)
    got = _run_views(dev, s, upstream=-UP)
    _check(f"E/{name}", got, ref)
    if name == "no-rows":
        assert float(got["d_cam_m"].abs().max()) == 0.0 and float(got["d_cam_c"].abs().max()) == 0.0


def test_view_table_without_camera_gradients(dev):
    """cam_m / cam_c given but only the renders require grad: no finishing kernel, same render gradients."""
    s = _device_scene(R.table_scene("n17"), dev)
    ref = R.reference_of(s, upstream=UP)
    got = _run_views(dev, s, cam_grads=False)
    assert got["d_cam_m"] is None
    _check("E/no-cam-grads", got, ref)
    assert torch.equal(got["d_renders"], _run_views(dev, s)["d_renders"])


def test_view_table_limits_raise(dev):
    """5 channels, or 33 images, handed straight to the library call: an error, not a launch."""
    from diff_gaussian_rasterization import _hip
    from gsdyn.losses import _window_1d
    for n, C in ((2, 5), (33, 3)):
        renders = torch.rand(n, C, 12, 9, device=dev)
        targets = [torch.rand(C, 12, 9, device=dev) for _ in range(n)]
        with pytest.raises(RuntimeError):
            _hip.views_loss_forward(_window_1d(), renders, targets, [-1] * n, [1.0] * n, None, None, 0.8, 0.2)
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------- F: plain batch chunks
@pytest.mark.parametrize("N,C", R.BATCH_CASES)
def test_plain_batch_chunks(dev, N, C):
    """image_loss on [N, C, 12, 9] with N * C above 32: the chunk boundary inside an image (and at an image edge), distinct upstream
    gradients per image."""
    from gsdyn import losses as L
    s = R.batch_scene(N, C)
    ref = R.reference_of(s, upstream=1.0)
    x = s["renders"].to(dev).requires_grad_(True)
    lb = L.image_loss(x, torch.stack(s["targets"]).to(dev))
    ups = torch.tensor(s["weights"], device=dev)
    total = (lb * ups).sum()
    (g,) = torch.autograd.grad(total, x)
    _check(f"F/{N}x{C}", dict(total=total.detach(), per=lb.detach(), d_renders=g, d_cam_m=None, d_cam_c=None), ref)


# ---------------------------------------------------------------------------------------------------------------- G: L1 ties
@pytest.mark.parametrize("affine", [False, True])
def test_l1_ties_and_sign(dev, affine):
    """pred == target exactly on a checkerboard, above it elsewhere on the left, below on the right.  C * H * W is a power of two, so
    w_l1 * sign / N is the same fp32 number in whichever order it is formed."""
    render, target, tie = R.tie_scene()
    C = render.shape[1]
    s = dict(renders=render, targets=[target.to(dev)], rows=[0 if affine else -1], weights=[1.0], cam_m=torch.zeros(1, C), cam_c=torch.zeros(1, C))
    tag = f"G/{'affine0' if affine else 'row-1'}"
    got = _run_views(dev, s, upstream=1.0, w_l1=0.8, w_ssim=0.0)
    r32 = R.reference_of(s, upstream=1.0, dtype=torch.float32, w_l1=0.8, w_ssim=0.0)
    d = got["d_renders"][0].cpu()
    assert bool((d[tie] == 0).all()), f"{tag}: a tied pixel has an L1 gradient"
    assert torch.equal(d.double(), r32["d_renders"][0]), f"{tag}: L1 gradient differs from w_l1 * sign / N"
    _check(f"{tag}/l1-only", got, R.reference_of(s, upstream=1.0, w_l1=0.8, w_ssim=0.0))
    for w_l1, w_ssim in ((0.8, 0.2), (0.0, 1.0)):
        _check(f"{tag}/w{w_l1}-{w_ssim}", _run_views(dev, s, w_l1=w_l1, w_ssim=w_ssim), R.reference_of(s, upstream=UP, w_l1=w_l1, w_ssim=w_ssim))


# ------------------------------------------------------------------------------------------------- H: ill-conditioned content
@pytest.mark.parametrize("kind", R.ILL_KINDS)
def test_ill_conditioned_content(dev, kind):
    """Flat images (variance is a cancellation) and a camera gain that takes pred outside [0, 1] (C - A*A cancels).  The only group that
    may use the referee rule.  Where x == y the fp64 gradient is ~0: the error is measured against one pixel's L1 gradient instead."""
    renders, target, m, c = R.ill_scene(kind)
    C, H, W = target.shape
    s = dict(renders=renders, targets=[target.to(dev)], rows=[0], weights=[1.0], cam_m=m, cam_c=c)
    ref = R.reference_of(s, upstream=UP)
    got = _run_views(dev, s)
    # x == y: one pixel's L1 gradient for the renders, a channel's H * W of them for its camera row
    scale = UP * R.l1_pixel_scale(R.W_L1, C, H, W) if kind == "flat-equal" else None
    cam_scale = scale * H * W if kind == "flat-equal" else None
    items = _items(got, ref, scale, cam_scale)
    ev, eg = _worst(items)
    _log(f"H/{kind}: value {ev:.3f} of its bound, gradient {eg:.3f} of TOL")
    if all(e <= bd for _, e, bd, _d in items):
        return
    r32 = R.reference_of(s, upstream=UP, dtype=torch.float32)
    yard = _items(r32, ref, scale, cam_scale)
    _REFEREED.append(kind)
    for (name, e, bd, dn), (name32, e32, _b, _d) in zip(items, yard):
        if e <= bd:
            continue
        assert dn > 0.0 and name.split()[0] == name32.split()[0], (kind, name)
        _log(f"H/{kind}: REFEREE {name}: HIP {e / dn:.2e} / fp32 CPU {e32 / dn:.2e} from fp64")
        assert e / dn <= 2.0 * (e32 / dn) + 2e-5, (kind, name, e / dn, e32 / dn)


# ------------------------------------------------------------------------------- I: existing properties on the ragged shapes
@pytest.mark.parametrize("H,W", [(55, 37), (109, 65)])
def test_determinism_and_converted_targets(dev, H, W):
    """A third evaluation (cached moments both times) gives the same bits; the loader's ``permute(2, 0, 1) / 255`` target -- not
    contiguous -- and its fp16 form give the result of their contiguous fp32 copies."""
    s = _device_scene(R.views_scene(H, W, n=3, rows=[1, -1, 1]), dev)
    outs = [_run_views(dev, s) for _ in range(3)]
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[1], outs[2])
    rng = np.random.default_rng([H, W, 9])
    hwc = [torch.tensor(rng.integers(0, 256, (H, W, 3)).astype(np.uint8), device=dev) for _ in range(3)]
    for conv in (lambda t: t.permute(2, 0, 1) / 255, lambda t: (t.permute(2, 0, 1) / 255).half()):
        views = [conv(t) for t in hwc]
        assert not views[0].is_contiguous()
        loader = dict(s, targets=views)
        copies = dict(s, targets=[v.contiguous().float() for v in views])
        a1, a2, b1 = _run_views(dev, loader), _run_views(dev, loader), _run_views(dev, copies)
        assert _same_bits(a1, b1) and _same_bits(a1, a2)
        _check(f"I/{H}x{W}/{views[0].dtype}", a1, R.reference_of(copies, upstream=UP))


def test_referee_use(dev):
    """At most three cases of group H went to the referee rule (runs last in this file)."""
    _log(f"referee: {len(_REFEREED)} case(s): {', '.join(_REFEREED) or 'none'}")
    assert len(_REFEREED) <= 3, _REFEREED
