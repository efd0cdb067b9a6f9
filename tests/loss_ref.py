"""Plain reference of the fused image terms (gsr_loss.hip) and the scenes its GPU tests run.

    loss_i = w_l1 * mean|pred_i - y_i| + w_ssim * (1 - mean SSIM(pred_i, y_i)),   total = sum_i weight_i * loss_i,
    pred_i = exp(cam_m[row_i]) * render_i + cam_c[row_i]   (row_i < 0: pred_i = render_i)

written with none of the package's own loss code: the 11 x 11 Gaussian window is applied as an explicit zero-padded separable
correlation -- eleven shifted slices along the rows, eleven along the columns -- in torch on the CPU, so autograd supplies every
gradient; |.| has torch's sign(0) = 0.  Only the eleven window values come from gsdyn.losses._window_1d(): they are the kernel's input,
not its arithmetic.  tests/test_loss_ref_cpu.py pins this file against calc_ssim / l1_loss_v1, the stored vectors of the imported
reference and a brute-force 2-D window sum.  dtype=torch.float32 runs the very same statements in fp32: the yardstick of the referee
rule (HIP no further from fp64 than twice that + 2e-5)."""
import itertools
import math

import numpy as np
import torch

C1, C2 = 0.01 ** 2, 0.03 ** 2
W_L1, W_SSIM = 0.8, 0.2

# ---- the kernel's geometry, which the shape lists below are chosen against: a 32 x 54 output tile, halo 5, 8 row segments of 7
TILE_W, TILE_H, HALO = 32, 54, 5
EDGE_H = (1, 5, 6, 10, 11, 53, 54, 55, 59, 60, 107, 108, 109)
EDGE_W = (1, 5, 6, 27, 31, 32, 33, 37, 38, 63, 64, 65)
EDGE_SHAPES = tuple(itertools.product(EDGE_H, EDGE_W))
FINISH_K1 = (1, 2, 63, 64, 65, 192, 193, 256, 257, 449, 513)     # tiles per plane at H = 3, W = 32 k - 5, one channel
FINISH_K3 = (64, 65, 86)                                          # ... again with three channels: 192 / 195 / 258 partials per image


def window(dtype=torch.float64):
    from gsdyn.losses import _window_1d
    return torch.tensor(_window_1d(), dtype=dtype)


def blur(t, win=None):
    """Zero-padded 11-tap correlation along the last axis, then along the one before it."""
    g = window(t.dtype) if win is None else win
    H, W = t.shape[-2:]
    p = torch.zeros(t.shape[:-2] + (H + 2 * HALO, W + 2 * HALO), dtype=t.dtype)
    p[..., HALO:HALO + H, HALO:HALO + W] = t
    h = sum(g[k] * p[..., :, k:k + W] for k in range(11))
    return sum(g[k] * h[..., k:k + H, :] for k in range(11))


def blur_brute(img):
    """The 2-D statement of the same window, one output pixel at a time (numpy fp64; [H, W] only, small images)."""
    g = window().numpy()
    H, W = img.shape
    out = np.zeros((H, W))
    for i in range(H):
        for j in range(W):
            s = 0.0
            for a in range(11):
                for b in range(11):
                    ii, jj = i + a - HALO, j + b - HALO
                    if 0 <= ii < H and 0 <= jj < W:
                        s += g[a] * g[b] * img[ii, jj]
            out[i, j] = s
    return out


def ssim_map(x, y):
    A, B = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - A * A, blur(y * y) - B * B, blur(x * y) - A * B
    return ((2 * A * B + C1) * (2 * sxy + C2)) / ((A * A + B * B + C1) * (sxx + syy + C2))


def image_term(pred, y, w_l1=W_L1, w_ssim=W_SSIM):
    """One image [C, H, W]."""
    return w_l1 * (pred - y).abs().mean() + w_ssim * (1.0 - ssim_map(pred, y).mean())


def target_moments(y, dtype=torch.float64):
    """blur(y), blur(y*y) of a target [C, H, W]: what the target-moments pass of the kernel stores."""
    y = y.detach().cpu().to(dtype)
    return blur(y), blur(y * y)


def views_reference(renders, targets, rows, weights, cam_m=None, cam_c=None, w_l1=W_L1, w_ssim=W_SSIM, upstream=1.0, dtype=torch.float64):
    """Everything the views path returns: dict(total, per [n], d_renders, d_cam_m, d_cam_c) for d(upstream * total).  The plain
    batch path is the same thing with rows -1 and the per-image upstream gradients as weights."""
    cv = lambda t: t.detach().cpu().to(dtype)   # noqa: E731
    r = cv(renders).requires_grad_(True)
    m = None if cam_m is None else cv(cam_m).requires_grad_(True)
    c = None if cam_c is None else cv(cam_c).requires_grad_(True)
    per = []
    for i, (t, row) in enumerate(zip(targets, rows)):
        pred = r[i] if row < 0 else torch.exp(m[row])[:, None, None] * r[i] + c[row][:, None, None]
        per.append(image_term(pred, cv(t), w_l1, w_ssim))
    total = sum(float(w) * l for w, l in zip(weights, per))
    leaves = [r] + ([m, c] if m is not None else [])
    g = torch.autograd.grad(total * float(upstream), leaves, allow_unused=True)
    g = [torch.zeros_like(l) if x is None else x for x, l in zip(g, leaves)]
    out = dict(total=total.detach().double(), per=torch.stack([l.detach() for l in per]).double(), d_renders=g[0].double())
    out["d_cam_m"], out["d_cam_c"] = (g[1].double(), g[2].double()) if m is not None else (None, None)
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def noise_ramp(rng, n, C, H, W, slope=(0.31, 0.17)):
    """Uniform noise plus a position ramp (different slopes along the rows and the columns, another offset per plane): a window that is
    shifted, transposed or taken from the wrong plane cannot cancel."""
    ii, jj = np.mgrid[0:H, 0:W]
    ramp = slope[0] * ii / max(H - 1, 1) + slope[1] * jj / max(W - 1, 1)
    off = 0.02 * np.arange(n * C).reshape(n, C, 1, 1)
    return torch.tensor((0.5 * rng.uniform(0, 1, (n, C, H, W)) + ramp[None, None] + off / max(n * C, 1)).astype(np.float32))


def views_scene(H, W, C=3, n=2, seed=0, rows=None, n_cams=None):
    """n renders / targets of noise_ramp content, camera rows (default: the first image on row 1 of 3, the rest -1), affines near 1."""
    rng = _rng(H, W, C, n, seed)
    rows = ([1] + [-1] * (n - 1)) if rows is None else list(rows)
    n_cams = max(3, max(rows) + 1) if n_cams is None else n_cams
    renders = noise_ramp(rng, n, C, H, W)
    targets = list(noise_ramp(rng, n, C, H, W, slope=(0.12, 0.35)).unbind(0))
    cam_m = torch.tensor(rng.uniform(-0.2, 0.2, (n_cams, C)).astype(np.float32))
    cam_c = torch.tensor(rng.uniform(-0.1, 0.1, (n_cams, C)).astype(np.float32))
    weights = [float(w) for w in rng.choice([50.0, 200.0, 1.0, 0.25], n)]
    return dict(renders=renders, targets=targets, rows=rows, weights=weights, cam_m=cam_m, cam_c=cam_c)


# tiles x planes of one launch = ceil(W/32) * ceil(H/54) * images * channels: below, at and above the 8 XCD slots, and not a multiple of 8
SLOT_CASES = {1: (12, 9, 1, 1), 7: (12, 9, 1, 7), 8: (55, 33, 1, 2), 9: (12, 9, 3, 3), 15: (12, 9, 3, 5), 16: (55, 33, 4, 1),
              17: (12, 9, 1, 17)}      # N -> (H, W, channels, images)


def tiles_times_planes(H, W, C, n):
    return ((W + TILE_W - 1) // TILE_W) * ((H + TILE_H - 1) // TILE_H) * C * n


# view tables at 12 x 9: name -> (n_images, channels, rows, n_cams)
def table_cases():
    mixed = lambda n: [-1 if i % 3 == 1 else (i * 5) % 4 for i in range(n)]   # noqa: E731
    cases = {f"n{n}": (n, 3, mixed(n), 5) for n in (1, 15, 16, 17, 31, 32)}
    cases["full-32x4"] = (32, 4, [i % 5 for i in range(32)], 5)          # sm / sc of the finishing kernel exactly full
    cases["one-row"] = (32, 3, [0] * 32, 2)
    cases["descending"] = (17, 3, [16 - i for i in range(17)], 17)
    cases["no-rows"] = (5, 3, [-1] * 5, 3)
    cases["c1"] = (17, 1, mixed(17), 5)
    cases["c2"] = (17, 2, mixed(17), 5)
    return cases


BATCH_CASES = ((10, 3), (11, 3), (21, 3), (22, 3), (33, 1), (3, 16))     # [N, C, 12, 9]: 30 / 33 / 63 / 66 / 33 / 48 channels, chunks of 32


def tie_scene(seed=0, H=64, W=64, C=2):
    """pred == target exactly on a checkerboard; on the other pixels pred is above the target in the left half, below in the right."""
    rng = _rng(seed, H, W)
    render = torch.tensor(rng.uniform(0.2, 0.8, (1, C, H, W)).astype(np.float32))
    ii, jj = np.mgrid[0:H, 0:W]
    tie = torch.tensor((ii + jj) % 2 == 0)[None].expand(C, H, W)
    delta = torch.tensor(rng.uniform(0.01, 0.1, (C, H, W)).astype(np.float32))
    sign = torch.where(torch.tensor(jj < W // 2), -1.0, 1.0)[None]       # target below pred on the left, above on the right
    target = torch.where(tie, render[0], render[0] + sign * delta)
    return render, target, tie


def ill_scene(kind, H=60, W=40, C=3, seed=0):
    """(renders [1,C,H,W], target, cam_m row, cam_c row) of the ill-conditioned contents; gain exp(1.5), offset -0.5 where named."""
    rng = _rng(seed, H, W, len(kind))
    flat = lambda v: torch.full((C, H, W), v, dtype=torch.float32)   # noqa: E731
    one, zero = torch.zeros(1, C), torch.zeros(1, C)
    gain, offs = torch.full((1, C), 1.5), torch.full((1, C), -0.5)
    if kind == "flat-equal":
        return flat(0.5)[None], flat(0.5), one, zero
    if kind == "flat-differ":
        return flat(0.3)[None], flat(0.7), one, zero
    if kind == "gain-smooth":
        return (flat(0.9) + 1e-3 * torch.tensor(rng.normal(size=(C, H, W)).astype(np.float32)))[None], flat(0.9), gain, offs
    if kind == "gain-random":
        return torch.tensor(rng.uniform(0, 1, (1, C, H, W)).astype(np.float32)), torch.tensor(rng.uniform(0, 1, (C, H, W)).astype(np.float32)), gain, offs
    if kind == "binary":
        return torch.tensor((rng.uniform(0, 1, (1, C, H, W)) < 0.5).astype(np.float32)), torch.tensor(rng.uniform(0, 1, (C, H, W)).astype(np.float32)), one, zero
    raise KeyError(kind)


ILL_KINDS = ("flat-equal", "flat-differ", "gain-smooth", "gain-random", "binary")


def l1_pixel_scale(w_l1, C, H, W):
    """The size of one non-tied pixel's L1 gradient: the scale of a gradient error where pred == target and the fp64 gradient is ~0."""
    return w_l1 / float(C * H * W)


def value_ok(got, want):
    """The two value bounds of tests/test_losses_step_gpu.py: 1e-5 relative (fixed shapes), or the soak's 2e-5 |ref| + 1e-7."""
    return abs(got - want) <= max(1e-5 * abs(want), 2e-5 * abs(want) + 1e-7)


def grad_err(got, want, scale=None):
    """max over the tensor of |got - want|, divided by max |want| (or ``scale``)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    s = float(want.abs().max()) if scale is None else float(scale)
    return float((got - want).abs().max()) / max(s, 1e-300)


assert all(tiles_times_planes(h, w, c, n) == k for k, (h, w, c, n) in SLOT_CASES.items()), "SLOT_CASES: counts do not match their keys"
assert math.isclose(sum(window().tolist()), 1.0, rel_tol=1e-6)


def finish_scene(k, C):
    """H = 3, W = 32 k - 5: k tiles per plane, two images, both with a camera row, so both finishing kernels run."""
    return views_scene(3, 32 * k - 5, C=C, n=2, rows=[0, 1], n_cams=2)


def slot_scene(N):
    H, W, C, n = SLOT_CASES[N]
    return views_scene(H, W, C=C, n=n, rows=[i % 2 if i % 3 else -1 for i in range(n)], n_cams=2)


def table_scene(name):
    n, C, rows, n_cams = table_cases()[name]
    s = views_scene(12, 9, C=C, n=n, rows=rows, n_cams=n_cams)
    s["weights"] = [(-1.0) ** i * (0.5 + 0.37 * i) if i % 7 else 0.0 for i in range(1, n + 1)]   # mixed signs, and zeros
    return s


def batch_scene(N, C):
    s = views_scene(12, 9, C=C, n=N, rows=[-1] * N)
    s["weights"] = [(-1.0) ** i * (0.5 + 0.37 * i) for i in range(N)]       # the per-image upstream gradients: all distinct
    return s


def random_cases():
    """(tag, scene builder) of every random-content case of tests/test_loss_kernels_gpu.py (groups A, C, D, E, F)."""
    out = [(f"A/{H}x{W}", (lambda H=H, W=W: views_scene(H, W))) for H, W in EDGE_SHAPES]
    out += [(f"C/N{N}", (lambda N=N: slot_scene(N))) for N in SLOT_CASES]
    out += [(f"D/k{k}-c{C}", (lambda k=k, C=C: finish_scene(k, C))) for C, ks in ((1, FINISH_K1), (3, FINISH_K3)) for k in ks]
    out += [(f"E/{name}", (lambda name=name: table_scene(name))) for name in table_cases()]
    out += [(f"F/{N}x{C}", (lambda N=N, C=C: batch_scene(N, C))) for N, C in BATCH_CASES]
    return out


def reference_of(scene, upstream=1.0, dtype=torch.float64, **kw):
    return views_reference(scene["renders"], scene["targets"], scene["rows"], scene["weights"], scene["cam_m"], scene["cam_c"],
                           upstream=upstream, dtype=dtype, **kw)
