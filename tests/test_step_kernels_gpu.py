"""The step-side kernels (gsr_rigidity.hip, gsr_step.hip) at every compiled variant and shape edge, each against a plain fp64
reference evaluated on the CPU (tests/step_ref.py): the neighbour terms at every lane-group size of the backward, both record
layouts, graph shapes that make empty / hub rows of the reverse adjacency, rest / coincident / underflowing states, the fused path's
flags and empty halves, the finishing sum's loop boundaries, the activations at saturation and overflow, the one-launch Adam at
every table shape, the radius bookkeeping.

Bars: term values 2e-5 relative + 1e-9; gradients TOL = 1e-4 of the tensor's maximum.  A gradient that misses TOL goes to the soak's
referee rule (test_soak_gpu._adjudicate): the same torch formulas in fp32 on the CPU, accepted if the HIP result is no further from fp64
than twice that + 2e-5 -- for at most 10 % of the cases (the last test counts them).  Margins are appended to step_kernels_parity.txt
next to hipcheck's row-margin log (profiles/step_kernels_parity.txt is one run of it)."""
import contextlib
import math
import os

import pytest
import torch

from hipcheck import _ROW_LOG, TOL, _margin
from step_ref import (BUILD_CASES, GRAPH_CASES, STATE_CASES, WEIGHTS5, WTS3, adam_reference, build_scene, lipschitz_row_bounds,
                      neighbour_reference, rel_max, shared_reference, to_device)

pytestmark = pytest.mark.gpu
_LOG = os.path.join(os.path.dirname(_ROW_LOG), "step_kernels_parity.txt")
_CASES, _REFEREED = [], []
SCALE, UP = 3.0, 0.5          # the fused path's `scale` (views per step) and the upstream gradient of its total


def _log(line):
    try:
        os.makedirs(os.path.dirname(_LOG), exist_ok=True)
        with open(_LOG, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass
    if os.environ.get("GSR_TEST_VERBOSE"):
        print(line)


def _value_check(tag, got, want):
    got, want = float(got), float(want)
    _log(f"{tag}: value {got:.9e} fp64 {want:.9e} rel {abs(got - want) / max(abs(want), 1e-300):.2e}")
    assert abs(got - want) <= 2e-5 * abs(want) + 1e-9, (tag, got, want)


def _grad_check(tag, got, want, fp32):
    """``got`` within TOL of max|want| (fp64), or within the referee's rule of what ``fp32()`` (same formulas, fp32, CPU) achieves."""
    _CASES.append(tag)
    err, scale = float((got.detach().cpu().double() - want).abs().max()), float(want.abs().max())
    m = _margin(tag, err, scale)
    _log(f"{tag}: err {err:.3e} of max {scale:.3e} -> {m:.2e}")
    if m <= TOL:
        return
    e32 = rel_max(fp32(), want)
    _REFEREED.append(tag)
    _log(f"{tag}: REFEREE HIP {m:.2e} / fp32 torch {e32:.2e} from fp64")
    assert m <= 2.0 * e32 + 2e-5, (tag, m, e32)


def _leaves(means, rots):
    return means.clone().requires_grad_(True), rots.clone().requires_grad_(True)


def _run_standalone(means, rots, v, wts=WTS3):
    from gsdyn.losses import rigidity_terms
    m, r = _leaves(means, rots)
    terms = rigidity_terms(m, r, v)
    sum(w * t for w, t in zip(wts, terms)).backward()
    return [t.detach() for t in terms], m.grad, r.grad


def _run_fused(means, rots, v, weights=WEIGHTS5):
    from gsdyn.step import _shared_terms
    m, r = _leaves(means, rots)
    total, each = _shared_terms(None, dict(means3D=m, rotations=r), v, weights, scale=SCALE)
    (total * UP).backward()
    return total.detach(), each, m.grad, r.grad


def _neighbour_case(dev, scene, path, tag):
    """One scene through the standalone (rigidity_terms: 7-float records) or the fused (_shared_terms: frames, 32-byte records) path
    against fp64: values, both gradients, bit-identical rerun; background rows exactly 0 on the standalone path."""
    means, rots, v = to_device(scene, dev)
    if path == "standalone":
        terms, gm, gr = _run_standalone(means, rots, v)
        ref, m64, r64 = neighbour_reference(scene["means"], scene["rots"], scene["variables"], WTS3)
        for name, a, b in zip(("rigid", "rot", "iso"), terms, ref):
            _value_check(f"{tag}/standalone/{name}", a, b)
        f32 = lambda i: (lambda: neighbour_reference(scene["means"], scene["rots"], scene["variables"], WTS3, dtype=torch.float32)[i])   # noqa: E731
        bg = v["bg_idx"]
        assert torch.all(gm[bg] == 0) and torch.all(gr[bg] == 0), tag
        again = _run_standalone(means, rots, v)
        assert all(torch.equal(a, b) for a, b in zip(terms, again[0]))
    else:
        total, each, gm, gr = _run_fused(means, rots, v)
        ref_total, ref, m64, r64 = shared_reference(scene["means"], scene["rots"], scene["variables"], WEIGHTS5, SCALE, upstream=UP)
        _value_check(f"{tag}/fused/total", total, ref_total)
        for name, a, b in zip(("rigid", "rot", "iso", "floor", "bg"), each, ref):
            _value_check(f"{tag}/fused/{name}", a, b)
        f32 = lambda i: (lambda: shared_reference(scene["means"], scene["rots"], scene["variables"], WEIGHTS5, SCALE, dtype=torch.float32, upstream=UP)[i])   # noqa: E731
        again = _run_fused(means, rots, v)
        assert torch.equal(total, again[0]) and torch.equal(each, again[1])
    _grad_check(f"{tag}/{path}/means3D", gm, m64, f32(-2))
    _grad_check(f"{tag}/{path}/rotations", gr, r64, f32(-1))
    assert torch.equal(gm, again[-2]) and torch.equal(gr, again[-1]), tag
    return gm, gr


# ------------------------------------------------------------------------------------------- 1. every build of the neighbour terms
@pytest.mark.parametrize("path", ["standalone", "fused"])
@pytest.mark.parametrize("n_fg,K", BUILD_CASES)
def test_every_build_of_the_neighbour_terms(dev, n_fg, K, path):
    """K picks the backward's lane group (<= 8 / 16 / 32 -> 8 / 16 / 32 lanes, larger -> 64, K > 64 strided), n_fg the partial blocks of
    the forward (32 points), the backward (256 / group) and the gather (32); with K >= n_fg the neighbour lists repeat indices."""
    _neighbour_case(dev, build_scene(n_fg, n_fg // 2 + 3, K), path, f"build/n{n_fg}-K{K}")


# ------------------------------------------------------------------------------------------------------------------ 2. graph shapes
@pytest.mark.parametrize("path", ["standalone", "fused"])
@pytest.mark.parametrize("graph,K", GRAPH_CASES)
def test_graph_shapes(dev, graph, K, path):
    n_fg = 1000
    scene = build_scene(n_fg, 131, K, graph=graph, seed=1)
    ptr = scene["variables"]["rev_ptr"].long()
    deg = ptr[1:] - ptr[:-1]
    if graph == "hub":
        assert int(deg[0]) >= n_fg                       # a reverse row every point is in: 8 lanes stride over 1000 + entries
    if graph == "chain":
        assert int(deg[0]) == 0 and int((deg == 0).sum()) == 1 and int(deg[1:-1].max()) == K     # point 0: an empty row
    gm, gr = _neighbour_case(dev, scene, path, f"graph/{graph}-K{K}")
    if graph == "self" and path == "standalone":         # offset exactly 0: what an edge gives its owner and its target cancels
        assert float(gm.abs().max()) == 0.0 and float(gr.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------ 3. states
@pytest.mark.parametrize("path", ["standalone", "fused"])
@pytest.mark.parametrize("state,K", STATE_CASES)
def test_ill_conditioned_states(dev, state, K, path):
    scene = build_scene(257, 131, K, state=state, seed=2)
    v = scene["variables"]
    if state == "coincident":
        assert int((v["neighbor_dist"] == 0).sum()) >= 100          # |off| = 0 before and now: mag = 1e-10 in the iso term
        fg = scene["means"][v["fg_idx"]]
        assert int(((fg[v["neighbor_indices"][:, 0]] - fg).abs().sum(-1) == 0).sum()) >= 100
    else:
        w = v["neighbor_weight"]
        tiny = torch.finfo(torch.float32).tiny
        assert int(((w > 0) & (w < tiny)).sum()) > 0 and int((w == 0).sum()) > 0 and int((w >= tiny).sum()) > 0
    gm, gr = _neighbour_case(dev, scene, path, f"state/{state}-K{K}")
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gr).all())


@pytest.mark.parametrize("path", ["standalone", "fused"])
@pytest.mark.parametrize("K", [20, 65])
def test_rest_state_is_finite_and_bounded(dev, K, path):
    """current = previous: every residual is rounding noise under sqrt(r^2 w + 1e-20), the gradient's direction is undefined and is
    not compared.  Values within 2 x (the fp32 CPU torch evaluation's distance from fp64) + 1e-7; every gradient row finite and
    inside the formula's own Lipschitz bound (step_ref.lipschitz_row_bounds), which a 0 / 0 or a lost guard breaks."""
    scene = build_scene(257, 131, K, state="rest", seed=3)
    means, rots, v = to_device(scene, dev)
    ref, _, _ = neighbour_reference(scene["means"], scene["rots"], scene["variables"], WTS3)
    r32, _, _ = neighbour_reference(scene["means"], scene["rots"], scene["variables"], WTS3, dtype=torch.float32)
    if path == "standalone":
        terms, gm, gr = _run_standalone(means, rots, v)
        factor = 1.0
    else:
        _, each, gm, gr = _run_fused(means, rots, v, dict(WEIGHTS5, floor=0.0, bg=0.0))
        terms, factor = each[:3], SCALE * UP
    for name, a, b, c in zip(("rigid", "rot", "iso"), terms, ref, r32):
        bar = 2.0 * abs(c - b) + 1e-7
        _log(f"rest-K{K}/{path}/{name}: HIP {float(a):.6e} fp64 {b:.6e} fp32 torch {c:.6e} bar {bar:.2e}")
        assert math.isfinite(float(a)) and abs(float(a) - b) <= bar, (name, float(a), b, c)
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gr).all())
    pts, rot = lipschitz_row_bounds(scene, [factor * w for w in WTS3])
    fg = v["fg_idx"]
    got_p, got_r = gm[fg].double().norm(dim=-1).cpu(), gr[fg].double().norm(dim=-1).cpu()
    _log(f"rest-K{K}/{path}: worst row / Lipschitz bound means3D {float((got_p / pts).max()):.3f} rotations {float((got_r / rot).max()):.3f}")
    assert bool((got_p <= pts * (1 + 1e-3)).all()) and bool((got_r <= rot * (1 + 1e-3)).all())


@pytest.mark.parametrize("state", ["identity", "zero_weight"])
@pytest.mark.parametrize("K", [20, 65])
def test_exact_zero_gradients(dev, state, K):
    """identity: identity rotations and prev_offset formed by the same fp32 subtraction -> the rigid and rot residuals are exactly 0 and
    so are their gradients.  zero_weight: every edge has weight 0 -> all three gradients are exactly 0 (0 / sqrt(1e-20), not 0 / 0)."""
    scene = build_scene(257, 131, K, state=state, seed=4)
    means, rots, v = to_device(scene, dev)
    _, gm, gr = _run_standalone(means, rots, v, wts=(200.0, 4.0, 0.0) if state == "identity" else WTS3)
    assert float(gm.abs().max()) == 0.0 and float(gr.abs().max()) == 0.0
    _, _, gm, gr = _run_fused(means, rots, v, dict(WEIGHTS5, iso=0.0 if state == "identity" else 1000.0, floor=0.0, bg=0.0))
    assert float(gm.abs().max()) == 0.0 and float(gr.abs().max()) == 0.0


def test_floor_and_background_ties(dev):
    """A foreground point exactly on the floor (y = 0: torch.clamp passes the gradient there) and a background point exactly at its
    initial position (the L1 tie: gradient 0), with the floor / bg terms alone."""
    scene = build_scene(257, 131, 20, seed=5)
    means, rots, v = to_device(scene, dev)
    w = dict(rigid=0.0, rot=0.0, iso=0.0, floor=2.0, bg=200.0)
    _, each, gm, gr = _run_fused(means, rots, v, w)
    _, ref, m64, r64 = shared_reference(scene["means"], scene["rots"], scene["variables"], w, SCALE, upstream=UP)
    i0, b0 = int(v["fg_idx"][0]), int(v["bg_idx"][0])
    assert float(means[i0, 1]) == 0.0 and abs(float(m64[i0, 1]) - 2.0 * SCALE * UP / 257) <= 1e-15
    assert abs(float(gm[i0, 1]) - float(m64[i0, 1])) <= 1e-6 * float(m64[i0, 1])
    assert float(gm[b0].abs().max()) == 0.0 and float(gr[b0].abs().max()) == 0.0 and float(m64[b0].abs().max()) == 0.0
    _value_check("ties/floor", each[3], ref[3])
    _value_check("ties/bg", each[4], ref[4])
    # sign gradients: exact up to the rounding of the one product that forms them
    assert rel_max(gm.cpu(), m64) <= 1e-6 and rel_max(gr.cpu(), r64) <= 1e-6


# ---------------------------------------------------------------------------------------------------------- 4. the fused path's flags
def _shared_on_device(v):
    from gsdyn.losses import _SHARED_KEYS
    return {k: v[k].contiguous() for k in _SHARED_KEYS}


@pytest.mark.parametrize("K", [20, 65])
def test_accumulate_into_and_work_reuse(dev, K):
    """The direct step's call shape: shared_terms_backward ADDS onto the rasterizer's gradients (gather accumulate = 1), with and
    without the forward's work buffer (frames reused, flags | 2)."""
    from diff_gaussian_rasterization import _hip
    scene = build_scene(1000, 503, K, seed=6)
    means, rots, v = to_device(scene, dev)
    sv = _shared_on_device(v)
    w5 = [SCALE * WEIGHTS5[k] for k in ("rigid", "rot", "iso", "floor", "bg")]
    _, _, m64, r64 = shared_reference(scene["means"], scene["rots"], scene["variables"], WEIGHTS5, SCALE)
    g = torch.Generator(device="cpu").manual_seed(60 + K)
    inc_m = (0.5 * float(m64.abs().max()) * torch.randn(means.shape, generator=g)).float()
    inc_r = (0.5 * float(r64.abs().max()) * torch.randn(rots.shape, generator=g)).float()
    one = torch.ones((1,), dtype=torch.float32, device=dev)
    terms, work = _hip.shared_terms_forward(means, rots, sv, w5)
    a_m, a_r = _hip.shared_terms_backward(means, rots, sv, w5, one, accumulate_into=(inc_m.to(dev), inc_r.to(dev)), work=work)
    _, work = _hip.shared_terms_forward(means, rots, sv, w5)
    b_m, b_r = _hip.shared_terms_backward(means, rots, sv, w5, one, accumulate_into=(inc_m.to(dev), inc_r.to(dev)), work=None)
    assert torch.equal(a_m, b_m) and torch.equal(a_r, b_r)
    c_m, c_r = _hip.shared_terms_backward(means, rots, sv, w5, one, work=work)
    d_m, d_r = _hip.shared_terms_backward(means, rots, sv, w5, one, work=None)
    assert torch.equal(c_m, d_m) and torch.equal(c_r, d_r)
    f32 = lambda i: (lambda: shared_reference(scene["means"], scene["rots"], scene["variables"], WEIGHTS5, SCALE, dtype=torch.float32)[i])   # noqa: E731
    _grad_check(f"flags/plain-K{K}/means3D", c_m, m64, f32(-2))
    _grad_check(f"flags/plain-K{K}/rotations", c_r, r64, f32(-1))
    _grad_check(f"flags/accumulate-K{K}/means3D", a_m, inc_m.double() + m64, lambda: inc_m + f32(-2)())
    _grad_check(f"flags/accumulate-K{K}/rotations", a_r, inc_r.double() + r64, lambda: inc_r + f32(-1)())


@pytest.mark.parametrize("n_fg,n_bg", [(257, 0), (0, 131), (1, 1), (1, 0)])
def test_empty_foreground_or_background(dev, n_fg, n_bg):
    """A mean over no elements is NaN in torch; the fused kernels define it as 0, so that a scene without
    background keeps a finite loss.  Pinned here: the empty terms are exactly 0, the torch path's are NaN, every other term and both
    gradients (which torch leaves finite: an empty term has nothing to send a gradient to) match fp64."""
    scene = build_scene(n_fg, n_bg, 20, seed=7)
    means, rots, v = to_device(scene, dev)
    total, each, gm, gr = _run_fused(means, rots, v)
    _, ref, m64, r64 = shared_reference(scene["means"], scene["rots"], scene["variables"], WEIGHTS5, SCALE, upstream=UP)
    names = ("rigid", "rot", "iso", "floor", "bg")
    empty = [n_fg == 0] * 4 + [n_bg == 0]
    want_total = 0.0
    for name, a, b, e in zip(names, each, ref, empty):
        if e:
            assert math.isnan(b) and float(a) == 0.0, (name, float(a), b)
        else:
            _value_check(f"empty/fg{n_fg}-bg{n_bg}/{name}", a, b)
            want_total += SCALE * WEIGHTS5[name] * b
    _value_check(f"empty/fg{n_fg}-bg{n_bg}/total", total, want_total)
    assert bool(torch.isfinite(m64).all()) and bool(torch.isfinite(r64).all())
    f32 = lambda i: (lambda: shared_reference(scene["means"], scene["rots"], scene["variables"], WEIGHTS5, SCALE, dtype=torch.float32, upstream=UP)[i])   # noqa: E731
    _grad_check(f"empty/fg{n_fg}-bg{n_bg}/means3D", gm, m64, f32(-2))
    _grad_check(f"empty/fg{n_fg}-bg{n_bg}/rotations", gr, r64, f32(-1))


# ------------------------------------------------------------------------------------------------------------- 5. the finishing sum
def _finish_sizes(nb):
    """(n_fg, n_bg) with nb partials of the edge kernel (32 points per block) AND nb of the point kernel (256 items per block)."""
    n_fg = 32 * (nb - 1) + 1
    return n_fg, 256 * (nb - 1) + 2 - n_fg


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 192, 193, 256, 257, 449])
def test_finishing_sum_boundaries(dev, nb):
    """shared_terms_finish_kernel sums nb partials per term with a 256-wide main loop and a 64-wide tail: nb on both sides of every
    boundary of the two loops, for the edge partials and the point partials at once.  Values against fp64."""
    from diff_gaussian_rasterization import _hip
    n_fg, n_bg = _finish_sizes(nb)
    lib = _hip.load_library()
    assert int(lib.gsr_rigidity_blocks(n_fg)) == nb and (n_fg + n_bg + 255) // 256 == nb
    assert int(lib.gsr_shared_terms_partials(n_fg, n_bg)) == 16 * n_fg + 3 * (nb + nb)
    scene = build_scene(n_fg, n_bg, 8, seed=8)
    means, rots, v = to_device(scene, dev)
    from gsdyn.step import _shared_terms
    with torch.no_grad():
        total, each = _shared_terms(None, dict(means3D=means, rotations=rots), v, WEIGHTS5, scale=SCALE)
    ref_total, ref, _, _ = shared_reference(scene["means"], scene["rots"], scene["variables"], WEIGHTS5, SCALE)
    _value_check(f"finish/nb{nb}/total", total, ref_total)
    for name, a, b in zip(("rigid", "rot", "iso", "floor", "bg"), each, ref):
        _value_check(f"finish/nb{nb}/{name}", a, b)


def test_reference_size(dev):
    """The reference's own size: 70 000 foreground points x 20 neighbours, 30 000 background (2188 + 391 partials)."""
    _neighbour_case(dev, build_scene(70_000, 30_000, 20, seed=9), "fused", "size/70k-K20")


# --------------------------------------------------------------------------------------------------------------------- 6. activations
_EXP_MAX = 88.72                # exp(88.72) = 3.39e38 < FLT_MAX < exp(88.73)


def _activation_inputs(P, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.randn(P, 4, generator=g)
    lo = 3 * torch.randn(P, 1, generator=g)
    ls = torch.randn(P, 3, generator=g)
    sat = torch.tensor([-120.0, -20.0, 0.0, 20.0, 120.0])
    n = min(P, 5)
    lo[:n, 0] = sat[:n] if P >= 5 else sat[[0, 4, 1, 3, 2]][:n]
    ls[P // 2, 0] = _EXP_MAX     # the largest finite scale
    if P > 1:
        ls[P // 2, 1] = 89.0     # one beyond: inf
        ls[0, 2] = -110.0        # underflows to 0
    if P >= 255:
        u[7], u[8], u[9] = 0.0, torch.tensor([1e-40, -2e-41, 0.0, 3e-42]), 1e18 * u[9]
    d = [torch.randn(P, 4, generator=g), torch.randn(P, 1, generator=g), torch.randn(P, 3, generator=g)]
    return (u, lo, ls), d


@pytest.mark.parametrize("P", [1, 255, 256, 257, 100_003])
def test_activations_against_fp64(dev, P):
    """normalize / sigmoid / exp and their chain against fp64 torch, element by element.  Bars from the fp32 format (eps = 2^-23): an
    activation is a handful of correctly rounded operations -> 2e-6 relative (16 eps) + the smallest fp32 step; sigmoid's gradient
    o (1 - o) carries the ABSOLUTE rounding of o near 1 -> + eps |d_op|; a rotation gradient row is five products of size |d_rot| / |q|
    -> 2e-6 of that.  Non-finite scales (exp beyond FLT_MAX) and their gradient products must equal fp32 torch's, inf / NaN included."""
    from gsdyn.losses import activate
    (u, lo, ls), d = _activation_inputs(P, 90 + P % 7)
    a = [t.to(dev).requires_grad_(True) for t in (u, lo, ls)]
    b = [t.double().requires_grad_(True) for t in (u, lo, ls)]
    c = [t.clone().requires_grad_(True) for t in (u, lo, ls)]
    outs = activate(*a)
    ref = (torch.nn.functional.normalize(b[0]), torch.sigmoid(b[1]), torch.exp(b[2]))
    t32 = (torch.nn.functional.normalize(c[0]), torch.sigmoid(c[1]), torch.exp(c[2]))
    sum((o * w.to(dev)).sum() for o, w in zip(outs, d)).backward()
    fin = torch.isfinite(t32[2])                                     # where fp32 exp is finite
    sum((o * w.double()).sum() for o, w in zip(ref[:2], d[:2])).backward()
    (ref[2] * d[2].double())[fin].sum().backward()
    sum((o * w).sum() for o, w in zip(t32, d)).backward()
    tiny = 1.5e-45
    for name, x, y in zip(("rotations", "opacities", "scales"), outs, ref):
        x, y = x.detach().cpu().double(), y.detach()
        ok = fin if name == "scales" else torch.ones_like(y, dtype=torch.bool)
        worst = float(((x - y).abs() / (y.abs() + 1e-30))[ok].max())
        _log(f"activations/P{P}/{name}: worst element-wise relative error {worst:.2e}")
        assert bool(((x - y).abs() <= 2e-6 * y.abs() + tiny)[ok].all()), name
    sc, sc32 = outs[2].detach().cpu(), t32[2].detach()
    assert torch.equal(sc[~fin], sc32[~fin]) and (P == 1 or bool(torch.isinf(sc[~fin]).all()) and int((~fin).sum()) == 1)
    assert float(sc[P // 2, 0]) < float("inf") and (P == 1 or float(sc[0, 2]) == 0.0)
    n = min(P, 5)
    op = outs[1].detach().cpu()[:n, 0]
    assert bool(((op == 0.0) | (op == 1.0) | (lo[:n, 0].abs() <= 20.0)).all())          # +-120: exactly 0 / 1
    g_lo = a[1].grad.cpu()
    assert bool((g_lo[:n, 0][lo[:n, 0].abs() == 120.0] == 0.0).all())                   # ... and a gradient of exactly 0
    eps = 2.0 ** -23
    assert bool(((g_lo.double() - b[1].grad).abs() <= 2e-6 * b[1].grad.abs() + eps * d[1].abs().double()).all())
    g_ls, w_ls = a[2].grad.cpu(), b[2].grad
    fin_g = torch.isfinite(c[2].grad)                                                   # d_sc * sc can overflow where sc itself does not
    assert bool(((g_ls.double() - w_ls).abs() <= 2e-6 * w_ls.abs() + tiny)[fin_g].all())
    assert torch.equal(g_ls[~fin_g], c[2].grad[~fin_g]) and bool((fin_g | fin == fin).all())   # d_sc * inf as torch forms it
    g_u, w_u = a[0].grad.cpu().double(), b[0].grad
    row_scale = d[0].double().norm(dim=1) / u.double().norm(dim=1).clamp_min(1e-12)
    assert bool(((g_u - w_u).abs().max(dim=1).values <= 2e-6 * row_scale).all())
    if P >= 255:
        assert torch.equal(outs[0][7].cpu(), torch.zeros(4)) and bool((g_u[7] == (d[0][7] * 1e12).double()).all())
        assert bool((g_u[8] == (d[0][8] * 1e12).double()).all())                        # |q| < 1e-12: normalize's clamped branch
        assert bool(torch.isfinite(outs[0][9]).all()) and abs(float(outs[0][9].detach().norm()) - 1.0) <= 1e-6


@pytest.mark.parametrize("used", [0, 1, 2])
def test_activations_with_unused_outputs(dev, used):
    """Each incoming gradient None in turn (two at a time): the unused outputs' parameter gradients are exactly 0, the used one's
    is what the full backward gives, bit for bit."""
    from gsdyn.losses import activate
    (u, lo, ls), d = _activation_inputs(257, 97)
    ls = ls.clamp(max=5.0)
    full = [t.to(dev).requires_grad_(True) for t in (u, lo, ls)]
    sum((o * w.to(dev)).sum() for o, w in zip(activate(*full), d)).backward()
    part = [t.to(dev).requires_grad_(True) for t in (u, lo, ls)]
    (activate(*part)[used] * d[used].to(dev)).sum().backward()
    for i in range(3):
        if i == used:
            assert torch.equal(part[i].grad, full[i].grad)
        else:
            assert float(part[i].grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------- 7. Adam
_ADAM_SIZES = (0, 1, 1023, 1024, 1025, 4097, 50_000)
_ADAM_LRS = (1e-4, 6.4e-4, 1e-3, 0.05)
_ADAM_STATS = {}


@contextlib.contextmanager
def _one_cpu_thread():
    """Hundreds of small CPU ops (the fp64 update and torch's Adam per tensor and step): run them on the calling thread.  Behind tests
    that leave another OpenMP pool spinning (the C oracle's), every parallel region of torch's pool waits for a time slice -- the
    Adam cases took 25 s each in a whole-suite run, 0.1 s alone."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _adam_inputs(count, step, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    sizes = []
    while len(sizes) < count:
        sizes += [_ADAM_SIZES[i] for i in torch.randperm(len(_ADAM_SIZES), generator=g).tolist()]
    sizes = sizes[:count] if count > 1 else [4097]
    tensors = []
    for k, n in enumerate(sizes):
        p = torch.randn(n, generator=g)
        m = torch.zeros(n) if step == 1 else 0.1 * torch.randn(n, generator=g)
        v = torch.zeros(n) if step == 1 else 0.01 * torch.rand(n, generator=g)
        grads = []
        for _ in range(3):
            gr = torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-3, 2, (1,), generator=g))
            gr[torch.rand(n, generator=g) < 0.1] = 0.0
            if n >= 4:
                gr[0], gr[1], gr[2], p[1] = 0.0, 1e-25, 1e18, 0.0
            grads.append(gr)
        tensors.append(dict(p=p, m=m, v=v, grads=grads, lr=_ADAM_LRS[k % len(_ADAM_LRS)]))
    return tensors


def _adam_run(cls, tensors, step, dev):
    """Three steps from the given state; returns per step and tensor (p, m, v before, p, m, v after) on the CPU."""
    ps = [torch.nn.Parameter(t["p"].clone().to(dev)) for t in tensors]
    opt = cls([{"params": [p], "lr": t["lr"]} for p, t in zip(ps, tensors)], lr=0.0, eps=1e-15)
    for p, t in zip(ps, tensors):
        opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=t["m"].clone().to(dev), exp_avg_sq=t["v"].clone().to(dev))
    snap = lambda: [(p.detach().cpu().clone(), opt.state[p]["exp_avg"].cpu().clone(), opt.state[p]["exp_avg_sq"].cpu().clone()) for p in ps]   # noqa: E731
    out = []
    for s in range(3):
        for p, t in zip(ps, tensors):
            p.grad = t["grads"][s].clone().to(dev)
        before = snap()
        opt.step()
        out.append((before, snap()))
    assert all(float(opt.state[p]["step"]) == step + 2 for p in ps)
    return out


@pytest.mark.parametrize("step", [1, 2, 1000, 100_000])
@pytest.mark.parametrize("count", [1, 16, 17, 35])
def test_adam_against_the_fp64_update(dev, count, step):
    """gsdyn.optim.FusedAdam (gsr_adam_step: one launch per 16 tensors, a block finds its tensor by walking first_block[]) against the
    update of gsr_step.hip's header evaluated in fp64 from the kernel's own fp32 state, one step at a time (no accumulation between
    the two).  fp32 torch.optim.Adam on the CPU, refereed the same way, is the yardstick: per element the kernel may be
    2 x torch's distance + 1e-6 |update| + one fp32 step of the parameter away (the parameter is STORED in fp32: an update below its
    last bit cannot land closer).  Moments: two terms of up to four roundings (2^-24 relative) each."""
    from diff_gaussian_rasterization import _hip
    from gsdyn.optim import FusedAdam
    assert _hip.ADAM_MAX_TENSORS == 16
    with _one_cpu_thread():
        worst_k, worst_t = _adam_case(FusedAdam, count, step, dev)
    _ADAM_STATS[(count, step)] = (worst_k, worst_t)
    _log(f"adam/count{count}-step{step}: worst element error / (|update| + fp32 step of p): HIP {worst_k:.2e}, fp32 torch (CPU) {worst_t:.2e}")
    assert worst_k <= 2.0 * worst_t + 1e-6, (worst_k, worst_t)


def _adam_case(FusedAdam, count, step, dev):
    tensors = _adam_inputs(count, step, 7000 + 100 * count + step % 97)
    hip = _adam_run(FusedAdam, tensors, step, dev)
    cpu = _adam_run(torch.optim.Adam, tensors, step, torch.device("cpu"))
    worst_k = worst_t = 0.0
    for s in range(3):
        for k, t in enumerate(tensors):
            dist = []
            for before, after in (hip[s], cpu[s]):
                (p0, m0, v0), (p1, m1, v1) = before[k], after[k]
                p64, m64, v64 = adam_reference(p0, t["grads"][s], m0, v0, t["lr"], 0.9, 0.999, 1e-15, step + s)
                dist.append(((p1.double() - p64).abs(), (p64 - p0.double()).abs(), p64, m1, m64, v1, v64, m0))
            (e_k, upd, p64, m1, m64, v1, v64, m0), (e_t, upd_t) = dist[0], dist[1][:2]
            if p64.numel() == 0:
                continue
            ulp = 2.0 ** (torch.floor(torch.log2(p64.abs().clamp_min(1e-38))) - 23)
            assert bool((e_k <= 2.0 * e_t + 1e-6 * upd + ulp).all()), (count, step, s, k, float((e_k - 2.0 * e_t - 1e-6 * upd - ulp).max()))
            moving = upd > 0
            if bool(moving.any()):
                worst_k = max(worst_k, float((e_k / (upd + ulp))[moving].max()))
                worst_t = max(worst_t, float((e_t / (upd_t + ulp))[moving].max()))
            gr = t["grads"][s].double()
            eps8 = 8 * 2.0 ** -24
            assert bool(((m1.double() - m64).abs() <= eps8 * (m0.double().abs() + gr.abs()) + 2e-45).all()), (count, step, s, k, "exp_avg")
            assert bool(((v1.double() - v64).abs() <= eps8 * v64.abs() + 2e-45).all()), (count, step, s, k, "exp_avg_sq")
    return worst_k, worst_t


# --------------------------------------------------------------------------------------------------------------- 8. radius bookkeeping
@pytest.mark.parametrize("P", [1, 256, 257, 10_001])
@pytest.mark.parametrize("view_step", [1, 2, 3])
@pytest.mark.parametrize("V", [1, 2, 7])
def test_radius_bookkeeping_exact(dev, V, view_step, P):
    """max_2D_radius[i] = max(itself, max over the rows 0, step, ... of radii[:, i]); seen[i] = any of those > 0.  Exact: integers."""
    from diff_gaussian_rasterization import _hip
    g = torch.Generator(device="cpu").manual_seed(1000 * V + 10 * view_step + P % 7)
    radii = torch.randint(0, 300, (V, P), generator=g, dtype=torch.int32)
    radii[:, torch.rand(P, generator=g) < 0.3] = 0                       # Gaussians no view sees
    if V > 1 and view_step > 1:
        radii[:, 0] = 0
        radii[1, 0] = 250                                                # seen only in a row the step skips
    m2r = (100.0 * torch.rand(P, generator=g)).float()
    m2r[P // 2] = 1000.0                                                 # already larger than every radius
    used = radii[::view_step]
    want_m2r = torch.maximum(m2r, used.max(0).values.float())
    want_seen = (used > 0).any(0)
    got_m2r = m2r.clone().to(dev)
    seen = _hip.radius_bookkeeping(radii.to(dev).contiguous(), view_step, got_m2r)
    assert seen.dtype == torch.bool and torch.equal(seen.cpu(), want_seen) and torch.equal(got_m2r.cpu(), want_m2r)
    assert float(got_m2r[P // 2]) == 1000.0
    if V > 1 and view_step > 1:
        assert not bool(seen[0]) and float(got_m2r[0]) == float(m2r[0])
    zero = torch.zeros((V, P), dtype=torch.int32, device=dev)          # rows that are all 0
    keep = m2r.clone().to(dev)
    assert not bool(_hip.radius_bookkeeping(zero, view_step, keep).any()) and torch.equal(keep.cpu(), m2r)


# --------------------------------------------------------------------------------------------------------- the referee's share (last)
def test_referee_share():
    """At most 10 % of the gradient comparisons of this file's run may have needed the fp32 referee."""
    _log(f"referee: {len(_REFEREED)} of {len(_CASES)} gradient comparisons: {_REFEREED}")
    assert len(_REFEREED) <= 0.1 * len(_CASES), _REFEREED
