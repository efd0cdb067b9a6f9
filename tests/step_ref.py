"""Plain references and scene builders for the step-side kernels (gsr_rigidity.hip, gsr_step.hip): tests/test_step_kernels_gpu.py
and the two neighbour-term tests of tests/test_losses_step_gpu.py share them.

References are the project's own torch formulas (gsdyn.losses) evaluated with autograd in the dtype and on the device of the tensors
handed in -- fp64 on the CPU is the referee, fp32 on the CPU the yardstick of what fp32 can do on an ill-conditioned case.
Scenes are built directly as tensors (CPU, fp32) so that the neighbour graph and the state can be chosen freely.

``python tests/step_ref.py`` prints, without a GPU, how far the fp32 CPU evaluation is from fp64 on every case of the GPU file
(the condition of its referee rule: at least 90 % of the cases inside TOL in fp32)."""
from __future__ import annotations

import itertools
import math

import torch

_TERMS = ("rigid", "rot", "iso", "floor", "bg")


def neighbour_terms(means, rots, v):
    """(rigid, rot, iso) of gsdyn.step._shared_terms, written out: ``means`` [P,3] / ``rots`` [P,4] (normalised) in any dtype on any
    device; the tensors of ``v`` are cast to match.  Differentiable w.r.t. means and rots."""
    from gsdyn.losses import build_rotation, quat_mult, weighted_l2_loss_v1, weighted_l2_loss_v2
    cast = lambda t: t.to(device=means.device, dtype=means.dtype)   # noqa: E731
    fg_idx, nbr = v["fg_idx"].to(means.device), v["neighbor_indices"].to(means.device)
    fg_pts, fg_rot = means.index_select(0, fg_idx), rots.index_select(0, fg_idx)
    rel = quat_mult(fg_rot, cast(v["prev_inv_rot_fg"]))
    R = build_rotation(rel)
    off = fg_pts[nbr] - fg_pts[:, None]
    offp = (off[:, :, :, None] * R[:, None, :, :]).sum(2)
    nw = cast(v["neighbor_weight"])
    rigid = weighted_l2_loss_v2(offp, cast(v["prev_offset"]), nw)
    rot = weighted_l2_loss_v2(rel[nbr], rel[:, None], nw)
    iso = weighted_l2_loss_v1(torch.sqrt((off ** 2).sum(-1) + 1e-20), cast(v["neighbor_dist"]), nw)
    return rigid, rot, iso


def cpu_variables(v, dtype):
    """The tensors of a variables dict on the CPU, floating ones in ``dtype``, without the reverse adjacency (so that
    gsdyn.step._shared_terms takes its torch path)."""
    return {k: (t.detach().cpu().to(dtype) if t.is_floating_point() else t.detach().cpu()) for k, t in v.items()
            if torch.is_tensor(t) and k not in ("rev_ptr", "rev_edge")}


def neighbour_reference(means, rots, v, wts, dtype=torch.float64):
    """Values (3 floats) and gradients of wts . (rigid, rot, iso) in ``dtype`` on the CPU."""
    m = means.detach().cpu().to(dtype).requires_grad_(True)
    r = rots.detach().cpu().to(dtype).requires_grad_(True)
    terms = neighbour_terms(m, r, cpu_variables(v, dtype))
    total = sum(w * t for w, t in zip(wts, terms))
    if total.requires_grad:
        total.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # noqa: E731
    return [float(t.detach()) for t in terms], zero(m), zero(r)


def shared_reference(means, rots, v, weights, scale, dtype=torch.float64, upstream=1.0):
    """(total, the five terms, d_means3D, d_rotations) of upstream * _shared_terms(...) in ``dtype`` on the CPU, torch path."""
    from gsdyn.step import _shared_terms
    m = means.detach().cpu().to(dtype).requires_grad_(True)
    r = rots.detach().cpu().to(dtype).requires_grad_(True)
    total, each = _shared_terms(None, dict(means3D=m, rotations=r), cpu_variables(v, dtype), weights, scale=scale)
    (total * upstream).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # noqa: E731
    return float(total.detach()), [float(x) for x in each], zero(m), zero(r)


# ------------------------------------------------------------------------------------------------------------------ scenes
_OFFSETS = sorted((o for o in itertools.product(range(-2, 3), repeat=3) if o != (0, 0, 0)), key=lambda o: (o[0] ** 2 + o[1] ** 2 + o[2] ** 2, o))

GRAPHS = ("knn", "hub", "chain", "self")
STATES = ("moved", "rest", "identity", "zero_weight", "coincident", "sparse")


def _lattice_knn(prev, n, K, side):
    """The K nearest of each point's 124 lattice-window candidates (wrapped; candidates repeat where the cloud is smaller than the
    window, and the list cycles where K > 124): a kNN-like graph in O(n) with in-degrees that vary with the jitter."""
    i = torch.arange(n)
    xyz = torch.stack([i % side, (i // side) % side, i // (side * side)], 1)
    off = torch.tensor(_OFFSETS)                                        # [124,3]
    c = (xyz[:, None, :] + off[None]) % side
    cand = (c[..., 0] + side * c[..., 1] + side * side * c[..., 2]) % n  # [n,124]
    d = (prev[cand] - prev[:, None]).norm(dim=-1)
    order = torch.argsort(d, dim=1, stable=True)
    cand = torch.gather(cand, 1, order)
    return cand[:, torch.arange(K) % cand.shape[1]].contiguous()


def build_scene(n_fg, n_bg, K, graph="knn", state="moved", seed=0):
    """Tensors of one t > 0 step (CPU, fp32): dict(means [P,3], rots [P,4] normalised, variables).  Foreground and background rows are
    interleaved in the P rows.  ``graph``: knn | hub (every point lists point 0 first) | chain (every point lists only its successor, the
    last one itself: nobody lists point 0) | self (j = i).  ``state``: moved | rest (current = previous) | identity (rest, identity
    rotations) | zero_weight (moved, every weight 0) | coincident (pairs at one position, listing each other first, moving together)
    | sparse (spacing 0.15: weights from normal through denormal to exactly 0)."""
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + 17 * n_fg + K)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    P = n_fg + n_bg
    perm = torch.randperm(P, generator=g)
    fg_idx, bg_idx = perm[:n_fg].sort().values.contiguous(), perm[n_fg:].sort().values.contiguous()
    h = 0.15 if state == "sparse" else 0.01
    side = max(1, math.ceil(n_fg ** (1.0 / 3.0) - 1e-9))
    i = torch.arange(n_fg)
    sites = torch.stack([i % side, (i // side) % side, i // (side * side)], 1).float()
    prev = (sites + 0.6 * (torch.rand(n_fg, 3, generator=g) - 0.5)) * h
    if n_fg:
        prev[:, 1] -= prev[:, 1].mean()                                  # the floor (y = 0) cuts through the cloud
    pairs = torch.arange(2, n_fg - 1, 2) if state == "coincident" else torch.zeros(0, dtype=torch.long)
    prev[pairs + 1] = prev[pairs]
    if graph == "self" or n_fg == 0:
        nbr = i[:, None].expand(n_fg, K).contiguous()
    elif graph == "chain":
        nbr = (i + 1).clamp(max=n_fg - 1)[:, None].expand(n_fg, K).contiguous()
    else:
        nbr = _lattice_knn(prev, n_fg, K, side)
        if graph == "hub":
            nbr[:, 0] = 0
    nbr[pairs, 0], nbr[pairs + 1, 0] = pairs + 1, pairs
    prev_rot = torch.nn.functional.normalize(rn(n_fg, 4))
    if state == "identity":
        prev_rot = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n_fg, 1)
    if state in ("rest", "identity"):
        cur, cur_rot = prev.clone(), prev_rot.clone()
    else:
        move = 0.15 * h * rn(n_fg, 3)
        move[pairs + 1] = move[pairs]
        cur = prev + move
        cur_rot = torch.nn.functional.normalize(prev_rot + 0.05 * rn(n_fg, 4))
        if n_fg:
            cur[0, 1] = 0.0                                              # a point exactly on the floor
    init_bg_pts = (torch.rand(n_bg, 3, generator=g) - 0.5) * (h * side + 0.1)
    init_bg_rot = torch.nn.functional.normalize(rn(n_bg, 4))
    bg, bg_rot = init_bg_pts + 0.01 * rn(n_bg, 3), torch.nn.functional.normalize(init_bg_rot + 0.05 * rn(n_bg, 4))
    if n_bg:
        bg[0], bg_rot[0] = init_bg_pts[0], init_bg_rot[0]                # a background point exactly where it started
    means, rots = torch.zeros(P, 3), torch.zeros(P, 4)
    means[fg_idx], means[bg_idx], rots[fg_idx], rots[bg_idx] = cur, bg, cur_rot, bg_rot
    prev_offset = prev[nbr] - prev[:, None]
    sq = (prev_offset ** 2).sum(-1)
    weight = torch.exp(-2000 * sq)
    if state == "zero_weight":
        weight = torch.zeros_like(weight)
    inv = prev_rot.clone()
    inv[:, 1:] = -inv[:, 1:]
    from gsdyn.losses import reverse_adjacency
    rev_ptr, rev_edge = reverse_adjacency(nbr) if n_fg else (torch.zeros(1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    variables = dict(fg_idx=fg_idx, bg_idx=bg_idx, neighbor_indices=nbr, neighbor_weight=weight.contiguous(), neighbor_dist=torch.sqrt(sq).contiguous(),
                     prev_inv_rot_fg=inv.contiguous(), prev_offset=prev_offset.contiguous(), init_bg_pts=init_bg_pts, init_bg_rot=init_bg_rot,
                     rev_ptr=rev_ptr, rev_edge=rev_edge)
    return dict(means=means, rots=rots, variables=variables)


def to_device(scene, dev):
    return scene["means"].to(dev), scene["rots"].to(dev), {k: t.to(dev) for k, t in scene["variables"].items()}


def lipschitz_row_bounds(scene, g3):
    """Per foreground point, what |dL/dp_i| and |dL/dq_i| of g3 . (rigid, rot, iso) cannot exceed whatever the residuals are: every
    edge term is sqrt(r^2 w + 1e-20), whose gradient w.r.t. r is at most sqrt(w) in norm.  An edge pushes both of its ends by at most
    (g_rigid + g_iso) sqrt(w); the relative quaternion of both ends by g_rot sqrt(w), and that of its owner by a further
    2 |off| g_rigid sqrt(w) / |q| through the rotation matrix (a rotated vector moves by at most 2 |off| |du| with the unit
    quaternion u, and u = q / |q|).  rot = q * conj(prev) with unit prev keeps the norm.  Returned in fp64: ([n_fg], [n_fg])."""
    v = scene["variables"]
    nbr, w = v["neighbor_indices"], v["neighbor_weight"].double()
    n, K = nbr.shape
    g1, g2, g3_ = (x / max(n * K, 1) for x in g3)
    sw = torch.sqrt(w)
    fg = scene["means"].double()[v["fg_idx"]]
    off = (fg[nbr] - fg[:, None]).norm(dim=-1)
    q = scene["rots"].double()[v["fg_idx"]].norm(dim=-1) * v["prev_inv_rot_fg"].double().norm(dim=-1)
    incoming = torch.zeros(n, dtype=torch.float64).index_add_(0, nbr.reshape(-1), sw.reshape(-1))
    pts = (g1 + g3_) * (sw.sum(1) + incoming)
    rot = (g2 * (sw.sum(1) + incoming) + 2 * g1 * (off * sw).sum(1) / q) * v["prev_inv_rot_fg"].double().norm(dim=-1)
    return pts, rot


# ----------------------------------------------------------------------------------------------------------- Adam, fp64
def adam_reference(p, g, m, v, lr, beta1, beta2, eps, step):
    """One update as gsr_step.hip's header writes it, in fp64 from fp32 inputs: returns (p, m, v) after the step."""
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    m = m + (1 - beta1) * (g - m)
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p - (lr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


# ------------------------------------------------------------------------------------------------- the cases of the GPU file
KS = (1, 7, 8, 9, 16, 17, 20, 32, 33, 64, 65, 100)
NFGS = (1, 31, 32, 33, 257, 3000)
BUILD_CASES = sorted({(n, K) for n in (33, 257) for K in KS} | {(n, K) for n in NFGS for K in (20, 65)})
GRAPH_CASES = [(gr, K) for gr in GRAPHS for K in (20, 65)]
STATE_CASES = [(st, K) for st in ("coincident", "sparse") for K in (20, 65)]
WTS3 = (200.0, 4.0, 1000.0)
WEIGHTS5 = dict(rigid=200.0, rot=4.0, iso=1000.0, floor=2.0, bg=200.0)


def rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-300)) if a.numel() else 0.0


def _conditioning_table():
    """fp32 CPU torch against fp64 on the parametrised neighbour-term cases: the referee rule's precondition."""
    rows = []
    for tag, scenes in (("build", [(f"n{n}-K{K}", build_scene(n, n // 2 + 3, K)) for n, K in BUILD_CASES]),
                        ("graph", [(f"{gr}-K{K}", build_scene(257, 131, K, graph=gr, seed=1)) for gr, K in GRAPH_CASES]),
                        ("state", [(f"{st}-K{K}", build_scene(257, 131, K, state=st, seed=2)) for st, K in STATE_CASES])):
        for name, sc in scenes:
            _, m64, r64 = neighbour_reference(sc["means"], sc["rots"], sc["variables"], WTS3)
            _, m32, r32 = neighbour_reference(sc["means"], sc["rots"], sc["variables"], WTS3, dtype=torch.float32)
            _, _, sm64, sr64 = shared_reference(sc["means"], sc["rots"], sc["variables"], WEIGHTS5, 3.0, upstream=0.5)
            _, _, sm32, sr32 = shared_reference(sc["means"], sc["rots"], sc["variables"], WEIGHTS5, 3.0, dtype=torch.float32, upstream=0.5)
            rows.append((f"{tag}/{name}", max(rel_max(m32, m64), rel_max(r32, r64)), max(rel_max(sm32, sm64), rel_max(sr32, sr64))))
    return rows


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "gs-dynamics_amd"))
    table = _conditioning_table()
    for name, a, b in table:
        print(f"{name:28s} fp32 torch vs fp64: standalone {a:.2e}  fused {b:.2e}")
    inside = sum(1 for _, a, b in table if max(a, b) <= 1e-4)
    print(f"{inside} of {len(table)} cases inside 1e-4 in fp32 ({100.0 * inside / len(table):.0f} %)")
