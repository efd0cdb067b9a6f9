"""Training batches of the propagation network -- the reference's ``DynDataset.__getitem__`` (its src/data/dataset.py:332-516) for B
samples at once: farthest point sampling and radius thinning of the tracked particles, the gather of ``n_his + n_future`` frames, noise, a
rotation, the relations of the last history frame, and the batch's graphs as one block-diagonal ``SplitGraph`` for ``dynamics_loss``.

Every random draw is an INPUT (``draw_batch_randomness`` makes them with the reference's distributions), so ``make_dynamics_batch`` is a
function of its arguments.  Two paths compute it.  The DEFINITION (``_definition``) is plain torch, one fp32 operation at a time; it serves
CPU tensors, other dtypes and shapes beyond the kernels' limits.  The DEVICE path (contiguous float32 on a HIP device, P <= 1024, max_nobj
<= 255, topk <= 16) is three launches of csrc/gsr_dyn_batch.hip and matches the definition in every bit; the relation counts are the one
host read of a call on either path.  DESIGN.md section 3o.

The definition, per sample b (N = max_nobj + 1 rows, the tool last):
  sampling   on frame pairs[b, n_his - 1] over the first n_particles[b] rows: ``farthest_point_sampler`` picks min(max_nobj, n_particles[b])
             points from start_idx[b] (squared distances (dx dx + dy dy) + dz dz, first maximum on ties); ``fps_radius`` thins them from
             thin_start[b] with fps_radius[b] (distances as torch.norm evaluates them on the host, first maximum on ties).  n_obj[b] = the
             kept count; the kept particles, in thinning order, are rows 0 .. n_obj[b] - 1 of every frame, the rows up to max_nobj are zero.
  frames     state = the n_his history frames (objects, zero rows, the tool); action = the tool's step from frame n_his - 1 to n_his in the
             tool row; tool_future[fi] / action_future[fi] = the tool at frame n_his + fi and its step to the next; state_future = the
             objects of the n_future frames; attrs column 0 = real object, column 1 = tool; p_instance = obj_mask = real object.
  noise      added to EVERY row of state (padding and tool included, as the reference does), then every vector x of state, action,
             tool_future, action_future and state_future becomes x rot: out[c] = (x0 r[0][c] + x1 r[1][c]) + x2 r[2][c], unfused.
  relations  of the noised, rotated last history frame under ``gsdyn.dynamics.construct_edges``' rule with the sample's own n_obj[b] and
             thr2 = adj_thresh[b] * adj_thresh[b] (fp32): both ends real, not both tools, (dx dx + dy dy) + dz dz < thr2 and, among objects,
             the sender one of the receiver's min(topk, n_obj) nearest objects (itself included, equal distances: the lower index first);
             ``connect_all`` relates every real object with the tool in both directions whatever the distance, never the tool with itself.
             The list is the adjacency matrix in row-major order (``nonzero``).  More than max_nR relations in a sample: ValueError.

Out of scope: reading episode files (actions.txt, hand-eye calibration, frame_pairs), the train / valid split."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from .dynamics import SplitGraph, farthest_point_sampler, fps_radius, split_graph

DEVICE_PATH_DEFAULT = True          # measured: DESIGN.md section 3o (profiles/dyn_batch_cost.txt)
MAX_P, MAX_NOBJ, MAX_TOPK = 1024, 255, 16      # the kernels' limits (include/gsr.h)


def _rotate(x: torch.Tensor, rot: torch.Tensor) -> torch.Tensor:
    """x [B, ..., 3] times rot [B, 3, 3], one rounding per operation."""
    r = rot.reshape((rot.shape[0],) + (1,) * (x.dim() - 2) + (3, 3))
    return (x[..., 0:1] * r[..., 0, :] + x[..., 1:2] * r[..., 1, :]) + x[..., 2:3] * r[..., 2, :]


def _sample_host(particles, frame, n_part, start_idx, thin_start, radius, max_nobj):
    """The sampling of the definition, sample by sample on the host (each pick depends on the one before) -> (fps_idx [B, max_nobj] int64
    padded with -1, n_obj [B] int32), on the CPU."""
    B, P = frame.shape[0], particles.shape[1]
    clouds = particles[frame].detach().to("cpu", torch.float32)
    n_part, start_idx, thin_start, radius = n_part.cpu(), start_idx.cpu(), thin_start.cpu(), radius.detach().to("cpu", torch.float32)
    fps_idx = torch.full((B, max_nobj), -1, dtype=torch.int64)
    n_obj = torch.zeros((B,), dtype=torch.int32)
    for b in range(B):
        n_p = min(max(int(n_part[b]), 0), P)
        npoints = min(max_nobj, n_p)
        if npoints == 0:
            continue
        cloud = clouds[b, :n_p]
        picks = farthest_point_sampler(cloud[None], npoints, start_idx=min(max(int(start_idx[b]), 0), n_p - 1))[0]
        _, kept = fps_radius(cloud[picks], float(radius[b]), start_idx=min(max(int(thin_start[b]), 0), npoints - 1))
        n_obj[b] = kept.shape[0]
        fps_idx[b, :kept.shape[0]] = picks[kept]
    return fps_idx, n_obj


def _relations_dense(last: torch.Tensor, n_obj: torch.Tensor, adj_thresh: torch.Tensor, topk: int, connect_all: bool) -> torch.Tensor:
    """last [B, N, 3], n_obj [B] -> the adjacency matrices [B, N, N] (bool; row = receiver, column = sender)."""
    B, N, _ = last.shape
    max_nobj = N - 1
    d = last[:, :, None, :] - last[:, None, :, :]
    dis = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    near = dis < (adj_thresh * adj_thresh)[:, None, None]
    rows = torch.arange(N, device=last.device)
    obj = rows[None, :] < n_obj[:, None].to(torch.int64)               # real objects (the tool's row, max_nobj, is never below n_obj)
    tool = (rows == max_nobj)[None, :].expand(B, N)
    oo = obj[:, :, None] & obj[:, None, :]
    # the k nearest objects of each object: a STABLE ascending sort puts equal distances in index order; columns that are no real object
    # sort last (inf) and are masked by `oo` anyway
    order = torch.argsort(torch.where(oo, dis, torch.full_like(dis, float("inf"))), dim=-1, stable=True)[..., :min(int(topk), max_nobj)]
    keep = torch.zeros((B, N, N), dtype=torch.bool, device=last.device)
    keep.scatter_(2, order, True)
    ot = (obj[:, :, None] & tool[:, None, :]) | (tool[:, :, None] & obj[:, None, :])
    return (oo & near & keep) | (ot & (near | bool(connect_all)))


def _check_counts(n_rel: torch.Tensor, max_nR: int):
    """The one host read of a call -> the counts as a list; raises where the reference's pad_torch fails."""
    counts = n_rel.cpu().tolist()
    for b, c in enumerate(counts):
        if c > max_nR:
            raise ValueError(f"make_dynamics_batch: sample {b} has {c} relations, more than max_nR = {max_nR}")
    return counts


def _frames(pairs, F):
    return pairs.to(torch.int64).clamp(0, F - 1)


def _definition(particles, eef, pairs, n_part, start_idx, thin_start, radius, adj_thresh, rot, noise, n_his, n_future, max_nobj, max_nR, topk,
                connect_all, dense):
    dev = particles.device
    F = particles.shape[0]
    B, N = pairs.shape[0], max_nobj + 1
    fr = _frames(pairs, F)
    fps_idx, n_obj = _sample_host(particles, fr[:, n_his - 1], n_part, start_idx, thin_start, radius, max_nobj)
    fps_idx, n_obj = fps_idx.to(dev), n_obj.to(dev)
    real = torch.arange(max_nobj, device=dev)[None, :] < n_obj[:, None].to(torch.int64)                   # [B, max_nobj]
    obj = particles[fr[:, :, None], fps_idx.clamp(min=0)[:, None, :]]                                       # [B, T, max_nobj, 3]
    obj = torch.where(real[:, None, :, None], obj, torch.zeros_like(obj))
    tool = eef[fr]                                                                                          # [B, T, 3]
    state = torch.cat([obj[:, :n_his], tool[:, :n_his, None]], 2)
    if noise is not None:
        state = state + noise
    zeros = lambda *s: torch.zeros(s, dtype=particles.dtype, device=dev)  # noqa: E731
    action = zeros(B, N, 3)
    action[:, max_nobj] = tool[:, n_his] - tool[:, n_his - 1]
    tool_future, action_future = zeros(B, n_future - 1, N, 3), zeros(B, n_future - 1, N, 3)
    tool_future[:, :, max_nobj] = tool[:, n_his:-1]
    action_future[:, :, max_nobj] = tool[:, n_his + 1:] - tool[:, n_his:-1]
    state, action, tool_future, action_future = _rotate(state, rot), _rotate(action, rot), _rotate(tool_future, rot), _rotate(action_future, rot)
    state_future = _rotate(obj[:, n_his:], rot)
    attrs = zeros(B, N, 2)
    attrs[:, :max_nobj, 0] = real.to(attrs.dtype)
    attrs[:, max_nobj, 1] = 1
    # ---- relations
    adj = _relations_dense(state[:, n_his - 1], n_obj, adj_thresh.to(state.dtype), topk, connect_all)
    n_rel = adj.sum((1, 2)).to(torch.int32)
    counts = _check_counts(n_rel, max_nR)
    rel = adj.nonzero()                                               # batch-major, then row-major: ascending receiver, then sender
    offs = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(n_rel, 0)
    e_loc = torch.arange(rel.shape[0], device=dev) - offs[rel[:, 0]]
    receivers = torch.full((B, max_nR), N, dtype=torch.int64, device=dev)
    senders = torch.full((B, max_nR), N, dtype=torch.int64, device=dev)
    receivers[rel[:, 0], e_loc] = rel[:, 1]
    senders[rel[:, 0], e_loc] = rel[:, 2]
    out = dict(state=state, action=action, tool_future=tool_future, action_future=action_future, state_future=state_future, attrs=attrs,
               p_instance=real.to(particles.dtype)[:, :, None], obj_mask=real, n_obj=n_obj, fps_idx=fps_idx, receivers=receivers, senders=senders,
               n_rel=n_rel, n_rel_rows=max_nR, graph=split_graph(rel[:, 0] * N + rel[:, 1], rel[:, 0] * N + rel[:, 2], B * N))
    if dense:
        out["Rr"], out["Rs"] = zeros(B, max_nR, N), zeros(B, max_nR, N)
        out["Rr"][rel[:, 0], e_loc, rel[:, 1]] = 1
        out["Rs"][rel[:, 0], e_loc, rel[:, 2]] = 1
    assert sum(counts) == rel.shape[0]
    return out


def _device(particles, eef, pairs, n_part, start_idx, thin_start, radius, adj_thresh, rot, noise, n_his, n_future, max_nobj, max_nR, topk,
            connect_all, dense):
    from diff_gaussian_rasterization import _hip
    dev = particles.device
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    out = _hip.dyn_batch_sample(particles, f32(eef), pairs.to(device=dev, dtype=torch.int64).contiguous(), i32(n_part), i32(start_idx),
                                i32(thin_start), f32(radius), f32(rot), None if noise is None else f32(noise), n_his, n_future, max_nobj)
    recv, send, n_rel, Rr, Rs = _hip.dyn_batch_relations(out["state"], out["n_obj"], f32(adj_thresh), topk, connect_all, max_nR, dense)
    counts = _check_counts(n_rel, max_nR)             # raises before anything else is launched
    N = max_nobj + 1
    out.update(receivers=recv, senders=send, n_rel=n_rel, n_rel_rows=max_nR,
               graph=SplitGraph(*_hip.dyn_batch_graph(recv, send, n_rel, N, sum(counts))))
    if dense:
        out["Rr"], out["Rs"] = Rr, Rs
    return out


def _device_ok(particles, eef, pairs, rot, noise, max_nobj, topk) -> bool:
    if not (particles.is_cuda and particles.dtype == torch.float32 and particles.is_contiguous()):
        return False
    if not all(t is None or (t.device == particles.device and t.dtype == torch.float32) for t in (eef, rot, noise)):
        return False
    return pairs.device == particles.device and particles.shape[1] <= MAX_P and max_nobj <= MAX_NOBJ and topk <= MAX_TOPK


def make_dynamics_batch(particles: torch.Tensor, eef: torch.Tensor, pairs: torch.Tensor, *, n_his: int, n_future: int, max_nobj: int, max_nR: int,
                        topk: int, connect_all: bool, start_idx: torch.Tensor, thin_start: torch.Tensor, fps_radius: torch.Tensor,
                        adj_thresh: torch.Tensor, rot: torch.Tensor, noise: Optional[torch.Tensor] = None,
                        n_particles: Optional[torch.Tensor] = None, dense: bool = True, device_path: Optional[bool] = None) -> Dict:
    """One training batch of ``dynamics_loss`` from tracked particles (the module's docstring has the definition).

    particles [F, P, 3]: the frames of one or more episodes, stacked along F and padded to a common P; ``n_particles`` [B]: the real
    particle count of each sample's episode (None: P); eef [F, 3]: the tool point per frame; pairs [B, n_his + n_future]: global frame
    indices.  The random draws, one per sample (``draw_batch_randomness``): start_idx [B] (first pick), thin_start [B] (first kept pick,
    an index into the picks), fps_radius / adj_thresh [B], rot [B, 3, 3], noise [B, n_his, N, 3] or None.

    -> dict: state [B, n_his, N, 3], action [B, N, 3], tool_future / action_future [B, n_future - 1, N, 3], state_future [B, n_future,
    max_nobj, 3], attrs [B, N, 2], p_instance [B, max_nobj, 1], obj_mask [B, max_nobj] bool, Rr / Rs [B, max_nR, N] (``dense`` only) -- the
    reference's dictionary, batched -- and n_obj [B] int32, fps_idx [B, max_nobj] int64 (indices into the episode's particles, -1 behind
    n_obj), receivers / senders [B, max_nR] int64 (local rows, padded with N), n_rel [B] int32, n_rel_rows = max_nR, graph: the B graphs as
    one ``SplitGraph`` over B N rows (node ids offset by b N, no padded relations, batch-major, ascending in the receiver, then the sender).

    ``device_path``: None for ``DEVICE_PATH_DEFAULT``, False for the definition.  The kernels are taken only for contiguous float32 tensors
    on a HIP device with P <= 1024, max_nobj <= 255 and topk <= 16; everything else runs the definition.  Raises ValueError when a sample has
    more than max_nR relations."""
    n_his, n_future, max_nobj, max_nR, topk = int(n_his), int(n_future), int(max_nobj), int(max_nR), int(topk)
    if particles.dim() != 3 or particles.shape[2] != 3 or eef.shape != (particles.shape[0], 3):
        raise ValueError("make_dynamics_batch: particles must be [F, P, 3] and eef [F, 3]")
    if n_his < 1 or n_future < 1 or max_nobj < 1 or topk < 1 or max_nR < 0 or particles.shape[0] < 1 or particles.shape[1] < 1:
        raise ValueError("make_dynamics_batch: n_his, n_future, max_nobj, topk, F and P must be at least 1")
    B = pairs.shape[0]
    if pairs.dim() != 2 or pairs.shape[1] != n_his + n_future or B < 1:
        raise ValueError("make_dynamics_batch: pairs must be [B, n_his + n_future]")
    N = max_nobj + 1
    for name, t, shape in (("start_idx", start_idx, (B,)), ("thin_start", thin_start, (B,)), ("fps_radius", fps_radius, (B,)),
                           ("adj_thresh", adj_thresh, (B,)), ("rot", rot, (B, 3, 3)), ("noise", noise, (B, n_his, N, 3)),
                           ("n_particles", n_particles, (B,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"make_dynamics_batch: {name} must have shape {shape}, got {tuple(t.shape)}")
    if n_particles is None:
        n_particles = torch.full((B,), particles.shape[1], dtype=torch.int32, device=particles.device)
    want = DEVICE_PATH_DEFAULT if device_path is None else bool(device_path)
    use = want and _device_ok(particles, eef, pairs, rot, noise, max_nobj, topk)
    dev = particles.device
    args = (particles, eef.to(dev), pairs.to(dev), n_particles, start_idx, thin_start, fps_radius.to(dev), adj_thresh.to(dev), rot.to(dev),
            None if noise is None else noise.to(dev), n_his, n_future, max_nobj, max_nR, topk, bool(connect_all), bool(dense))
    return (_device if use else _definition)(*args)


def draw_batch_randomness(B: int, n_points, *, n_his: int, max_nobj: int, fps_radius_range, adj_radius_range, state_noise: float,
                          generator: Optional[torch.Generator] = None, device=None) -> Dict:
    """The random inputs of ``make_dynamics_batch`` with the reference's distributions (dataset.py:376-382, 463-468, 488; its
    data/utils.py:38): start_idx uniform in [0, n_points) (``n_points``: an int, or [B] per-sample particle counts), thin_start uniform in
    [0, min(max_nobj, n_points)), fps_radius ~ U(fps_radius_range), adj_thresh ~ U(adj_radius_range), rot = the rotation about z by
    U(-pi, pi), noise ~ U(-state_noise, state_noise) [B, n_his, max_nobj + 1, 3].  Drawn on the generator's device (the CPU without one),
    returned on ``device``.  The same generator state gives the same draws."""
    gdev = generator.device if generator is not None else torch.device("cpu")
    u = lambda *s: torch.rand(s, generator=generator, device=gdev, dtype=torch.float32)  # noqa: E731
    n = torch.as_tensor(n_points, dtype=torch.int64, device=gdev).expand(B)
    start_idx = torch.minimum((u(B).double() * n).to(torch.int64), n - 1)
    npick = torch.clamp(n, max=int(max_nobj))
    thin_start = torch.minimum((u(B).double() * npick).to(torch.int64), npick - 1)
    span = lambda r, x: float(r[0]) + (float(r[1]) - float(r[0])) * x  # noqa: E731
    fps_r, adj = span(fps_radius_range, u(B)), span(adj_radius_range, u(B))
    ang = (2.0 * u(B) - 1.0) * math.pi
    c, s, z, o = torch.cos(ang), torch.sin(ang), torch.zeros_like(ang), torch.ones_like(ang)
    rot = torch.stack([c, -s, z, s, c, z, z, z, o], 1).reshape(B, 3, 3)
    noise = (2.0 * u(B, int(n_his), int(max_nobj) + 1, 3) - 1.0) * float(state_noise)
    out = dict(start_idx=start_idx, thin_start=thin_start, fps_radius=fps_r, adj_thresh=adj, rot=rot, noise=noise)
    return {k: v.to(device) if device is not None else v for k, v in out.items()}
