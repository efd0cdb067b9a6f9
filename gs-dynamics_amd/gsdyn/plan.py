"""The planner's rollout: B sampled push sequences advance B copies of ONE particle state through the dynamics model in one batch
(/root/reference/src/real_world/plan.py:24-154, ``dynamics``, driven by the MPPI loop of /root/reference/src/real_world/utils/planner.py).
The sampling / weighting loop and the cost are the caller's; this is the pure-compute part -- the only place where the propagation
network runs at a batch size that can fill a GPU.

Semantics (the reference's, restated).  An action row is (x_start, y_start, theta, length); ``decode_action`` turns it into the push's end
points and ``repeat = int(length)`` model calls.  For every look-ahead step ``li``:
  * the object history is ``n_his`` copies of the previous look-ahead state (the given state at ``li = 0``), the tool sits at
    (x_start, y_start, lowest object z) in every history frame and moves by (x_end - x_start, y_end - y_start, 0) per model call;
  * attributes mark object / tool, the instance column is all ones, the relations are rebuilt from the newest positions before every
    model call (``gsdyn.dynamics.construct_edges``' rule);
  * after a model call the history shifts by one frame: the predicted objects and the tool at (last x, y + displacement, lowest
    predicted z); a sample's state of step ``li`` is the prediction of its ``repeat``-th call.
Two stated departures: the reference passes ``no_self_edge=True`` to a function that has no such parameter ("known defects") --
here self-relations are included, as at training time; and ``repeat < 1``, for which the reference would leave zeros, is a ``ValueError``.

On a HIP device, for a model the split propagation accepts and at most 127 particles, one model call for ALL samples is
gsr_plan_step_head -> gsr_construct_edges_batch -> ``DynamicsPredictor._propagate_split`` -> gsr_plan_step_tail: the B graphs are laid out
block-diagonally (sample b owns the rows b R .. b R + R - 1, R = n_obj + 1; one dummy row behind the last sample collects the padded
relations) and are one graph to the two GNN kernels.  No host synchronisation inside the loops.  Everything else -- CPU tensors, a model
the split path refuses, more than 127 particles -- takes ``_rollout_reference``, a per-sample loop in plain torch that is also the
semantic definition.

Behind the rollout: ``running_cost`` (the reference's real_world/plan.py ``running_cost``: chamfer distance of the last look-ahead state to a
target cloud, a collision term at every push's start point, a box term) and ``mppi_update`` (utils/plan_utils.py ``optimize_action_mppi``)
are one launch each on a HIP device -- gsr_plan_cost, gsr_plan_mppi_update (csrc/gsr_plan_cost.hip) -- and plain torch elsewhere;
``sample_action_seq`` / ``clip_actions`` restate the reference's sampler; ``plan_actions`` is the whole planning step: per chunk and
iteration sample -> ``rollout_actions`` -> ``running_cost`` -> ``mppi_update``, the best chunk wins.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from .dynamics import DynamicsPredictor, construct_edges

MAX_DEVICE_PARTICLES = 127          # gsr_construct_edges_batch: a sample's objects + tool fit two 64-lane ballots
MAX_COST_PARTICLES = 1024           # gsr_plan_cost: a sample's particles in LDS
COST_TABLE_ENTRIES = 1 << 24        # _running_cost_reference: the [b, M, n_obj] distance table of one slice of B stays below this


def decode_action(action: torch.Tensor, push_length: float = 0.01) -> Tuple[torch.Tensor, torch.Tensor]:
    """action [B, T, 4] = (x_start, y_start, theta, length) -> (decoded [B, T, 4] = (x_start, y_start, x_end, y_end), repeat [B, T] int32)
    (/root/reference/src/real_world/utils/plan_utils.py:135-144)."""
    x_start, y_start, theta = action[:, :, 0], action[:, :, 1], action[:, :, 2]
    repeat = action[:, :, 3].detach().to(torch.int32)
    x_end = x_start - push_length * torch.cos(theta)
    y_end = y_start - push_length * torch.sin(theta)
    return torch.stack([x_start, y_start, x_end, y_end], dim=-1), repeat


def _device_path_ok(model: DynamicsPredictor, probe: torch.Tensor, n_obj: int) -> bool:
    """The batched HIP path serves what the graphed rollout step's fused glue serves (split propagation, positions or nothing as the state
    input, a 3-wide action, no motion input) at up to ``MAX_DEVICE_PARTICLES`` object particles; everything else takes the fallback."""
    c = model.model_config
    return bool(model._split_ok(probe) and model.motion_dim == 0 and c["state_dim"] in (0, 3) and c["action_dim"] == 3 and c["attr_dim"] >= 2
                and 1 <= int(n_obj) <= MAX_DEVICE_PARTICLES)


def _sample_constants(model: DynamicsPredictor, n_obj: int, dev, dtype):
    """One sample's constant rows: attributes (object / tool), instance column (ones for the objects), masks."""
    R = n_obj + 1
    a = torch.zeros((R, model.model_config["attr_dim"]), dtype=dtype, device=dev)
    a[:n_obj, 0] = 1.0
    a[n_obj, 1] = 1.0
    g = torch.zeros((R, 1), dtype=dtype, device=dev)
    g[:n_obj] = 1.0
    mask = torch.ones(R, dtype=torch.bool, device=dev)
    tool = torch.zeros(R, dtype=torch.bool, device=dev)
    tool[n_obj] = True
    return a, g, mask, tool


def _rollout_reference(model: DynamicsPredictor, state: torch.Tensor, decoded: torch.Tensor, repeat_host: List[List[int]], adj_thresh: float,
                       topk: int, n_his: int, trace: list = None) -> torch.Tensor:
    """The semantic definition: one sample at a time, ``construct_edges`` + ``model._propagate`` per model call.  A sample runs exactly its
    own ``repeat`` calls per look-ahead step (the calls the reference makes beyond that are discarded by it).  ``trace``: a list that
    receives (sample, li, ai, newest positions [R, 3], receivers, senders) per model call."""
    B, T, n_obj = decoded.shape[0], decoded.shape[1], state.shape[0]
    dev, dtype = state.device, state.dtype
    a, g, mask, tool = _sample_constants(model, n_obj, dev, dtype)
    c = model.model_config
    out = torch.zeros((B, T, n_obj, 3), dtype=dtype, device=dev)
    for b in range(B):
        prev = state
        for li in range(T):
            hist = prev[None].repeat(n_his, 1, 1)                                       # [n_his, n_obj, 3]
            eef = torch.stack([decoded[b, li, 0], decoded[b, li, 1], prev[:, 2].min()])[None].repeat(n_his, 1)   # [n_his, 3]
            delta = torch.stack([decoded[b, li, 2] - decoded[b, li, 0], decoded[b, li, 3] - decoded[b, li, 1], torch.zeros((), dtype=dtype, device=dev)])
            act = torch.zeros((n_obj + 1, c["action_dim"]), dtype=dtype, device=dev)
            if c["action_dim"] > 0:
                act[n_obj, :3] = delta
            pred = prev
            for ai in range(1, repeat_host[b][li] + 1):
                states = torch.cat([hist, eef[:, None]], 1)                             # [n_his, R, 3], the tool last
                recv, send = construct_edges(states[-1], adj_thresh, mask, tool, topk=topk, n_tool=1)
                if trace is not None:
                    trace.append((b, li, ai, states[-1].clone(), recv, send))
                state_t = states.transpose(0, 1).reshape(n_obj + 1, n_his * 3)
                pos, _ = model._propagate(state_t, a, g, act, recv, send)
                pred = pos[:n_obj]
                eef_new = torch.stack([eef[-1, 0] + delta[0], eef[-1, 1] + delta[1], pred[:, 2].min()])
                hist = torch.cat([hist[1:], pred[None]], 0)
                eef = torch.cat([eef[1:], eef_new[None]], 0)
            out[b, li] = pred
            prev = pred
    return out


def _rollout_device(model: DynamicsPredictor, state: torch.Tensor, decoded: torch.Tensor, repeat: torch.Tensor, max_repeat: List[int],
                    adj_thresh: float, topk: int, n_his: int, trace: list = None) -> torch.Tensor:
    """All samples of a chunk per model call (module docstring).  ``max_repeat[li]``: the chunk's largest repeat count of step ``li`` (host
    integers, read before the loops).  ``trace``: receives (li, ai, states_last [B, R, 3], receivers, senders, count) per model call."""
    from diff_gaussian_rasterization import _hip
    B, T, n_obj = int(decoded.shape[0]), int(decoded.shape[1]), int(state.shape[0])
    R, dev, c = n_obj + 1, state.device, model.model_config
    a1, g1, _, _ = _sample_constants(model, n_obj, dev, torch.float32)
    zero_a, zero_g = torch.zeros((1, a1.shape[1]), device=dev), torch.zeros((1, 1), device=dev)
    a = torch.cat([a1.repeat(B, 1), zero_a], 0).contiguous()                             # [B R + 1, A]: the dummy row's are zero
    g = torch.cat([g1.repeat(B, 1), zero_g], 0).contiguous()
    n_valid = torch.full((1,), n_obj, dtype=torch.int32, device=dev)
    e_cap = _hip.plan_edge_capacity(B, n_obj, topk)
    repeat = repeat.contiguous()
    out = torch.zeros((B, T, n_obj, 3), dtype=torch.float32, device=dev)
    hist = torch.empty((B, n_his, n_obj, 3), dtype=torch.float32, device=dev)
    eef_hist = torch.empty((B, n_his, 3), dtype=torch.float32, device=dev)
    delta = torch.zeros((B, 3), dtype=torch.float32, device=dev)
    for li in range(T):
        prev = state[None].expand(B, -1, -1) if li == 0 else out[:, li - 1]
        hist.copy_(prev[:, None].expand(-1, n_his, -1, -1))
        eef_hist[:, :, :2] = decoded[:, li, None, :2]
        eef_hist[:, :, 2] = prev[:, :, 2].min(dim=1).values[:, None]
        delta[:, :2] = decoded[:, li, 2:4] - decoded[:, li, 0:2]
        for ai in range(1, max_repeat[li] + 1):
            _, p_in, nodes, last = _hip.plan_step_head(hist, eef_hist, delta, a, g.view(-1), c["state_dim"] == 3)
            recv, send, cnt, rows = _hip.construct_edges_batch(last, n_valid, adj_thresh, topk, e_cap)
            if trace is not None:
                trace.append((li, ai, last.clone(), recv, send, cnt))
            _, mot = model._propagate_split(None, a, g, None, recv, send, dummy_last_row=True, p_in=p_in, nodes=nodes, row_start=rows, motion_only=True)
            _hip.plan_step_tail(mot.contiguous(), delta, repeat, hist, eef_hist, out, ai, li, model.motion_clamp)
    return out


@torch.no_grad()
def rollout_actions(model: DynamicsPredictor, state: torch.Tensor, actions: torch.Tensor, *, push_length: float, adj_thresh: float, topk: int = 5,
                    n_his: int = 3, chunk: int = 1000, _trace: list = None) -> Dict[str, torch.Tensor]:
    """state [n_obj, 3], actions [B, T, 4] -> {"state_seqs": [B, T, n_obj, 3], "action_seqs": [B, T, 4]} (module docstring).  ``chunk``
    splits B as the reference's planner does; the results are concatenated, and a sample's result does not depend on the chunking beyond
    the fp32 summation order of the matrix products.  ``repeat < 1`` anywhere is a ``ValueError``."""
    if state.dim() != 2 or state.shape[1] != 3 or actions.dim() != 3 or actions.shape[2] != 4:
        raise ValueError("rollout_actions: state [n_obj, 3] and actions [B, T, 4], please")
    if int(model.model_config["n_his"]) != int(n_his):
        raise ValueError(f"rollout_actions: n_his = {n_his}, the model was built for {model.model_config['n_his']}")
    if actions.device != state.device:
        raise ValueError("rollout_actions: state and actions on one device, please")
    B, T, n_obj = int(actions.shape[0]), int(actions.shape[1]), int(state.shape[0])
    chunk = max(1, int(chunk))
    decoded, repeat = decode_action(actions, push_length)
    if B == 0 or T == 0:
        return {"state_seqs": torch.zeros((B, T, n_obj, 3), dtype=state.dtype, device=state.device), "action_seqs": decoded}
    device_path = _device_path_ok(model, state, n_obj) and decoded.dtype == torch.float32
    bounds = [(s, min(s + chunk, B)) for s in range(0, B, chunk)]
    if device_path:
        # the ONE host read of the call: the smallest repeat count, and every chunk's largest per look-ahead step (the loop bounds)
        stats = torch.cat([repeat.amin().view(1)] + [repeat[s:e].amax(0) for s, e in bounds]).cpu().tolist()
        lo, maxes = stats[0], [stats[1 + k * T:1 + (k + 1) * T] for k in range(len(bounds))]
    else:
        repeat_host = repeat.cpu().tolist()
        lo = min(min(r) for r in repeat_host)
    if lo < 1:
        raise ValueError(f"rollout_actions: every action must repeat at least once (int(length) >= 1), found {lo}")
    parts = []
    for k, (s, e) in enumerate(bounds):
        tr = None
        if _trace is not None:
            tr = []
            _trace.append((s, e, tr))
        if device_path:
            parts.append(_rollout_device(model, state.contiguous(), decoded[s:e].contiguous(), repeat[s:e], maxes[k], adj_thresh, topk, n_his, tr))
        else:
            parts.append(_rollout_reference(model, state, decoded[s:e], repeat_host[s:e], adj_thresh, topk, n_his, tr))
    return {"state_seqs": torch.cat(parts, 0), "action_seqs": decoded}


# ------------------------------------------------------------------------------------------ cost
def _box4(bbox, dev, dtype) -> torch.Tensor:
    """The reference's bounding box ([>= 2, >= 2]: rows x, y; columns lo, hi; tensor or numpy) -> (x_lo, x_hi, y_lo, y_hi) on ``dev``: sliced
    and moved, never read."""
    return torch.as_tensor(bbox)[:2, :2].to(device=dev, dtype=dtype).reshape(4)


def _running_cost_reference(state_seqs: torch.Tensor, actions: torch.Tensor, state_cur: torch.Tensor, target: torch.Tensor, box: torch.Tensor,
                            pusher_size: float, sharpness: float, penalty_weight: float):
    """The semantic definition in plain torch, any dtype (``box`` = (x_lo, x_hi, y_lo, y_hi)).  The [b, M, n_obj] distance table is built for
    slices of B that keep it below ``COST_TABLE_ENTRIES``."""
    B, T, n_obj = state_seqs.shape[0], state_seqs.shape[1], state_seqs.shape[2]
    M = target.shape[0]
    last = state_seqs[:, T - 1]
    step = max(1, COST_TABLE_ENTRIES // max(1, M * n_obj))
    parts = []
    for s in range(0, B, step):
        P = last[s:s + step]                                                         # [b, n_obj, 3]
        d2 = sum((target[None, :, None, c] - P[:, None, :, c]) ** 2 for c in range(3))   # [b, M, n_obj]: the minimum on the square, the root after
        parts.append(d2.min(dim=2).values.sqrt().mean(dim=1) + d2.min(dim=1).values.sqrt().mean(dim=1))
    chamfer = torch.cat(parts, 0)
    frames = torch.cat([state_cur[None, None, :, :2].expand(B, 1, n_obj, 2), state_seqs[:, :T - 1, :, :2]], 1)   # [B, T, n_obj, 2]: the state a push meets
    d2 = ((actions[:, :, None, :2] - frames) ** 2).sum(-1).min(dim=2).values
    zero = torch.zeros((), dtype=state_seqs.dtype, device=state_seqs.device)
    collision = torch.exp(-sharpness * torch.maximum(d2.sqrt() - pusher_size, zero))
    lo, hi = state_seqs.min(dim=2).values, state_seqs.max(dim=2).values              # [B, T, 3]
    margins = torch.stack([lo[..., 0] - box[0], box[1] - hi[..., 0], lo[..., 1] - box[2], box[3] - hi[..., 1]], -1)
    box_pen = torch.exp(-sharpness * torch.maximum(margins, zero)).max(dim=-1).values
    reward = -chamfer - penalty_weight * collision.mean(dim=1) - penalty_weight * box_pen.mean(dim=1)
    return reward, chamfer, collision, box_pen


def _cost_device_ok(*tensors) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 and t.device == tensors[0].device for t in tensors)


@torch.no_grad()
def running_cost(state_seqs: torch.Tensor, actions: torch.Tensor, state_cur: torch.Tensor, target: torch.Tensor, bbox, *, pusher_size: float = 0.01,
                 sharpness: float = 100.0, penalty_weight: float = 5.0) -> Dict[str, torch.Tensor]:
    """state_seqs [B, T, n_obj, 3], actions [B, T, 4] (columns 0, 1: the push's start point), state_cur [n_obj, 3], target [M, 3], bbox [>= 2,
    >= 2] (rows x, y; columns lo, hi; tensor or numpy) -> {"reward_seqs" [B], "chamfer" [B], "collision" [B, T], "box" [B, T]}:
      chamfer   = mean_m min_n |target_m - P_n| + mean_n min_m |target_m - P_n| with P the LAST look-ahead state;
      collision = exp(-sharpness max(min_n |start_t - Q_n| - pusher_size, 0)), Q the xy of the state push t meets (state_cur, then step t - 1);
      box       = max over the four walls of exp(-sharpness max(margin, 0)): 1 at or beyond a wall (the reference's rule, restated);
      reward    = -chamfer - penalty_weight mean_t collision - penalty_weight mean_t box.
    Minima and maxima keep a NaN: a diverged sample's reward is NaN.  float32 tensors on a HIP device with at most 1024 particles take
    gsr_plan_cost (one launch, no host read, bit-identical from run to run); everything else ``_running_cost_reference``."""
    if (state_seqs.dim() != 4 or state_seqs.shape[3] != 3 or actions.dim() != 3 or actions.shape[2] != 4 or actions.shape[:2] != state_seqs.shape[:2]
            or tuple(state_cur.shape) != (state_seqs.shape[2], 3) or target.dim() != 2 or target.shape[1] != 3):
        raise ValueError("running_cost: state_seqs [B, T, n_obj, 3], actions [B, T, 4], state_cur [n_obj, 3] and target [M, 3], please")
    if min(state_seqs.shape[0], state_seqs.shape[1], state_seqs.shape[2], target.shape[0]) < 1:
        raise ValueError("running_cost: B, T, n_obj and M must be at least 1")
    box = _box4(bbox, state_seqs.device, state_seqs.dtype)
    if _cost_device_ok(state_seqs, actions, state_cur, target) and int(state_seqs.shape[2]) <= MAX_COST_PARTICLES:
        from diff_gaussian_rasterization import _hip
        r, ch, co, bp = _hip.plan_cost(state_seqs.contiguous(), actions.contiguous(), state_cur.contiguous(), target.contiguous(), box.contiguous(),
                                       pusher_size, sharpness, penalty_weight)
    else:
        r, ch, co, bp = _running_cost_reference(state_seqs, actions, state_cur, target.to(state_seqs.dtype), box, pusher_size, sharpness, penalty_weight)
    return {"reward_seqs": r, "chamfer": ch, "collision": co, "box": bp}


# ------------------------------------------------------------------------------------------ sampling and the update
def clip_actions(action: torch.Tensor, lower, upper) -> torch.Tensor:
    """The reference's clip (utils/plan_utils.py ``clip_actions``), restated exactly: column 0 through ((v + pi) mod 2 pi) - pi, then every column
    clamped to its limits.  Column 0 is x, not the angle -- a defect of the reference, harmless in a workspace
    narrower than +-pi, where it moves x by one rounding."""
    lower = torch.as_tensor(lower, dtype=action.dtype, device=action.device)
    upper = torch.as_tensor(upper, dtype=action.dtype, device=action.device)
    new = action.clone()
    new[..., 0] = ((action[..., 0] + math.pi) % (2 * math.pi)) - math.pi
    return torch.minimum(torch.maximum(new, lower), upper)


def _mppi_update_reference(act_seqs: torch.Tensor, rewards: torch.Tensor, reward_weight: float, lower, upper, push_length: float):
    """The semantic definition in plain torch, any dtype; the displacement form, as the kernel."""
    B = act_seqs.shape[0]
    nan = torch.isnan(rewards)
    hit = torch.where(nan.any(), nan, rewards == rewards.max())                    # a NaN counts as the maximum
    best = torch.where(hit, torch.arange(B, device=rewards.device), B).min()        # the lowest index that attains it
    rmax = rewards[best]
    e = torch.exp(reward_weight * (rewards - rmax))                                 # the subtraction first
    w = (e / e.sum())[:, None]
    x, y, th, ln = act_seqs[:, :, 0], act_seqs[:, :, 1], act_seqs[:, :, 2], act_seqs[:, :, 3]
    dx = (w * (ln * push_length * torch.cos(th))).sum(0)
    dy = (w * (ln * push_length * torch.sin(th))).sum(0)
    seq = torch.stack([(w * x).sum(0), (w * y).sum(0), torch.atan2(dy, dx), torch.hypot(dx, dy) / push_length], -1)
    return clip_actions(seq, lower, upper), best, rmax


@torch.no_grad()
def mppi_update(act_seqs: torch.Tensor, reward_seqs: torch.Tensor, *, reward_weight: float, lower, upper, push_length: float) -> Dict[str, torch.Tensor]:
    """act_seqs [B, T, 4] = (x, y, theta, length), reward_seqs [B] -> {"act_seq" [T, 4], "best_index" (int64 scalar), "best_reward" (scalar)}.
    best_index is the lowest b that attains the largest reward, a NaN counting as the largest (torch.argmax).  Weights w_b = softmax of
    reward_weight (r_b - r_best) -- the subtraction before the multiplication; per step x = sum w x, y = sum w y, the displacement (dx, dy) =
    sum w length push_length (cos theta, sin theta), theta = atan2(dy, dx), length = hypot(dx, dy) / push_length, then ``clip_actions``.  The
    reference sums the end points and differences the two sums: the same in exact arithmetic, a cancellation in floating point; the
    displacement is summed directly here, on both paths.  -inf rewards get weight 0; a NaN reward makes act_seq NaN.  float32 tensors on a HIP
    device take gsr_plan_mppi_update (one launch, no host read); everything else ``_mppi_update_reference``."""
    if act_seqs.dim() != 3 or act_seqs.shape[2] != 4 or tuple(reward_seqs.shape) != (act_seqs.shape[0],) or act_seqs.shape[0] < 1 or act_seqs.shape[1] < 1:
        raise ValueError("mppi_update: act_seqs [B, T, 4] and reward_seqs [B] with B, T >= 1, please")
    lower = torch.as_tensor(lower, dtype=act_seqs.dtype, device=act_seqs.device)
    upper = torch.as_tensor(upper, dtype=act_seqs.dtype, device=act_seqs.device)
    if _cost_device_ok(act_seqs, reward_seqs):
        from diff_gaussian_rasterization import _hip
        seq, best, rmax = _hip.plan_mppi_update(act_seqs.contiguous(), reward_seqs.contiguous(), reward_weight, push_length, lower.contiguous(),
                                                upper.contiguous())
        best, rmax = best.view(()), rmax.view(())
    else:
        seq, best, rmax = _mppi_update_reference(act_seqs, reward_seqs, reward_weight, lower, upper, push_length)
    return {"act_seq": seq, "best_index": best, "best_reward": rmax}


def sample_action_seq(act_seq: torch.Tensor, lower, upper, n_sample: int, *, iter_index: int, noise_level: float, push_length: float,
                      generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """act_seq [T, 4] -> [n_sample, T, 4], the reference's sampler (utils/plan_utils.py ``sample_action_seq``) restated.  Iteration 0 is
    uniform in the limits.  Later iterations perturb, per look-ahead step i, the push's start point and end point with 0.1 * 10^i * N(0,
    noise_level), re-derive angle and length from the two points and clip; sample 0 stays ``act_seq``.  The random numbers are drawn on the
    generator's device (``act_seq``'s without one) and moved, so one CPU generator gives the same samples on every device."""
    dev, dtype = act_seq.device, act_seq.dtype
    gdev = generator.device if generator is not None else dev
    lower = torch.as_tensor(lower, dtype=dtype, device=dev)
    upper = torch.as_tensor(upper, dtype=dtype, device=dev)
    if act_seq.dim() != 2 or act_seq.shape[1] != 4:
        raise ValueError("sample_action_seq: act_seq [T, 4] = (x, y, theta, length), please")
    T = act_seq.shape[0]
    if iter_index == 0:
        u = torch.rand((n_sample, T, 4), generator=generator, dtype=dtype, device=gdev).to(dev)
        return u * (upper - lower) + lower
    seqs = act_seq[None].repeat(n_sample, 1, 1)
    xs, ys, th, ln = seqs[:, :, 0], seqs[:, :, 1], seqs[:, :, 2], seqs[:, :, 3]
    x_ends = xs - ln * push_length * torch.cos(th)
    y_ends = ys - ln * push_length * torch.sin(th)
    for i in range(T):
        res = (0.1 * (10 ** i)) * (torch.randn((n_sample, 4), generator=generator, dtype=dtype, device=gdev) * noise_level).to(dev)
        x0, y0, x1, y1 = xs[:, i] + res[:, 0], ys[:, i] + res[:, 1], x_ends[:, i] + res[:, 2], y_ends[:, i] + res[:, 3]
        step = torch.stack([x0, y0, torch.atan2(y0 - y1, x0 - x1), torch.hypot(x1 - x0, y1 - y0) / push_length], -1)
        seqs[1:, i] = clip_actions(step, lower, upper)[1:]
    return seqs


@torch.no_grad()
def plan_actions(model: DynamicsPredictor, state: torch.Tensor, target: torch.Tensor, bbox, act_seq: torch.Tensor, *, lower, upper, push_length: float,
                 adj_thresh: float, n_sample: int = 10000, chunk: int = 1000, n_update_iter: int = 1, reward_weight: float = 500.0,
                 noise_level: float = 1.0, topk: int = 5, n_his: int = 3, rollout_best: bool = True,
                 generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """One planning step: the reference's ``trajectory_optimization_mppi`` per chunk of ``chunk`` samples and ``merge_res`` across the chunks
    (real_world/utils/planner.py).  state [n_obj, 3], target [M, 3], bbox as ``running_cost`` takes it, act_seq [T, 4] the initial push
    sequence -> {"act_seq" [T, 4], "reward" (scalar), "state_seqs" [T, n_obj, 3], "chunk_rewards" [n_chunk]}.
    Per chunk and iteration: ``sample_action_seq`` -> ``rollout_actions`` -> ``running_cost`` -> ``mppi_update``.  A chunk keeps the best
    SAMPLE it has seen; the weighted mean only seeds the next iteration's sampler, as in the reference.  ``rollout_best`` rolls that sample
    out once more at B = 1 and scores it (otherwise the sample's own rollout and reward stand); the chunk whose reward is largest wins.
    Host reads: the one ``rollout_actions`` makes per call for its loop bounds, and one at the very end to pick the chunk.  The cost and the
    update make none: the best sample is gathered by a device index and compared on the device.  Nothing is printed.
    A NaN reward ranks as the largest at every stage, as ``torch.argmax`` has it in the reference: one diverged sample makes its chunk's
    result, and then the call's, that sample with a NaN "reward" -- check the reward before acting on the push."""
    if act_seq.dim() != 2 or act_seq.shape[1] != 4:
        raise ValueError("plan_actions: act_seq [T, 4] = (x, y, theta, length), please")
    dev, dtype = state.device, state.dtype
    lower = torch.as_tensor(lower, dtype=dtype, device=dev)
    upper = torch.as_tensor(upper, dtype=dtype, device=dev)
    act_seq = act_seq.to(device=dev, dtype=dtype)
    target = target.to(device=dev, dtype=dtype)
    bbox = torch.as_tensor(bbox)[:2, :2].to(device=dev, dtype=dtype)          # moved once; ``running_cost`` then only reshapes it
    n_sample, chunk = int(n_sample), max(1, int(chunk))
    if n_sample < 1 or n_update_iter < 1:
        raise ValueError("plan_actions: n_sample and n_update_iter must be at least 1")
    roll = dict(push_length=push_length, adj_thresh=adj_thresh, topk=topk, n_his=n_his)
    seqs, rewards, states = [], [], []
    for s in range(0, n_sample, chunk):
        n = min(chunk, n_sample - s)
        seed, best = act_seq, None
        for it in range(int(n_update_iter)):
            acts = sample_action_seq(seed, lower, upper, n, iter_index=it, noise_level=noise_level, push_length=push_length, generator=generator)
            out = rollout_actions(model, state, acts, chunk=n, **roll)["state_seqs"]
            cost = running_cost(out, acts, state, target, bbox)
            upd = mppi_update(acts, cost["reward_seqs"], reward_weight=reward_weight, lower=lower, upper=upper, push_length=push_length)
            seed = upd["act_seq"]
            idx = upd["best_index"].view(1)
            cand = (acts.index_select(0, idx)[0], upd["best_reward"], out.index_select(0, idx)[0])
            if best is None:
                best = cand
            else:
                take = cand[1] > best[1]
                best = tuple(torch.where(take, c, o) for c, o in zip(cand, best))
        seq, reward, st = best
        if rollout_best:
            st = rollout_actions(model, state, seq[None], chunk=1, **roll)["state_seqs"]
            reward = running_cost(st, seq[None], state, target, bbox)["reward_seqs"][0]
            st = st[0]
        seqs.append(seq)
        rewards.append(reward)
        states.append(st)
    chunk_rewards = torch.stack(rewards)
    win = int(torch.argmax(chunk_rewards))                  # the one host read of the cost / update side: which chunk won
    return {"act_seq": seqs[win], "reward": chunk_rewards[win], "state_seqs": states[win], "chunk_rewards": chunk_rewards}
