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

The gradient planner (the reference's planner type 'GD'; the last section of this file): ``rollout_actions_grad`` is the rollout with an
autograd graph to the pushes and the model's parameters, ``running_cost_grad`` the cost with a DEFINED gradient -- on a HIP device values and
gradients in one launch, gsr_plan_cost_grad (csrc/gsr_plan_cost_grad.hip) --, ``plan_actions_gd`` the loop: Adam on the candidates, clip,
the best candidate seen.
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
                       topk: int, n_his: int, trace: list = None, detach_steps: bool = False) -> torch.Tensor:
    """The semantic definition: one sample at a time, ``construct_edges`` + ``model._propagate`` per model call.  A sample runs exactly its
    own ``repeat`` calls per look-ahead step (the calls the reference makes beyond that are discarded by it).  ``trace``: a list that
    receives (sample, li, ai, newest positions [R, 3], receivers, senders) per model call.  Run under ``enable_grad`` it is also the
    definition of the differentiable rollout (``rollout_actions_grad``); ``detach_steps`` then starts look-ahead step li from the DETACHED
    state of li - 1, the reference's rule (values unchanged)."""
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
            prev = pred.detach() if detach_steps else pred
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


# ------------------------------------------------------------------------------------------ the gradient planner
# The reference's planner has a 'GD' type (utils/planner.py ``trajectory_optimization_gd``: Adam on the sampled pushes, loss = -mean reward).
# Its own model function is decorated ``no_grad`` and detaches the state between look-ahead steps, so it cannot be run against it; the
# differentiable rollout is therefore defined HERE: ``_rollout_reference`` under autograd (``detach_steps=True`` is the reference's detach).
def _first_arg(v: torch.Tensor, dim: int, largest: bool = False) -> torch.Tensor:
    """The LOWEST index along ``dim`` that attains the minimum (maximum), a NaN counting as the extreme (torch.min / torch.max keep it):
    ``torch.argmax`` of a mask returns the first."""
    nan = torch.isnan(v)
    ext = (v.max(dim=dim, keepdim=True) if largest else v.min(dim=dim, keepdim=True)).values
    hit = torch.where(nan.any(dim=dim, keepdim=True), nan, v == ext)
    return hit.to(torch.uint8).argmax(dim=dim)


def _root0(d2: torch.Tensor) -> torch.Tensor:
    """sqrt whose gradient at zero is zero (the subgradient torch.norm uses) instead of inf; a NaN stays."""
    zero = d2 == 0
    return torch.where(zero, torch.zeros((), dtype=d2.dtype, device=d2.device), torch.sqrt(torch.where(zero, torch.ones((), dtype=d2.dtype, device=d2.device), d2)))


def _gate(x: torch.Tensor) -> torch.Tensor:
    """max(x, 0) that keeps a NaN and is open iff x > 0 (torch.maximum splits the gradient at x = 0)."""
    return torch.where(x <= 0, torch.zeros((), dtype=x.dtype, device=x.device), x)


class _PoisonRows(torch.autograd.Function):
    """reward -> reward; toward ``state_seqs`` and ``actions`` it sends NaN into every row of a sample whose reward is not finite (and +0 into
    the others): the definition's rule for diverged samples, which plain autograd would spread over some rows only."""

    @staticmethod
    def forward(ctx, reward, state_seqs, actions):
        ctx.save_for_backward(reward)
        ctx.shapes = (state_seqs.shape, actions.shape)
        return reward.clone()

    @staticmethod
    def backward(ctx, d_reward):
        (reward,) = ctx.saved_tensors
        bad = ~torch.isfinite(reward)
        fill = torch.where(bad, torch.full_like(reward, math.nan), torch.zeros_like(reward))
        s_shape, a_shape = ctx.shapes
        return d_reward, fill[:, None, None, None].expand(s_shape), fill[:, None, None].expand(a_shape)


def _running_cost_grad_reference(state_seqs: torch.Tensor, actions: torch.Tensor, state_cur: torch.Tensor, target: torch.Tensor, box: torch.Tensor,
                                 pusher_size: float, sharpness: float, penalty_weight: float):
    """The definition of the cost's gradient (include/gsr.h, gsr_plan_cost_grad) in plain torch, any dtype; the values are
    ``_running_cost_reference``'s.  Every minimum / maximum is resolved to ONE index -- the lowest among equal values -- under ``no_grad``
    (the [b, M, n_obj] table in slices of B, as the fallback builds it); the chosen points are gathered and only the O(B (M + n_obj))
    distances between them go through autograd.  A zero distance has a zero gradient; the collision and box gates are open iff their
    argument is > 0; a sample whose reward is not finite sends NaN into all its rows."""
    B, T, n_obj = state_seqs.shape[0], state_seqs.shape[1], state_seqs.shape[2]
    M = target.shape[0]
    last = state_seqs[:, T - 1]
    with torch.no_grad():
        step = max(1, COST_TABLE_ENTRIES // max(1, M * n_obj))
        near_p, near_t = [], []
        for s in range(0, B, step):
            P = last[s:s + step]
            d2 = sum((target[None, :, None, c] - P[:, None, :, c]) ** 2 for c in range(3))   # [b, M, n_obj]
            near_p.append(_first_arg(d2, 2))                                         # [b, M]: target m's nearest particle
            near_t.append(_first_arg(d2, 1))                                         # [b, n_obj]: particle n's nearest target
        near_p, near_t = torch.cat(near_p, 0), torch.cat(near_t, 0)
    Pn = last.gather(1, near_p[:, :, None].expand(-1, -1, 3))                        # [B, M, 3]
    Qn = target[near_t]                                                              # [B, n_obj, 3]
    d_a = _root0(sum((target[None, :, c] - Pn[:, :, c]) ** 2 for c in range(3)))
    d_b = _root0(sum((Qn[:, :, c] - last[:, :, c]) ** 2 for c in range(3)))
    chamfer = d_a.mean(dim=1) + d_b.mean(dim=1)
    frames = torch.cat([state_cur[None, None, :, :2].expand(B, 1, n_obj, 2), state_seqs[:, :T - 1, :, :2]], 1)   # [B, T, n_obj, 2]
    with torch.no_grad():
        hit = _first_arg(((actions[:, :, None, :2] - frames) ** 2).sum(-1), 2)       # [B, T]
    q = frames.gather(2, hit[:, :, None, None].expand(-1, -1, 1, 2))[:, :, 0]        # [B, T, 2]
    collision = torch.exp(-sharpness * _gate(_root0(((actions[:, :, :2] - q) ** 2).sum(-1)) - pusher_size))
    x, y = state_seqs[..., 0], state_seqs[..., 1]                                    # [B, T, n_obj]
    with torch.no_grad():
        ix = [_first_arg(x, 2), _first_arg(x, 2, largest=True), _first_arg(y, 2), _first_arg(y, 2, largest=True)]
    pick = lambda v, i: v.gather(2, i[:, :, None])[:, :, 0]  # noqa: E731
    margins = torch.stack([pick(x, ix[0]) - box[0], box[1] - pick(x, ix[1]), pick(y, ix[2]) - box[2], box[3] - pick(y, ix[3])], -1)
    e = torch.exp(-sharpness * _gate(margins))                                       # [B, T, 4]
    with torch.no_grad():
        wall = _first_arg(e, 2, largest=True)
    box_pen = e.gather(2, wall[:, :, None])[:, :, 0]
    reward = -chamfer - penalty_weight * collision.mean(dim=1) - penalty_weight * box_pen.mean(dim=1)
    if state_seqs.requires_grad or actions.requires_grad:
        reward = _PoisonRows.apply(reward, state_seqs, actions)
    return reward, chamfer.detach(), collision.detach(), box_pen.detach()


class _PlanCostGrad(torch.autograd.Function):
    """gsr_plan_cost_grad: the four values and, saved for the backward, the per-sample gradients; the backward scales row b by d_reward[b]."""

    @staticmethod
    def forward(ctx, state_seqs, actions, state_cur, target, box, pusher_size, sharpness, penalty_weight):
        from diff_gaussian_rasterization import _hip
        r, ch, co, bp, g_state, g_act = _hip.plan_cost_grad(state_seqs.contiguous(), actions.contiguous(), state_cur.contiguous(), target.contiguous(),
                                                            box.contiguous(), pusher_size, sharpness, penalty_weight)
        ctx.save_for_backward(g_state, g_act)
        ctx.mark_non_differentiable(ch, co, bp)
        return r, ch, co, bp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_reward, *_):
        g_state, g_act = ctx.saved_tensors
        return g_state * d_reward[:, None, None, None], g_act * d_reward[:, None, None], None, None, None, None, None, None


def running_cost_grad(state_seqs: torch.Tensor, actions: torch.Tensor, state_cur: torch.Tensor, target: torch.Tensor, bbox, *, pusher_size: float = 0.01,
                      sharpness: float = 100.0, penalty_weight: float = 5.0) -> Dict[str, torch.Tensor]:
    """``running_cost`` with a gradient: the same dictionary, the same values; "reward_seqs" carries an autograd graph to ``state_seqs`` and
    ``actions`` (columns 0, 1; columns 2, 3 receive zeros from the cost -- their gradient comes through the rollout), the other three
    entries are detached.  The gradient is DEFINED (include/gsr.h, gsr_plan_cost_grad; ``_running_cost_grad_reference`` states it in torch):
    every minimum and maximum hands its gradient to the lowest index among equal values, a zero distance contributes a zero vector and
    never a NaN, the collision and box gates are open iff their argument is > 0, and a sample whose reward is not finite gets NaN in all
    its rows.  float32 tensors on a HIP device with at most 1024 particles take gsr_plan_cost_grad -- values and gradients in one launch,
    no [B, M, n_obj] table, once differentiable, bit-identical from run to run; everything else (CPU tensors, other dtypes, a ``state_cur``,
    ``target`` or ``bbox`` that requires a gradient) takes the torch statement."""
    if (state_seqs.dim() != 4 or state_seqs.shape[3] != 3 or actions.dim() != 3 or actions.shape[2] != 4 or actions.shape[:2] != state_seqs.shape[:2]
            or tuple(state_cur.shape) != (state_seqs.shape[2], 3) or target.dim() != 2 or target.shape[1] != 3):
        raise ValueError("running_cost_grad: state_seqs [B, T, n_obj, 3], actions [B, T, 4], state_cur [n_obj, 3] and target [M, 3], please")
    if min(state_seqs.shape[0], state_seqs.shape[1], state_seqs.shape[2], target.shape[0]) < 1:
        raise ValueError("running_cost_grad: B, T, n_obj and M must be at least 1")
    box = _box4(bbox, state_seqs.device, state_seqs.dtype)
    side_grad = state_cur.requires_grad or target.requires_grad or box.requires_grad
    if _cost_device_ok(state_seqs, actions, state_cur, target) and int(state_seqs.shape[2]) <= MAX_COST_PARTICLES and not side_grad:
        r, ch, co, bp = _PlanCostGrad.apply(state_seqs, actions, state_cur, target, box, pusher_size, sharpness, penalty_weight)
    else:
        r, ch, co, bp = _running_cost_grad_reference(state_seqs, actions, state_cur, target.to(state_seqs.dtype), box, pusher_size, sharpness,
                                                     penalty_weight)
    return {"reward_seqs": r, "chamfer": ch, "collision": co, "box": bp}


def _batched_call_grad(model: DynamicsPredictor, states: List[torch.Tensor], delta: torch.Tensor, a: torch.Tensor, g: torch.Tensor,
                       n_valid: torch.Tensor, adj_thresh: float, topk: int, e_cap: int):
    """ONE differentiable model call for all samples: states = n_his frames [B, R, 3] (each sample's tool row last), delta [B, 3] the tool's
    motion, a / g the constant rows [B R + 1, .] -> (predicted positions [B, R, 3], (receivers, senders, count, row_start)).  The B graphs
    are one block-diagonal graph (sample b owns the rows b R .. b R + R - 1, one zero dummy row last collects the padded relations); the
    relations come from gsr_construct_edges_batch on the DETACHED newest frame -- relations are discrete -- and the network is
    ``propagate_split_grad``.  The sender-side reverse list is built with a stable sort and a search: no host read."""
    from diff_gaussian_rasterization import _hip
    from .dynamics import SplitGraph
    B, R, dev = int(delta.shape[0]), int(states[0].shape[1]), delta.device
    N = B * R + 1
    state_t = torch.cat([torch.cat(states, 2).reshape(B * R, 3 * len(states)), torch.zeros((1, 3 * len(states)), device=dev)], 0)
    act = torch.cat([torch.cat([torch.zeros((B, R - 1, 3), device=dev), delta[:, None]], 1).reshape(B * R, 3), torch.zeros((1, 3), device=dev)], 0)
    recv, send, cnt, rows = _hip.construct_edges_batch(states[-1].detach().contiguous(), n_valid, adj_thresh, topk, e_cap)
    order = torch.argsort(send, stable=True)
    rev_ptr = torch.searchsorted(send[order].contiguous(), torch.arange(N + 1, device=dev, dtype=torch.int64))
    graph = SplitGraph(recv, send, rows, rev_ptr, order.contiguous())
    pos, _ = model.propagate_split_grad(state_t, a, g, act, graph, dummy_last_row=True)
    return pos[:B * R].view(B, R, 3), (recv, send, cnt, rows)


def _batched_constants(model: DynamicsPredictor, B: int, n_obj: int, topk: int, dev):
    """The constant rows of B samples and the dummy row, the valid count and the relation capacity of ``_batched_call_grad``."""
    from diff_gaussian_rasterization import _hip
    a1, g1, _, _ = _sample_constants(model, n_obj, dev, torch.float32)
    a = torch.cat([a1.repeat(B, 1), torch.zeros((1, a1.shape[1]), device=dev)], 0).contiguous()
    g = torch.cat([g1.repeat(B, 1), torch.zeros((1, 1), device=dev)], 0).contiguous()
    return a, g, torch.full((1,), n_obj, dtype=torch.int32, device=dev), _hip.plan_edge_capacity(B, n_obj, topk)


def _rollout_device_grad(model: DynamicsPredictor, state: torch.Tensor, decoded: torch.Tensor, repeat: torch.Tensor, max_repeat: List[int],
                         adj_thresh: float, topk: int, n_his: int, detach_steps: bool, trace: list = None) -> torch.Tensor:
    """``_rollout_device``'s structure with the glue as differentiable torch operations around ``_batched_call_grad``.  No host read inside
    the loops.  ``trace``: receives (li, ai, newest frame [B, R, 3], receivers, senders, count) per model call."""
    B, T, n_obj = int(decoded.shape[0]), int(decoded.shape[1]), int(state.shape[0])
    dev = state.device
    a, g, n_valid, e_cap = _batched_constants(model, B, n_obj, topk, dev)
    zero_col = torch.zeros((B, 1), device=dev)
    outs, prev = [], state[None].expand(B, -1, -1)
    for li in range(T):
        hist = [prev] * n_his                                                        # each [B, n_obj, 3]
        eef = [torch.cat([decoded[:, li, :2], prev[:, :, 2].min(dim=1).values[:, None]], 1)] * n_his      # each [B, 3]
        delta = torch.cat([decoded[:, li, 2:4] - decoded[:, li, 0:2], zero_col], 1)  # [B, 3]
        out_li = torch.zeros((B, n_obj, 3), device=dev)
        for ai in range(1, max_repeat[li] + 1):
            states = [torch.cat([h, e[:, None]], 1) for h, e in zip(hist, eef)]      # n_his x [B, R, 3], the tool last
            pos, (recv, send, cnt, _) = _batched_call_grad(model, states, delta, a, g, n_valid, adj_thresh, topk, e_cap)
            if trace is not None:
                trace.append((li, ai, states[-1].detach().clone(), recv, send, cnt))
            pred = pos[:, :n_obj]
            out_li = torch.where((repeat[:, li] == ai)[:, None, None], pred, out_li)
            hist = hist[1:] + [pred]
            eef = eef[1:] + [torch.cat([eef[-1][:, :2] + delta[:, :2], pred[:, :, 2].min(dim=1).values[:, None]], 1)]
        outs.append(out_li)
        prev = out_li.detach() if detach_steps else out_li
    return torch.stack(outs, 1)


def _grad_device_path_ok(model: DynamicsPredictor, probe: torch.Tensor, n_obj: int) -> bool:
    """``_device_path_ok`` for the differentiable rollout: ``split_grad_ok`` in place of the inference condition."""
    c = model.model_config
    return bool(model.split_grad_ok(probe) and model.motion_dim == 0 and c["state_dim"] in (0, 3) and c["action_dim"] == 3 and c["attr_dim"] >= 2
                and 1 <= int(n_obj) <= MAX_DEVICE_PARTICLES)


def rollout_actions_grad(model: DynamicsPredictor, state: torch.Tensor, actions: torch.Tensor, *, push_length: float, adj_thresh: float, topk: int = 5,
                         n_his: int = 3, detach_steps: bool = False, device_path: Optional[bool] = None, _trace: list = None) -> Dict[str, torch.Tensor]:
    """``rollout_actions`` with a gradient: state [n_obj, 3], actions [B, T, 4] -> {"state_seqs": [B, T, n_obj, 3], "action_seqs": [B, T, 4]}
    with an autograd graph to ``actions`` (columns 0 - 2; ``repeat = int(length)`` has none) and to the model's parameters.  The DEFINITION
    is ``_rollout_reference`` run under ``enable_grad``: the reference's own model function is ``no_grad`` and detaches the state between
    look-ahead steps, so its GD planner cannot run against it -- a departure by necessity.  ``detach_steps=True`` is the reference's rule:
    look-ahead step li starts from the detached state of li - 1 (values unchanged).  The relations are discrete: they are built from the
    detached newest positions; the tool's z follows the lowest particle through its arg-min.  No chunking: the caller chunks (activations
    grow with B times the sum of the repeat counts).
    ``device_path``: None -- the batched device path (``_rollout_device_grad``: one ``propagate_split_grad`` call for all samples per model
    call, no host read inside the loops) wherever it can run: float32 on a HIP device, a model the split path accepts, at most 127
    particles; the definition everywhere else.  True asks for the device path and raises where it cannot run; False is the definition."""
    if state.dim() != 2 or state.shape[1] != 3 or actions.dim() != 3 or actions.shape[2] != 4:
        raise ValueError("rollout_actions_grad: state [n_obj, 3] and actions [B, T, 4], please")
    if int(model.model_config["n_his"]) != int(n_his):
        raise ValueError(f"rollout_actions_grad: n_his = {n_his}, the model was built for {model.model_config['n_his']}")
    if actions.device != state.device:
        raise ValueError("rollout_actions_grad: state and actions on one device, please")
    B, T, n_obj = int(actions.shape[0]), int(actions.shape[1]), int(state.shape[0])
    with torch.enable_grad():
        decoded, repeat = decode_action(actions, push_length)
        if B == 0 or T == 0:
            return {"state_seqs": torch.zeros((B, T, n_obj, 3), dtype=state.dtype, device=state.device), "action_seqs": decoded}
        can = _grad_device_path_ok(model, state, n_obj) and decoded.dtype == torch.float32
        if device_path and not can:
            raise RuntimeError("rollout_actions_grad: the device path needs float32 on a HIP device, a model the split path accepts and at most "
                               f"{MAX_DEVICE_PARTICLES} particles")
        use_device = can if device_path is None else bool(device_path)
        if use_device:
            stats = torch.cat([repeat.amin().view(1), repeat.amax(0)]).cpu().tolist()    # the ONE host read: the loop bounds
            lo, maxes = stats[0], stats[1:]
        else:
            repeat_host = repeat.cpu().tolist()
            lo = min(min(r) for r in repeat_host)
        if lo < 1:
            raise ValueError(f"rollout_actions_grad: every action must repeat at least once (int(length) >= 1), found {lo}")
        if use_device:
            out = _rollout_device_grad(model, state.contiguous(), decoded, repeat, maxes, adj_thresh, topk, n_his, detach_steps, _trace)
        else:
            out = _rollout_reference(model, state, decoded, repeat_host, adj_thresh, topk, n_his, _trace, detach_steps=detach_steps)
    return {"state_seqs": out, "action_seqs": decoded}


def _best_index(rewards: torch.Tensor) -> torch.Tensor:
    """The lowest b that attains the largest reward, a NaN counting as the largest -- ``mppi_update``'s ranking; no host read."""
    return _first_arg(rewards, 0, largest=True)


def plan_actions_gd(model: DynamicsPredictor, state: torch.Tensor, target: torch.Tensor, bbox, act_seq: torch.Tensor, *, lower, upper, push_length: float,
                    adj_thresh: float, n_sample: int = 32, n_update_iter: int = 10, lr: float = 1e-3, init: Optional[torch.Tensor] = None, topk: int = 5,
                    n_his: int = 3, detach_steps: bool = False, rollout_best: bool = True,
                    generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """The reference's ``trajectory_optimization_gd`` (utils/planner.py, planner type 'GD') for one chunk: Adam on B candidate push sequences
    with loss = -sum(reward) / B, ``clip_actions`` after every step, the best candidate returned.  state [n_obj, 3], target [M, 3], bbox as
    ``running_cost`` takes it, act_seq [T, 4] -> {"act_seq" [T, 4], "reward" (scalar), "state_seqs" [T, n_obj, 3], "reward_history"
    [n_update_iter]: the best reward seen up to each iteration}.
    The candidates are ``init`` ([B, T, 4] -- for instance MPPI's best samples, to refine them) or ``sample_action_seq(act_seq, ...,
    iter_index=0)`` with ``n_sample`` rows.  Per iteration: ``rollout_actions_grad`` -> ``running_cost_grad`` -> the gradient toward the
    candidates only (the model's parameters accumulate nothing) -> non-finite gradient rows set to zero on the device -> Adam(lr, betas =
    (0.9, 0.999)) -> ``clip_actions``.  The length column receives a zero gradient (``repeat = int(length)``) and Adam leaves it where it is.
    Two stated departures from the reference.  It keeps the best (sample, reward, rollout) seen AT EVALUATION TIME, ranked as
    ``plan_actions`` ranks (the lowest index among equals, a NaN as the largest); the reference indexes the stepped actions with the
    pre-step rewards.  And the differentiable rollout is defined here (``rollout_actions_grad``); ``detach_steps=True`` is the reference's
    detach between look-ahead steps.  The last iteration's step could never be evaluated and is not taken.
    ``rollout_best`` as in ``plan_actions``.  Host reads: the one ``rollout_actions_grad`` makes per call for its loop bounds; the ranking and
    the gradient clean-up make none.  Nothing is printed."""
    if act_seq.dim() != 2 or act_seq.shape[1] != 4:
        raise ValueError("plan_actions_gd: act_seq [T, 4] = (x, y, theta, length), please")
    if int(n_update_iter) < 1:
        raise ValueError("plan_actions_gd: n_update_iter must be at least 1")
    dev, dtype = state.device, state.dtype
    lower = torch.as_tensor(lower, dtype=dtype, device=dev)
    upper = torch.as_tensor(upper, dtype=dtype, device=dev)
    act_seq = act_seq.to(device=dev, dtype=dtype)
    target = target.to(device=dev, dtype=dtype)
    bbox = torch.as_tensor(bbox)[:2, :2].to(device=dev, dtype=dtype)
    if init is not None:
        if init.dim() != 3 or init.shape[1:] != act_seq.shape or init.shape[0] < 1:
            raise ValueError("plan_actions_gd: init [B, T, 4] with act_seq's T, please")
        acts = init.detach().to(device=dev, dtype=dtype).clone()
    else:
        if int(n_sample) < 1:
            raise ValueError("plan_actions_gd: n_sample must be at least 1")
        acts = sample_action_seq(act_seq, lower, upper, int(n_sample), iter_index=0, noise_level=1.0, push_length=push_length, generator=generator)
    acts = acts.contiguous().requires_grad_(True)
    B = int(acts.shape[0])
    opt = torch.optim.Adam([acts], lr=lr, betas=(0.9, 0.999))
    roll = dict(push_length=push_length, adj_thresh=adj_thresh, topk=topk, n_his=n_his)
    best, history = None, []
    for it in range(int(n_update_iter)):
        final = it == int(n_update_iter) - 1
        with torch.set_grad_enabled(not final):
            out = rollout_actions_grad(model, state, acts, detach_steps=detach_steps, **roll)["state_seqs"] if not final else \
                rollout_actions(model, state, acts.detach(), chunk=B, **roll)["state_seqs"]
            cost = running_cost_grad(out, acts, state, target, bbox) if not final else running_cost(out, acts.detach(), state, target, bbox)
        rewards = cost["reward_seqs"]
        with torch.no_grad():
            idx = _best_index(rewards.detach()).view(1)
            cand = (acts.detach().index_select(0, idx)[0].clone(), rewards.detach().index_select(0, idx)[0], out.detach().index_select(0, idx)[0])
            if best is None:
                best = cand
            else:
                take = cand[1] > best[1]
                best = tuple(torch.where(take, c, o) for c, o in zip(cand, best))
            history.append(best[1])
        if final:
            break
        (grad,) = torch.autograd.grad(-rewards.sum() / B, acts)
        with torch.no_grad():
            ok = torch.isfinite(grad).all(dim=2).all(dim=1)[:, None, None]
            acts.grad = torch.where(ok, grad, torch.zeros_like(grad))
        opt.step()
        with torch.no_grad():
            acts.data.copy_(clip_actions(acts.data, lower, upper))
    seq, reward, st = best
    if rollout_best:
        with torch.no_grad():
            st = rollout_actions(model, state, seq[None], chunk=1, **roll)["state_seqs"]
            reward = running_cost(st, seq[None], state, target, bbox)["reward_seqs"][0]
            st = st[0]
    return {"act_seq": seq, "reward": reward, "state_seqs": st, "reward_history": torch.stack(history)}
