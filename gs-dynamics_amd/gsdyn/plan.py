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
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from .dynamics import DynamicsPredictor, construct_edges

MAX_DEVICE_PARTICLES = 127          # gsr_construct_edges_batch: a sample's objects + tool fit two 64-lane ballots


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
