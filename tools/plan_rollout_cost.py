"""The cost of the planner's rollout (profiles/plan_rollout_cost.txt): ``gsdyn.rollout_actions`` at the reference planner's shape -- one chunk
of B = 1000 action samples, 100 particles, T = 3 look-ahead steps, repeat counts 1 .. 5, the rope.yaml widths (512) -- on the batched HIP
path, against the two ways the tree could serve it before:
  (a) a Python loop over the samples, each through the single-graph path (``DynamicsPredictor.forward`` with index-form relations, its
      propagation replayed from a hipGraph) -- timed on the first ``--loop-samples`` samples and scaled to B;
  (b) the dense ``B > 1`` ``forward`` (one-hot ``Rr / Rs``, batched gathers and ``scatter_add_``) fed by a torch batched relation builder
      (a [B, N, N] distance / topk / nonzero chain), the reference's own structure.
Medians of passes that alternate between the three (a drift of the machine lands on all of them), each pass synchronised at both ends.
Also recorded: the share of the relation list's ``e_cap`` rows that were padding -- those rows go through the relation encoder.

    python tools/plan_rollout_cost.py [--out profiles/plan_rollout_cost.txt] [--B 1000] [--reps 3] [--loop-samples 20]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-dynamics_amd")]


def batched_relations_dense(last, thr, topk):
    """last [B, R, 3] (the tool last) -> one-hot Rr, Rs [B, E_max, R], zero rows behind a sample's relations: ``construct_edges``' rule for
    all samples at once in torch (one host read: the largest relation count)."""
    import torch
    B, R, _ = last.shape
    n_obj = R - 1
    d = ((last[:, :, None] - last[:, None]) ** 2).sum(-1)
    d[:, n_obj, n_obj] = 1e10
    adj = d < thr * thr
    near = torch.topk(d[:, :n_obj, :n_obj], k=min(topk, n_obj), dim=-1, largest=False)[1]
    keep = torch.zeros((B, n_obj, n_obj), dtype=torch.bool, device=last.device)
    keep.scatter_(2, near, True)
    adj[:, :n_obj, :n_obj] &= keep
    idx = adj.nonzero()
    counts = adj.sum((1, 2))
    e_max = int(counts.max())
    offs = torch.cumsum(counts, 0) - counts
    pos = torch.arange(idx.shape[0], device=last.device) - offs[idx[:, 0]]
    Rr = torch.zeros((B, e_max, R), device=last.device)
    Rs = torch.zeros((B, e_max, R), device=last.device)
    Rr[idx[:, 0], pos, idx[:, 1]] = 1
    Rs[idx[:, 0], pos, idx[:, 2]] = 1
    return Rr, Rs


def dense_rollout(model, state, actions, push_length, thr, topk, n_his):
    """(b): the reference's ``dynamics`` loop on the dense batched ``forward``."""
    import torch
    from gsdyn.plan import decode_action
    dev = state.device
    B, T, n_obj = actions.shape[0], actions.shape[1], state.shape[0]
    dec, rep = decode_action(actions, push_length)
    maxes = rep.amax(0).cpu().tolist()
    out = torch.zeros((B, T, n_obj, 3), device=dev)
    attrs = torch.zeros((B, n_obj + 1, 2), device=dev)
    attrs[:, :n_obj, 0] = 1.0
    attrs[:, n_obj, 1] = 1.0
    p_inst = torch.ones((B, n_obj, 1), device=dev)
    for li in range(T):
        prev = state[None].expand(B, -1, -1) if li == 0 else out[:, li - 1]
        eef = torch.cat([dec[:, li, :2], prev[:, :, 2].min(dim=1).values[:, None]], 1)
        states = torch.cat([prev, eef[:, None]], 1)[:, None].repeat(1, n_his, 1, 1)
        act = torch.zeros((B, n_obj + 1, 3), device=dev)
        act[:, n_obj, :2] = dec[:, li, 2:4] - dec[:, li, 0:2]
        for ai in range(1, maxes[li] + 1):
            Rr, Rs = batched_relations_dense(states[:, -1], thr, topk)
            pred, _ = model(state=states, attrs=attrs, p_instance=p_inst, action=act, Rr=Rr, Rs=Rs)
            keep = rep[:, li] == ai
            out[keep, li] = pred[keep]
            eef = states[:, -1, n_obj] + act[:, n_obj]
            eef[:, 2] = pred[:, :, 2].min(dim=1).values
            states = torch.cat([states[:, 1:], torch.cat([pred, eef[:, None]], 1)[:, None]], 1)
    return out


def loop_rollout(model, state, actions, push_length, thr, topk, n_his):
    """(a): one sample at a time through the single-graph path (``forward`` with index-form relations)."""
    import torch
    from gsdyn.dynamics import construct_edges
    from gsdyn.plan import decode_action
    dev = state.device
    B, T, n_obj = actions.shape[0], actions.shape[1], state.shape[0]
    dec, rep = decode_action(actions, push_length)
    rep_h = rep.cpu().tolist()
    attrs = torch.zeros((1, n_obj + 1, 2), device=dev)
    attrs[0, :n_obj, 0] = 1.0
    attrs[0, n_obj, 1] = 1.0
    p_inst = torch.ones((1, n_obj, 1), device=dev)
    mask = torch.ones(n_obj + 1, dtype=torch.bool, device=dev)
    tool = torch.zeros(n_obj + 1, dtype=torch.bool, device=dev)
    tool[n_obj] = True
    out = torch.zeros((B, T, n_obj, 3), device=dev)
    for b in range(B):
        prev = state
        for li in range(T):
            eef = torch.cat([dec[b, li, :2], prev[:, 2].min().view(1)])
            states = torch.cat([prev, eef[None]], 0)[None].repeat(n_his, 1, 1)
            act = torch.zeros((1, n_obj + 1, 3), device=dev)
            act[0, n_obj, :2] = dec[b, li, 2:4] - dec[b, li, 0:2]
            for ai in range(rep_h[b][li]):
                recv, send = construct_edges(states[-1], thr, mask, tool, topk=topk, n_tool=1)
                pred, _ = model(state=states[None], attrs=attrs, p_instance=p_inst, action=act, receivers=recv, senders=send)
                eef = states[-1, n_obj] + act[0, n_obj]
                eef[2] = pred[0, :, 2].min()
                states = torch.cat([states[1:], torch.cat([pred[0], eef[None]], 0)[None]], 0)
            prev = states[-1, :n_obj]
            out[b, li] = prev
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_rollout_cost.txt"))
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-samples", type=int, default=20)
    ap.add_argument("--width", type=int, default=512)
    a = ap.parse_args()
    import torch
    from gsdyn import rollout_actions
    from gsdyn.dynamics import DynamicsPredictor
    dev = torch.device("cuda:0")
    n_obj, T, n_his, thr, topk, push = 100, 3, 3, 0.08, 5, 0.01
    cfg = dict(nf_particle=a.width, nf_relation=a.width, nf_effect=a.width, attr_dim=2, state_dim=0, action_dim=3, pstep=3, rel_attr_dim=2,
               rel_group_dim=1, rel_distance_dim=3, n_his=n_his)
    torch.manual_seed(0)
    model = DynamicsPredictor(cfg, device=dev).eval()
    with torch.no_grad():                               # untrained weights move a particle by ~0.3 per call: scaled to the rope's few millimetres
        model.non_rigid_predictor.linear_2.weight.mul_(0.01)
        model.non_rigid_predictor.linear_2.bias.mul_(0.01)
    g = torch.Generator().manual_seed(1)
    ix = torch.arange(n_obj, dtype=torch.float32)
    state = torch.stack([(ix % 10) * 0.05, torch.div(ix, 10, rounding_mode="floor") * 0.05, torch.zeros(n_obj)], 1)
    state = (state + (torch.rand((n_obj, 3), generator=g) - 0.5) * 0.01).to(dev)
    xy = torch.rand((a.B, T, 2), generator=g) * 0.45
    theta = (torch.rand((a.B, T, 1), generator=g) * 2 - 1) * math.pi
    length = torch.randint(1, 6, (a.B, T, 1), generator=g).float() + 0.5
    actions = torch.cat([xy, theta, length], 2).to(dev)
    kw = dict(push_length=push, adj_thresh=thr, topk=topk, n_his=n_his)
    n_loop = min(a.loop_samples, a.B)
    paths = {
        "batched (this path)": lambda: rollout_actions(model, state, actions, chunk=a.B, **kw)["state_seqs"],
        "dense B>1 forward + torch relations": lambda: dense_rollout(model, state, actions, push, thr, topk, n_his),
        f"per-sample loop ({n_loop} samples)": lambda: loop_rollout(model, state, actions[:n_loop], push, thr, topk, n_his),
    }
    with torch.no_grad():
        trace = []
        got = rollout_actions(model, state, actions, chunk=a.B, _trace=trace, **kw)["state_seqs"]
        (_, _, tr), = trace
        counts = torch.stack([t[5] for t in tr]).view(-1).cpu()
        e_cap = int(tr[0][3].shape[0])
        pad_share = 1.0 - float(counts.double().mean()) / e_cap
        ref = paths["dense B>1 forward + torch relations"]()
        one = list(paths.values())[2]()
        disp = float((ref - state[None, None]).abs().max())
        agree_dense = float((got - ref).abs().max())
        agree_loop = float((got[:n_loop] - one).abs().max())
        times = {k: [] for k in paths}
        for _ in range(max(a.reps, 1)):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    loop_key = list(paths)[2]
    base = med["batched (this path)"]
    lines = [f"rollout_actions: B = {a.B}, n_obj = {n_obj}, T = {T}, repeats 1..5 ({len(tr)} model calls), width {a.width}, n_his = {n_his}, topk = {topk}, "
             f"{torch.cuda.get_device_name(0)}",
             f"median of {max(a.reps, 1)} alternating passes behind one warm-up pass of each, ms per rollout of all B samples:"]
    for k in paths:
        v = med[k] * (a.B / n_loop if k == loop_key else 1.0)
        note = f"  (measured {med[k]:.1f} ms for {n_loop} samples, scaled by {a.B / n_loop:.0f})" if k == loop_key else ""
        lines.append(f"  {k:40s} {v:10.1f} ms   {v / base:7.2f} x batched   passes {min(times[k]):.1f}..{max(times[k]):.1f}{note}")
    lines.append(f"relation list: e_cap = {e_cap} rows per model call, real relations {int(counts.min())}..{int(counts.max())}: {100 * pad_share:.1f} % of the rows "
                 f"the relation encoder processes are padding")
    lines.append(f"agreement (largest displacement {disp:.3e}): batched vs dense {agree_dense:.3e}, batched vs per-sample loop {agree_loop:.3e} (max abs)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
