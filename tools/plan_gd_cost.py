#!/usr/bin/env python
"""What one iteration of the gradient planner costs on one GPU, every comparison against the definition or fallback on the same device.

One iteration = gsdyn.rollout_actions_grad -> gsdyn.running_cost_grad -> the gradient of -sum(reward) / B toward the candidates (what
gsdyn.plan_actions_gd runs before its Adam step).  Measured:
  (1) ms per iteration of the batched device path (``device_path=True``) against the per-sample definition (``device_path=False``), in
      alternating passes after a warm-up of each, a host clock around a device synchronise; the median, the smallest and the largest pass;
  (2) torch.cuda.max_memory_allocated of one device-path iteration per shape (activations grow with B x the sum of the repeat counts);
  (3) the cost alone, values + gradients: gsr_plan_cost_grad against ``_running_cost_grad_reference`` on the device at B = 1000;
  (4) where a device-path iteration's GPU time goes -- the GEMM library, this project's kernels, everything else (the torch glue) -- and
      how much of the wall time the GPU is busy at all, from torch.profiler's kernel records in a run of its own.
Shapes: the network width of the shipped configurations (512), pstep 3, n_his 3, 100 particles on a jittered grid, B in {16, 64, 256}
candidates, T in {1, 2} look-ahead steps of about 10 model calls each (lengths 8.5 .. 12.5), M in {1000, 10000} target points.

    python tools/plan_gd_cost.py [--passes 5] [--def-passes 3] [--out profiles/plan_gd_cost.txt] [--skip-definition-above 256]
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-dynamics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WIDTH, N_OBJ, PUSH, THR, TOPK = 512, 100, 0.01, 0.12, 5
BBOX = [[-0.2, 1.2], [-0.2, 1.2]]


def make_model(dev, seed=0):
    from gsdyn.dynamics import DynamicsPredictor
    torch.manual_seed(seed)
    cfg = dict(nf_particle=WIDTH, nf_relation=WIDTH, nf_effect=WIDTH, attr_dim=2, state_dim=0, motion_dim=0, action_dim=3, pstep=3,
               rel_attr_dim=2, rel_group_dim=1, rel_distance_dim=3, n_his=3)
    m = DynamicsPredictor(cfg).eval()
    with torch.no_grad():                       # small motions, as a trained model's: the particles stay a rope-like cloud
        m.non_rigid_predictor.linear_2.weight.mul_(0.01)
        m.non_rigid_predictor.linear_2.bias.mul_(0.01)
    return m.to(dev)


def make_case(B, T, M, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    ix = torch.arange(N_OBJ, dtype=torch.float32)
    grid = torch.stack([(ix % 10) * 0.1, torch.div(ix, 10, rounding_mode="floor") * 0.1, torch.zeros(N_OBJ)], 1)
    state = grid + (torch.rand((N_OBJ, 3), generator=g) - 0.5) * torch.tensor([0.02, 0.02, 0.01])
    target = torch.rand((M, 3), generator=g) * torch.tensor([1.0, 1.0, 0.02])
    acts = torch.cat([torch.rand((B, T, 2), generator=g), (torch.rand((B, T, 1), generator=g) * 2 - 1) * math.pi,
                      8.5 + torch.randint(0, 5, (B, T, 1), generator=g).float()], 2)
    return state.to(dev), target.to(dev), acts.to(dev)


def iteration(model, state, target, acts, device_path):
    import gsdyn
    a = acts.detach().clone().requires_grad_(True)
    out = gsdyn.rollout_actions_grad(model, state, a, push_length=PUSH, adj_thresh=THR, topk=TOPK, device_path=device_path)["state_seqs"]
    r = gsdyn.running_cost_grad(out, a, state, target, BBOX)["reward_seqs"]
    (g,) = torch.autograd.grad(-r.sum() / a.shape[0], a)
    return g


def timed(fn, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps * 1e3


def spread(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"


def kernel_shares(fn, dev, steps=3):
    """(wall ms, GPU-busy ms, {class: ms}, launches) per iteration from torch.profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize(dev)
    wall = (time.perf_counter() - t0) / steps * 1e3
    shares, launches = {"GEMM library": 0.0, "project kernels": 0.0, "torch glue": 0.0}, 0
    for ev in prof.events():
        if getattr(ev, "device_type", None) is None or "cuda" not in str(ev.device_type).lower():
            continue
        name, us = ev.name, float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0) or 0.0)
        if us <= 0.0:
            continue
        launches += 1
        low = name.lower()
        key = "GEMM library" if ("cijk" in low or "gemm" in low or "rocblas" in low or "hipblas" in low) else \
            "project kernels" if ("gsr_" in low or "gnn" in low or "pcgrad" in low or "relations" in low or "gsr" in low) else "torch glue"
        shares[key] += us / 1e3 / steps
    return wall, sum(shares.values()), shares, launches // steps


def main():
    from gsdyn import plan
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--def-passes", type=int, default=3)
    ap.add_argument("--batches", default="16,64,256")
    ap.add_argument("--skip-definition-above", type=int, default=256, help="the definition is timed up to this B (it is a Python loop over the samples)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("plan_gd_cost.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    model = make_model(dev)
    lines = [f"# tools/plan_gd_cost.py on {torch.cuda.get_device_name(dev)}: width {WIDTH}, pstep 3, n_his 3, n_obj {N_OBJ}, about 10 model calls per look-ahead "
             f"step; alternating passes after a warm-up of each path; ms per iteration = rollout_actions_grad + running_cost_grad + gradient toward the "
             f"candidates: median (smallest .. largest pass)"]

    def say(line):
        lines.append(line)
        print(line, flush=True)
    batches = [int(b) for b in args.batches.split(",")]
    warm = make_case(4, 1, 1000, dev)
    for path in (True, False):
        iteration(model, *warm, path)
    for B in batches:
        for T in (1, 2):
            for M in (1000, 10000):
                state, target, acts = make_case(B, T, M, dev)
                calls = int(acts[:, :, 3].to(torch.int32).amax(0).sum())
                run = {p: (lambda p=p: iteration(model, state, target, acts, p)) for p in (True, False)}
                with_def = B <= args.skip_definition_above
                g_dev = run[True]()
                torch.cuda.synchronize(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                run[True]()
                torch.cuda.synchronize(dev)
                peak = torch.cuda.max_memory_allocated(dev) / 2 ** 20
                t = {True: [], False: []}
                n_def = (args.def_passes if B < 256 else min(args.def_passes, 2)) if with_def else 0
                for k in range(args.passes):
                    order = (True, False) if k % 2 == 0 else (False, True)
                    for p in order:
                        if p or k < n_def:
                            t[p].append(timed(run[p], 3 if p else 1, dev))
                head = f"B={B:3d} T={T} M={M:5d} ({calls:2d} batched model calls)"
                if t[False]:
                    g_def = run[False]()
                    rel = float((g_dev - g_def).abs().max() / g_def.abs().max())
                    say(f"{head}: device path {spread(t[True])}, definition {spread(t[False])} [{len(t[False])} passes], definition / device "
                        f"{statistics.median(t[False]) / statistics.median(t[True]):6.1f}; peak memory of a device-path iteration {peak:8.1f} MiB; "
                        f"gradients differ by {rel:.1e} of the largest")
                else:
                    say(f"{head}: device path {spread(t[True])}, definition not measured; peak memory of a device-path iteration {peak:8.1f} MiB")
    say("# the cost alone, values + gradients toward state_seqs and actions, B = 1000, T = 2, n_obj = 100: gsr_plan_cost_grad against the torch statement on the device")
    for M in (1000, 10000):
        g = torch.Generator().manual_seed(M)
        scale = torch.tensor([1.0, 1.0, 0.02])
        seqs = (torch.rand((1000, 2, N_OBJ, 3), generator=g) * scale).to(dev)
        acts = torch.cat([torch.rand((1000, 2, 2), generator=g), torch.zeros((1000, 2, 1)), torch.full((1000, 2, 1), 10.0)], 2).to(dev)
        cur, target = (torch.rand((N_OBJ, 3), generator=g) * scale).to(dev), (torch.rand((M, 3), generator=g) * scale).to(dev)
        box = plan._box4(BBOX, dev, torch.float32)

        def cost(kernel):
            s, a = seqs.clone().requires_grad_(True), acts.clone().requires_grad_(True)
            if kernel:
                r = plan.running_cost_grad(s, a, cur, target, BBOX)["reward_seqs"]
            else:
                r = plan._running_cost_grad_reference(s, a, cur, target, box, 0.01, 100.0, 5.0)[0]
            return torch.autograd.grad(r.sum(), (s, a))
        cost(True), cost(False)
        t = {True: [], False: []}
        for k in range(args.passes):
            for p in ((True, False) if k % 2 == 0 else (False, True)):
                t[p].append(timed(lambda p=p: cost(p), 5 if p else 1, dev))
        torch.cuda.reset_peak_memory_stats(dev)
        cost(True)
        torch.cuda.synchronize(dev)
        pk = torch.cuda.max_memory_allocated(dev) / 2 ** 20
        torch.cuda.reset_peak_memory_stats(dev)
        cost(False)
        torch.cuda.synchronize(dev)
        pf = torch.cuda.max_memory_allocated(dev) / 2 ** 20
        say(f"M={M:5d}: kernel {spread(t[True])} ms, torch statement {spread(t[False])} ms, statement / kernel {statistics.median(t[False]) / statistics.median(t[True]):6.1f}; "
            f"peak memory {pk:.1f} / {pf:.1f} MiB")
    say("# where a device-path iteration's GPU time goes (torch.profiler kernel records, a run of its own; the profiler slows the host)")
    for B, T in ((64, 2), (256, 2)):
        if B not in batches:
            continue
        state, target, acts = make_case(B, T, 1000, dev)
        try:
            wall, busy, shares, launches = kernel_shares(lambda: iteration(model, state, target, acts, True), dev)
            say(f"B={B:3d} T={T} M= 1000: wall {wall:.2f} ms, GPU busy {busy:.2f} ms ({100 * busy / wall:.0f} % of the wall time), {launches} launches; "
                + ", ".join(f"{k} {v:.2f} ms ({100 * v / busy:.0f} % of busy)" for k, v in shares.items()))
        except Exception as e:  # noqa: BLE001  (a profiler that cannot record kernels here: the rest of the file stands)
            say(f"B={B:3d} T={T}: kernel shares not measured ({type(e).__name__}: {e})")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
