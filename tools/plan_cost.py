"""The cost of the planner's cost and update (profiles/plan_cost.txt): ``gsdyn.running_cost`` + ``gsdyn.mppi_update`` for one chunk of B = 1000
samples of 100 particles, T in {1, 3} look-ahead steps, a target cloud of M in {1 000, 10 000} points, on the device path (gsr_plan_cost +
gsr_plan_mppi_update, two launches) against the torch fallback (``_running_cost_reference`` + ``_mppi_update_reference``) on the same GPU and
the same tensors.  If the fallback runs out of memory, that is what the table says.  Then the share of a whole ``plan_actions`` chunk --
sampler, ``rollout_actions`` (the rope.yaml widths, repeat counts 1 .. 5, as tools/plan_rollout_cost.py), cost, update -- that cost + update
are with either path.
Medians of passes that alternate between the paths (a drift of the machine lands on both), each pass synchronised at both ends, behind one
warm-up pass of each.

    python tools/plan_cost.py [--out profiles/plan_cost.txt] [--B 1000] [--reps 5] [--width 512]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-dynamics_amd")]


def timed(fns, reps):
    """{name: fn} -> {name: [ms per pass]}: one warm-up pass of each, then ``reps`` rounds that alternate between them.  A path that raises
    an out-of-memory error is recorded as the string "out of memory" and left out of the later rounds."""
    import torch
    times = {k: [] for k in fns}
    for rnd in range(reps + 1):
        for k, fn in fns.items():
            if isinstance(times[k], str):
                continue
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rnd > 0:
                    times[k].append((time.perf_counter() - t0) * 1e3)
            except torch.cuda.OutOfMemoryError:
                times[k] = "out of memory"
                torch.cuda.empty_cache()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_cost.txt"))
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=512)
    a = ap.parse_args()
    import torch
    from gsdyn import mppi_update, plan, rollout_actions, running_cost, sample_action_seq
    from gsdyn.dynamics import DynamicsPredictor
    dev = torch.device("cuda:0")
    B, n_obj, n_his, thr, topk, push, rw = a.B, 100, 3, 0.08, 5, 0.01, 500.0
    bbox = torch.tensor([[-0.05, 0.55], [-0.05, 0.55]])
    lower = torch.tensor([-0.05, -0.05, -math.pi, 1.0], device=dev)
    upper = torch.tensor([0.55, 0.55, math.pi, 5.99], device=dev)
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
    box4 = plan._box4(bbox, dev, torch.float32)
    lines = [f"running_cost + mppi_update: one chunk of B = {B} samples, n_obj = {n_obj}, reward_weight = {rw:g}, {torch.cuda.get_device_name(0)}",
             f"median of {a.reps} alternating passes behind one warm-up pass of each, ms per chunk; rollout: width {a.width}, repeats 1..5, topk = {topk}",
             f"{'T':>2s} {'M':>6s} | {'device path':>12s} {'torch fallback':>15s} {'ratio':>7s} | {'sampler':>8s} {'rollout':>9s} | cost + update share of the chunk: fallback -> device"]
    with torch.no_grad():
        for T in (1, 3):
            seed = torch.zeros((T, 4), device=dev)
            acts = sample_action_seq(seed, lower, upper, B, iter_index=0, noise_level=1.0, push_length=push, generator=g)
            kw = dict(push_length=push, adj_thresh=thr, topk=topk, n_his=n_his, chunk=B)
            seqs = rollout_actions(model, state, acts, **kw)["state_seqs"]
            chunk = timed({"sampler": lambda: sample_action_seq(seed, lower, upper, B, iter_index=0, noise_level=1.0, push_length=push),
                           "rollout": lambda: rollout_actions(model, state, acts, **kw)}, a.reps)
            t_s, t_r = statistics.median(chunk["sampler"]), statistics.median(chunk["rollout"])
            for M in (1000, 10000):
                target = (torch.rand((M, 3), generator=g) * torch.tensor([0.5, 0.5, 0.02])).to(dev)

                def device_path():
                    c = running_cost(seqs, acts, state, target, bbox)
                    return mppi_update(acts, c["reward_seqs"], reward_weight=rw, lower=lower, upper=upper, push_length=push)

                def fallback():
                    r = plan._running_cost_reference(seqs, acts, state, target, box4, 0.01, 100.0, 5.0)[0]
                    return plan._mppi_update_reference(acts, r, rw, lower, upper, push)

                t = timed({"device": device_path, "fallback": fallback}, a.reps)
                d = statistics.median(t["device"])
                if isinstance(t["fallback"], str):
                    lines.append(f"{T:2d} {M:6d} | {d:12.3f} {t['fallback']:>15s} {'-':>7s} | {t_s:8.3f} {t_r:9.1f} | - -> {100 * d / (t_s + t_r + d):.2f} %")
                    continue
                f = statistics.median(t["fallback"])
                agree = float((device_path()["act_seq"] - fallback()[0]).abs().max())
                lines.append(f"{T:2d} {M:6d} | {d:12.3f} {f:15.3f} {f / d:6.1f}x | {t_s:8.3f} {t_r:9.1f} | {100 * f / (t_s + t_r + f):.2f} % -> {100 * d / (t_s + t_r + d):.2f} %"
                             f"   (passes {min(t['device']):.3f}..{max(t['device']):.3f} / {min(t['fallback']):.3f}..{max(t['fallback']):.3f}; act_seq agrees to {agree:.1e})")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
