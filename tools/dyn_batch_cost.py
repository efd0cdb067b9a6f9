#!/usr/bin/env python
"""What building one training batch of the propagation network costs, next to the training step it feeds, on the same GPU.

Per shape, in alternating passes after a warm-up of each (a host clock around a device synchronise, one call per pass; reported: the
median over the passes, the smallest and the largest):
  (a) gsdyn.make_dynamics_batch on the device path, dense=False and dense=True;
  (b) its definition (device_path=False) on the same GPU tensors;
  (c) its definition on CPU tensors plus the copy of the batch to the device -- a stand-in for one loader worker of the reference;
  (d) one gsdyn.train_dynamics_step on the builder's batch, which carries the block-diagonal graph;
  (e) the same step on the dense dictionary alone: the graph derived from Rr / Rs by nonzero and a stable sort, as before the builder.
Shapes: the batch size, particle cap and relation cap of the reference's rope and cloth configurations as plain numbers, 1000 tracked
particles over 40 frames, n_his 3, n_future 5, the network width of those configurations (512), pstep 3, Adam.

    python tools/dyn_batch_cost.py [--passes 5] [--shapes rope,cloth] [--out profiles/dyn_batch_cost.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-dynamics_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

# name: B, max_nobj, max_nR, topk, connect_all, extent of the particle sheet, fps_radius_range, adj_radius_range
SHAPES = {
    "rope": dict(B=16, max_nobj=100, max_nR=500, topk=5, connect_all=False, extent=(0.5, 0.02, 0.01), fps=(0.011, 0.018), adj=(0.03, 0.06)),
    "cloth": dict(B=64, max_nobj=150, max_nR=1200, topk=6, connect_all=True, extent=(0.3, 0.3, 0.01), fps=(0.005, 0.02), adj=(0.03, 0.06)),
}
P, FRAMES, N_HIS, N_FUTURE, WIDTH = 1000, 40, 3, 5, 512


def make_inputs(s, seed):
    import gsdyn
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand((P, 3), generator=gen) * torch.tensor(s["extent"])
    t = torch.arange(FRAMES, dtype=torch.float32)[:, None, None]
    particles = base[None] + 0.002 * t * torch.tensor([1.0, 0.5, 0.0]) + 0.003 * torch.sin(0.3 * t + 9.0 * base[None, :, 0:1]) * torch.tensor([0.0, 1.0, 0.3])
    eef = torch.tensor([0.1, 0.01, 0.03]) + 0.004 * t[:, 0] * torch.tensor([1.0, 0.3, 0.0])
    first = torch.randint(0, FRAMES - (N_HIS + N_FUTURE) + 1, (s["B"],), generator=gen)
    pairs = first[:, None] + torch.arange(N_HIS + N_FUTURE)[None, :]
    draws = gsdyn.draw_batch_randomness(s["B"], P, n_his=N_HIS, max_nobj=s["max_nobj"], fps_radius_range=s["fps"], adj_radius_range=s["adj"],
                                        state_noise=0.003, generator=gen)
    kw = dict(n_his=N_HIS, n_future=N_FUTURE, max_nobj=s["max_nobj"], max_nR=s["max_nR"], topk=s["topk"], connect_all=s["connect_all"], **draws)
    return (particles.contiguous(), eef.contiguous(), pairs), kw


def to(dev, args, kw):
    return tuple(a.to(dev) for a in args), {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}


def make_model(dev):
    from gsdyn.dynamics import DynamicsPredictor
    torch.manual_seed(0)
    cfg = dict(nf_particle=WIDTH, nf_relation=WIDTH, nf_effect=WIDTH, attr_dim=2, state_dim=0, motion_dim=0, action_dim=3, pstep=3,
               rel_attr_dim=2, rel_group_dim=1, rel_distance_dim=3, n_his=N_HIS)
    return DynamicsPredictor(cfg).to(dev)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main():
    import gsdyn
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--dry", action="store_true", help="build each shape's batch once with the definition on the CPU and print its counts (no GPU)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.dry:
        for name in args.shapes.split(","):
            a, kw = make_inputs(SHAPES[name], 1)
            b = gsdyn.make_dynamics_batch(*a, **kw, dense=False)
            print(f"{name}: n_obj {b['n_obj'].min().item()} .. {b['n_obj'].max().item()}, n_rel {b['n_rel'].min().item()} .. {b['n_rel'].max().item()}")
        return
    if not torch.cuda.is_available():
        sys.exit("dyn_batch_cost.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    lines = [f"# tools/dyn_batch_cost.py on {torch.cuda.get_device_name(dev)}: P {P}, n_his {N_HIS}, n_future {N_FUTURE}, width {WIDTH}, pstep 3, Adam; "
             f"{args.passes} alternating passes of one call after {args.warmup} warm-up calls each; ms per call: median (min .. max)"]
    for name in args.shapes.split(","):
        s = SHAPES[name]
        host_a, host_kw = make_inputs(s, 1)
        dev_a, dev_kw = to(dev, host_a, host_kw)
        full = gsdyn.make_dynamics_batch(*dev_a, **dev_kw, dense=True, device_path=True)
        dense_only = {k: v for k, v in full.items() if k not in ("graph", "receivers", "senders", "n_rel", "n_rel_rows", "n_obj", "fps_idx")}
        steps = {}
        for key, batch in (("d", full), ("e", dense_only)):
            model = make_model(dev)
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            steps[key] = lambda model=model, opt=opt, batch=batch: gsdyn.train_dynamics_step(model, opt, batch, n_future=N_FUTURE, device_path=True)

        def worker():
            b = gsdyn.make_dynamics_batch(*host_a, **host_kw, dense=True)
            return {k: v.to(dev) for k, v in b.items() if isinstance(v, torch.Tensor)}

        runs = {
            "a device, lists": lambda: gsdyn.make_dynamics_batch(*dev_a, **dev_kw, dense=False, device_path=True),
            "a device, dense": lambda: gsdyn.make_dynamics_batch(*dev_a, **dev_kw, dense=True, device_path=True),
            "b definition on the GPU": lambda: gsdyn.make_dynamics_batch(*dev_a, **dev_kw, dense=True, device_path=False),
            "c definition on the CPU + copy": worker,
            "d step, graph from the builder": steps["d"],
            "e step, graph from Rr / Rs": steps["e"],
        }
        l_d, l_e = float(steps["d"]()), float(steps["e"]())            # the first step of each from the same weights
        for fn in runs.values():
            for _ in range(args.warmup):
                fn()
        t = {k: [] for k in runs}
        order = list(runs)
        for k in range(args.passes):
            for key in (order if k % 2 == 0 else order[::-1]):
                t[key].append(timed(runs[key], dev))
        n_obj, n_rel = full["n_obj"].float(), full["n_rel"].float()
        lines.append(f"{name}: B={s['B']} max_nobj={s['max_nobj']} max_nR={s['max_nR']} topk={s['topk']} connect_all={s['connect_all']}; objects per sample "
                     f"{n_obj.mean().item():.1f} ({int(n_obj.min())} .. {int(n_obj.max())}), relations {n_rel.mean().item():.1f} ({int(n_rel.min())} .. "
                     f"{int(n_rel.max())}); first losses d / e {l_d:.6e} / {l_e:.6e}")
        for key, v in t.items():
            lines.append(f"  ({key[0]}) {key[2:]:32}: {statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})")
        lines.append(f"  builder, lists, as a share of step (d): {statistics.median(t['a device, lists']) / statistics.median(t['d step, graph from the builder']):.3f}; "
                     f"definition on the CPU + copy / builder, dense: "
                     f"{statistics.median(t['c definition on the CPU + copy']) / statistics.median(t['a device, dense']):.0f}")
        for ln in lines[-8:]:
            print(ln, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
