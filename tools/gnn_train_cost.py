#!/usr/bin/env python
"""What one training step of the propagation network costs on the device path and on the eager path, on the same GPU.

One step = gsdyn.train_dynamics_step: zero_grad, the n_future predictions of dynamics_loss, backward, Adam.  The two paths run in
alternating passes after a warm-up of each (the first calls load code objects and let the GEMM library pick its kernels); per pass K steps
are timed with a host clock around a device synchronise.  Reported: the median over the passes, the smallest and the largest pass.
In a run of its own (``--kernels``) the library's HIP-event timing gives the two backward kernels' (and the forward kernels') own times.

Shapes: the batch size, particle count (objects + one tool) and relation cap of the reference's shipped configurations, as plain numbers,
with the network width of those configurations (512), pstep 3 and n_his 3; 80 % of the relation cap is filled with real relations, the
rest is padding, as the dataset pads.  ``rope x4`` is the rope shape with four times the relations.

    python tools/gnn_train_cost.py [--passes 7] [--steps 5] [--n-future 2] [--out profiles/gnn_train_cost.txt] [--kernels]
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

# name: (batch size, object particles, relation cap, state_dim, topk as in the file -- unused here, the relations are drawn at random)
SHAPES = {
    "rope": (16, 100, 500, 0),
    "deer": (64, 100, 900, 1),
    "cloth": (64, 150, 1200, 1),
    "rope x4": (16, 100, 2000, 0),
}
WIDTH, FILL = 512, 0.8


def make_batch(B, n_obj, n_rel, n_future, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    N, n_his = n_obj + 1, 3
    last = torch.rand((B, N, 3), generator=gen) * torch.tensor([0.4, 0.4, 0.05])
    steps = (torch.rand((B, n_his, N, 3), generator=gen) - 0.5) * 0.02
    steps[:, -1] = 0.0
    state = last[:, None] + torch.flip(torch.cumsum(torch.flip(steps, [1]), 1), [1])
    attrs = torch.zeros((B, N, 2))
    attrs[:, :n_obj, 0] = 1.0
    attrs[:, n_obj, 1] = 1.0
    n_real = int(FILL * n_rel)
    recv = torch.sort(torch.randint(0, N, (B, n_real), generator=gen), 1)[0]
    send = (recv + torch.randint(1, N, (B, n_real), generator=gen)) % N           # never the receiver itself
    Rr, Rs = torch.zeros((B, n_rel, N)), torch.zeros((B, n_rel, N))
    Rr[:, :n_real].scatter_(2, recv[..., None], 1.0)
    Rs[:, :n_real].scatter_(2, send[..., None], 1.0)
    walk = torch.cumsum((torch.rand((B, n_future, N, 3), generator=gen) - 0.5) * 0.02, 1) + last[:, None]
    act = torch.zeros((B, n_future, N, 3))
    act[:, :, n_obj, :2] = (torch.rand((B, n_future, 2), generator=gen) - 0.5) * 0.05
    batch = dict(state=state, attrs=attrs, p_instance=torch.ones((B, n_obj, 1)), action=act[:, 0].contiguous(), Rr=Rr, Rs=Rs,
                 state_future=walk[:, :, :n_obj].contiguous(), tool_future=walk[:, :max(n_future - 1, 0)].contiguous(),
                 action_future=act[:, 1:].contiguous())
    return {k: v.to(dev) for k, v in batch.items()}


def make_model(state_dim, dev, seed=0):
    from gsdyn.dynamics import DynamicsPredictor
    torch.manual_seed(seed)
    cfg = dict(nf_particle=WIDTH, nf_relation=WIDTH, nf_effect=WIDTH, attr_dim=2, state_dim=state_dim, motion_dim=0, action_dim=3, pstep=3,
               rel_attr_dim=2, rel_group_dim=1, rel_distance_dim=3, n_his=3)
    return DynamicsPredictor(cfg).to(dev)


def timed(fn, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    import gsdyn
    from diff_gaussian_rasterization import _hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-future", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--kernels", action="store_true", help="the kernels' own times by HIP events instead of the step comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gnn_train_cost.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    lines = [f"# tools/gnn_train_cost.py on {torch.cuda.get_device_name(dev)}: width {WIDTH}, pstep 3, n_his 3, n_future {args.n_future}, Adam; "
             f"{args.passes} alternating passes of {args.steps} steps after {args.warmup} warm-up steps per path; ms per step"]
    for name in args.shapes.split(","):
        B, n_obj, n_rel, state_dim = SHAPES[name]
        batch = make_batch(B, n_obj, n_rel, args.n_future, 1, dev)
        runs = {}
        for path in (True, False):
            model = make_model(state_dim, dev)
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            runs[path] = lambda model=model, opt=opt, path=path: gsdyn.train_dynamics_step(model, opt, batch, n_future=args.n_future, device_path=path)
        head = f"{name:8} B={B:3d} N={n_obj + 1:4d} n_rel={n_rel:5d} ({int(FILL * n_rel) * B} real relations)"
        if args.kernels:
            for _ in range(args.warmup):
                runs[True]()
            torch.cuda.synchronize(dev)
            _hip.profile_begin()
            for _ in range(args.steps):
                runs[True]()
            torch.cuda.synchronize(dev)
            prof = _hip.profile_end()
            lines.append(head + ": " + "; ".join(f"{k} {ms / n * 1e3:.1f} us x {n // args.steps} per step" for k, (ms, n) in sorted(prof.items())))
            print(lines[-1], flush=True)
            continue
        l_dev, l_eager = float(runs[True]()), float(runs[False]())          # the first step of each path from the same weights
        for _ in range(args.warmup - 1):
            runs[True](), runs[False]()
        t = {True: [], False: []}
        for k in range(args.passes):
            for path in ((True, False) if k % 2 == 0 else (False, True)):
                t[path].append(timed(runs[path], args.steps, dev))
        med = {p: statistics.median(v) for p, v in t.items()}
        lines.append(f"{head}: device path {med[True]:8.2f} ({min(t[True]):.2f} .. {max(t[True]):.2f}), eager {med[False]:8.2f} "
                     f"({min(t[False]):.2f} .. {max(t[False]):.2f}), eager / device {med[False] / med[True]:.2f}; first losses {l_dev:.6e} / {l_eager:.6e}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
