#!/usr/bin/env python
"""What the rigid-alignment term costs on one GPU: the fit alone, and inside a training step.

(a) ``gsdyn.umeyama_fit`` through the kernel gsr_rigid_fit against the torch statement (batched ``torch.linalg.svd``) on the same GPU;
(b) one ``gsdyn.train_dynamics_step`` on the device path with ``rigid_weight`` 0, with 0.05 through the kernel, and with 0.05 and the
    torch statement forced (``_rigid_kernel=False``).  ``rigid_weight`` 0 is timed as two variants ("0" and "0 again"):
    the same code, so their distance is the round-to-round spread every other difference is read against.

The variants run in alternating passes (the order rotates by one every pass) after a warm-up of each (first calls load code objects and let
the libraries pick their kernels); per pass K calls are timed with a host clock around a device synchronise.  Reported: the median over
the passes, the smallest and the largest pass.  Last, in a phase of its own, the library's HIP-event timing gives the kernel's own time.

Shapes: batch size and object particles of the reference's rope (16, 100) and cloth (64, 150) configurations; the step's network as in
tools/gnn_train_cost.py (width 512, pstep 3, n_his 3, Adam), n_future 2; every tenth object row is masked out.

    python tools/rigid_loss_cost.py [--passes 7] [--steps 20] [--calls 2000] [--n-future 2] [--out profiles/rigid_loss_cost.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-dynamics_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from gnn_train_cost import SHAPES, make_batch, make_model, timed  # noqa: E402

NAMES = ("rope", "cloth")
RIGID, LENGTH = 0.05, 0.05


def alternate(variants, passes, steps, dev):
    """{name: fn} -> {name: [ms per call, one per pass]}, the order rotated by one every pass."""
    names = list(variants)
    t = {n: [] for n in names}
    for k in range(passes):
        for n in names[k % len(names):] + names[:k % len(names)]:
            t[n].append(timed(variants[n], steps, dev))
    return t


def fmt(v):
    return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    import gsdyn
    from diff_gaussian_rasterization import _hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed pass")
    ap.add_argument("--calls", type=int, default=2000, help="umeyama_fit calls per timed pass")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-future", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rigid_loss_cost.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    lines = [f"# tools/rigid_loss_cost.py on {torch.cuda.get_device_name(dev)}: {args.passes} alternating passes after {args.warmup} warm-up "
             f"calls per variant; ms per call: median (smallest .. largest pass)"]
    say = lambda s: (lines.append(s), print(s, flush=True))  # noqa: E731
    for name in NAMES:
        B, n_obj, n_rel, state_dim = SHAPES[name]
        batch = make_batch(B, n_obj, n_rel, args.n_future, 1, dev)
        mask = torch.ones((B, n_obj), dtype=torch.bool, device=dev)
        mask[:, ::10] = False
        batch["obj_mask"] = mask
        # ---- (a) the fit alone: the oldest history frame onto the newest, over the mask
        X, Y = batch["state"][:, 0, :n_obj].contiguous(), batch["state"][:, -1, :n_obj].contiguous()
        fits = {"kernel": lambda: gsdyn.umeyama_fit(X, Y, mask, kernel=True), "torch": lambda: gsdyn.umeyama_fit(X, Y, mask, kernel=False)}
        a, b = fits["kernel"](), fits["torch"]()
        dist = float((a["R"] - b["R"]).abs().max())
        for _ in range(args.warmup):
            fits["kernel"](), fits["torch"]()
        t = alternate(fits, args.passes, args.calls, dev)
        say(f"(a) {name:6} B={B:3d} N={n_obj:4d} umeyama_fit, {args.calls} calls per pass: kernel {fmt(t['kernel'])}, torch statement {fmt(t['torch'])}, "
            f"torch / kernel {statistics.median(t['torch']) / statistics.median(t['kernel']):.2f}; max |R kernel - R torch| {dist:.2e}")
        # ---- (b) one training step
        def step_variant(weight, kernel):
            model = make_model(state_dim, dev)
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)

            return lambda: gsdyn.train_dynamics_step(model, opt, batch, n_future=args.n_future, length_weight=LENGTH, rigid_weight=weight,
                                                     device_path=True, _rigid_kernel=None if kernel else False)
        steps = {"0": step_variant(0.0, True), "kernel": step_variant(RIGID, True), "torch": step_variant(RIGID, False), "0 again": step_variant(0.0, True)}
        first = {n: float(f()) for n, f in steps.items()}
        for _ in range(args.warmup - 1):
            for f in steps.values():
                f()
        t = alternate(steps, args.passes, args.steps, dev)
        med = {n: statistics.median(v) for n, v in t.items()}
        say(f"(b) {name:6} B={B:3d} N={n_obj + 1:4d} n_rel={n_rel:5d} train_dynamics_step, n_future {args.n_future}, {args.steps} steps per pass: "
            f"rigid_weight 0 {fmt(t['0'])}, 0 again {fmt(t['0 again'])}, {RIGID} kernel {fmt(t['kernel'])}, {RIGID} torch statement {fmt(t['torch'])}; "
            f"the term costs {med['kernel'] - med['0']:+.3f} (kernel) / {med['torch'] - med['0']:+.3f} (torch) per step; "
            f"first losses {first['0']:.6e} / {first['kernel']:.6e} / {first['torch']:.6e}")
        # ---- the kernel's own time, by HIP events
        _hip.profile_begin()
        for _ in range(args.calls):
            fits["kernel"]()
        torch.cuda.synchronize(dev)
        prof = _hip.profile_end()
        say(f"    {name:6} kernel's own time (HIP events): " + "; ".join(f"{k} {ms / n * 1e3:.1f} us" for k, (ms, n) in sorted(prof.items())))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
