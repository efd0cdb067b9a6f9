"""The cost of SH colours in the multi-view call (profiles/sh_views_cost.txt): forward + backward of
``rasterize_gaussians_views(shs=...)`` with all gradients, 800 x 800, 100 000 Gaussians, M = 16 at degree 3, V in {1, 4, 8} views, with
``batched_sh`` off (the per-view path: the baseline, measured in the same session) and on.

    python tools/sh_views_cost.py                     the table: one fresh child process per V, each under its own time limit; stops at
                                                      the first child that fails
    python tools/sh_views_cost.py --child V           one configuration: off and on alternated pass by pass behind a warm-up of both,
                                                      the median of the passes of each (as bench.py's _time_ms does)
    python tools/sh_views_cost.py --child V --only on a few steps of one path, for a kernel-stats run of its own:
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/sh_views_cost.py --child 4 --only on
      (sh_bwd_views_kernel's average is in <dir>/run_kernel_stats.csv; its HBM roofline uses the traffic formula of DESIGN.md section 3h:
      P (24 M + 24 + 20 V) bytes, dL_dmeans3D's read-modify-write counted on both sides.)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, W, H, M, DEG = 100_000, 800, 800, 16, 3
VIEWS = (1, 4, 8)
CHILD_LIMIT_S = 240


def child(V, only, iters, reps, warmup):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-dynamics_amd"), os.path.join(ROOT, "tests")]
    import torch
    from diff_gaussian_rasterization import rasterize_gaussians_views
    from hipcheck import _settings
    from util import random_gaussians, ring_camera
    dev = torch.device("cuda:0")
    g = random_gaussians(P, seed=21, scale_lo=0.005, scale_hi=0.05, sh_M=M)
    rs = [_settings(ring_camera(W, H, v=v, V=max(V, 4), sh_degree=DEG, bg=(0.1, 0.2, 0.3)), dev) for v in range(V)]
    t = {k: torch.tensor(g[k], device=dev, requires_grad=True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
    dc = torch.rand((V, 3, H, W), device=dev) - 0.5

    def step(on):
        out = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                                        batched_sh=on)
        (out[0] * dc).sum().backward()
        for x in list(t.values()) + [m2]:
            x.grad = None

    def one_pass(on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            step(on)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters
    modes = (False, True) if only is None else (only == "on",)
    for on in modes:
        for _ in range(max(warmup, 1)):
            step(on)
    passes = {on: [] for on in modes}
    for _ in range(reps):          # alternated: a drift of the machine lands on both paths
        for on in modes:
            passes[on].append(one_pass(on))
    med = {on: statistics.median(v) for on, v in passes.items()}
    if only is None:
        print(f"V={V}: batched_sh off {med[False]:.3f} ms, on {med[True]:.3f} ms, on/off {med[True] / med[False]:.3f}  "
              f"(median of {reps} passes of {iters} steps; off passes {min(passes[False]):.3f}..{max(passes[False]):.3f}, "
              f"on passes {min(passes[True]):.3f}..{max(passes[True]):.3f})", flush=True)
    else:
        print(f"V={V}: batched_sh {only} {med[modes[0]]:.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int)
    ap.add_argument("--only", choices=("on", "off"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.only, a.iters, max(a.reps, 1), a.warmup)
    print(f"rasterize_gaussians_views(shs=...) fwd + bwd, {W} x {H}, P = {P}, M = {M}, degree {DEG}, all gradients", flush=True)
    for V in VIEWS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(V), "--iters", str(a.iters), "--reps", str(a.reps),
                            "--warmup", str(a.warmup)], timeout=CHILD_LIMIT_S)
        if r.returncode != 0:
            sys.exit(f"V={V}: the child ended with status {r.returncode}; stopping")


if __name__ == "__main__":
    main()
