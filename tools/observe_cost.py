"""The cost of the perception step (profiles/observe_cost.txt): ``gsdyn.depth_to_cloud`` through the kernels of csrc/gsr_voxel.hip against the
plain-torch statement of the same definition ON THE SAME DEVICE and the same tensors, and ``gsdyn.observe_state`` end to end, on a synthetic
tabletop seen by four 1280x720 cameras (the reference's rig: 3.7 M pixels per planning step) at 5 mm and at 1 mm voxels.
The scene: a board with a 1 mm ripple and a 20 x 12 x 5 cm block on it, cameras 0.9 - 1.0 m away looking at its middle, 0.5 % of the pixels
flying (a random depth), 2 % without a return (depth 0); the workspace box is 60 x 50 x 22 cm.
Medians of ``--reps`` passes that alternate between the paths (a drift of the machine lands on both), each pass synchronised at both ends,
behind one warm-up pass of each; the spread is (max - min) of the passes.  Per voxel size also: kept pixels, voxels, and the per-kernel
split of one ``depth_to_cloud`` call (the library's HIP-event timing, a run of its own).

    python tools/observe_cost.py [--out profiles/observe_cost.txt] [--reps 7] [--size 1280x720] [--voxels 0.005,0.001]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-dynamics_amd")]

CAM_POS = [(0.65, 0.55, 0.6), (-0.6, 0.6, 0.65), (-0.55, -0.65, 0.6), (0.7, -0.5, 0.55)]
BBOX = [[-0.3, 0.3], [-0.25, 0.25], [-0.02, 0.2]]


def timed(fns, reps):
    """{name: fn} -> {name: [ms per pass]}: one warm-up pass of each, then ``reps`` rounds that alternate between them."""
    import torch
    times = {k: [] for k in fns}
    for rnd in range(reps + 1):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd > 0:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def run_heads(observe, depths, K4, R, t, bbox, vs):
    """Runs of equal voxel keys among the 64 consecutive pixels of a wave: how many sets of atomics the aggregated kernel issues."""
    import torch
    g = observe._grid(bbox[:, 0], bbox[:, 1], vs, torch.float32)
    w = observe._world_torch(depths, K4, R, t).reshape(-1, 3)
    d = depths.reshape(-1)
    keep = (d > 0.0) & (d < 2.0) & observe._inside(w, g)
    c = torch.floor((w - torch.tensor(g["lo"], device=w.device)) * g["inv_h"]).to(torch.int64)
    key = torch.where(keep, (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], torch.full_like(c[:, 0], -1))
    head = torch.ones_like(keep)
    head[1:] = key[1:] != key[:-1]
    head[::64] = True
    return int((head & keep).sum())


def tabletop(V, H, W, dev):
    """depths [V, H, W], K4, R, t, colors on ``dev``: every pixel's ray is cut at the board (z = a 1 mm ripple), or at the top of the block."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(0)
    depths, K4, R, t = [], [], [], []
    for v in range(V):
        pos = torch.tensor(CAM_POS[v % 4], dtype=torch.float64)
        z = -pos / pos.norm()
        x = torch.linalg.cross(z, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        Rv = torch.stack([x, y, z], 1)
        f = 0.72 * W * (1.0 + 0.03 * v)
        k = (f, f * 1.01, 0.5 * W - 3.5 + v, 0.5 * H + 2.25 - v)
        px, py = torch.meshgrid(torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="xy")
        ray = torch.stack([(px - k[2]) / k[0], (py - k[3]) / k[1], torch.ones_like(px)], -1) @ Rv.T      # board frame
        ripple = 0.001 * torch.rand((H, W), generator=g, dtype=torch.float64)
        d_board = (ripple - pos[2]) / ray[..., 2]
        d_top = (0.05 + ripple - pos[2]) / ray[..., 2]
        hit = pos + ray * d_top[..., None]
        on_block = (hit[..., 0].abs() < 0.1) & (hit[..., 1].abs() < 0.06)
        d = torch.where(on_block, d_top, d_board)
        u = torch.rand((H, W), generator=g)
        d = torch.where(u < 0.005, torch.rand((H, W), generator=g, dtype=torch.float64) * 1.5 + 0.2, d)
        d = torch.where(u > 0.98, torch.zeros_like(d), d)
        depths.append(d.float())
        K4.append(torch.tensor(k, dtype=torch.float32))
        R.append(Rv.float())
        t.append(pos.float())
    colors = torch.randint(0, 256, (V, H, W, 3), generator=g, dtype=torch.uint8)
    return [torch.stack(a).contiguous().to(dev) for a in (depths, K4, R, t)] + [colors.to(dev)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "observe_cost.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--voxels", default="0.005,0.001")
    a = ap.parse_args()
    import numpy as np
    import torch
    from diff_gaussian_rasterization import _hip
    from gsdyn import depth_to_cloud, observe, observe_state
    dev = torch.device("cuda:0")
    W, H = (int(s) for s in a.size.split("x"))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    depths, K4, R, t, colors = tabletop(a.views, H, W, dev)
    bbox = np.array(BBOX, np.float32)
    say(f"observe_cost: {torch.cuda.get_device_name(0)}, {a.views} views of {W}x{H} ({depths.numel()} pixels), medians of {a.reps} alternating passes [ms] "
        f"(spread = max - min), one warm-up pass of each; colours given")
    say(f"{'voxel':>7}{'kept px':>10}{'voxels':>9}{'kernels':>10}{'spread':>9}{'torch':>10}{'spread':>9}{'torch/kernels':>14}{'observe_state':>15}{'spread':>9}{'state rows':>11}")
    splits, forms = [], []
    for vs in [float(s) for s in a.voxels.split(",") if s]:
        def kernels():
            return depth_to_cloud(depths, K4, R, t, bbox, colors=colors, voxel_size=vs)

        def fallback():
            keep = observe.KERNEL_MAX_N
            observe.KERNEL_MAX_N = 0          # nobody is small enough for the kernels: the plain-torch statement runs, on the device
            try:
                return depth_to_cloud(depths, K4, R, t, bbox, colors=colors, voxel_size=vs)
            finally:
                observe.KERNEL_MAX_N = keep

        def per_lane():
            os.environ["GSR_VOXEL_PER_LANE"] = "1"      # read per call: every kept pixel issues its own atomics (the form that was not kept)
            try:
                return depth_to_cloud(depths, K4, R, t, bbox, colors=colors, voxel_size=vs)
            finally:
                os.environ.pop("GSR_VOXEL_PER_LANE", None)

        def state():
            return observe_state(depths, K4, R, t, bbox, colors=colors, voxel_size=vs)
        one, two, three = kernels(), fallback(), per_lane()
        same = all(torch.equal(one[k], two[k]) and torch.equal(one[k], three[k]) for k in one)
        tt = timed({"kernels": kernels, "torch": fallback, "per_lane": per_lane}, a.reps)
        ts = timed({"state": state}, max(3, a.reps // 2))["state"]
        rows = int(state()["state"].shape[0])
        mk, mt, ms = (statistics.median(x) for x in (tt["kernels"], tt["torch"], ts))
        say(f"{vs:>7.3f}{int(one['counts'].sum()):>10}{one['points'].shape[0]:>9}{mk:>10.3f}{max(tt['kernels']) - min(tt['kernels']):>9.3f}{mt:>10.2f}"
            f"{max(tt['torch']) - min(tt['torch']):>9.2f}{mt / mk:>14.1f}{ms:>15.2f}{max(ts) - min(ts):>9.2f}{rows:>11}"
            + ("" if same else "   KERNELS AND TORCH DIFFER"))
        torch.cuda.synchronize()
        _hip.profile_begin()
        kernels()
        torch.cuda.synchronize()
        prof = _hip.profile_end()
        _hip.profile_begin()
        per_lane()
        torch.cuda.synchronize()
        naive = _hip.profile_end()["vox_depth"][0] * 1e3
        runs = run_heads(observe, depths, K4, R, t, bbox, vs)
        forms.append(f"{vs:>7.3f}{statistics.median(tt['per_lane']):>12.3f}{max(tt['per_lane']) - min(tt['per_lane']):>9.3f}{mk:>12.3f}{naive:>14.1f}"
                     f"{prof['vox_depth'][0] * 1e3:>14.1f}{runs:>12}{int(one['counts'].sum()) / max(runs, 1):>10.2f}")
        splits.append(f"{vs:>7.3f}  " + ", ".join(f"{k} {ms_ * 1e3:.1f}" for k, (ms_, _) in sorted(prof.items(), key=lambda kv: -kv[1][0])) +
                      f"  (sum {sum(v[0] for v in prof.values()) * 1e3:.1f}; the four clears of the scratch are not in it)")
    say()
    say("the accumulation: one set of atomics per kept pixel (GSR_VOXEL_PER_LANE=1; tried, not kept) against one per run of equal keys among the lanes of a wave (built)")
    say("(call times in ms as above; 'its kernel' = vox_depth alone, HIP events; runs = sets of atomics the built form issues)")
    say(f"{'voxel':>7}{'per pixel':>12}{'spread':>9}{'per run':>12}{'its kernel us':>14}{'its kernel us':>14}{'runs':>12}{'px / run':>10}")
    for s in forms:
        say(s)
    say()
    say("per-kernel split of one depth_to_cloud call [us] (HIP events around every launch, a run of its own: the events serialise the launches)")
    for s in splits:
        say(s)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
