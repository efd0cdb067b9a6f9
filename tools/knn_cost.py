"""The cost of the neighbour search (profiles/knn_cost.txt): the dense path of ``make_rigidity_variables`` / ``remove_statistical_outliers``
(``torch.cdist`` of 4096 rows against all points, then ``torch.topk``) against ``gsdyn.knn_points`` (csrc/gsr_knn.hip) on the same GPU and the
same tensors, for the two calls of the pipelines -- (k = 21, exclude_self): the rigidity lists; (k = 50): one pass of the outlier filter --
on two kinds of cloud at N in {10 000, 70 000, 500 000}: SynthScene-v1 positions (uniform in a cube) and a tabletop cloud (U(0,1)^3 x (0.5,
0.5, 0.02) plus 1 % outliers in U(-3, 3)^3).
Medians of ``--reps`` passes that alternate between the paths (a drift of the machine lands on both), each pass synchronised at both ends,
behind one warm-up pass of each; the spread is (max - min) of the passes.  From ``--dense-sample-from`` points on, the dense path is timed
on 4 of its chunks and scaled to all of them; the table says so.  Per shape also: the share of queries the brute-force pass finished, the
mean shells per query of the others, and the cell-size rule's occupancy (points per occupied cell).
``--scales``: additionally time the grid path with other factors of the cell-size rule (GSR_KNN_CELL_SCALE, read per call).

    python tools/knn_cost.py [--out profiles/knn_cost.txt] [--reps 5] [--sizes 10000,70000,500000] [--scales 0.75,1.5]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-dynamics_amd")]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_cost.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="10000,70000,500000")
    ap.add_argument("--scales", default="")
    ap.add_argument("--dense-sample-from", type=int, default=200_000)
    a = ap.parse_args()
    import torch
    from diff_gaussian_rasterization import _hip
    from gsdyn import knn_points, synth_scene_params
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def tabletop(n):
        g = torch.Generator().manual_seed(n)
        n_out = n // 100
        slab = torch.rand(n - n_out, 3, generator=g) * torch.tensor([0.5, 0.5, 0.02])
        out = torch.rand(n_out, 3, generator=g) * 6 - 3
        return torch.cat([slab, out])[torch.randperm(n, generator=g)].contiguous().to(dev)

    clouds = {"synth (cube)": lambda n: synth_scene_params(n, device=dev)["means3D"].detach().contiguous(), "tabletop + 1 % far": tabletop}
    say(f"knn_cost: {torch.cuda.get_device_name(0)}, medians of {a.reps} alternating passes [ms] (spread = max - min), one warm-up pass of each")
    say(f"{'cloud':<20}{'N':>8}{'k':>4}{'self':>6}{'dense':>11}{'spread':>9}{'grid':>10}{'spread':>9}{'dense/grid':>11}  "
        f"{'brute %':>8}{'shells':>7}{'pts/cell':>9}{'cell h':>10}  note")
    scales = [float(s) for s in a.scales.split(",") if s]
    sweep = []
    for cname, make in clouds.items():
        for n in [int(s) for s in a.sizes.split(",")]:
            pts = make(n)
            starts = list(range(0, n, 4096))
            sampled = n >= a.dense_sample_from and len(starts) > 4
            use = [starts[i * (len(starts) - 1) // 4] for i in range(4)] if sampled else starts
            for k, ex in ((21, True), (50, False)):
                def dense():
                    for s in use:
                        d = torch.cdist(pts[s:s + 4096], pts)
                        if ex:      # make_rigidity_variables: k + 1 columns, the first dropped
                            dk, ik = torch.topk(d, k + 1, dim=1, largest=False)
                            dk = dk[:, 1:] ** 2
                        else:       # remove_statistical_outliers: the mean of the k smallest
                            dk = torch.topk(d, k, dim=1, largest=False)[0].mean(1)

                def grid():
                    knn_points(pts, k, exclude_self=ex)
                os.environ.pop("GSR_KNN_CELL_SCALE", None)
                t = timed({"dense": dense, "grid": grid}, a.reps)
                f = len(starts) / len(use)
                td, tg = [x * f for x in t["dense"]], t["grid"]
                st = _hip.knn(pts, k, exclude_self=ex, stats=True)[2]
                md, mg = statistics.median(td), statistics.median(tg)
                note = f"dense: {len(use)} of {len(starts)} chunks timed, scaled" if sampled else ""
                say(f"{cname:<20}{n:>8}{k:>4}{str(ex):>6}{md:>11.2f}{max(td) - min(td):>9.2f}{mg:>10.3f}{max(tg) - min(tg):>9.3f}{md / mg:>11.1f}  "
                    f"{100 * st['brute_share']:>8.2f}{st['mean_shells']:>7.2f}{st['per_cell']:>9.2f}{st['h']:>10.3g}  {note}")
                for sc in scales:
                    os.environ["GSR_KNN_CELL_SCALE"] = repr(sc)
                    ts = timed({"grid": grid}, a.reps)["grid"]
                    ss = _hip.knn(pts, k, exclude_self=ex, stats=True)[2]
                    sweep.append(f"{cname:<20}{n:>8}{k:>4}{sc:>7.2f}{statistics.median(ts):>10.3f}{max(ts) - min(ts):>9.3f}  "
                                 f"{100 * ss['brute_share']:>8.2f}{ss['mean_shells']:>7.2f}{ss['per_cell']:>9.2f}")
                os.environ.pop("GSR_KNN_CELL_SCALE", None)
            del pts
            torch.cuda.empty_cache()
    if sweep:
        say()
        say("the grid path with other factors of the cell-size rule (h = factor x median k-th neighbour distance of 256 sample queries; built-in: 1.0)")
        say(f"{'cloud':<20}{'N':>8}{'k':>4}{'factor':>7}{'grid':>10}{'spread':>9}  {'brute %':>8}{'shells':>7}{'pts/cell':>9}")
        for s in sweep:
            say(s)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
