#!/usr/bin/env python
"""bench.py -- fwd+bwd Mpix/s of the differentiable Gaussian rasterizer on MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W`` (N>1: launched by torch.distributed.run, one rank per GPU
over RCCL).  One STEP = one optimiser step of the tracking loop's rasterizer path over one batch of synthetic views
(/root/reference/src/tracking/train_gs.py:25-39):

  default, N = 1 -- BASELINE.json's metric configuration (configs[2]): 4 views (800x800) of SynthScene-v1 (100 000 Gaussians), fused
             activations + colour render forward + backward with ALL gradients (fixed seeded dL/dcolour), no optimiser step.
             value = 4*H*W / t_step.  The same JSON line carries ``scale_n1``: the 8-view + Adam step below on this one GPU.
  default, N > 1 -- STRONG scaling on BASELINE.json configs[3]: ONE fixed step of 8 views; rank r renders views r, r+N, ...
             Timed region = fused activations + forward + backward for the rank's views (the per-Gaussian backward kernel writes the
             parameter gradients straight into the flat 17-float-per-Gaussian bucket) + ONE RCCL all-reduce of that bucket + the Adam
             step (FusedAdam, one launch).  value = 8*H*W / t_step; compare with the N = 1 run's ``scale_n1.value``.  The line also
             reports ``rccl_ranks`` (sum of ones over the communicator), per-rank step time min / max, and the all-reduce alone.
             ``--config 3`` = ``--views 4 --no-optimizer``; ``--views 8`` on one GPU = the scale_n1 step as the top-level line.
  --weak  -- weak scaling: every rank renders ``--views`` (default 4) views of a 4N-camera ring, then all-reduce + Adam.
  --config 5 -- forward only, BASELINE.json configs[4]: 500k Gaussians, 1920x1080, predict.py's frame (4 cameras x colour +
             mask render), (frame, camera) pairs sharded over the ranks, no collective (gsdyn/predict.py).

Inputs are resident in HBM before the timed region.  Prints ONE JSON line on rank 0 with the contract's keys plus
  "roofline":     dominant kernel: algorithmic bytes per launch / HIP-event duration vs 8 TB/s, per-kernel fractions,
                  measured-peak VALU model (tools/micro/valu_table.hip), replayed PMC traffic (flagged "replayed")
  "cpu_baseline": the CPU oracle (kind "port": the reference has no CPU path and its CUDA extension is absent)
                  timed on this box's host cores on ONE view fwd+bwd of the same workload.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "gs-dynamics_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

P_GAUSS, W, H = 100_000, 800, 800
HBM_PEAK = 8.0e12       # B/s, MI355X spec (MI355X_MICROARCH.md)
HBM_ACHIEVABLE_GBPS = 6300.0   # GB/s a streaming kernel reaches (VERDICT r04 item 2 asks for the fractions against it too)
VALU_PEAK = 78.6e12     # fp32 lane-instructions/s at 2.4 GHz: one wave-64 op per 2 cycles per SIMD (157.3 TFLOP/s / 2)


def algorithmic_bytes(P, D, Npx):
    """SURVEY.md section 8d compulsory traffic per view, per kernel group (bytes)."""
    return {
        "preprocess_fwd": 116 * P, "scan": 8 * P, "emit_entries": 24 * P + 12 * D, "sort": 24 * D,
        "tile_ranges": 8 * D, "render_fwd": 44 * D + 24 * Npx, "render_bwd": 76 * D + 20 * Npx,
        "preprocess_bwd": 140 * P,
        "fwd": 148 * P + 88 * D + 24 * Npx, "bwd": 140 * P + 76 * D + 20 * Npx,
        "total": 288 * P + 164 * D + 44 * Npx,
    }


# kernel name (GSR_PROF label in libgsr_hip.so) -> section-8d group
KERNEL_GROUP = {"preprocess_fwd": "preprocess_fwd", "scan_exclusive": "scan", "emit_entries": "emit_entries", "radix_hist": "sort",
                "bin_count": "emit_entries", "bin_emit": "emit_entries", "bin_scan": "tile_ranges", "bin_scan_order": "tile_ranges",
                "bin_colprefix": "tile_ranges",
                "radix_scatter": "sort", "tile_sort": "sort", "tile_ranges": "tile_ranges", "tile_order": "tile_ranges",
                "render_fwd": "render_fwd", "render_bwd": "render_bwd", "preprocess_bwd_views": "preprocess_bwd",
                "preprocess_bwd": "preprocess_bwd"}


PROFILE_ROUND = "r06"      # the round whose committed rocprofv3 --pmc runs (tools/prof_round.sh) the roofline object replays: this one, never an older one


def _load_json(name):
    try:
        return json.load(open(os.path.join(ROOT, "profiles", name)))
    except Exception:  # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--views", type=int, default=None, help="views of the step (strong scaling: total, default 8; --weak: per rank, default 4)")
    ap.add_argument("--weak", action="store_true", help="weak scaling: --views views per rank")
    ap.add_argument("--config", type=int, default=4, choices=(3, 4, 5), help="3 = --views 4 --no-optimizer on one GPU; 5 = forward-only predict frame")
    ap.add_argument("--no-optimizer", action="store_true", help="leave the Adam step out of the timed region")
    ap.add_argument("--autograd", action="store_true", help="go through rasterize_gaussians_views + autograd (round-1 call pattern) instead of "
                    "the direct library calls of gsdyn.step.render_step_views")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--frozen-colours", action="store_true",
                    help="rgb_colors.requires_grad = False as in the reference's training (train_utils.py:133): no colour gradient is computed. "
                         "The default keeps ALL gradients (the metric's 'all backward gradients'); an N = 1 run reports this variant as "
                         "``frozen_colours``")
    ap.add_argument("--no-extras", action="store_true", help="skip the get_loss-shaped step and the other secondary timings")
    ap.add_argument("--with-rollout", action="store_true", help="--config 5: run gsdyn.predict.predict_episode (GNN rollout + sharded renders, "
                    "one call per rank) over --steps frames and report rollout ms and render ms separately")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step (rank 0) as DIR/<name>.npy "
                         "(float32 / float64, at most 64 MB in all: larger outputs are cut to a fixed seeded sample)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.config == 5 and args.with_rollout and args.steps < 2:
        ap.error("--config 5 --with-rollout: --steps must be at least 2 (the rollout needs two frames)")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU path exists)")
    single_dev = os.environ.get("GSR_BENCH_SINGLE_DEVICE") == "1"   # smoke test of the N > 1 code path on a 1-GPU box
    # GSR_BENCH_FORCE_DIST=1 with one rank: the `nccl` (= RCCL) process group is created all the same and the step runs its reduce leg --
    # bucket packing, ONE RCCL all-reduce on the flat bucket, the all-reduce timing pass -- over a communicator of one: what a 1-GPU box can
    # execute of the N > 1 path's RCCL calls (tests/test_multirank_gpu.py)
    force_dist = os.environ.get("GSR_BENCH_FORCE_DIST") == "1" and world == 1
    if single_dev:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if single_dev:   # all ranks share cuda:0; the collective goes through gloo on a host copy (NOT a perf number)
            dist.init_process_group("gloo", rank=rank, world_size=world)
            _ar = dist.all_reduce

            def _host_all_reduce(t, *a, **k):
                h = t.cpu()
                _ar(h, *a, **k)
                t.copy_(h)
            dist.all_reduce = _host_all_reduce
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    if force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    rccl_ranks = None
    if (world > 1 and not single_dev) or force_dist:      # one RCCL all-reduce of ones before anything is timed: the communicator exists and spans `world` ranks
        ones = torch.ones((1,), device=dev)
        dist.all_reduce(ones)
        rccl_ranks = int(ones.item())
        assert rccl_ranks == dist.get_world_size() == world, (rccl_ranks, world)
        _flush_c_stdio()                   # RCCL's banner leaves every rank's C stdout buffer now, not at exit behind the JSON line

    if args.gpus != world and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)

    if args.config == 5:
        return bench_config5(args, dev, rank, world)
    if args.config == 3:
        args.views, args.no_optimizer = args.views or 4, True

    from diff_gaussian_rasterization import _hip, rasterize_gaussians_views
    from gsdyn import initialize_optimizer, params2rendervar, synth_ring_cameras, synth_scene_params
    from gsdyn.dp import GradBucket, shard_views
    from gsdyn.step import params2rendervar_fused, render_step_views

    rng = np.random.default_rng(1234)
    GRAD_KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
    Npx = H * W

    def timed(fn, steps, warmup):
        """(wall mean s, median of per-step HIP-event s) of `steps` steps after `warmup`, bracketed as the contract says."""
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        t0 = time.perf_counter()
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        t_local = (time.perf_counter() - t0) / steps       # this rank's own time, before it waits for the others
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        return dt, statistics.median(a.elapsed_time(b) for a, b in evs) * 1e-3, t_local

    def measure(total_views, view_ids, with_opt, frozen_colours, want_roofline=True, dump_dir=None):
        """One configuration: the step over `view_ids` of a `total_views`-camera ring (this rank's share), timed per the contract.
        ``dump_dir``: write the outputs of the last timed step there (``dump_outputs``)."""
        cams_all = synth_ring_cameras(total_views, W, H, device=dev)
        dL_all = torch.tensor(np.random.default_rng(1234).uniform(-1, 1, (total_views, 3, H, W)).astype(np.float32), device=dev)
        params = synth_scene_params(P_GAUSS, seed=0, device=dev)
        params["rgb_colors"].requires_grad_(not frozen_colours)   # default: colour gradient computed and reduced (the 17-float bucket of 8e);
        cams = [cams_all[i] for i in view_ids]                     # frozen: the reference's own setting (train_utils.py:133, lr 0 at :155)
        dL = dL_all[view_ids].contiguous() if view_ids else dL_all[:0]
        bucket = GradBucket(params)
        opt = initialize_optimizer(params, 4.0) if with_opt else None     # gsdyn.optim.FusedAdam: one launch for all groups
        m2 = torch.zeros((len(cams), P_GAUSS, 3), device=dev, requires_grad=True) if args.autograd else None
        with_reduce = world > 1 or force_dist
        grad_out = bucket.views() if with_reduce else None     # the backward writes straight into the all-reduce bucket (no packing copy)
        ar_ev = [None]           # (start, end) HIP events around the all-reduce of ONE step, set by the separate pass below
        last = {}                # the per-view outputs of the latest step (references only: nothing is copied in the timed region)

        def step():
            bucket.zero()
            if cams:
                if args.autograd:
                    rv = params2rendervar_fused(params)
                    im, _, _ = rasterize_gaussians_views(cams, rv["means3D"], m2, rv["opacities"], colors_precomp=rv["colors_precomp"],
                                                         scales=rv["scales"], rotations=rv["rotations"])
                    im.backward(gradient=dL)
                    last["images"] = im
                    m2.grad = None
                else:
                    ims, g = render_step_views(params, cams, dL, want_colour_grad=not frozen_colours, grad_out=grad_out)
                    last.update(images=ims, means2D=g["means2D"], radii=g["radii"])
                    for k in GRAD_KEYS:
                        params[k].grad = g.get(k)
            if with_reduce:
                if ar_ev[0] is not None:
                    ar_ev[0][0].record()
                if force_dist:               # (a communicator of one: GradBucket.all_reduce would skip the collective)
                    dist.all_reduce(bucket.pack())
                else:
                    bucket.all_reduce()      # gradients already sit in the flat bucket: ONE all-reduce, .grad = bucket slices
                if ar_ev[0] is not None:
                    ar_ev[0][1].record()
            if opt is not None:
                opt.step()

        # entry counts per view, once (spy on the backend call; not in the timed region)
        num_rendered = []
        orig_b = _hip.rasterize_forward_batch

        def spy_b(*a, **k):
            k["no_host_sync"] = False
            out = orig_b(*a, **k)
            num_rendered.extend(st.num_rendered for st in out[3])
            torch.cuda.synchronize()
            for st in out[3]:
                try:
                    visit_stats.append(contributing_visits(_hip, st))
                except Exception as e:  # noqa: BLE001
                    visit_stats.append({"error": repr(e)})
            return out
        visit_stats = []
        _hip.rasterize_forward_batch = spy_b
        step()
        _hip.rasterize_forward_batch = orig_b
        torch.cuda.synchronize()
        t_step, t_event, t_local = timed(step, args.steps, args.warmup)
        if dump_dir is not None and rank == 0:     # before any further step overwrites the buffers of the last timed one
            outs = dict(last)
            outs.update({f"grad_{k}": params[k].grad for k in GRAD_KEYS if params[k].grad is not None})
            if with_opt:
                outs.update({f"param_{k}": params[k] for k in GRAD_KEYS})
            dump_outputs(dump_dir, outs)
        t_min = t_max = t_local
        if world > 1:
            t = torch.tensor([t_step, t_event, t_local, -t_local], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            t_step, t_event, t_max, t_min = float(t[0]), float(t[1]), float(t[2]), -float(t[3])
        allreduce_us = None
        if with_reduce:      # the all-reduce alone, HIP events around bucket.all_reduce() on the compute stream, a separate pass of 5 steps
            spans = []
            for _ in range(5):
                ar_ev[0] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                step()
                torch.cuda.synchronize()
                spans.append(ar_ev[0][0].elapsed_time(ar_ev[0][1]) * 1e3)
                ar_ev[0] = None
            tt = torch.tensor([statistics.median(spans)], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            allreduce_us = float(tt[0])
        D = float(np.mean(num_rendered)) if num_rendered else 0.0
        res = {"value": total_views * Npx / t_step / 1e6, "unit": "Mpix/s", "ms_per_step": t_step * 1e3, "ms_per_step_event_median": t_event * 1e3,
               "num_rendered_per_view": D, "views_total": total_views, "views_on_rank0": len(cams), "optimizer_in_timed_region": bool(with_opt),
               "rank_step_ms_min": t_min * 1e3, "rank_step_ms_max": t_max * 1e3, "allreduce_us": allreduce_us,
               "grad_bucket_floats": sum(p.numel() for p in bucket.params)}
        if want_roofline:
            res["roofline"] = kernel_roofline(_hip, step, max(len(cams), 1), D, t_step, args.steps)
            good = [v for v in visit_stats if "error" not in v]
            if good and "render_bwd" in res["roofline"].get("per_kernel_us_per_launch", {}):
                visits = sum(v["visits"] for v in good) * len(visit_stats) / len(good)
                slots = sum(v["lockstep_slots_bb80"] for v in good) * len(visit_stats) / len(good)
                us = res["roofline"]["per_kernel_us_per_launch"]["render_bwd"]
                floor_us = visits / 1024.0 * BWD_VISIT_NS_PER_SIMD * 1e-3
                res["roofline"]["issue_floor"] = {
                    "kernel": "render_bwd", "contributing_visits_per_launch": visits, "ns_per_visit_per_simd": BWD_VISIT_NS_PER_SIMD,
                    "floor_us": floor_us, "measured_us": us, "frac_of_floor": floor_us / us, "lockstep_factor": slots / max(visits, 1.0),
                    "floor_times_lockstep_us": floor_us * slots / max(visits, 1.0),
                    "what": "render_bwd is VALU-issue bound, not HBM bound: visits (quad, entry pairs some pixel blended, counted in this run from the forward's "
                            "contribution bytes) x the visit body's own cost (tools/micro/visit_peak.hip, six waves per SIMD: profiles/r05_visit_peak.txt, "
                            "a committed measurement) / 1024 SIMDs; lockstep_factor = wave slots the four waves of a tile occupy per visit "
                            "(every 80-entry batch lasts as long as its longest per-quad list)"}
        return res

    default_n1 = world == 1 and not force_dist and not args.weak and args.config == 4 and args.views is None and not args.no_optimizer
    if args.weak:
        vpr = args.views or 4
        total_views = vpr * world
        my_ids = list(range(vpr * rank, vpr * rank + vpr))
    else:
        total_views = args.views or 8
        my_ids = shard_views(total_views, rank, world)

    scale_n1 = weak_n1 = frozen = extras = cpu_baseline = None
    if default_n1:
        # ONE GPU, no flags: the top-level line is the configuration BASELINE.json's metric is quoted on (configs[2]: 4 x 800^2, fwd + bwd,
        # all gradients, no optimiser); the 8-view + Adam step of configs[3] -- what `--gpus N` times on N > 1 -- rides along as `scale_n1`
        main_res = measure(4, list(range(4)), False, args.frozen_colours, dump_dir=args.dump_outputs)
        scale_n1 = measure(8, list(range(8)), True, args.frozen_colours)
        scale_n1["workload"] = ("configs[3] on ONE GPU: the fixed 8-view step (8x800^2, 100k Gaussians) fwd+bwd + Adam, all 8 views on this rank -- "
                                "the N = 1 point of the strong-scaling curve `bench.py --gpus N` measures (N > 1: views r, r+N, ... per rank + 1 RCCL all-reduce)")
        # ... and the per-GPU work of a WEAK-scaling run (`--weak`: 4 views per rank + Adam; N ranks render a 4N-camera ring) as `weak_n1`:
        # the N = 1 point of the curve whose per-GPU work does not shrink with N
        weak_n1 = measure(4, list(range(4)), True, args.frozen_colours, want_roofline=False)
        weak_n1["workload"] = ("`bench.py --weak --gpus N` at N = 1: 4 views per GPU (4x800^2, 100k Gaussians) fwd+bwd + Adam; N > 1: every rank renders its own 4 "
                               "cameras of a 4N-camera ring, then 1 RCCL all-reduce of the gradient bucket.  Strong scaling of the fixed 8-view step (scale_n1) is "
                               "predicted at 3.1 - 3.5x on 8 GPUs (DESIGN.md section 7: one view's dependent kernel chain + the all-reduce are floor terms)")
        total_views, my_ids, with_opt = 4, list(range(4)), False
    else:
        with_opt = not args.no_optimizer
        main_res = measure(total_views, my_ids, with_opt, args.frozen_colours, dump_dir=args.dump_outputs)
    if rank == 0 and world == 1 and not args.weak and args.config == 4 and not args.no_extras and not args.frozen_colours and not args.autograd:
        # the 8-view step with rgb_colors frozen, as the reference trains (no dL/dcolour: six sums per list entry)
        frozen = measure(8, list(range(8)), True, True, want_roofline=False)
        frozen["workload"] = ("the 8-view + Adam step with rgb_colors.requires_grad = False (/root/reference/src/tracking/train_utils.py:133,155): "
                              "every gradient the reference's optimiser uses, no dL/dcolour")
    if rank == 0 and world == 1 and not args.no_extras:
        extras = run_extras(dev, synth_scene_params(P_GAUSS, seed=0, device=dev), synth_ring_cameras(4, W, H, device=dev),
                            synth_ring_cameras, synth_scene_params)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cam0 = synth_ring_cameras(total_views, W, H, device=dev)[0]
        dL0 = torch.tensor(rng.uniform(-1, 1, (3, H, W)).astype(np.float32), device=dev)
        cpu_baseline = run_cpu_baseline(synth_scene_params(P_GAUSS, seed=0, device=dev), cam0, dL0, params2rendervar)

    if rank == 0:
        n_on0 = main_res["views_on_rank0"]
        cfg_name = "configs[2]" if (total_views == 4 and not with_opt and world == 1) else ("configs[3]" if total_views == 8 and not args.weak else "custom")
        if args.weak:
            workload = f"weak scaling: {n_on0} views per GPU of a {total_views}-camera ring, 100k Gaussians, 800x800, fwd+bwd" + ("+Adam" if with_opt else "")
        else:
            workload = (f"{cfg_name}: {total_views}x800^2 views, 100k Gaussians, fwd+bwd (all grads)" + ("+Adam" if with_opt else ", no optimiser") +
                        f", {world} GPU(s)" + (" strong scaling" if world > 1 or total_views == 8 else "") + "; SynthScene-v1")
        workload += (f"; view r -> rank r mod N ({n_on0} on rank 0), colour render fwd+bwd per view" +
                     (" (rgb_colors frozen: no colour gradient)" if args.frozen_colours else "") +
                     ("" if world == 1 else f", backward writes into the {main_res['grad_bucket_floats']}-float bucket, 1 RCCL all-reduce") +
                     (", Adam step (FusedAdam)" if with_opt else "") +
                     ("; the 8-view + Adam step of configs[3] on this GPU: see scale_n1" if default_n1 else ""))
        line = {
            "metric": f"fwd+bwd Mpix/s at 100k Gaussians, {total_views}x800^2 views",
            "value": main_res["value"], "unit": "Mpix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": main_res["ms_per_step"], "ms_per_step_event_median": main_res["ms_per_step_event_median"], "higher_is_better": True,
            "scaling": "weak" if args.weak else "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload, "gaussians": P_GAUSS, "views_total": total_views, "views_on_rank0": n_on0, "image": [H, W],
                       "num_rendered_per_view": main_res["num_rendered_per_view"], "parallelism": f"view-sharded dp{world}",
                       "grad_bucket_floats": main_res["grad_bucket_floats"], "optimizer_in_timed_region": with_opt,
                       "call_pattern": "rasterize_gaussians_views + autograd" if args.autograd else
                                       "gsdyn.step.render_step_views: activations, ONE multi-view forward (capacity mode), ONE multi-view backward, direct library calls"},
            "roofline": main_res.get("roofline"),
            "rccl_ranks": rccl_ranks, "rank_step_ms_min": main_res["rank_step_ms_min"], "rank_step_ms_max": main_res["rank_step_ms_max"],
            "allreduce_us": main_res["allreduce_us"],
            "scale_n1": scale_n1, "weak_n1": weak_n1, "frozen_colours": frozen, "cpu_baseline": cpu_baseline, "extras": extras,
        }
        _emit(line)
    if world > 1 or force_dist:
        dist.destroy_process_group()
        _flush_c_stdio()


DUMP_BUDGET_BYTES = 64_000_000


def dump_outputs(out_dir, arrays):
    """``arrays`` (name -> tensor) as ``out_dir/<name>.npy``: float64 stays float64, everything else becomes float32.  At most
    DUMP_BUDGET_BYTES in all: taken smallest first, an array larger than an even share of what is left is cut to a sample of its
    flattened elements at indices drawn from a generator seeded by its name and size -- the same elements in every run."""
    import zlib
    os.makedirs(out_dir, exist_ok=True)
    host = {}
    for k, t in arrays.items():
        if t is None:
            continue
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        host[k] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    left, sampled = DUMP_BUDGET_BYTES - 256 * len(host), []      # (room for the .npy headers)
    for i, k in enumerate(sorted(host, key=lambda k: (host[k].nbytes, k))):
        a = host[k]
        share = left // (len(host) - i)
        if a.nbytes > share:
            n = share // a.itemsize
            idx = np.sort(np.random.default_rng(zlib.crc32(f"{k}:{a.size}".encode())).choice(a.size, n, replace=False))
            a = a.reshape(-1)[idx]
            sampled.append(k)
        np.save(os.path.join(out_dir, f"{k}.npy"), a)
        left -= a.nbytes
    print(f"[bench] wrote {len(host)} outputs to {out_dir}" + (f" (sampled: {', '.join(sampled)})" if sampled else ""), file=sys.stderr)


def _flush_c_stdio():
    """RCCL writes its version banner to the C stdout stream at communicator creation; behind a pipe that buffer is flushed at exit, i.e.
    AFTER anything Python printed.  Flush it now so that the JSON line is the last thing on stdout."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001
        pass


def _emit(line):
    """The ONE JSON line of the contract, as the last line of stdout."""
    _flush_c_stdio()
    sys.stdout.write(json.dumps(line) + "\n")
    sys.stdout.flush()


BWD_VISIT_NS_PER_SIMD = 103.3      # profiles/r05_visit_peak.txt: the backward's visit body alone, six waves per SIMD


def contributing_visits(_hip, st):
    """(quad, entry) visits of one view's backward, from the contribution bytes the tracking forward left behind the tile lists (the last
    align256(D) bytes of the binning state), restricted to the entries below each tile's deepest used position; and the wave slots the
    lockstep of a tile's four waves makes of them (batches of 80 entries)."""
    D, H, W = int(st.num_rendered), int(st.H), int(st.W)
    v = _hip.debug_views(st)
    rg = v["ranges"].cpu().numpy().astype(np.int64)
    nc = v["n_contrib"].cpu().numpy()
    gy, gx = (H + 15) // 16, (W + 15) // 16
    pad = np.zeros((gy * 16, gx * 16), nc.dtype)
    pad[:H, :W] = nc
    max_last = pad.reshape(gy, 16, gx, 16).max((1, 3)).reshape(-1).astype(np.int64)
    # where gsr_carve_binning (csrc/gsr_common.h) puts the bytes for D entries: behind tkey[2] (4 D each), dg[2] (8 D each), point_list (4 D) and
    # the radix block histograms (1 KiB x (ceil(D / 2048) + 1)), every sub-array 256-byte aligned.  (The spied call is synchronous: the
    # library carves its states with the true entry count, whatever size the caller's buffer has.)
    al = lambda x: (x + 255) // 256 * 256      # noqa: E731
    nb = max(1, (D + 2047) // 2048)
    off = 2 * al(4 * D) + 2 * al(8 * D) + al(4 * D) + al(1024 * (nb + 1))
    c = st.binning[off:off + D].cpu().numpy()
    pop = np.unpackbits(c[:, None], axis=1)[:, 4:]
    visits = slots = 0
    for t in range(rg.shape[0]):
        lo, ml = rg[t, 0], max_last[t]
        if ml <= 0:
            continue
        bits = pop[lo:lo + ml][::-1]
        nb = (ml + 79) // 80
        padb = np.zeros((nb * 80, 4), np.int64)
        padb[:ml] = bits
        per = padb.reshape(nb, 80, 4).sum(1)
        visits += int(per.sum())
        slots += int(4 * per.max(1).sum())
    return {"visits": visits, "lockstep_slots_bb80": slots}


def kernel_roofline(_hip, step, vpl, D, t_step, steps):
    """The ``roofline`` object of a step: per-kernel HIP-event pass (outside the timed region, same call pattern), algorithmic bytes of
    SURVEY.md section 8d per kernel group, dominant kernel = the slower blend kernel.  ``vpl``: views per launch on this rank."""
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    _hip.profile_begin()
    prof_steps = max(3, min(10, steps))
    for _ in range(prof_steps):
        step()
    torch.cuda.synchronize()
    prof = _hip.profile_end()
    per_launch_us = {k: 1e3 * ms / max(n, 1) for k, (ms, n) in prof.items()}
    per_step_us = {k: 1e3 * ms / prof_steps for k, (ms, n) in prof.items()}
    busy_us = sum(per_step_us.values())
    Npx = H * W
    ab = algorithmic_bytes(P_GAUSS, D, Npx)
    path_bytes = vpl * ab["total"]
    dom = max((k for k in per_step_us if k in ("render_fwd", "render_bwd")), key=lambda k: per_step_us[k], default="render_bwd")
    dom_us = per_launch_us.get(dom, float("nan"))
    dom_bytes = ab[dom] * vpl
    dom_achieved = dom_bytes / (dom_us * 1e-6) / 1e9 if dom_us == dom_us and dom_us > 0 else None
    groups = {}
    for k, us in per_step_us.items():
        g = KERNEL_GROUP.get(k)
        if g:
            groups.setdefault(g, {"kernels": [], "us_per_step": 0.0})
            groups[g]["kernels"].append(k)
            groups[g]["us_per_step"] += us
    per_kernel = {}
    for g, v in groups.items():
        b = ab[g] * vpl
        gbps = b / (v["us_per_step"] * 1e-6) / 1e9 if v["us_per_step"] > 0 else None
        per_kernel[g] = {"kernels": sorted(v["kernels"]), "us_per_step": round(v["us_per_step"], 2), "algorithmic_MB_per_step": round(b / 1e6, 2),
                         "GBps": round(gbps, 1) if gbps else None, "frac_of_hbm_peak": round(gbps / (HBM_PEAK / 1e9), 4) if gbps else None,
                         "frac_of_hbm_achievable": round(gbps / HBM_ACHIEVABLE_GBPS, 4) if gbps else None}
    roofline = {
        "bound": "hbm", "kernel": dom, "achieved": dom_achieved, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
        "frac": (dom_achieved / (HBM_PEAK / 1e9)) if dom_achieved else None, "traffic": None,
        "algorithmic_bytes_per_launch": dom_bytes, "views_per_launch": vpl, "avg_launch_us": dom_us,
        "path": {"algorithmic_bytes_per_step_per_gpu": path_bytes, "achieved_GBps": path_bytes / t_step / 1e9,
                 "frac_of_hbm_peak": path_bytes / t_step / HBM_PEAK, "frac_of_hbm_achievable": path_bytes / t_step / 1e9 / HBM_ACHIEVABLE_GBPS},
        "hbm_achievable_GBps": HBM_ACHIEVABLE_GBPS,      # what a streaming copy reaches on this part (MI355X_MICROARCH.md); `frac` stays against the 8 TB/s peak
        "per_kernel": per_kernel,
        "per_kernel_us_per_launch": {k: round(v, 2) for k, v in sorted(per_launch_us.items())},
        "gsr_kernels_busy_us_per_step": round(busy_us, 1), "step_us": round(t_step * 1e6, 1),
        "per_kernel_timing": "HIP events around every launch of the library (on the launch stream), separate pass after the timed region, same call pattern",
        "frac_source": "in-run HIP events (this run); the rocprofv3 --kernel-trace --stats averages of the same command are committed as "
                       f"profiles/{PROFILE_ROUND}_kernel_stats_v{vpl}.txt (blend kernels read 3-5 % longer there, the small kernels shorter): "
                       "`frac_rocprof` below is the same fraction from that file's average, when it is in the tree",
    }
    # the same fraction from the committed rocprofv3 --kernel-trace --stats summary of this command (what a reader recomputing from profiles/ gets)
    try:
        for ln in open(os.path.join(ROOT, "profiles", f"{PROFILE_ROUND}_kernel_stats_v{vpl}.txt")):
            f = ln.split()
            if len(f) == 5 and f[0] == dom:
                roofline["frac_rocprof"] = {"avg_launch_us": float(f[3]), "frac": dom_bytes / (float(f[3]) * 1e-6) / HBM_PEAK,
                                            "profile": f"profiles/{PROFILE_ROUND}_kernel_stats_v{vpl}.txt"}
    except OSError:
        pass
    # HBM traffic of the blend kernels from a committed rocprofv3 --pmc run of this round (tools/prof_round.sh), corrected with the
    # calibration factors measured on known byte counts (tools/prof_calib.sh): REPLAYED from profiles/, not measured in this run
    # (ONE named profile, no fall-back to older rounds, and refused when it was taken at another entry count)
    tj, tname = None, next((n for n in (f"{PROFILE_ROUND}_pmc_traffic_v{vpl}.json",) if _load_json(n)), None)
    if tname:
        tj = _load_json(tname)
        d_prof = float(tj.get("entries_per_view") or 0.0)
        if tj.get("views_per_launch") != vpl or dom not in tj or not D or abs(d_prof - D) > 1e-3 * D:
            roofline["traffic_detail"] = {"replayed": False, "refused": f"profiles/{tname}: views_per_launch {tj.get('views_per_launch')} / entries_per_view {d_prof} "
                                                                          f"do not match this run ({vpl} / {D})"}
            tj = None
    if tj:
        roofline["traffic"] = tj[dom]["hbm_bytes_per_launch"]
        roofline["traffic_detail"] = {"replayed": True, "profile": f"profiles/{tname}", "entries_per_view_of_profile": tj.get("entries_per_view"),
                                      "source": tj.get("source"), **{k: tj[dom].get(k) for k in
                                      ("FETCH_SIZE_KiB_raw", "WRITE_SIZE_KiB_raw", "fabric_bytes_per_launch", "note") if k in tj[dom]}}
    # VALU: measured issue model (profiles/r02_valu_table.json) + committed SQ counters (REPLAYED)
    sj = _load_json(f"{PROFILE_ROUND}_sq_counters_v{vpl}.json")
    if sj and sj.get("views_per_launch") != vpl:
        sj = None
    valu = {"peak_lane_instr_per_s_spec": VALU_PEAK,
            "measured_issue_model": "one wave-64 VALU op per ~2.2 SIMD-cycles at >= 2 waves per SIMD (1 per ~4.7 cycles from ONE wave); DPP ops ~3.0, "
                                    "v_exp/v_rcp/permlane-swap ~6.0 (tools/micro/valu_table.hip -> profiles/r02_valu_table.json)",
            "pixel_gaussian_pairs_per_view": 256.0 * D}
    if sj:
        occ = {}
        for kname in ("render_fwd", "render_bwd"):
            if kname in sj and kname in per_launch_us:
                n_valu = sj[kname].get("SQ_INSTS_VALU", 0.0)
                simd_cycles = per_launch_us[kname] * 1e-6 * sj.get("clock_hz", 2.2e9) * 1024.0
                occ[kname] = {"valu_wave_instructions": n_valu, "cycles_per_valu_instr_per_simd": simd_cycles / max(n_valu, 1.0),
                              "valu_utilisation_at_2.2_cycles_per_op": 2.2 * n_valu / simd_cycles}
        valu["measured"] = occ
        valu["measured_detail"] = {"replayed": True, "source": sj.get("source")}
    roofline["valu"] = valu
    return roofline


def bench_config5(args, dev, rank, world):
    """Forward only, BASELINE.json configs[4]: predict.py's render loop (4 cameras x (colour + all-ones mask), bg black) on 500k
    Gaussians at 1920x1080; (frame, camera) pairs sharded round-robin over the ranks, no collective (gsdyn/predict.py)."""
    from diff_gaussian_rasterization import _hip
    from gsdyn import params2rendervar, synth_scene_params
    from gsdyn.predict import FrameShard, ring_poses
    P5, W5, H5, CAMS = 500_000, 1920, 1080, 4
    params = synth_scene_params(P5, seed=0, device=dev)
    with torch.no_grad():
        data_in = {k: v.detach() for k, v in params2rendervar(params).items()}
        # once per episode, as gsdyn.predict.collect_scene_data does: the Gaussians in Morton order of their positions (the binning
        # stage's entry scatter coalesces when index neighbours are space neighbours; the images do not depend on the order)
        from gsdyn.dynamics import spatial_order
        perm = spatial_order(data_in["means3D"])
        data = {k: v[perm].contiguous() for k, v in data_in.items()}
    frames = max(args.steps, 1)
    if args.with_rollout:
        return bench_config5_episode(args, dev, rank, world, params, P5, W5, H5, CAMS)
    # every frame from scratch (speculative=False): the workload as defined.  The frame SEQUENCE with speculative depth cuts (each frame bins only
    # what the previous frame of the same cameras needed, validated by the blend, failed frames redone: gsdyn.render.DepthCuts) is timed
    # below as `ms_per_step_depth_cuts` -- on this loop's STATIC scene the guesses are perfect; the episode (--with-rollout) has the moving one.
    shard = FrameShard(dev, W5, H5, ring_poses(CAMS, W5, H5), rank, world, speculative=False)
    pairs = shard.my_pairs(frames)

    last = [{}]

    def run(n_frames, d=None):
        for f in range(n_frames):
            last[0] = shard.render_frame(f, data if d is None else d)

    num_rendered = []
    orig_b = _hip.rasterize_forward_batch

    def spy_b(*a, **k):
        out = orig_b(*a, **k)
        num_rendered.extend(st.num_rendered for st in out[3])
        return out
    _hip.rasterize_forward_batch = spy_b
    run(1)
    _hip.rasterize_forward_batch = orig_b
    run(args.warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(frames)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs is not None and rank == 0:     # this rank's cameras of the last timed frame
        dump_outputs(args.dump_outputs, {f"cam{c}_{n}": t for c, ts in last[0].items() for n, t in zip(("image", "depth", "mask"), ts)})
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    n_prof = min(frames, 5)
    _hip.profile_begin()
    run(n_prof)
    torch.cuda.synchronize()
    prof = _hip.profile_end()
    per_step_us = {k: 1e3 * ms / n_prof for k, (ms, n) in prof.items()}
    # the same frames with the mask BLENDED as the reference does (a second render with colours = 1, fused with the colour render:
    # shared lists and records) instead of taken from the colour render's final transmittance
    shard.mask_from_alpha = False
    run(2)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    run(frames)
    torch.cuda.synchronize()
    dt_blend = time.perf_counter() - t1
    shard.mask_from_alpha = True
    run(2, data_in)                                  # the Gaussians in SynthScene-v1's own (random) index order
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    run(frames, data_in)
    torch.cuda.synchronize()
    dt_input_order = time.perf_counter() - t1
    # the frame sequence with speculative depth cuts (static scene: every guess holds) + its per-kernel times
    shard_c = FrameShard(dev, W5, H5, ring_poses(CAMS, W5, H5), rank, world, speculative=True)
    sink = {}
    for f in range(3):
        shard_c.render_frame(f, data)
    shard_c.validate(sink, lambda f: data)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for f in range(frames):
        shard_c.render_frame(f, data)
    redone = shard_c.validate(sink, lambda f: data)
    torch.cuda.synchronize()
    dt_cuts = time.perf_counter() - t1
    _hip.profile_begin()
    for f in range(n_prof):
        shard_c.render_frame(f, data)
    torch.cuda.synchronize()
    prof_c = _hip.profile_end()
    shard_c.validate(sink, lambda f: data)
    per_step_us_cuts = {k: 1e3 * ms / n_prof for k, (ms, n) in prof_c.items()}
    D = float(np.mean([d for d in num_rendered if d > 0])) if any(num_rendered) else 0.0
    Npx = W5 * H5
    ab = algorithmic_bytes(P5, D, Npx)
    renders = 2 * CAMS * frames                    # colour + mask per (frame, camera) pair, all ranks together
    mpix = renders * Npx / dt / 1e6
    cams_here = len(pairs) / frames                # cameras this rank renders per frame, on average
    fwd_us = per_step_us.get("render_fwd", float("nan"))
    fwd_bytes = ab["render_fwd"] * cams_here
    if rank == 0:
        _emit(({
            "metric": "fwd Mpix/s, predict.py frame (colour + mask render per camera), 500k Gaussians, 1920x1080", "value": mpix, "unit": "Mpix/s",
            "n_gpus": world, "steps": frames, "warmup": args.warmup, "ms_per_step": dt / frames * 1e3, "higher_is_better": True,
            "ms_per_step_mask_blended": dt_blend / frames * 1e3, "ms_per_step_input_order": dt_input_order / frames * 1e3,
            "ms_per_step_depth_cuts": dt_cuts / frames * 1e3, "depth_cuts": {
                "frames_redone": len(redone), "per_kernel_us_per_frame": {k: round(v, 2) for k, v in sorted(per_step_us_cuts.items())},
                "note": "the same frames as a SEQUENCE: each frame bins only the (Gaussian, tile) pairs in front of the per-tile depth the previous frame of "
                        "the same cameras needed (x 1.01, up to 128 list positions deeper), the blend validates the guess and failed frames are rendered again "
                        "(none here: the loop's scene is static -- the best case; the deforming scene is `--with-rollout`)"},
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[4] render loop: 4 cameras x (colour + all-ones mask) per frame, (frame, camera) pairs "
                                   "sharded round-robin over ranks, no collective; the mask image = 1 - final transmittance of the colour "
                                   "render (the all-ones render's value up to fp32 rounding: ONE blend pass per camera; the frame with the mask "
                                   "blended as well is ms_per_step_mask_blended); Gaussians handed over in Morton order of their positions, permuted once outside "
                                   "the timed loop as collect_scene_data does per episode (SynthScene-v1's random index order: ms_per_step_input_order); "
                                   "GNN rollout not included", "gaussians": P5, "image": [H5, W5],
                       "cameras": CAMS, "num_rendered_per_camera": D, "pairs_on_rank0_per_frame": cams_here},
            "roofline": {"bound": "hbm", "kernel": "render_fwd", "achieved": fwd_bytes / (fwd_us * 1e-6) / 1e9 if fwd_us == fwd_us else None,
                         "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": fwd_bytes / (fwd_us * 1e-6) / HBM_PEAK if fwd_us == fwd_us else None,
                         "traffic": None, "algorithmic_bytes_per_launch": fwd_bytes,
                         "path": {"algorithmic_bytes_per_frame_per_gpu": ab["fwd"] * cams_here,
                                  "frac_of_hbm_peak": ab["fwd"] * cams_here / (dt / frames) / HBM_PEAK},
                         "per_kernel_us_per_frame": {k: round(v, 2) for k, v in sorted(per_step_us.items())}},
            "cpu_baseline": None}))
    if world > 1:
        dist.destroy_process_group()


def bench_config5_episode(args, dev, rank, world, params, P5, W5, H5, CAMS):
    """BASELINE.json configs[4] end to end: predict.py's episode (/root/reference/src/predict.py:74-164) as ONE call per rank --
    collect_scene_data (GNN rollout of --steps frames with rope.yaml-width random weights, smoothing, packing; every rank runs it) and
    this rank's (frame, camera) renders.  Rollout and render times are reported separately; value = render throughput of the episode."""
    from gsdyn.dynamics import DynamicsPredictor
    from gsdyn.predict import predict_episode, ring_poses
    cfg = dict(nf_particle=512, nf_relation=512, nf_effect=512, attr_dim=2, state_dim=0, action_dim=3, pstep=3,
               rel_attr_dim=2, rel_group_dim=1, rel_distance_dim=3, n_his=3)
    torch.manual_seed(0)
    model = DynamicsPredictor(cfg, device=dev).eval()
    frames = max(args.steps, 2)
    p = {k: v.detach() for k, v in params.items()}
    eef = torch.tensor([[0.0, 0.2, 0.0]], device=dev) + torch.tensor([[0.02, 0.0, 0.01]], device=dev) * torch.arange(frames, device=dev, dtype=torch.float32)[:, None]
    # outlier filtering (Open3D's statistical filter in the reference, a dense cdist/top-k restatement here) is left out of the timed
    # episode: it is data preparation done once per episode on frame 0 and costs seconds at 500k points either way
    roll = dict(max_nobj=100, fps_radius=0.3, adj_thresh=0.6, topk=5, connect_all=False, dist_thresh=0.005, n_fps_all=1000, remove_outliers=False)
    poses = ring_poses(CAMS, W5, H5)
    predict_episode(model, p, eef[:2], poses, W5, H5, rollout_cfg=roll, rank=rank, world=world)          # warm-up (capacities, allocator)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    out, _vis, tm = predict_episode(model, p, eef, poses, W5, H5, rollout_cfg=roll, rank=rank, world=world)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    tt = torch.tensor([dt, tm["rollout_ms"], tm["render_ms"]], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt, roll_ms, rend_ms = (float(x) for x in tt)
    # the same episode with the renders overlapped with the rollout (second host thread + second stream; frames rendered as they
    # become final): the rollout is host-issue-bound, the renders GPU-bound
    predict_episode(model, p, eef[:2], poses, W5, H5, rollout_cfg=roll, rank=rank, world=world, overlap=True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    predict_episode(model, p, eef, poses, W5, H5, rollout_cfg=roll, rank=rank, world=world, overlap=True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    to = torch.tensor([time.perf_counter() - t1], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(to, op=dist.ReduceOp.MAX)
    dt_overlap = float(to)
    if args.dump_outputs is not None and rank == 0:     # the last frame of the timed episode, this rank's cameras
        dump_outputs(args.dump_outputs, {f"cam{c}_{n}": t for (f, c), ts in out.items() if f == frames - 1
                                         for n, t in zip(("image", "depth", "mask"), ts)})
    # the pipelined episode (predict_episode(pipeline=True)): rank 0 rolls out and broadcasts one 8.8 KB skinning packet per moving step, the
    # other ranks move the Gaussians with it (one skinning launch per frame) and render.  world = 1: its two sides are timed separately
    # on this GPU -- the producer's streaming rollout with a packet hook, and a render rank's frame production from recorded packets --
    # which is what the prediction below is made of; world > 1: the episode itself is timed.
    from gsdyn.predict import collect_scene_data
    dt_pipe = prod_ms = prod_light_ms = cons_ms = None
    if world > 1:
        predict_episode(model, p, eef[:2], poses, W5, H5, rollout_cfg=roll, rank=rank, world=world, pipeline=True)
        torch.cuda.synchronize()
        dist.barrier()
        t2 = time.perf_counter()
        predict_episode(model, p, eef, poses, W5, H5, rollout_cfg=roll, rank=rank, world=world, pipeline=True)
        torch.cuda.synchronize()
        dist.barrier()
        tp = torch.tensor([time.perf_counter() - t2], device=dev, dtype=torch.float64)
        dist.all_reduce(tp, op=dist.ReduceOp.MAX)
        dt_pipe = float(tp)
    else:
        packets = {}
        noop = lambda f, d, ev: None  # noqa: E731
        for rounds in range(2):
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            collect_scene_data(model, p, eef, on_frame=noop, on_skin=lambda i, pk: packets.__setitem__(i, pk.clone()), **roll)
            torch.cuda.synchronize()
            prod_ms = (time.perf_counter() - t2) * 1e3
        for rounds in range(2):       # what the producer of predict_episode(pipeline=True) runs when it renders nothing: its tracked particles only
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            collect_scene_data(model, p, eef, on_skin=lambda i, pk: packets.__setitem__(-1, pk), tracked_only=True, **roll)
            torch.cuda.synchronize()
            prod_light_ms = (time.perf_counter() - t2) * 1e3
        for rounds in range(2):
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            collect_scene_data(None, p, eef, on_frame=noop, skin_source=lambda i: packets[i], **roll)
            torch.cuda.synchronize()
            cons_ms = (time.perf_counter() - t2) * 1e3
    if rank == 0:
        renders = 2 * CAMS * frames
        _emit(({
            "metric": "fwd Mpix/s, predict.py episode end to end (GNN rollout + colour + mask render per camera), 500k Gaussians, 1920x1080",
            "value": renders * W5 * H5 / dt / 1e6, "unit": "Mpix/s", "n_gpus": world, "steps": frames, "warmup": 1, "ms_per_step": dt / frames * 1e3,
            "ms_per_step_overlapped": dt_overlap / frames * 1e3,
            "ms_per_step_pipelined": None if dt_pipe is None else dt_pipe / frames * 1e3,
            "pipeline_parts_ms_per_frame": None if prod_ms is None else {
                "producer_rollout_streaming": prod_ms / frames, "producer_tracked_only": prod_light_ms / frames,
                "render_rank_frames_from_packets": cons_ms / frames,
                "note": "one GPU, each side alone: the rank that rolls out (sampling, relations, GNN, rotation fit, skinning, smoothing; packets "
                        "handed to a hook) -- with all Gaussians (a producer that also renders) and with its tracked particles only (the default "
                        "producer, which renders nothing: same packets) -- and a render rank's frame production from recorded packets (skinning + "
                        "smoothing; no network); `pipelined` below uses the tracked-only producer"},
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[4] END TO END: gsdyn.predict.predict_episode = rollout (every rank) + (frame, camera) pairs "
                                   "sharded round-robin, 4 cameras x (colour + mask)", "gaussians": tm["gaussians"], "image": [H5, W5], "cameras": CAMS,
                       "frames": frames, "gnn": "DynamicsPredictor width 512, pstep 3, random weights, 100 bones"},
            "depth_cuts": {"calls_with_cuts": tm.get("depth_cut_calls"), "frames_redone": tm.get("frames_redone"),
                           "note": "speculative per-tile depth cuts of the frame sequence (gsdyn.render.DepthCuts; GSDYN_DEPTH_CUTS=0 switches them off): "
                                   "validated by the blend, failed frames rendered again -- every frame handed out is exact"},
            "rollout_ms_total": roll_ms, "rollout_ms_per_frame": roll_ms / max(frames - 1, 1), "render_ms_total": rend_ms,
            "render_ms_per_frame_this_rank": rend_ms / frames, "render_only_Mpix_per_s": renders * W5 * H5 / (rend_ms * 1e-3) / 1e6,
            # the rollout is replicated on every rank (autoregressive), only the renders shard: predicted episode time per frame on N GPUs from
            # THIS run's parts (world = 1 only: render_ms is then the whole episode's renders); `overlapped` = the renders on a second
            # stream behind the rollout (predict_episode(overlap=True)): max of the two parts instead of their sum
            "predicted_ms_per_frame_by_gpus": None if world > 1 else {
                str(n): {"sequential": roll_ms / max(frames - 1, 1) + rend_ms / frames / n,
                         "overlapped": max(roll_ms / max(frames - 1, 1), rend_ms / frames / n),
                         # pipelined: the producer's rollout against a render rank's skinning + its share of the renders (N - 1 render ranks)
                         "pipelined": None if n == 1 else max(prod_light_ms / frames, cons_ms / frames + rend_ms / frames / (n - 1)),
                         "pipelined_speedup_vs_1": None if n == 1 else (roll_ms / max(frames - 1, 1) + rend_ms / frames)
                         / max(prod_light_ms / frames, cons_ms / frames + rend_ms / frames / (n - 1)),
                         "speedup_vs_1": (roll_ms / max(frames - 1, 1) + rend_ms / frames) / (roll_ms / max(frames - 1, 1) + rend_ms / frames / n)}
                for n in (1, 2, 4, 8)},
            "roofline": None, "cpu_baseline": None}))
    if world > 1:
        dist.destroy_process_group()


class _Timed(float):
    """A secondary timing: the MEDIAN of ``reps`` wall-clock passes (json sees a float); ``.min`` / ``.max`` / ``.reps`` ride along."""
    min = max = None
    reps = 0


def _median_of(passes_ms):
    v = sorted(passes_ms)
    t = _Timed(v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))
    t.min, t.max, t.reps = v[0], v[-1], len(v)
    return t


def _time_ms(fn, iters, warmup, reps=5):
    """ms per call: ``warmup`` untimed calls, then the median of ``reps`` passes of ``iters`` calls each (a single pass put a
    first-touch allocation or a capacity repeat into the number the driver recorded)."""
    for _ in range(max(warmup, 1)):
        fn()
    passes = []
    for _ in range(max(reps, 1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        passes.append((time.perf_counter() - t0) * 1e3 / iters)
    return _median_of(passes)


def run_extras(dev, params, cams, synth_ring_cameras, synth_scene_params):
    """Reported beside the headline: the full get_loss-shaped step of train_gs.py
    (2 renders + SSIM/L1 + rigidity terms + backward, per view) and BASELINE configs[1] (forward only)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gsdyn import LossWeights, get_loss, get_loss_views, loss_and_grads_views, params2rendervar, synth_targets
    from gsdyn.dp import init_variables
    from gsdyn.step import make_rigidity_variables
    out = {}
    try:
        im_gt, seg_gt = synth_targets(W, H, device=dev)
        variables = init_variables(P_GAUSS, dev)
        variables.update(make_rigidity_variables(params, num_knn=20))
        w = LossWeights(im=50.0, seg=200.0, rigid=200.0, iso=1000.0, rot=4.0, bg=200.0)  # assets/datasets.md weights
        views = [dict(cam=c, im=im_gt, seg=seg_gt, id=i) for i, c in enumerate(cams)]

        def make_step(initial, mode):
            def getloss_step():
                for p in params.values():
                    p.grad = None
                if mode == "all_direct":     # the same library calls back to back, no autograd graph
                    loss_and_grads_views(params, views, variables, initial, w)
                    return
                if mode in ("all", "all_colour_grads"):   # all cameras, colour + seg renders: ONE rasterizer call (8 views)
                    loss, _, _ = get_loss_views(params, views, variables, initial, w, frozen_colours=(mode == "all"))
                    loss.backward()
                    return
                for d in views:
                    if mode == "pair_direct":
                        loss_and_grads_views(params, [d], variables, initial, w)
                        continue
                    if mode == "pair":       # the reference's pattern, one camera per iteration: colour + seg as a 2-view call
                        loss, _, _ = get_loss_views(params, [d], variables, initial, w, frozen_colours=True)
                    else:                    # two separate GaussianRasterizer calls per camera, as train_utils.py writes it
                        loss, _ = get_loss(params, d, variables, initial, w)
                    loss.backward()
            return getloss_step
        for name, initial in (("getloss_step_t0", True), ("getloss_step", False)):
            res = {}
            for mode in ("separate", "pair", "pair_direct", "all_colour_grads", "all", "all_direct"):
                ms = _time_ms(make_step(initial, mode), 12, 4)
                res[mode] = {"ms_per_step": ms, "ms_per_view": ms / len(views)}
            out[name] = {"views": len(views), **res["all_direct"], "through_autograd": res["all"],
                         "with_seg_colour_gradient": res["all_colour_grads"],
                         "per_camera_2view_call": res["pair_direct"], "per_camera_2view_call_through_autograd": res["pair"],
                         "separate_calls": res["separate"],
                         "what": "train_gs.py get_loss (colour+seg renders, fused 0.8 L1 + 0.2 (1-SSIM)"
                                 + ("" if initial else ", rigid/rot/iso/floor/bg terms") + ") + backward, "
                                 + ("t = 0" if initial else "t > 0") + "; headline = all cameras in one rasterizer call, library calls back to back (gsdyn.step.loss_and_grads_views)"}
    except Exception as e:  # noqa: BLE001
        out["getloss_step"] = {"error": repr(e)}
    try:   # one whole training iteration of the tracking loop, one camera per iteration as train_gs.py runs it: loss + backward + Adam
        from gsdyn import initialize_optimizer
        res = {}
        for name, initial in (("t0", True), ("t>0", False)):
            for mode in ("reference_shape", "fused"):
                p3 = synth_scene_params(P_GAUSS, seed=0, device=dev)
                v3 = init_variables(P_GAUSS, dev)
                v3.update(make_rigidity_variables(p3, num_knn=20))
                views3 = [dict(cam=c, im=im_gt, seg=seg_gt, id=i) for i, c in enumerate(cams)]
                if mode == "fused":
                    opt = initialize_optimizer(p3, 4.0)                    # gsdyn.optim.FusedAdam on a HIP device
                else:
                    lrs = {g["name"]: g["lr"] for g in initialize_optimizer(p3, 4.0).param_groups}
                    opt = torch.optim.Adam([{"params": [v], "name": k, "lr": lrs[k]} for k, v in p3.items()], lr=0.0, eps=1e-15)
                it = [0]

                def iteration():
                    d = views3[it[0] % len(views3)]
                    it[0] += 1
                    if mode == "fused":
                        loss_and_grads_views(p3, [d], v3, initial, w)
                    else:
                        loss, _ = get_loss(p3, d, v3, initial, w)
                        loss.backward()
                    opt.step()
                    opt.zero_grad(set_to_none=True)
                res[name + " " + mode] = _time_ms(iteration, 20, 5)
        out["train_iteration_one_camera"] = {"ms": res, "what": "train_gs.py iteration (one camera: colour + seg render, losses, backward, Adam step); "
                                             "reference_shape = gsdyn.get_loss (two GaussianRasterizer calls, torch loss ops) + torch.optim.Adam; "
                                             "fused = loss_and_grads_views + gsdyn.optim.FusedAdam"}
    except Exception as e:  # noqa: BLE001
        out["train_iteration_one_camera"] = {"error": repr(e)}
    try:   # the REFERENCE's own workload shapes: 1280x720 with 4 cameras (/root/reference/src/tracking/utils/metadata.py:96-97,
        #    src/render/renderer.py:13-14), one random camera per iteration (src/tracking/train_utils.py:82-86), ~9 k - 50 k Gaussians
        #    (assets/demo/gs_orig.splat holds 8 957; the demo fit runs at 640x480)
        from gsdyn import initialize_optimizer
        shapes = {}
        for label, (Pn, Wn, Hn) in (("1280x720_50k_4cams", (50_000, 1280, 720)), ("640x480_9k_4cams", (8_957, 640, 480))):
            im_n, seg_n = synth_targets(Wn, Hn, device=dev)
            cams_n = synth_ring_cameras(4, Wn, Hn, device=dev)
            res = {}
            for mode in ("reference_shape", "fused"):
                pn = synth_scene_params(Pn, seed=0, device=dev)
                vn = init_variables(Pn, dev)
                vn.update(make_rigidity_variables(pn, num_knn=20))
                views_n = [dict(cam=c, im=im_n, seg=seg_n, id=i) for i, c in enumerate(cams_n)]
                if mode == "fused":
                    opt = initialize_optimizer(pn, 4.0)
                else:
                    lrs = {g["name"]: g["lr"] for g in initialize_optimizer(pn, 4.0).param_groups}
                    opt = torch.optim.Adam([{"params": [v], "name": k, "lr": lrs[k]} for k, v in pn.items()], lr=0.0, eps=1e-15)
                it = [0]

                def iteration():
                    d = views_n[it[0] % 4]
                    it[0] += 1
                    if mode == "fused":
                        loss_and_grads_views(pn, [d], vn, False, w)
                    else:
                        loss, _ = get_loss(pn, d, vn, False, w)
                        loss.backward()
                    opt.step()
                    opt.zero_grad(set_to_none=True)
                ms = _time_ms(iteration, 20, 5)
                res[mode] = {"ms_per_iteration": ms, "iterations_per_s": 1e3 / ms}
            shapes[label] = res
        out["reference_shapes"] = {**shapes, "what": "train_gs.py iteration at the reference's own sizes (t > 0: colour + seg render of ONE camera, "
                                   "0.8 L1 + 0.2 (1 - SSIM) on both, rigid / rot / iso / floor / bg terms, backward, Adam), 4 ring cameras taken in turn; "
                                   "reference_shape = gsdyn.get_loss as train_utils.py writes it (two GaussianRasterizer calls through the C++ autograd node, "
                                   "torch loss ops) + torch.optim.Adam; fused = loss_and_grads_views + FusedAdam"}
    except Exception as e:  # noqa: BLE001
        out["reference_shapes"] = {"error": repr(e)}
    try:
        p2 = synth_scene_params(50_000, seed=0, device=dev)
        with torch.no_grad():
            rv = {k: v.detach() for k, v in params2rendervar(p2).items()}
        cam = cams[0]

        def fwd():
            with torch.no_grad():
                GaussianRasterizer(raster_settings=cam)(**rv)
        import diff_gaussian_rasterization as dgr
        if dgr._C is not None:       # a FULL forward per call: the same frame rendered again would be served from the remembered tile lists
            dgr.layer_state(dev).list_reuse = False
        ms = _time_ms(fwd, 20, 5)
        ms_same = None
        if dgr._C is not None:
            dgr.layer_state(dev).list_reuse = True
            ms_same = _time_ms(fwd, 20, 5)
        out["forward_only_cfg2"] = {"ms_per_view": ms, "Mpix_per_s": H * W / ms / 1e3, "ms_per_view_same_geometry_again": ms_same,
                                    "what": "BASELINE.json configs[1]: 50k Gaussians, 1 view 800x800, forward only (tile-list reuse off: every call "
                                            "bins and sorts; *_same_geometry_again: the unchanged frame rendered again reuses the lists)"}
    except Exception as e:  # noqa: BLE001
        out["forward_only_cfg2"] = {"error": repr(e)}
    try:   # predict.py's frame (row A11): every camera rendered twice, colours and an all-ones mask (predict.py:100-123)
        from gsdyn.camera import look_at_w2c
        from gsdyn.render import Renderer
        import math
        rdr = Renderer(dev, w=W, h=H)
        with torch.no_grad():
            data = {k: v.detach() for k, v in params2rendervar(params).items()}      # incl. the means2D holder, as the reference passes it
        kmat = [[float(W), 0.0, W / 2.0], [0.0, float(W), H / 2.0], [0.0, 0.0, 1.0]]
        poses = [(look_at_w2c((4.0 * math.cos(0.3 + 1.57 * i), 0.8, 4.0 * math.sin(0.3 + 1.57 * i))), kmat) for i in range(4)]

        def frame_fused():
            rdr.render_cameras_with_mask(poses, data)

        def frame_reference():
            for w2c, k in poses:
                rdr.render(w2c, k, data, bg=(0.0, 0.0, 0.0))
                ones = dict(data)
                ones["colors_precomp"] = torch.ones_like(data["colors_precomp"])
                rdr.render(w2c, k, ones, bg=(0.0, 0.0, 0.0))
        ms_f, ms_r = _time_ms(frame_fused, 10, 3), _time_ms(frame_reference, 10, 3)
        out["predict_frame_4cams"] = {"ms_per_frame": ms_f, "ms_per_frame_reference_calls": ms_r, "Mpix_per_s": 8 * H * W / ms_f / 1e3,
                                      "what": "predict.py frame: 4 cameras x (colour + all-ones mask render), 100k Gaussians, 800x800, forward only; "
                                              "fused = one multi-view call, ONE blend per camera, the mask from its final transmittance (gsdyn.render); reference_calls = 8 Renderer.render calls"}
    except Exception as e:  # noqa: BLE001
        out["predict_frame_4cams"] = {"error": repr(e)}
    try:   # BASELINE.json configs[0]-shaped rollout step on the device (row N4): rope.yaml GNN dims, random weights
        from gsdyn.dynamics import DynamicsPredictor, farthest_point_sampler, rollout_step
        cfg = dict(nf_particle=512, nf_relation=512, nf_effect=512, attr_dim=2, state_dim=0, action_dim=3, pstep=3,
                   rel_attr_dim=2, rel_group_dim=1, rel_distance_dim=3, n_his=3)
        torch.manual_seed(0)
        model = DynamicsPredictor(cfg, device=dev).eval()
        with torch.no_grad():
            rv = {k: v.detach() for k, v in params2rendervar(params).items()}
        t_fps = _time_ms(lambda: farthest_point_sampler(rv["means3D"][None], 1000, start_idx=0), 3, 2)
        pick = farthest_point_sampler(rv["means3D"][None], 100, start_idx=0)[0]
        bones = rv["means3D"][pick]
        hist, eef = bones[None].repeat(3, 1, 1), torch.zeros((3, 1, 3), device=dev)
        t_step = _time_ms(lambda: rollout_step(model, hist, eef, eef[-1] + 0.02, rv["means3D"], rv["rotations"], 0.5, 5), 10, 3)
        out["rollout_step_cfg1"] = {"ms_per_step": t_step, "fps_1000_of_100k_ms": t_fps,
                                    "what": "row N4: relations + DynamicsPredictor (rope.yaml width 512, random weights, 100 bones) + "
                                            "bone fitting + skinning of 100k Gaussians (gsr_lbs); FPS timed separately (gsr_fps)"}
    except Exception as e:  # noqa: BLE001
        out["rollout_step_cfg1"] = {"error": repr(e)}
    try:   # BASELINE.json configs[4]'s frames as a SEQUENCE (row A11): 500k Gaussians, 1920x1080, 4 cameras x (colour + mask), a scene that drifts ~3 px per frame
        from gsdyn.dynamics import spatial_order
        from gsdyn.predict import FrameShard, ring_poses
        P5, W5, H5, NF = 500_000, 1920, 1080, 12
        p5 = synth_scene_params(P5, seed=0, device=dev)
        with torch.no_grad():
            d5 = {k: v.detach() for k, v in params2rendervar(p5).items()}
            perm = spatial_order(d5["means3D"])
            d5 = {k: v[perm].contiguous() for k, v in d5.items()}
            seq = []
            for f in range(NF):
                e = dict(d5)
                e["means3D"] = d5["means3D"] + torch.tensor([0.006, 0.0, 0.003], device=dev) * f       # 0.006 units at distance 4, fx = 1920: ~3 px
                seq.append(e)
        res = {}
        for name, spec in (("from_scratch", False), ("depth_cuts", True)):
            # the WHOLE sequence once untimed (every output of every frame has been allocated once, every capacity estimate has settled), then the
            # median of five timed passes, each on a fresh shard (a pass starts without proposals, as an episode does)
            FrameShard(dev, W5, H5, ring_poses(4, W5, H5), 0, 1, speculative=spec).render_episode(seq)
            passes = []
            for _ in range(5):
                shard = FrameShard(dev, W5, H5, ring_poses(4, W5, H5), 0, 1, speculative=spec)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                shard.render_episode(seq)
                torch.cuda.synchronize()
                passes.append((time.perf_counter() - t0) / NF * 1e3)
            res[name] = _median_of(passes)
            if spec:
                redone = shard.cuts.redone
        out["predict_sequence_cfg5"] = {"ms_per_frame_from_scratch": res["from_scratch"], "ms_per_frame_depth_cuts": res["depth_cuts"],
                                        "min_ms_per_frame_from_scratch": res["from_scratch"].min, "min_ms_per_frame_depth_cuts": res["depth_cuts"].min,
                                        "timing": "one untimed pass over the whole sequence, then median (min beside it) of 5 timed passes, a fresh FrameShard each",
                                        "frames_with_a_repeated_view": redone, "frames": NF,
                                        "what": "BASELINE.json configs[4] frames as a sequence: 500k Gaussians, 1920x1080, 4 cameras x (colour + mask), the scene drifting ~3 px "
                                                "per frame; depth_cuts = every frame bins only what the previous frame of the same cameras needed, the blend validates the "
                                                "guess, failed views are rendered again (gsdyn.render.DepthCuts: every frame handed out is exact); `--config 5 [--with-rollout]` "
                                                "has the full lines"}
    except Exception as e:  # noqa: BLE001
        out["predict_sequence_cfg5"] = {"error": repr(e)}
    try:   # the graphed rollout step of configs[4] (row N4): 500k Gaussians, 1000 tracked particles, 100 bones, GNN width 512 -- one hipGraph replay per step
        from gsdyn import dynamics as Dm
        with torch.no_grad():
            xyz5 = p5["means3D"].detach()
            quat5 = torch.nn.functional.normalize(p5["unnorm_rotations"].detach())
            torch.manual_seed(0)
            model5 = Dm.DynamicsPredictor(dict(nf_particle=512, nf_relation=512, nf_effect=512, attr_dim=2, state_dim=0, action_dim=3, pstep=3,
                                               rel_attr_dim=2, rel_group_dim=1, rel_distance_dim=3, n_his=3), device=dev).eval()
            t_fps5 = _time_ms(lambda: Dm.farthest_point_sampler(xyz5[None], 1000), 2, 1)
            track = Dm.farthest_point_sampler(xyz5[None], 1000)[0]
            gs = Dm._graphed_step_for(model5, P5, 1000, 3, 100, 0.3, 0, 0.6, 5, dev)
            gs.load(track, xyz5[track], xyz5[track][None].repeat(3, 1, 1), torch.zeros((3, 1, 3), device=dev), xyz5, quat5)
            eef5 = torch.tensor([[0.02, 0.0, 0.01]], device=dev)
            t_gs = _time_ms(lambda: gs.step(eef5), 50, 5)
        out["rollout_graphed_step_cfg5"] = {"ms_per_step": t_gs, "fps_1000_of_500k_ms": t_fps5, "bones_kept": int(gs.n_valid),
                                            "what": "configs[4]'s rollout step as ONE hipGraph replay (bone sampling + thinning, relations, propagation network, rotation "
                                                    "fit, skinning of 500k Gaussians, history shift: 33 graph nodes) and the episode's one-off farthest-point sampling"}
    except Exception as e:  # noqa: BLE001
        out["rollout_graphed_step_cfg5"] = {"error": repr(e)}
    return out


def run_cpu_baseline(params, cam, dL, params2rendervar):
    """Oracle O2 (C, OpenMP over tiles) on the host cores: ONE view fwd+bwd of the same workload."""
    try:
        from oracle import OracleCamera, TiledOracle
    except Exception as e:  # noqa: BLE001
        return {"error": f"oracle unavailable: {e}"}
    with torch.no_grad():
        rv = {k: v.detach().cpu().numpy() for k, v in params2rendervar(params).items()}
    ocam = OracleCamera(H, W, cam.tanfovx, cam.tanfovy, cam.bg.cpu().numpy(), 1.0,
                        cam.viewmatrix.cpu().numpy().reshape(-1), cam.projmatrix.cpu().numpy().reshape(-1), 0,
                        cam.campos.cpu().numpy())
    cores = os.cpu_count() or 1
    threads = min(cores, 64)
    g = dL.cpu().numpy()
    passes, t0 = [], time.perf_counter()
    while True:  # bounded sample: whole views, each timed by itself, until ~20 s of CPU-core time (threads x wall); at least 3, at most 16 views
        t1 = time.perf_counter()
        o2 = TiledOracle(ocam, rv["means3D"], rv["opacities"], colors_precomp=rv["colors_precomp"], scales=rv["scales"],
                         rotations=rv["rotations"], nthreads=threads)
        o2.backward(g)
        passes.append(time.perf_counter() - t1)
        dt = time.perf_counter() - t0
        if (dt * threads >= 20.0 and len(passes) >= 3) or len(passes) >= 16:
            break
    med = float(_median_of(passes))
    return {"value": H * W / med / 1e6, "unit": "Mpix/s", "cores": threads, "kind": "port",
            "sample": f"median of {len(passes)} x (1 view 800x800, 100k Gaussians, fwd+bwd) with oracle/gsr_oracle.c, OpenMP over tiles",
            "value_best_pass": H * W / min(passes) / 1e6, "value_worst_pass": H * W / max(passes) / 1e6,
            "seconds": dt, "host_cpu_count": cores}


if __name__ == "__main__":
    main()
