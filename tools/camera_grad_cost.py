"""The price of camera gradients (profiles/camera_grad_cost.txt): the configs[2] shape -- 100 000 Gaussians, four 800 x 800 views in one
rasterize_gaussians_views call, frozen colours -- fwd + bwd steps with a colour loss, camera gradients off or on:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/camera_grad_cost.py {plain|camera}

prints the median wall time of a step; the per-kernel averages land in <dir>/run_kernel_stats.csv (camera_bwd_kernel, camera_reduce_kernel,
preprocess_bwd_views_waves*_kernel<4>, render_bwd_*)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-dynamics_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch
from diff_gaussian_rasterization import rasterize_gaussians_views
from hipcheck import _settings
from util import random_gaussians, ring_camera
if len(sys.argv) != 2 or sys.argv[1] not in ("plain", "camera"):
    sys.exit("usage: tools/camera_grad_cost.py {plain|camera}")
camera = sys.argv[1] == "camera"
dev = torch.device("cuda:0")
P, W, H, V, K = 100_000, 800, 800, 4, 20
g = random_gaussians(P, seed=21, scale_lo=0.005, scale_hi=0.05)
rs = [_settings(ring_camera(W, H, v=v, V=V, bg=(0.1, 0.2, 0.3)), dev) for v in range(V)]
if camera:   # every view's camera tensors are leaves that want a gradient
    rs = [r._replace(**{k: getattr(r, k).clone().requires_grad_(True) for k in ("bg", "viewmatrix", "projmatrix", "campos")}) for r in rs]
t = {k: torch.tensor(v, device=dev, requires_grad=k != "colors_precomp") for k, v in g.items()}
m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
dc = torch.rand((V, 3, H, W), device=dev) - 0.5
times = []
for i in range(K + 3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                                    rotations=t["rotations"], camera_gradients=camera)
    (out[0] * dc).sum().backward()
    torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
    for v in list(t.values()) + [m2] + ([x for r in rs for x in (r.bg, r.viewmatrix, r.projmatrix, r.campos)] if camera else []):
        v.grad = None
print(f"camera_gradients={camera}: median step {1e3 * float(np.median(times[3:])):.3f} ms over {K}")
