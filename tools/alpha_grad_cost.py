"""The price of the rendered alpha (profiles/alpha_grad_cost.txt): the configs[2] shape -- 100 000 Gaussians, four 800 x 800 views in one
rasterize_gaussians_views call, frozen colours -- fwd + bwd steps with a colour loss, or with return_alpha=True and a colour + alpha loss:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/alpha_grad_cost.py {noalpha|alpha}

prints the median wall time of a step; the per-kernel averages land in <dir>/run_kernel_stats.csv (alpha_views: the forward's alpha
kernel, render_bwd_*: the blend backward with and without the alpha term)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-dynamics_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch
from diff_gaussian_rasterization import rasterize_gaussians_views
from hipcheck import _settings
from util import random_gaussians, ring_camera
if len(sys.argv) != 2 or sys.argv[1] not in ("noalpha", "alpha"):
    sys.exit("usage: tools/alpha_grad_cost.py {noalpha|alpha}")
alpha = sys.argv[1] == "alpha"
dev = torch.device("cuda:0")
P, W, H, V, K = 100_000, 800, 800, 4, 20
g = random_gaussians(P, seed=21, scale_lo=0.005, scale_hi=0.05)
cams = [ring_camera(W, H, v=v, V=V, bg=(0.1, 0.2, 0.3)) for v in range(V)]
rs = [_settings(c, dev) for c in cams]
t = {k: torch.tensor(v, device=dev, requires_grad=k != "colors_precomp") for k, v in g.items()}
m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
dc = torch.rand((V, 3, H, W), device=dev) - 0.5
da = torch.rand((V, 1, H, W), device=dev) - 0.5
times = []
for i in range(K + 3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                                    rotations=t["rotations"], return_alpha=alpha)
    loss = (out[0] * dc).sum() + ((out[3] * da).sum() if alpha else 0.0)
    loss.backward()
    torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
    for v in list(t.values()) + [m2]:
        v.grad = None
print(f"alpha={alpha}: median step {1e3 * float(np.median(times[3:])):.3f} ms over {K}")
