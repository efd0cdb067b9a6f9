"""The price of anti-aliasing (profiles/antialias_cost.txt): the configs[2] shape -- 100 000 Gaussians, four 800 x 800 views in one
rasterize_gaussians_views call, frozen colours -- fwd + bwd steps with a colour loss, antialiasing off or on:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/antialias_cost.py {plain|aa}

prints the list entries per view (num_rendered: o c < o shortens the lists) and the median wall time of a step; the per-kernel averages
land in <dir>/run_kernel_stats.csv (preprocess_fwd_kernel / preprocess_fwd_aa_kernel, preprocess_bwd_views_waves*_kernel<4>, render_fwd_*,
render_bwd_*)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-dynamics_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch
from diff_gaussian_rasterization import _hip, rasterize_gaussians_views
from hipcheck import _settings
from util import random_gaussians, ring_camera
if len(sys.argv) != 2 or sys.argv[1] not in ("plain", "aa"):
    sys.exit("usage: tools/antialias_cost.py {plain|aa}")
aa = sys.argv[1] == "aa"
dev = torch.device("cuda:0")
P, W, H, V, K = 100_000, 800, 800, 4, 20
g = random_gaussians(P, seed=21, scale_lo=0.005, scale_hi=0.05)
cams = [ring_camera(W, H, v=v, V=V, bg=(0.1, 0.2, 0.3)) for v in range(V)]
rs = [_settings(c, dev) for c in cams]
t = {k: torch.tensor(v, device=dev, requires_grad=k != "colors_precomp") for k, v in g.items()}
with torch.no_grad():
    st = _hip.rasterize_forward_batch(rs, t["means3D"], t["opacities"], t["colors_precomp"], None, t["scales"], t["rotations"], None,
                                      antialiasing=aa)[3]
print(f"antialiasing={aa}: num_rendered per view {[s.num_rendered for s in st]}, total {sum(s.num_rendered for s in st)}")
del st
m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
dc = torch.rand((V, 3, H, W), device=dev) - 0.5
times = []
for i in range(K + 3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                                    rotations=t["rotations"], antialiasing=aa)
    (out[0] * dc).sum().backward()
    torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
    for v in list(t.values()) + [m2]:
        v.grad = None
print(f"antialiasing={aa}: median step {1e3 * float(np.median(times[3:])):.3f} ms over {K}")
