"""CPU tests of the two oracles (no GPU): golden vectors, O1-vs-O2 cross-check, finite differences and
closed-form known-answer cases.  PARITY UNPINNED for the rasterizer itself."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import TiledOracle, OracleCamera
from oracle.dense_oracle import dense_rasterize, finite_difference
from oracle.tiled import mark_visible
from util import look_at, mixed_err, oracle_camera, random_gaussians, rel_err, ring_camera, row_err


def _cam_from_vec(v):
    H, W = int(v[0]), int(v[1])
    return OracleCamera(H, W, float(v[2]), float(v[3]), v[4:7].astype(np.float32), 1.0,
                        v[7:23].astype(np.float32), v[23:39].astype(np.float32), 0, v[39:42].astype(np.float32))


def _load_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "raster_cases.npz"))
    return z, [str(n) for n in z["names"]]


def test_o2_reproduces_committed_goldens(golden_dir):
    z, names = _load_cases(golden_dir)
    for n in names:
        g = {k: z[f"{n}/in_{k}"] for k in ("means3D", "scales", "rotations", "opacities", "colors_precomp")}
        o2 = TiledOracle(_cam_from_vec(z[f"{n}/cam"]), g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"],
                         scales=g["scales"], rotations=g["rotations"])
        assert np.array_equal(o2.radii, z[f"{n}/radii"])
        assert np.array_equal(o2.point_list, z[f"{n}/point_list"])
        assert np.array_equal(o2.ranges, z[f"{n}/ranges"])
        assert np.array_equal(o2.n_contrib, z[f"{n}/n_contrib"])
        np.testing.assert_allclose(o2.color, z[f"{n}/color"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(o2.depth, z[f"{n}/depth"], rtol=0, atol=1e-5)
        gr = o2.backward(z[f"{n}/dL_dcolor"])
        for k in ("means3D", "means2D", "colors_precomp", "opacities", "scales", "rotations"):
            assert rel_err(gr[k], z[f"{n}/grad_{k}"]) < 1e-5, (n, k)


def test_o2_reproduces_committed_multi_view_goldens(golden_dir):
    """raster_cases_views.npz (tests/golden/gen_raster_view_goldens.py): per-view outputs, per-view screen-space and colour
    gradients, and the sum over views of the remaining input gradients -- what the batched entry point must return."""
    z = np.load(os.path.join(golden_dir, "raster_cases_views.npz"))
    for n in [str(x) for x in z["names"]]:
        g = {k: z[f"{n}/in_{k}"] for k in ("means3D", "scales", "rotations", "opacities")}
        cols = z[f"{n}/in_colours"]
        sums = {k: 0.0 for k in ("means3D", "opacities", "scales", "rotations")}
        for vi in range(len(z[f"{n}/view_cam"])):
            o2 = TiledOracle(_cam_from_vec(z[f"{n}/cam"][vi]), g["means3D"], g["opacities"],
                             colors_precomp=cols[z[f"{n}/view_colour"][vi]], scales=g["scales"], rotations=g["rotations"])
            assert np.array_equal(o2.radii, z[f"{n}/radii"][vi])
            np.testing.assert_allclose(o2.color, z[f"{n}/color"][vi], rtol=0, atol=1e-6)
            np.testing.assert_allclose(o2.depth, z[f"{n}/depth"][vi], rtol=0, atol=1e-5)
            gr = o2.backward(z[f"{n}/dL_dcolor"][vi])
            assert rel_err(gr["means2D"], z[f"{n}/grad_means2D"][vi]) < 1e-5
            assert rel_err(gr["colors_precomp"], z[f"{n}/grad_colours_per_view"][vi]) < 1e-5
            for k in sums:
                sums[k] = sums[k] + gr[k].astype(np.float64)
        for k in sums:
            assert rel_err(sums[k], z[f"{n}/grad_sum_{k}"]) < 1e-5, (n, k)
        same_cam = z[f"{n}/view_cam"]
        if n.startswith("pairs"):          # views of one camera share geometry: identical radii / depth, different colours
            for a in range(len(same_cam)):
                for b in range(a + 1, len(same_cam)):
                    if same_cam[a] == same_cam[b]:
                        assert np.array_equal(z[f"{n}/radii"][a], z[f"{n}/radii"][b])
                        assert np.array_equal(z[f"{n}/depth"][a], z[f"{n}/depth"][b])


def _o1(cam, g, sh_degree=0, dL=None):
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in g.items()}
    color, radii, depth, m2 = dense_rasterize(
        cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, torch.tensor(cam.bg), cam.scale_modifier,
        torch.tensor(cam.viewmatrix), torch.tensor(cam.projmatrix), sh_degree, torch.tensor(cam.campos),
        t["means3D"], t["opacities"], colors_precomp=t.get("colors_precomp"), scales=t.get("scales"),
        rotations=t.get("rotations"), shs=t.get("shs"), cov3D_precomp=t.get("cov3D_precomp"))
    if dL is not None:
        (color * torch.tensor(dL, dtype=torch.float64)).sum().backward()
    return color, radii, depth, m2, t


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_o2_vs_o1_spherical_harmonics(deg):
    W, H, P = 40, 36, 60
    g = random_gaussians(P, seed=20 + deg, scale_lo=0.05, scale_hi=0.4, sh_M=16)
    del g["colors_precomp"]
    cam = ring_camera(W, H, v=1, bg=(0.1, 0.0, 0.2), sh_degree=deg)
    o2 = TiledOracle(cam, g["means3D"], g["opacities"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"])
    dL = np.random.default_rng(1).uniform(-1, 1, (3, H, W)).astype(np.float32)
    gr = o2.backward(dL)
    color, radii, depth, m2, t = _o1(cam, g, sh_degree=deg, dL=dL)
    amb = o2.ambiguous
    assert np.array_equal(radii.numpy(), o2.radii)
    assert np.abs(color.detach().numpy() - o2.color)[:, ~amb].max() < 2e-5
    assert rel_err(gr["shs"], t["shs"].grad.numpy()) < 1e-4
    assert rel_err(gr["means3D"], t["means3D"].grad.numpy()) < 1e-4
    assert rel_err(gr["scales"], t["scales"].grad.numpy()) < 1e-4
    ncoef = (deg + 1) ** 2
    assert np.all(gr["shs"][:, ncoef:] == 0)  # inactive coefficients get exactly zero gradient


def test_o2_vs_o1_cov3d_precomp():
    W, H, P = 50, 34, 80
    g = random_gaussians(P, seed=31, scale_lo=0.05, scale_hi=0.3)
    probe = TiledOracle(ring_camera(W, H), g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"],
                        scales=g["scales"], rotations=g["rotations"])
    cov = probe.cov3D
    ref_color = probe.color
    g2 = dict(means3D=g["means3D"], opacities=g["opacities"], colors_precomp=g["colors_precomp"], cov3D_precomp=cov)
    cam = ring_camera(W, H)
    o2 = TiledOracle(cam, g2["means3D"], g2["opacities"], colors_precomp=g2["colors_precomp"], cov3D_precomp=cov)
    np.testing.assert_allclose(o2.color, ref_color, atol=1e-6)
    dL = np.random.default_rng(2).uniform(-1, 1, (3, H, W)).astype(np.float32)
    gr = o2.backward(dL)
    color, radii, depth, m2, t = _o1(cam, g2, dL=dL)
    assert rel_err(gr["cov3D_precomp"], t["cov3D_precomp"].grad.numpy()) < 1e-4
    assert rel_err(gr["means3D"], t["means3D"].grad.numpy()) < 1e-4
    assert np.all(gr["scales"] == 0) and np.all(gr["rotations"] == 0)


def test_o1_finite_differences():
    """The autograd oracle's calculus against central differences (fp64), away from thresholds."""
    W, H, P = 16, 16, 3
    g = random_gaussians(P, seed=40, scale_lo=0.3, scale_hi=0.5, spread=0.3)
    g["opacities"][:] = 0.5
    cam = ring_camera(W, H)
    dL = torch.tensor(np.random.default_rng(3).uniform(-1, 1, (3, H, W)))
    color, radii, depth, m2, t = _o1(cam, g, dL=dL.numpy())

    def make_fn(key):
        def fn(x):
            args = {k: (x if k == key else v.detach()) for k, v in t.items()}
            c, _, _, _ = dense_rasterize(H, W, cam.tanfovx, cam.tanfovy, torch.tensor(cam.bg), 1.0,
                                         torch.tensor(cam.viewmatrix), torch.tensor(cam.projmatrix), 0,
                                         torch.tensor(cam.campos), args["means3D"], args["opacities"],
                                         colors_precomp=args["colors_precomp"], scales=args["scales"],
                                         rotations=args["rotations"])
            return (c * dL).sum()
        return fn
    for key in ("means3D", "scales", "rotations", "opacities", "colors_precomp"):
        fd = finite_difference(make_fn(key), t[key].detach().clone(), eps=1e-6)
        assert rel_err(fd.numpy(), t[key].grad.numpy()) < 2e-4, key  # conic backward carries the 1e-7 epsilon (A.5)


# ------------------------------------------------------------------ known-answer cases
def _single(W=64, H=64, z=3.0, s=0.05, op=0.8, bg=(0, 0, 0), xy=(0.0, 0.0)):
    w2c = np.eye(4)
    w2c[2, 3] = z  # camera looks down +z at the origin from distance z
    cam = oracle_camera(W, H, w2c, bg=bg)
    g = dict(means3D=np.array([[xy[0], xy[1], 0.0]], np.float32), scales=np.full((1, 3), s, np.float32),
             rotations=np.array([[1, 0, 0, 0]], np.float32), opacities=np.array([[op]], np.float32),
             colors_precomp=np.array([[1.0, 0.5, 0.25]], np.float32))
    return cam, g


def test_known_answer_single_isotropic_gaussian():
    W = H = 64
    z, s, op = 3.0, 0.05, 0.8
    cam, g = _single(W, H, z, s, op)
    o2 = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"],
                     rotations=g["rotations"])
    # pixel mean: fx*x/z + cx - 0.5 (A-8); 2D variance (fx*s/z)^2 + 0.3
    var = (W * s / z) ** 2 + 0.3
    np.testing.assert_allclose(o2.means2D[0], [W / 2 - 0.5, H / 2 - 0.5], atol=1e-4)
    assert o2.radii[0] == math.ceil(3 * math.sqrt(var))
    np.testing.assert_allclose(o2.conic_opacity[0], [1 / var, 0, 1 / var, op], rtol=1e-5, atol=1e-7)
    r = o2.radii[0]
    mx = my = W / 2 - 0.5
    exp_rect = [int((mx - r) / 16), int((my - r) / 16), int((mx + r + 15) / 16), int((my + r + 15) / 16)]
    assert list(o2.rect[0]) == exp_rect
    # closed-form alpha profile along the row through the centre
    y = 32
    for x in (28, 31, 32, 36, 40):
        d2 = (x - mx) ** 2 + (y - my) ** 2
        a = min(0.99, op * math.exp(-0.5 * d2 / var))
        expect = a if a >= 1 / 255 else 0.0
        assert abs(o2.color[0, y, x] - expect * 1.0) < 1e-5
        assert abs(o2.color[1, y, x] - expect * 0.5) < 1e-5
        assert abs(o2.depth[0, y, x] - expect * z) < 1e-4
        assert abs(o2.final_T[y, x] - (1 - expect)) < 1e-6


def test_known_answer_two_overlapping_order_and_transmittance():
    W = H = 32
    w2c = np.eye(4); w2c[2, 3] = 3.0
    cam = oracle_camera(W, H, w2c, bg=(0.25, 0.25, 0.25))
    means = np.array([[0, 0, 0.5], [0, 0, -0.5]], np.float32)  # index 1 is nearer (view z 2.5 < 3.5)
    g = dict(means3D=means, scales=np.full((2, 3), 0.2, np.float32), rotations=np.tile([1, 0, 0, 0], (2, 1)).astype(np.float32),
             opacities=np.array([[0.6], [0.5]], np.float32), colors_precomp=np.array([[1, 0, 0], [0, 1, 0]], np.float32))
    o2 = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"])
    assert list(o2.point_list[:2]) == [1, 0]  # front-to-back: nearer Gaussian first
    y = x = 16
    def alpha(i):
        mx, my = o2.means2D[i]; A, B, C, o = o2.conic_opacity[i]
        dx, dy = mx - x, my - y
        return min(0.99, o * math.exp(-0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy))
    a1, a0 = alpha(1), alpha(0)
    T = (1 - a1) * (1 - a0)
    np.testing.assert_allclose(o2.color[:, y, x], [a0 * (1 - a1) + T * 0.25, a1 + T * 0.25, T * 0.25], atol=1e-5)
    np.testing.assert_allclose(o2.depth[0, y, x], 2.5 * a1 + 3.5 * a0 * (1 - a1), atol=1e-4)


def test_known_answer_near_plane_cull_and_mark_visible():
    W = H = 32
    w2c = np.eye(4)
    cam = oracle_camera(W, H, w2c)
    means = np.array([[0, 0, 0.2], [0, 0, 0.2000001 + 1e-6], [0, 0, -1.0], [0, 0, 1.0]], np.float32)
    g = dict(means3D=means, scales=np.full((4, 3), 0.01, np.float32), rotations=np.tile([1, 0, 0, 0], (4, 1)).astype(np.float32),
             opacities=np.full((4, 1), 0.5, np.float32), colors_precomp=np.ones((4, 3), np.float32))
    o2 = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"])
    assert o2.radii[0] == 0 and o2.radii[2] == 0          # z <= 0.2 and behind the camera: culled
    assert o2.radii[1] > 0 and o2.radii[3] > 0
    assert list(mark_visible(cam.viewmatrix, means)) == [False, True, False, True]


def test_known_answer_alpha_clamp_and_early_stop():
    W = H = 16
    w2c = np.eye(4); w2c[2, 3] = 2.0
    cam = oracle_camera(W, H, w2c, bg=(1, 1, 1))
    P = 6
    means = np.zeros((P, 3), np.float32); means[:, 2] = np.linspace(0, 0.5, P)
    g = dict(means3D=means, scales=np.full((P, 3), 1.0, np.float32), rotations=np.tile([1, 0, 0, 0], (P, 1)).astype(np.float32),
             opacities=np.full((P, 1), 1.0, np.float32), colors_precomp=np.ones((P, 3), np.float32) * 0.5)
    o2 = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"])
    # huge opaque Gaussians: alpha clamps to 0.99 everywhere; T: 1 -> 1e-2 -> 1e-4 (kept: 1e-4 is not < 1e-4?) ...
    y = x = 8
    T, n = 1.0, 0
    for _ in range(P):
        t2 = np.float32(T) * (np.float32(1.0) - np.float32(0.99))
        if t2 < np.float32(1e-4):
            break
        T, n = float(t2), n + 1
    assert o2.n_contrib[y, x] == n
    assert abs(o2.final_T[y, x] - T) < 1e-7
    assert abs(o2.color[0, y, x] - (0.5 * (1 - T) + T)) < 1e-5


def test_equal_depth_ties_resolve_by_index():
    W = H = 16
    w2c = np.eye(4); w2c[2, 3] = 2.0
    cam = oracle_camera(W, H, w2c)
    P = 5
    g = dict(means3D=np.zeros((P, 3), np.float32), scales=np.full((P, 3), 0.1, np.float32),
             rotations=np.tile([1, 0, 0, 0], (P, 1)).astype(np.float32), opacities=np.full((P, 1), 0.3, np.float32),
             colors_precomp=np.random.default_rng(0).uniform(0, 1, (P, 3)).astype(np.float32))
    o2 = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"])
    assert list(o2.point_list) == list(range(P))


def test_empty_and_all_culled():
    cam = oracle_camera(20, 20, np.eye(4), bg=(0.3, 0.6, 0.9))
    g = random_gaussians(4, seed=1)
    g["means3D"][:, 2] = -5  # behind the camera
    o2 = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"])
    assert o2.num_rendered == 0 and np.all(o2.radii == 0)
    np.testing.assert_allclose(o2.color[:, 3, 4], [0.3, 0.6, 0.9])
    assert np.all(o2.depth == 0)
    gr = o2.backward(np.ones((3, 20, 20), np.float32))
    assert all(np.all(v == 0) for k, v in gr.items() if v is not None)


def test_threaded_oracle_equals_single_thread():
    W, H, P = 70, 50, 200
    g = random_gaussians(P, seed=50)
    cam = ring_camera(W, H)
    a = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"], nthreads=1)
    b = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"], nthreads=4)
    assert np.array_equal(a.color, b.color) and np.array_equal(a.point_list, b.point_list)
    dL = np.ones((3, H, W), np.float32)
    ga, gb = a.backward(dL), b.backward(dL)
    for k in ga:
        if ga[k] is not None:
            assert np.array_equal(ga[k], gb[k]), k  # per-entry partial layout makes the threaded backward deterministic


def test_fp64_build_of_o2_pins_the_explicit_backward_and_measures_fp32_conditioning():
    """oracle/libgsr_oracle64.so = the SAME C file with every float a double.  (i) Against O1 (fp64 dense autograd, no hand-derived
    backward) the explicit backward of O2 now agrees to < 1e-6 (binary32 literals in the C file) instead of ~1e-5: what was left between the two oracles was fp32
    rounding, not a formula.  (ii) Against its own fp32 build (same tile lists: the fp64 run takes over the fp32 run's radii, rects and
    binary32 depth keys) it measures how far ANY fp32 evaluation is from the exact gradients, per Gaussian: worst rows ~1e-4 of the
    row's own magnitude -- the reason the GPU tests assert the row-wise bound at 5e-4 for every row and 1e-4 for 99.9 % of them."""
    W, H, P = 48, 40, 120
    g = random_gaussians(P, seed=77, scale_lo=0.05, scale_hi=0.4)
    cam = ring_camera(W, H, v=2, bg=(0.2, 0.1, 0.0))
    kw = dict(colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"])
    o32 = TiledOracle(cam, g["means3D"], g["opacities"], **kw)
    o64 = TiledOracle(cam, g["means3D"], g["opacities"], f64=True, decisions_of=o32, **kw)
    assert np.array_equal(o32.radii, o64.radii) and np.array_equal(o32.point_list, o64.point_list) and np.array_equal(o32.ranges, o64.ranges)
    ok = ~o32.ambiguous
    dL = np.random.default_rng(5).uniform(-1, 1, (3, H, W)).astype(np.float32)
    dL[:, ~ok] = 0.0
    g32, g64 = o32.backward(dL), o64.backward(dL)
    color, radii, depth, m2, t = _o1(cam, g, dL=dL)
    assert np.abs(color.detach().numpy() - o64.color)[:, ok].max() < 1e-7     # (the C file's constants are binary32 literals: 0.3f, 1/255.0f ...)
    for k, tk in (("means3D", "means3D"), ("scales", "scales"), ("rotations", "rotations"), ("opacities", "opacities"), ("colors_precomp", "colors_precomp")):
        ref = t[tk].grad.numpy().reshape(g64[k].shape)
        assert rel_err(g64[k], ref) < 1e-6, (k, rel_err(g64[k], ref))
        assert rel_err(g32[k], g64[k]) < 1e-4 and row_err(g32[k], g64[k])[0] < 5e-4, k
    # a larger scene: the fp32 build is off by up to ~1e-4 of a row's own magnitude
    g = random_gaussians(5000, seed=4, scale_lo=0.02, scale_hi=0.25)
    cam = ring_camera(256, 192, v=4, bg=(0.1, 0.3, 0.5))
    kw = dict(colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"])
    o32 = TiledOracle(cam, g["means3D"], g["opacities"], nthreads=4, **kw)
    o64 = TiledOracle(cam, g["means3D"], g["opacities"], nthreads=4, f64=True, decisions_of=o32, **kw)
    assert np.array_equal(o32.point_list, o64.point_list)
    ok = ~o32.ambiguous
    dL = np.random.default_rng(4).uniform(-1, 1, (3, 192, 256)).astype(np.float32)
    dL[:, ~ok] = 0.0
    g32, g64 = o32.backward(dL), o64.backward(dL)
    worst = max(row_err(g32[k], g64[k])[0] for k in ("means3D", "scales", "rotations", "opacities", "colors_precomp", "means2D"))
    assert 2e-5 < worst < 5e-4, worst


# ---- the frustum clamp decision (A.1-4) at its edge: recorded, and taken over by the fp64 referee

def _clamp_edge_oracles(f64_decisions=True):
    from util import clamp_edge_camera, clamp_edge_scene
    cam = clamp_edge_camera()
    g, edge = clamp_edge_scene(cam, seed=0)
    kw = dict(colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"], nthreads=4)
    o32 = TiledOracle(cam, g["means3D"], g["opacities"], **kw)
    o64 = TiledOracle(cam, g["means3D"], g["opacities"], f64=True, decisions_of=o32 if f64_decisions else None, **kw)
    return cam, g, edge, o32, o64


def test_clamp_edge_scene_is_adversarial():
    """The scene builder's promise, on the host: every edge Gaussian's fp32 txtz / tytz is within 8 ulp of the limit, at least 16 of
    them are decided differently by the forward's fp32 arithmetic and the old backward's mixed one (both axes, both signs, both sides),
    and the fp32 oracle's recorded flags are the forward replica's."""
    from util import clamp_edge_camera, clamp_edge_scene, frustum_decisions_fp32, frustum_decisions_mixed
    cam = clamp_edge_camera()
    g, edge = clamp_edge_scene(cam, seed=0)
    c32, t32, lim = frustum_decisions_fp32(cam, g["means3D"])
    cmix = frustum_decisions_mixed(cam, g["means3D"])
    dist = np.abs(np.abs(t32[edge]) - lim[None]) / np.spacing(lim)[None]
    assert (dist.min(1) <= 8).all()
    differ = c32 != cmix
    assert differ[edge].any(1).sum() >= 16, differ[edge].any(1).sum()
    for ax in (0, 1):
        for sgn in (1, -1):
            rows = edge[differ[edge, ax] & (np.sign(t32[edge, ax]) == sgn)]
            assert len(rows) > 0, (ax, sgn)
        assert c32[edge][differ[edge, ax], ax].any() and not c32[edge][differ[edge, ax], ax].all(), ax
    o32 = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"])
    vis = o32.radii > 0
    assert vis[edge].sum() >= 0.9 * len(edge), "edge Gaussians must reach into the image"
    assert np.array_equal(o32.frustum_clamped.astype(bool)[vis], c32[vis])


def test_fp64_oracle_takes_over_the_frustum_clamp():
    """With decisions_of the fp64 build reports (and uses) the fp32 run's clamp flags; without, it decides at least one edge Gaussian
    differently -- so without the take-over a comparison at the edge would be against another function."""
    _, _, edge, o32, o64 = _clamp_edge_oracles()
    assert np.array_equal(o64.frustum_clamped, o32.frustum_clamped)
    _, _, _, _, o64_own = _clamp_edge_oracles(f64_decisions=False)
    assert (o64_own.frustum_clamped[edge] != o32.frustum_clamped[edge]).any()


def test_fp64_referee_with_taken_clamp_is_close_to_fp32_on_edge_rows():
    """Taking over the flags makes the two builds differentiate the same function: on the edge rows the fp32 oracle's means3D gradient is
    within fp32 conditioning of the fp64 one (without the take-over, rows whose decision flips are off by O(1))."""
    cam, g, edge, o32, o64 = _clamp_edge_oracles()
    dL = np.random.default_rng(5).uniform(-1, 1, (3, cam.image_height, cam.image_width)).astype(np.float32)
    dL[:, o32.ambiguous] = 0.0
    g32, g64 = o32.backward(dL), o64.backward(dL)
    assert row_err(g32["means3D"][edge], g64["means3D"][edge])[0] < 1e-3


def test_oracle_outputs_unchanged_without_decisions(golden_dir):
    """Without decisions_of both builds compute exactly what they did before the clamp flags were recorded (golden generated by the
    earlier oracle: tests/golden/gen_clamp_edge_goldens.py): radii, fp32 colour and depth, and every gradient, bit for bit."""
    from util import clamp_edge_camera
    GRADS = ("means3D", "means2D", "colors_precomp", "opacities", "scales", "rotations")
    dL = np.random.default_rng(5).uniform(-1, 1, (3, 80, 96)).astype(np.float32)     # as gen_clamp_edge_goldens.loss_image
    z = np.load(os.path.join(golden_dir, "clamp_edge_oracle.npz"))
    cam = clamp_edge_camera()
    g = {k: z[f"in_{k}"] for k in ("means3D", "scales", "rotations", "opacities", "colors_precomp")}
    for tag, f64 in (("f32", False), ("f64", True)):
        o = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"],
                        rotations=g["rotations"], nthreads=4, f64=f64)
        assert np.array_equal(o.radii, z[f"{tag}/radii"]), tag
        if not f64:
            assert np.array_equal(o.color, z[f"{tag}/color"]) and np.array_equal(o.depth, z[f"{tag}/depth"])
        gr = o.backward(dL)
        for k in GRADS:
            assert np.array_equal(gr[k], z[f"{tag}/grad_{k}"]), (tag, k)
