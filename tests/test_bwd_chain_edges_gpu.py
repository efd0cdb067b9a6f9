"""The per-Gaussian backward chain (view_chain, gsr_preprocess_bwd.hip) against the fp64 oracle where it is ill-conditioned or where
its discrete decisions matter: at the frustum-clamp edge (single view and through every kernel build), in multi-view sums (including
views whose gradients cancel) and in scenes far from the world origin.

The reference of every test is the fp64 build of the tiled oracle taking over the fp32 run's discrete decisions (``decisions_of``):
radii, tile rects, depth keys and the frustum-clamp flags -- so at the clamp edge both sides differentiate the same function.  Multi-view
references are sums of the per-view fp64 runs.
"""
import numpy as np
import pytest
import torch

from hipcheck import ROW_TOL_WORST, TOL, _run_hip, _settings
from oracle import TiledOracle
from util import (clamp_edge_camera, clamp_edge_scene, frustum_decisions_fp32, frustum_decisions_mixed, look_at, oracle_camera,
                  random_gaussians, rel_err, ring_camera, row_err)

pytestmark = pytest.mark.gpu

EDGE_ROW_TOL = 1e-4
GEOM = ("means3D", "opacities", "scales", "rotations")


def _cov3d(g):
    q = g["rotations"].astype(np.float64)
    r, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    M = R * g["scales"].astype(np.float64)[:, None, :]
    S = M @ np.transpose(M, (0, 2, 1))
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def _variant(g, cam, kind):
    """The clamp-edge scene as colors_precomp, SH degree 3 or cov3D_precomp input."""
    g = dict(g)
    if kind == "sh3":
        rng = np.random.default_rng(17)
        g["shs"] = (rng.normal(size=(g["means3D"].shape[0], 16, 3)) * 0.4).astype(np.float32)
        del g["colors_precomp"]
        cam = clamp_edge_camera(cam.image_width, cam.image_height, sh_degree=3)
    elif kind == "cov3d":
        g["cov3D_precomp"] = _cov3d(g)
        del g["scales"], g["rotations"]
    return g, cam


def _oracles(cam, g):
    kw = dict(colors_precomp=g.get("colors_precomp"), shs=g.get("shs"), scales=g.get("scales"), rotations=g.get("rotations"),
              cov3D_precomp=g.get("cov3D_precomp"), nthreads=4)
    o32 = TiledOracle(cam, g["means3D"], g["opacities"], **kw)
    o64 = TiledOracle(cam, g["means3D"], g["opacities"], f64=True, decisions_of=o32, **kw)
    return o32, o64


def _loss(cam, o32, seed):
    dL = np.random.default_rng(seed).uniform(-1, 1, (3, cam.image_height, cam.image_width)).astype(np.float32)
    dL[:, o32.ambiguous] = 0.0      # threshold-ambiguous pixels: no gradient on either side
    return dL


def _keys(g):
    return [k for k in ("means3D", "means2D", "opacities", "scales", "rotations", "colors_precomp", "shs", "cov3D_precomp") if k in g or k == "means2D"]


def _referee(tag, got, r32, r64, keys, within_tol=True):
    """The soak referee's rule, norm-wise: the HIP path no further from fp64 than twice the fp32 oracle + 2e-5; and within TOL
    (``within_tol``) -- or, where the fp32 forward itself is further than TOL from fp64, max(TOL, 2 x fp32 oracle + 2e-5) as
    test_soak_gpu._adjudicate."""
    out = {}
    for k in keys:
        e_hip, e_o = rel_err(got[k], r64[k]), rel_err(r32[k], r64[k])
        out[k] = (e_hip, e_o)
        note = f"{tag} {k}: HIP {e_hip:.2e} / fp32 oracle {e_o:.2e} from fp64"
        print(note)
        if within_tol:
            assert e_hip <= 2.0 * e_o + 2e-5 and e_hip <= TOL, note
        else:
            assert e_hip <= max(TOL, 2.0 * e_o + 2e-5), note
    return out


def _edge_checks(tag, got, r64, keys, edge):
    for k in keys:
        e = rel_err(got[k], r64[k])
        assert e <= TOL, f"{tag} {k}: norm-wise {e:.3e} from fp64"
        w, row = row_err(got[k], r64[k])
        assert w <= ROW_TOL_WORST, f"{tag} {k}: row {row} off by {w:.3e} from fp64"
        we, rowe = row_err(got[k][edge], r64[k][edge])
        assert we <= EDGE_ROW_TOL, f"{tag} {k}: edge row {edge[rowe]} off by {we:.3e} from fp64"
        print(f"{tag} {k}: norm-wise {e:.2e}, worst row {w:.2e}, worst edge row {we:.2e}")


@pytest.fixture(scope="module")
def edge_scene():
    cam = clamp_edge_camera()
    g, edge = clamp_edge_scene(cam, seed=0)
    # the scene is adversarial for the old backward: its mixed-precision decision differs from the forward's on >= 16 Gaussians
    c32, _, _ = frustum_decisions_fp32(cam, g["means3D"])
    assert (c32 != frustum_decisions_mixed(cam, g["means3D"])).any(1).sum() >= 16
    return cam, g, edge


@pytest.mark.parametrize("kind", ["colors", "sh3", "cov3d"])
def test_clamp_edge_single_view(dev, edge_scene, kind):
    """C.1: ~200 Gaussians within 8 ulp of the 1.3 tanfov limit (both axes, signs and sides) among 300 ordinary ones, 96x80, off-centre
    principal point: every gradient within TOL norm-wise and ROW_TOL_WORST per row of fp64, the edge rows within 1e-4."""
    cam, g, edge = edge_scene
    g, cam = _variant(g, cam, kind)
    o32, o64 = _oracles(cam, g)
    assert (o32.radii[edge] > 0).sum() >= 0.9 * len(edge)
    dL = _loss(cam, o32, 3)
    _, radii, _, got, _ = _run_hip(cam, g, dev, dL)
    assert np.array_equal(radii, o32.radii)
    r64 = o64.backward(dL)
    _edge_checks(f"clamp edge {kind}", got, r64, _keys(g), edge)


def _views(cams, g, dev, dLc, fuse=False):
    """rasterize_gaussians_views with frozen per-view colours; a fresh settings object per view (no fusion) unless ``fuse``: then views
    with the same camera object share one settings object and the forward pairs them."""
    from diff_gaussian_rasterization import rasterize_gaussians_views
    t = {k: torch.tensor(g[k], device=dev, requires_grad=True) for k in GEOM}
    V, P = len(cams), g["means3D"].shape[0]
    m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
    memo = {}
    rs = [memo.setdefault(id(c), _settings(c, dev)) if fuse else _settings(c, dev) for c in cams]
    col = torch.tensor(g["colors_precomp"], device=dev)      # [P,3], or [V,P,3] per view
    seen = {}
    from diff_gaussian_rasterization import _hip
    orig = _hip.rasterize_forward_batch

    def spy(*a, **k):
        out = orig(*a, **k)
        seen["states"] = out[3]
        return out
    _hip.rasterize_forward_batch = spy
    try:
        im, _, _ = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], colors_precomp=col, scales=t["scales"],
                                             rotations=t["rotations"])
    finally:
        _hip.rasterize_forward_batch = orig
    (im * torch.tensor(dLc, device=dev)).sum().backward()
    torch.cuda.synchronize()
    out = {k: v.grad.detach().cpu().numpy() for k, v in t.items()}
    out["means2D"] = m2.grad.detach().cpu().numpy()
    return out, seen.get("states")


def _sum_ref(cams, g, dLc, cols=None):
    """Per-view fp32 oracle and fp64 referee, summed over views (fp64 sums); per-view means2D; and sum over views of |g_v|."""
    s32, s64, sabs = {k: 0.0 for k in GEOM}, {k: 0.0 for k in GEOM}, {k: 0.0 for k in GEOM}
    m2_32, m2_64 = [], []
    runs = {}
    for v, cam in enumerate(cams):
        gv = dict(g, colors_precomp=g["colors_precomp"] if cols is None else cols[v])
        key = (id(cam), v if cols is not None else -1)
        if key not in runs:
            runs[key] = _oracles(cam, gv)
        o32, o64 = runs[key]
        a, b = o32.backward(dLc[v]), o64.backward(dLc[v])
        for k in GEOM:
            s32[k] = s32[k] + np.asarray(a[k], np.float64)
            s64[k] = s64[k] + np.asarray(b[k], np.float64)
            sabs[k] = sabs[k] + np.abs(np.asarray(b[k], np.float64))
        m2_32.append(a["means2D"])
        m2_64.append(b["means2D"])
    s32["means2D"], s64["means2D"] = np.stack(m2_32), np.stack(m2_64)
    return s32, s64, sabs


def _losses(cams, seed):
    rng = np.random.default_rng(seed)
    dL = rng.uniform(-1, 1, (len(cams), 3, cams[0].image_height, cams[0].image_width)).astype(np.float32)
    return dL


def _mask_ambiguous(cams, g, dL, cols=None):
    for v, cam in enumerate(cams):
        gv = dict(g, colors_precomp=g["colors_precomp"] if cols is None else cols[v])
        o = TiledOracle(cam, gv["means3D"], gv["opacities"], colors_precomp=gv["colors_precomp"], scales=gv["scales"],
                        rotations=gv["rotations"], nthreads=4)
        dL[v][:, o.ambiguous] = 0.0
    return dL


@pytest.mark.parametrize("V", [1, 3, 6, 12])
def test_clamp_edge_multi_view_builds(dev, edge_scene, V):
    """C.2: the clamp-edge scene through the multi-view call: V = 1 (loop kernel), V = 3 / 6 / 12 distinct settings of the edge camera
    (wave kernels, MAXW = 4 / 8 / 16); the view sum against the sum of the fp64 referee's views."""
    cam, g, edge = edge_scene
    cams = [cam] * V
    dL = _mask_ambiguous(cams, g, _losses(cams, 20 + V))
    got, states = _views(cams, g, dev, dL)
    assert states[0].geometry_of is None
    _, r64, _ = _sum_ref(cams, g, dL)
    _edge_checks(f"clamp edge V={V}", got, r64, GEOM, edge)
    for v in range(V):
        assert rel_err(got["means2D"][v], r64["means2D"][v]) <= TOL, v


def test_clamp_edge_fused_pair(dev, edge_scene):
    """C.2: two views of ONE settings object with different frozen colours, which the forward fuses (geometry_of = [0, 0]), plus a
    third view: against the fp64 referee's view sum."""
    cam, g, edge = edge_scene
    rng = np.random.default_rng(31)
    P = g["means3D"].shape[0]
    cols = rng.uniform(0, 1, (3, P, 3)).astype(np.float32)
    cam2 = ring_camera(cam.image_width, cam.image_height, v=1, V=4)
    cams = [cam, cam, cam2]
    gv = dict(g, colors_precomp=cols)
    dL = _mask_ambiguous(cams, g, _losses(cams, 32), cols=cols)
    got, states = _views(cams, gv, dev, dL, fuse=True)
    assert list(states[0].geometry_of) == [0, 0, 2], "the forward did not pair the two views of one camera"
    _, r64, _ = _sum_ref(cams, g, dL, cols=cols)
    _edge_checks("clamp edge fused pair", got, r64, GEOM, edge)


def test_clamp_edge_depth_build(dev, edge_scene):
    """C.2: the differentiable-depth build (colour + random depth gradient) against the fp64 referee through the colour-channel identity
    (colour z_i as a channel, background 0, plus dz/dmeans3D), single view and V = 3 (wave kernel)."""
    from test_depth_grad_gpu import _hip, _oracle_ref, _views_call
    cam, g, edge = edge_scene
    H, W = cam.image_height, cam.image_width
    rng = np.random.default_rng(41)
    dLc = rng.uniform(-1, 1, (3, H, W)).astype(np.float32)
    dLd = rng.uniform(-1, 1, (1, H, W)).astype(np.float32)
    r32, oc = _oracle_ref(cam, g, dLc, dLd)
    amb = oc.ambiguous | r32["_runs"][1].ambiguous
    dLc[:, amb] = 0.0
    dLd[:, amb] = 0.0
    r32, _ = _oracle_ref(cam, g, dLc, dLd)
    r64, _ = _oracle_ref(cam, g, dLc, dLd, decisions_of=r32["_runs"])
    _, _, got = _hip(cam, g, dev, dLc, dLd)
    _edge_checks("clamp edge depth", got, r64, GEOM, edge)
    # V = 3: three distinct camera objects of the same view (no fusion), a wave kernel of the depth build
    cams = [clamp_edge_camera() for _ in range(3)]
    dLcv = np.stack([dLc * s for s in (1.0, -0.5, 0.25)]).astype(np.float32)
    dLdv = np.stack([dLd * s for s in (0.5, 1.0, -1.0)]).astype(np.float32)
    _, _, gotv = _views_call(cams, g, dev, dLcv, dLdv)
    ref = {k: 0.0 for k in GEOM}
    for v in range(3):
        rv, _ = _oracle_ref(cam, g, dLcv[v], dLdv[v], decisions_of=r32["_runs"])
        for k in GEOM:
            ref[k] = ref[k] + rv[k]
    _edge_checks("clamp edge depth V=3", gotv, ref, GEOM, edge)


def _row_sum_check(tag, got, r64, sabs, floor_frac=1e-6):
    """Per row: |HIP - fp64| <= 1e-4 * max_j sum_v |g_v,ij| + floor, floor = 1e-6 of the tensor's largest sum_v |g_v|: the bar is relative
    to the conditioning of the view sum, not to the row's own (possibly cancelled) value."""
    worst = 0.0
    for k in GEOM:
        a, b, s = (np.asarray(x, np.float64).reshape(x.shape[0], -1) for x in (got[k], r64[k], sabs[k]))
        bar = 1e-4 * s.max(1) + floor_frac * s.max()
        r = np.abs(a - b).max(1) / bar
        i = int(np.argmax(r))
        worst = max(worst, float(r[i]) * 1e-4)
        print(f"{tag} {k}: worst row {i} |HIP - fp64| = {r[i] * 1e-4:.2e} of its sum of |g_v| (bar 1e-4)")
        assert r[i] <= 1.0, f"{tag} {k}: row {i} off by {r[i]:.2f} bars"
    return worst


@pytest.mark.parametrize("V", [2, 5, 8, 16])
def test_multi_view_sum_ring(dev, V):
    """C.3: V ring cameras, 600 Gaussians: view sums against the fp64 referee's view sum, norm-wise (referee rule) and per row
    relative to sum_v |g_v|."""
    P, W, H = 600, 96, 80
    g = random_gaussians(P, seed=50 + V, scale_lo=0.03, scale_hi=0.25)
    cams = [ring_camera(W, H, v=v, V=V, cx=0.45 * W) for v in range(V)]
    dL = _mask_ambiguous(cams, g, _losses(cams, 60 + V))
    got, _ = _views(cams, g, dev, dL)
    r32, r64, sabs = _sum_ref(cams, g, dL)
    _referee(f"ring V={V}", got, r32, r64, GEOM)
    _row_sum_check(f"ring V={V}", got, r64, sabs)


def _cancelling_losses(cams, g, seed):
    """Loss images for pairs of opposite cameras (views 2k, 2k+1) whose means3D gradients cancel in the view sum.  View 2k gets a random
    image; view 2k+1 a combination of 3P + 64 random images, solved by least squares (the gradient is linear in the loss image; the
    fp64 referee gives each image's gradient) so that its dL/dmeans3D is minus view 2k's."""
    rng = np.random.default_rng(seed)
    H, W = cams[0].image_height, cams[0].image_width
    P = g["means3D"].shape[0]
    dL = np.zeros((len(cams), 3, H, W), np.float32)
    for k in range(0, len(cams), 2):
        oa, ob = _oracles(cams[k], g), _oracles(cams[k + 1], g)
        okb = ~ob[0].ambiguous
        dL[k] = rng.uniform(-1, 1, (3, H, W)).astype(np.float32)
        dL[k][:, oa[0].ambiguous] = 0.0
        target = -np.asarray(oa[1].backward(dL[k])["means3D"], np.float64).reshape(-1)
        basis = rng.uniform(-1, 1, (3 * P + 64, 3, H, W)).astype(np.float32) * okb
        G = np.stack([np.asarray(ob[1].backward(b)["means3D"], np.float64).reshape(-1) for b in basis], 1)
        alpha = np.linalg.lstsq(G, target, rcond=None)[0]
        dL[k + 1] = np.tensordot(alpha, basis.astype(np.float64), 1).astype(np.float32)
    return dL


def test_multi_view_sum_cancelling(dev):
    """C.3: four pairs of opposite cameras (V = 8), loss images chosen so that each pair's means3D gradients cancel: the view-summed
    dL/dmeans3D of most rows is <= 1e-2 of sum_v |g_v|.  The per-row bar is relative to sum_v |g_v|, not to the cancelled sum."""
    P, W, H, V = 40, 64, 48, 8
    g = random_gaussians(P, seed=71, scale_lo=0.05, scale_hi=0.2, spread=0.5)
    cams = []
    for k in range(4):
        th = np.pi / 2 * k + 0.4
        c = np.array([4.0 * np.cos(th), 0.3 * (k - 1.5), 4.0 * np.sin(th)])
        cams += [oracle_camera(W, H, look_at(c)), oracle_camera(W, H, look_at(-c))]
    dL = _cancelling_losses(cams, g, 72)
    got, _ = _views(cams, g, dev, dL)
    r32, r64, sabs = _sum_ref(cams, g, dL)
    live = sabs["means3D"].max(1) > 0
    ratio = np.abs(r64["means3D"]).max(1)[live] / sabs["means3D"].max(1)[live]
    print(f"cancelling V=8: means3D rows |sum_v g_v| / sum_v |g_v|: median {np.median(ratio):.2e}, <= 1e-2 for {(ratio <= 1e-2).mean():.0%}")
    assert (ratio <= 1e-2).mean() >= 0.75, "the loss images do not cancel"
    _referee("cancelling V=8", got, r32, r64, ("opacities", "scales", "rotations"))
    _row_sum_check("cancelling V=8", got, r64, sabs)


def _translated(offset):
    P, W, H, V = 500, 96, 80, 4
    g = random_gaussians(P, seed=81, scale_lo=0.03, scale_hi=0.25)
    d = np.array([1.0, 0.6, -0.8]) / np.linalg.norm([1.0, 0.6, -0.8]) * offset
    g["means3D"] = (g["means3D"].astype(np.float64) + d).astype(np.float32)
    cams = []
    for v in range(V):
        th = 2 * np.pi * v / V + 0.3
        c = np.array([4.0 * np.cos(th), 0.8, 4.0 * np.sin(th)])
        cams.append(oracle_camera(W, H, look_at(c + d, target=d), cx=0.45 * W))
    return g, cams


@pytest.mark.parametrize("offset", [0.0, 50.0, 500.0])
def test_translated_scene(dev, offset):
    """C.4: a 500-Gaussian, 4-view scene and its cameras moved by the same rigid offset: the referee rule against fp64 at every offset;
    at 500 the HIP path as far from fp64 as the fp32 oracle, norm-wise, for means3D, scales and rotations.

    Both distances are the fp32 FORWARD's (already ~1e-3 at offset 50): the HIP path and the fp32 oracle share its bits, so the ratio is
    1.00 +- 0.001 with or without the fp64 chain's widened operands (measured: means3D 1.001, scales 1.000, rotations 0.999, the same
    before the widening).  This test does not discriminate the chain's arithmetic; the 1 % allowance only pins that the chain adds
    nothing measurable to the forward's error."""
    g, cams = _translated(offset)
    dL = _mask_ambiguous(cams, g, _losses(cams, 90))
    got, _ = _views(cams, g, dev, dL)
    r32, r64, _ = _sum_ref(cams, g, dL)
    # far from the origin the fp32 forward (pvz, hw: small differences of large terms) is itself ~1e-3 from fp64 at offset 500, in the
    # HIP path and the fp32 oracle alike: the referee's max(TOL, ...) form
    errs = _referee(f"offset {offset:g}", got, r32, r64, GEOM, within_tol=False)
    if offset >= 500.0:
        for k in ("means3D", "scales", "rotations"):
            e_hip, e_o = errs[k]
            print(f"offset {offset:g} {k}: HIP / fp32 oracle distance to fp64 = {e_hip / max(e_o, 1e-300):.3f}")
            assert e_hip <= 1.01 * e_o, f"offset {offset:g} {k}: HIP {e_hip:.2e} further from fp64 than the fp32 oracle {e_o:.2e}"
