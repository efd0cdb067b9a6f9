"""Rendered alpha (GaussianRasterizer(..., return_alpha=True), rasterize_gaussians(..., return_alpha=True),
rasterize_gaussians_views(..., return_alpha=True)): the fourth output A = 1 - final_T and its gradient.

References are the unedited oracles through two identities (tests/test_alpha_cpu.py checks them in fp64):
  (I1) A is channel 0 of a render with colours_precomp = 1 and background 0;
  (I2) A is 1 + channel 0 of a render with colours_precomp = 0 and background (-1, 0, 0) -- the blend backward's own arithmetic.
Geometry gradients are linear in the incoming gradients: the reference of a colour + alpha loss is the ordinary render's backward(dLc) plus
the I1 render's backward((dLa, 0, 0)), summed over the geometry inputs.  Rows that miss the fp32 bars go to the fp64 build of the oracle as
referee, with the rule of test_depth_grad_gpu._compare.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hipcheck import ROW_TOL_WORST, TOL, _row_check, _settings
from oracle import OracleCamera, TiledOracle
from util import random_gaussians, rel_err, ring_camera, row_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = ("means3D", "means2D", "opacities", "scales", "rotations", "cov3D_precomp")


def _with_bg(cam, bg):
    return OracleCamera(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, np.asarray(bg, np.float32), cam.scale_modifier,
                        cam.viewmatrix, cam.projmatrix, cam.sh_degree, cam.campos)


def _geo(g):
    return dict(scales=g.get("scales"), rotations=g.get("rotations"), cov3D_precomp=g.get("cov3D_precomp"))


def _oracle_ref(cam, g, dLc, dLa, decisions_of=None):
    """Gradients of sum(dLc * colour) + sum(dLa * alpha) from the unedited tiled oracle (I1 for the alpha term).  ``decisions_of``: the
    (colour, alpha) runs of an earlier fp32 call -- then the fp64 build, taking over their discrete decisions (the referee)."""
    P = g["means3D"].shape[0]
    H, W = cam.image_height, cam.image_width
    f64 = decisions_of is not None
    oc = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g.get("colors_precomp"), shs=g.get("shs"), nthreads=4, f64=f64,
                     decisions_of=decisions_of[0] if f64 else None, **_geo(g))
    oa = TiledOracle(_with_bg(cam, (0, 0, 0)), g["means3D"], g["opacities"], colors_precomp=np.ones((P, 3), np.float32), nthreads=4,
                     f64=f64, decisions_of=decisions_of[1] if f64 else None, **_geo(g))
    z = np.zeros((H, W), np.float32)
    gra = oa.backward(np.stack([dLa.reshape(H, W), z, z]))
    out = {}
    if dLc is not None:
        out = {k: np.asarray(v, np.float64) for k, v in oc.backward(dLc).items() if v is not None}
    for k in GEOM:
        if gra.get(k) is not None:
            out[k] = out.get(k, 0.0) + np.asarray(gra[k], np.float64)
    if dLc is None:
        out["colors_precomp"] = np.zeros((P, 3))
    out["_runs"] = (oc, oa)
    return out, oc


def _hip(cam, g, dev, dLc, dLa, frozen=(), sh_degree=None, depth=False, dLd=None):
    """One GaussianRasterizer(return_alpha=True) call, loss sum(dLc * colour) + sum(dLa * alpha) [+ sum(dLd * depth)]."""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = {k: torch.tensor(v, device=dev, requires_grad=k not in frozen) for k, v in g.items()}
    m2 = torch.zeros((g["means3D"].shape[0], 3), device=dev, requires_grad=True)
    r = GaussianRasterizer(raster_settings=_settings(cam, dev, sh_degree=sh_degree), differentiable_depth=depth, return_alpha=True)
    out = r(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], shs=t.get("shs"), colors_precomp=t.get("colors_precomp"),
            scales=t.get("scales"), rotations=t.get("rotations"), cov3D_precomp=t.get("cov3D_precomp"))
    assert len(out) == 4
    color, _, dimg, alpha = out
    loss = (alpha * torch.tensor(dLa.reshape(alpha.shape), device=dev)).sum()
    if dLc is not None:
        loss = loss + (color * torch.tensor(dLc, device=dev)).sum()
    if dLd is not None:
        loss = loss + (dimg * torch.tensor(dLd.reshape(dimg.shape), device=dev)).sum()
    loss.backward()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in t.items() if v.grad is not None}
    grads["means2D"] = m2.grad.detach().cpu().numpy()
    torch.cuda.synchronize()
    return color.detach().cpu().numpy(), alpha.detach().cpu().numpy(), grads


def _compare(tag, got, ref, keys, cam=None, g=None, dLc=None, dLa=None):
    """The fp32 bars against the oracle reference; a tensor that misses them goes to the fp64 referee with test_depth_grad_gpu._compare's
    rule (the HIP path no further from fp64 than twice the fp32 oracle + 2e-5 norm-wise, four times + 1e-4 in its worst row)."""
    ref64 = None
    for k in keys:
        if k not in got or k not in ref:
            continue
        try:
            e = rel_err(got[k], ref[k])
            assert e < TOL, f"{tag} grad {k}: rel err {e:.3e}"
            _row_check(f"alpha {tag} grad {k}", got[k], ref[k])
        except AssertionError:
            if cam is None:
                raise
            if ref64 is None:
                ref64, _ = _oracle_ref(cam, g, dLc, dLa, decisions_of=ref["_runs"])
            e_hip, e_o = rel_err(got[k], ref64[k]), rel_err(ref[k], ref64[k])
            r_hip, r_o = row_err(got[k], ref64[k])[0], row_err(ref[k], ref64[k])[0]
            note = f"{tag} grad {k} vs fp64: norm-wise HIP {e_hip:.2e} / fp32 oracle {e_o:.2e}, worst row HIP {r_hip:.2e} / fp32 oracle {r_o:.2e}"
            assert e_hip <= max(TOL, 2.0 * e_o + 2e-5), note
            assert r_hip <= max(ROW_TOL_WORST, 4.0 * r_o + 1e-4), note


def _loss_images(cam, seed, ok, V=None):
    H, W = cam.image_height, cam.image_width
    rng = np.random.default_rng(seed)
    lead = () if V is None else (V,)
    dLc = rng.uniform(-1, 1, lead + (3, H, W)).astype(np.float32)
    dLa = rng.uniform(-1, 1, lead + (1, H, W)).astype(np.float32)
    dLc[..., ~ok] = 0.0        # threshold-ambiguous pixels: no gradient on either side
    dLa[..., ~ok] = 0.0
    return dLc, dLa


def _probe(cam, g):
    return TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=np.ones((g["means3D"].shape[0], 3), np.float32), **_geo(g))


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("pynode", [False, True])
def test_forward_single_view(dev, monkeypatch, pynode):
    """alpha = 1 - final_T of the forward's own image state, bit for bit (the ctypes forward of the same call is deterministic); within
    1e-4 of the oracle's 1 - final_T on unambiguous pixels; within 1e-4 of channel 0 of the colours-1-on-black render (the mask render)."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer, _hip
    monkeypatch.setattr(dgr, "_PY_NODE", pynode)
    P, W, H = 3000, 200, 150
    g = random_gaussians(P, seed=31, scale_lo=0.02, scale_hi=0.25)
    cam = ring_camera(W, H, v=2, bg=(0.1, 0.3, 0.5))
    rs = _settings(cam, dev)
    t = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    kw = dict(means3D=t["means3D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    seen = {}
    orig = _hip.rasterize_forward
    if pynode:
        def spy(*a, **k):
            seen["out"] = orig(*a, **k)
            return seen["out"]
        monkeypatch.setattr(_hip, "rasterize_forward", spy)
    m2 = torch.zeros((P, 3), device=dev)
    color, radii, depth, alpha = GaussianRasterizer(rs, return_alpha=True)(means2D=m2, colors_precomp=t["colors_precomp"], **kw)
    assert alpha.shape == (1, H, W) and alpha.dtype == torch.float32
    if pynode:
        state = seen["out"][3]
    else:
        state = orig(rs, t["means3D"], t["opacities"], t["colors_precomp"], None, t["scales"], t["rotations"], None)[3]
    want = 1.0 - _hip.final_transmittance(state)
    assert torch.equal(alpha[0], want)
    c3, _, d3 = GaussianRasterizer(rs)(means2D=m2, colors_precomp=t["colors_precomp"], **kw)
    assert torch.equal(color, c3) and torch.equal(depth, d3)
    oc = _probe(cam, g)
    ok = ~oc.ambiguous
    a = alpha[0].cpu().numpy()
    assert np.abs(a - (1.0 - oc.final_T))[ok].max() < 1e-4
    rs0 = _settings(_with_bg(cam, (0, 0, 0)), dev)
    mask, _, _ = GaussianRasterizer(rs0)(means2D=m2, colors_precomp=torch.ones_like(t["colors_precomp"]), **kw)
    assert (alpha[0] - mask[0]).abs().max().item() < 1e-4
    assert a.max() > 0.5 and a.min() >= 0.0


def _spy(monkeypatch, name, rewrite=None):
    """Wrap _hip.<name>; record its results (forward: the states) and optionally rewrite its keyword arguments."""
    from diff_gaussian_rasterization import _hip
    orig, seen = getattr(_hip, name), {}

    def spy(*a, **k):
        if rewrite is not None:
            k = rewrite(k)
        seen["kw"] = k
        out = orig(*a, **k)
        seen["out"] = out
        return out
    monkeypatch.setattr(_hip, name, spy)
    return seen


@pytest.mark.parametrize("mode", ["grad", "forward_only", "pair", "pair_forward_only", "sh"])
def test_forward_batch(dev, monkeypatch, mode):
    """Batch calls: alpha[v] = 1 - final_T of view v's state bit for bit -- with grad, forward-only (torch.no_grad()), a fused pair of
    one camera (the partner's transmittance is written by its owner's tile pass), and SH colours (per-view single-view states)."""
    from diff_gaussian_rasterization import _hip, rasterize_gaussians_views
    P, W, H = 2500, 144, 112
    g = random_gaussians(P, seed=17, scale_lo=0.02, scale_hi=0.25, sh_M=16)
    cams = [ring_camera(W, H, v=v, V=3, bg=(0.1, 0.2, 0.3), sh_degree=2) for v in range(3)]
    rs = [_settings(c, dev) for c in cams]
    if mode.startswith("pair"):
        rs = [rs[0], rs[0], rs[2]]
    t = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in g.items()}
    m2 = torch.zeros((3, P, 3), device=dev, requires_grad=True)
    col = {"shs": t["shs"]} if mode == "sh" else {"colors_precomp": torch.tensor(np.random.default_rng(2).uniform(0, 1, (3, P, 3)).astype(np.float32), device=dev)
                                                 if mode.startswith("pair") else t["colors_precomp"]}
    fwd = _spy(monkeypatch, "rasterize_forward_batch")
    with torch.set_grad_enabled(not mode.endswith("forward_only")):
        im, radii, depth, alpha = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], scales=t["scales"], rotations=t["rotations"],
                                                            return_alpha=True, **col)
    states = fwd["out"][3]
    if mode.startswith("pair"):
        assert list(states[0].geometry_of) == [0, 0, 2], "the forward did not pair the two views of one camera"
    assert alpha.shape == (3, 1, H, W)
    for v in range(3):
        assert torch.equal(alpha[v, 0], 1.0 - _hip.final_transmittance(states[v])), v
    with torch.set_grad_enabled(not mode.endswith("forward_only")):     # the same call without the keyword: the same three outputs
        base = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], scales=t["scales"], rotations=t["rotations"], **col)
    assert len(base) == 3 and torch.equal(base[0], im) and torch.equal(base[1], radii) and torch.equal(base[2], depth)
    if mode.startswith("pair"):
        assert torch.equal(alpha[0], alpha[1])
    for v in range(3):
        oc = _probe(cams[0 if mode.startswith("pair") and v == 1 else v], g)
        ok = ~oc.ambiguous
        assert np.abs(alpha[v, 0].detach().cpu().numpy() - (1.0 - oc.final_T))[ok].max() < 1e-4, v


def test_zero_gaussians(dev):
    from diff_gaussian_rasterization import GaussianRasterizer
    cam = ring_camera(40, 30, v=1)
    e = torch.zeros((0, 3), device=dev, requires_grad=True)
    out = GaussianRasterizer(_settings(cam, dev), return_alpha=True)(
        means3D=e, means2D=torch.zeros((0, 3), device=dev), opacities=torch.zeros((0, 1), device=dev),
        colors_precomp=torch.zeros((0, 3), device=dev), scales=torch.zeros((0, 3), device=dev), rotations=torch.zeros((0, 4), device=dev))
    assert len(out) == 4 and out[3].shape == (1, 30, 40) and not out[3].any()


# ---------------------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("colour_loss", [False, True])
@pytest.mark.parametrize("colour_grad", [False, True])
@pytest.mark.parametrize("P,W,H,seed", [(37, 33, 17, 2), (700, 130, 94, 3), (3000, 200, 150, 5)])
def test_precomputed_colours_vs_tiled_oracle(dev, P, W, H, seed, colour_loss, colour_grad):
    """Alpha-only and colour + alpha losses; colour gradient wanted (nine-sum build) or not (six-sum, !COL build).  The alpha term never
    reaches the colours: an alpha-only loss leaves dL/dcolour at exactly zero."""
    g = random_gaussians(P, seed=seed, scale_lo=0.02, scale_hi=0.25)
    cam = ring_camera(W, H, v=seed, bg=(0.1, 0.3, 0.5))
    dLc, dLa = _loss_images(cam, seed, ~_probe(cam, g).ambiguous)
    if not colour_loss:
        dLc = None
    ref, _ = _oracle_ref(cam, g, dLc, dLa)
    _, _, got = _hip(cam, g, dev, dLc, dLa, frozen=() if colour_grad else ("colors_precomp",))
    assert ("colors_precomp" in got) == colour_grad
    if colour_grad and not colour_loss:
        assert not got["colors_precomp"].any()
    _compare(f"P={P} {W}x{H} colour_loss={colour_loss} colour_grad={colour_grad}", got, ref,
             ("means3D", "means2D", "opacities", "scales", "rotations", "colors_precomp"), cam, g, dLc, dLa)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_spherical_harmonics_vs_tiled_oracle(dev, deg):
    P, W, H = 900, 120, 90
    g = random_gaussians(P, seed=50 + deg, scale_lo=0.03, scale_hi=0.3, sh_M=16)
    del g["colors_precomp"]
    cam = ring_camera(W, H, v=2, bg=(0.2, 0.1, 0.0), sh_degree=deg)
    dLc, dLa = _loss_images(cam, 17 + deg, ~_probe(cam, g).ambiguous)
    ref, _ = _oracle_ref(cam, g, dLc, dLa)
    _, _, got = _hip(cam, g, dev, dLc, dLa, sh_degree=deg)
    _compare(f"SH {deg}", got, ref, ("means3D", "means2D", "opacities", "scales", "rotations", "shs"), cam, g, dLc, dLa)
    # the alpha term does not reach the SHs: an alpha-only loss gives them exactly zero
    _, _, only = _hip(cam, g, dev, None, dLa, sh_degree=deg)
    assert not only["shs"].any()


def _cov3d(g):
    q = g["rotations"].astype(np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * g["scales"].astype(np.float64)[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def test_cov3d_precomp_vs_tiled_oracle(dev):
    P, W, H = 500, 96, 80
    g = random_gaussians(P, seed=71, scale_lo=0.03, scale_hi=0.3)
    g["cov3D_precomp"] = _cov3d(g)
    del g["scales"], g["rotations"]
    cam = ring_camera(W, H, v=3, bg=(0.0, 0.0, 0.0))
    dLc, dLa = _loss_images(cam, 21, ~_probe(cam, g).ambiguous)
    ref, _ = _oracle_ref(cam, g, dLc, dLa)
    _, _, got = _hip(cam, g, dev, dLc, dLa)
    _compare("cov3D_precomp", got, ref, ("means3D", "means2D", "opacities", "cov3D_precomp", "colors_precomp"), cam, g, dLc, dLa)


_PC_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = sys.argv[2].split("|")
loss_images = np.load(sys.argv[3])
from hipcheck import _settings
from util import random_gaussians, ring_camera
from diff_gaussian_rasterization import rasterize_gaussians_views
P, W, H, V = 30000, 256, 192, 2
g = random_gaussians(P, seed=91, scale_lo=0.03, scale_hi=0.3)
dev = torch.device("cuda:0")
cams = [ring_camera(W, H, v=v, V=V, bg=(0.1, 0.2, 0.3)) for v in range(V)]
t = {k: torch.tensor(v, device=dev, requires_grad=k != "colors_precomp") for k, v in g.items()}
m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
dLc = torch.tensor(loss_images["dLc"], device=dev)
dLa = torch.tensor(loss_images["dLa"], device=dev)
im, _, _, a = rasterize_gaussians_views([_settings(c, dev) for c in cams], t["means3D"], m2, t["opacities"], colors_precomp=t["colors_precomp"],
                                       scales=t["scales"], rotations=t["rotations"], return_alpha=True)
((im * dLc).sum() + (a * dLa).sum()).backward()
out = {k: v.grad.cpu().numpy() for k, v in t.items() if v.grad is not None}
out["means2D"] = m2.grad.cpu().numpy()
out["alpha"] = a.detach().cpu().numpy()
np.savez(sys.argv[1], **out)
"""


def test_producer_consumer_build(tmp_path):
    """render_bwd_pc (forced with GSR_BWD_PC=1 in a child process: the switch is read once per process) takes the alpha term in its
    consumer's per-tile constants: bit-identical to the barrier form (GSR_BWD_PC=0), and against the oracle."""
    P, W, H, V = 30000, 256, 192, 2
    g = random_gaussians(P, seed=91, scale_lo=0.03, scale_hi=0.3)
    cams = [ring_camera(W, H, v=v, V=V, bg=(0.1, 0.2, 0.3)) for v in range(V)]
    imgs = [_loss_images(cams[v], 95 + v, ~_probe(cams[v], g).ambiguous) for v in range(V)]
    dLc, dLa = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    np.savez(str(tmp_path / "loss.npz"), dLc=dLc, dLa=dLa)
    paths = "|".join([ROOT, os.path.join(ROOT, "gs-dynamics_amd"), os.path.join(ROOT, "tests")])
    res = {}
    for pc in (0, 1):
        out = str(tmp_path / f"pc{pc}.npz")
        subprocess.run([sys.executable, "-c", _PC_CHILD, out, paths, str(tmp_path / "loss.npz")], check=True, timeout=300,
                       env=dict(os.environ, GSR_BWD_PC=str(pc)), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        res[pc] = np.load(out)
    for k in res[0].files:
        assert np.array_equal(res[0][k], res[1][k]), f"{k}: producer / consumer backward differs from the barrier form"
    refs = [_oracle_ref(cams[v], g, dLc[v], dLa[v])[0] for v in range(V)]
    for k in ("means3D", "opacities", "scales", "rotations"):
        e = rel_err(res[1][k], sum(r[k] for r in refs))
        assert e < TOL, f"producer / consumer grad {k}: rel err {e:.3e}"
    for v in range(V):
        assert rel_err(res[1]["means2D"][v], refs[v]["means2D"]) < TOL, v


def test_backends_agree(dev, monkeypatch):
    """The two single-view backends -- the C++ node, and the Python node over the ctypes binding, chosen by the switch and forced by a spy
    on the ctypes forward -- give the same alpha and the same gradients of a colour + alpha loss."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _hip as hip
    P, W, H = 2500, 150, 110
    g = random_gaussians(P, seed=27, scale_lo=0.02, scale_hi=0.25)
    cam = ring_camera(W, H, v=1, bg=(0.3, 0.1, 0.2))
    dLc, dLa = _loss_images(cam, 28, np.ones((H, W), bool))
    runs = [_hip(cam, g, dev, dLc, dLa)]
    monkeypatch.setattr(dgr, "_PY_NODE", True)
    bwd = _spy(monkeypatch, "rasterize_backward")
    runs.append(_hip(cam, g, dev, dLc, dLa))
    assert bwd["kw"].get("grad_alpha") is not None, "the switch did not run the ctypes backward with an alpha gradient"
    monkeypatch.setattr(dgr, "_PY_NODE", False)
    orig, called = hip.rasterize_forward, []

    def spy(*a, **k):
        called.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(hip, "rasterize_forward", spy)
    runs.append(_hip(cam, g, dev, dLc, dLa))
    assert called
    for r in runs[1:]:
        assert np.array_equal(r[1], runs[0][1])
        for k in runs[0][2]:
            a, b = np.asarray(r[2][k], np.float64), np.asarray(runs[0][2][k], np.float64)
            assert np.abs(a - b).max() <= 1e-5 * (np.abs(b).max() + 1e-30), k


def test_against_dense_fp64_oracle(dev):
    """fp64 dense oracle, I1 (colours 1, background 0), autograd."""
    from oracle.dense_oracle import dense_rasterize
    P, W, H = 60, 40, 36
    g = random_gaussians(P, seed=24, scale_lo=0.05, scale_hi=0.4)
    cam = ring_camera(W, H, v=1, bg=(0.3, 0.2, 0.1))
    _, dLa = _loss_images(cam, 25, ~_probe(cam, g).ambiguous)
    f64 = torch.float64
    t = {k: torch.tensor(v, dtype=f64, requires_grad=True) for k, v in g.items()}
    color, _, _, _ = dense_rasterize(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, dtype=f64), 1.0, torch.tensor(cam.viewmatrix),
                                     torch.tensor(cam.projmatrix), 0, torch.tensor(cam.campos), t["means3D"], t["opacities"],
                                     colors_precomp=torch.ones((P, 3), dtype=f64), scales=t["scales"], rotations=t["rotations"])
    (color[0] * torch.tensor(dLa[0], dtype=f64)).sum().backward()
    _, _, got = _hip(cam, g, dev, None, dLa, frozen=("colors_precomp",))
    for k in ("means3D", "opacities", "scales", "rotations"):
        e = rel_err(got[k], t[k].grad.numpy())
        assert e < TOL, f"dense fp64 grad {k}: rel err {e:.3e}"


def test_alpha_and_depth_together(dev):
    """return_alpha and differentiable_depth at once: the sum of the three oracle terms (colour, depth channel, alpha channel)."""
    from test_depth_grad_gpu import _oracle_ref as _depth_ref
    P, W, H = 1500, 128, 96
    g = random_gaussians(P, seed=33, scale_lo=0.02, scale_hi=0.25)
    cam = ring_camera(W, H, v=2, bg=(0.1, 0.3, 0.5))
    dLc, dLa = _loss_images(cam, 34, ~_probe(cam, g).ambiguous)
    dLd = np.random.default_rng(35).uniform(-1, 1, (1, H, W)).astype(np.float32)
    dLd[:, _probe(cam, g).ambiguous] = 0.0
    ref_cd, _ = _depth_ref(cam, g, dLc, dLd)
    ref_a, _ = _oracle_ref(cam, g, None, dLa)
    _, _, got = _hip(cam, g, dev, dLc, dLa, frozen=("colors_precomp",), depth=True, dLd=dLd)
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        want = ref_cd[k] + ref_a[k]
        e = rel_err(got[k], want)
        assert e < TOL, f"alpha + depth grad {k}: rel err {e:.3e}"
    # and both terms are really there
    _, _, no_a = _hip(cam, g, dev, dLc, np.zeros_like(dLa), frozen=("colors_precomp",), depth=True, dLd=dLd)
    assert rel_err(no_a["opacities"], got["opacities"]) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- multi-view
def _views_call(cams, g, dev, dLc, dLa, per_view_col=None, retain=False, alpha=True, dLd=None):
    from diff_gaussian_rasterization import rasterize_gaussians_views
    t = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in g.items() if k != "colors_precomp"}
    col = torch.tensor(g["colors_precomp"] if per_view_col is None else per_view_col, device=dev)
    V = len(cams)
    m2 = torch.zeros((V, g["means3D"].shape[0], 3), device=dev, requires_grad=True)
    memo = {}      # the same camera object twice -> ONE settings object (the forward pairs views by their camera tensors)
    rs = [memo.setdefault(id(c), _settings(c, dev)) for c in cams]
    kw = dict(return_alpha=True) if alpha else {}
    if dLd is not None:
        kw["differentiable_depth"] = True
    out = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], colors_precomp=col, scales=t["scales"], rotations=t["rotations"], **kw)
    loss = (out[0] * torch.tensor(dLc, device=dev)).sum()
    if dLa is not None:
        loss = loss + (out[3] * torch.tensor(dLa, device=dev)).sum()
    if dLd is not None:
        loss = loss + (out[2] * torch.tensor(dLd, device=dev)).sum()
    loss.backward(retain_graph=retain)
    grads = {k: v.grad.detach().cpu().numpy() for k, v in t.items()}
    grads["means2D"] = m2.grad.detach().cpu().numpy()
    if retain:        # a second backward over the same states: the same gradients
        for v in list(t.values()) + [m2]:
            v.grad = None
        loss.backward()
        for k, v in list(t.items()) + [("means2D", m2)]:
            assert np.array_equal(grads[k], v.grad.detach().cpu().numpy()), f"second backward: {k}"
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in out], grads


def test_multiview_equals_sum_of_single_views(dev):
    """V = 4, alpha loss on views 0 and 2 (zero images elsewhere): the batch equals the sum of the single-view calls; each view's alpha
    term lands in its own means2D rows."""
    P, W, H, V = 3000, 160, 120, 4
    g = random_gaussians(P, seed=42, scale_lo=0.02, scale_hi=0.25)
    cams = [ring_camera(W, H, v=v, V=V, bg=(0.2, 0.1, 0.3)) for v in range(V)]
    rng = np.random.default_rng(43)
    dLc = rng.uniform(-1, 1, (V, 3, H, W)).astype(np.float32)
    dLa = rng.uniform(-1, 1, (V, 1, H, W)).astype(np.float32)
    dLa[1] = 0.0
    dLa[3] = 0.0
    _, got = _views_call(cams, g, dev, dLc, dLa)
    single = [_hip(cams[v], g, dev, dLc[v], dLa[v], frozen=("colors_precomp",))[2] for v in range(V)]
    for k in ("means3D", "opacities", "scales", "rotations"):
        assert rel_err(got[k], sum(s[k].astype(np.float64) for s in single)) < TOL, k
    for v in range(V):
        assert rel_err(got["means2D"][v], single[v]["means2D"]) < TOL, v
    _, noalpha = _views_call(cams, g, dev, dLc, None)
    for v in (1, 3):       # no alpha loss on these views: their means2D rows are the colour-only ones
        assert rel_err(got["means2D"][v], noalpha["means2D"][v]) < TOL, v
    for v in (0, 2):
        assert rel_err(got["means2D"][v], noalpha["means2D"][v]) > 1e-3, v


@pytest.mark.parametrize("depth", [False, True])
def test_multiview_fused_pair(dev, monkeypatch, depth):
    """Views 0 and 1 share one camera (ONE settings object) and have different frozen colours: the forward fuses them (geometry_of =
    [0, 0, 2]).  With alpha alone the backward keeps the pair fused (gsr_backward_batch_ex, no depth entries: the pair pass adds each
    view's own alpha term); with depth as well it runs unfused.  Either way: the sum of one single-view call per view, and a second
    retain_graph backward repeats the first."""
    P, W, H = 2000, 128, 96
    g = random_gaussians(P, seed=44, scale_lo=0.02, scale_hi=0.25)
    cam, cam2 = ring_camera(W, H, v=1, bg=(0.0, 0.0, 0.0)), ring_camera(W, H, v=3, bg=(0.0, 0.0, 0.0))
    rng = np.random.default_rng(45)
    cols = rng.uniform(0, 1, (3, P, 3)).astype(np.float32)
    dLc = rng.uniform(-1, 1, (3, 3, H, W)).astype(np.float32)
    dLa = rng.uniform(-1, 1, (3, 1, H, W)).astype(np.float32)
    dLd = rng.uniform(-1, 1, (3, 1, H, W)).astype(np.float32) if depth else None
    fwd = _spy(monkeypatch, "rasterize_forward_batch")
    bwd = _spy(monkeypatch, "rasterize_backward_batch")
    _, got = _views_call([cam, cam, cam2], g, dev, dLc, dLa, per_view_col=cols, retain=True, dLd=dLd)
    states = fwd["out"][3]
    assert list(states[0].geometry_of) == [0, 0, 2], "the forward did not pair the two views of one camera"
    assert states[1].binning is None
    assert bwd["kw"]["grad_alpha"] is not None and (bwd["kw"].get("grad_depth") is not None) == depth
    assert bwd["kw"]["want_color_grad"] is False      # frozen colours, no depth: the fused pair pass
    single = []
    for v, c in enumerate((cam, cam, cam2)):
        gv = dict(g, colors_precomp=cols[v])
        single.append(_hip(c, gv, dev, dLc[v], dLa[v], frozen=("colors_precomp",), depth=depth, dLd=None if dLd is None else dLd[v])[2])
    for k in ("means3D", "opacities", "scales", "rotations"):
        assert rel_err(got[k], sum(s[k].astype(np.float64) for s in single)) < TOL, k
    for v in range(3):
        assert rel_err(got["means2D"][v], single[v]["means2D"]) < TOL, v


# ---------------------------------------------------------------------------------------------------------------- defaults
def _plain(cam, g, dev, dLc, frozen, alpha_out, zero_alpha_grad=False):
    from diff_gaussian_rasterization import GaussianRasterizer
    t = {k: torch.tensor(v, device=dev, requires_grad=k not in frozen) for k, v in g.items()}
    m2 = torch.zeros((g["means3D"].shape[0], 3), device=dev, requires_grad=True)
    r = GaussianRasterizer(_settings(cam, dev), return_alpha=True) if alpha_out else GaussianRasterizer(_settings(cam, dev))
    out = r(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
            rotations=t["rotations"])
    assert len(out) == (4 if alpha_out else 3)
    loss = (out[0] * torch.tensor(dLc, device=dev)).sum()
    if zero_alpha_grad:
        loss = loss + (out[3] * 0.0).sum()
    loss.backward()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in t.items() if v.grad is not None}
    grads["means2D"] = m2.grad.detach().cpu().numpy()
    return [o.detach().cpu().numpy() for o in out[:3]], grads


@pytest.mark.parametrize("pynode", [False, True])
def test_default_unchanged(dev, monkeypatch, pynode):
    """return_alpha=False against return_alpha=True with alpha unused, and with a zero alpha gradient: outputs and every gradient bit for
    bit; the same for a batch call.  pynode: the Python node over the ctypes binding."""
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_PY_NODE", pynode)
    bwd = _spy(monkeypatch, "rasterize_backward") if pynode else None
    P, W, H = 2000, 130, 94
    g = random_gaussians(P, seed=63, scale_lo=0.02, scale_hi=0.25)
    cam = ring_camera(W, H, v=3, bg=(0.1, 0.3, 0.5))
    dLc = np.random.default_rng(64).uniform(-1, 1, (3, H, W)).astype(np.float32)
    for frozen in ((), ("colors_precomp",)):
        base = _plain(cam, g, dev, dLc, frozen, False)
        for run in (_plain(cam, g, dev, dLc, frozen, True), _plain(cam, g, dev, dLc, frozen, True, zero_alpha_grad=True)):
            for a, b in zip(run[0], base[0]):
                assert np.array_equal(a, b)
            assert set(run[1]) == set(base[1])
            for k in base[1]:
                assert np.array_equal(run[1][k], base[1][k]), k
    if pynode:
        assert "out" in bwd, "the Python node did not run the ctypes backward"
    cams = [ring_camera(W, H, v=v, V=4) for v in range(4)]
    dLcv = np.random.default_rng(65).uniform(-1, 1, (4, 3, H, W)).astype(np.float32)
    base = _views_call(cams, g, dev, dLcv, None, alpha=False)
    for run in (_views_call(cams, g, dev, dLcv, None), _views_call(cams, g, dev, dLcv, np.zeros((4, 1, H, W), np.float32))):
        for a, b in zip(run[0], base[0]):
            assert np.array_equal(a, b)
        for k in base[1]:
            assert np.array_equal(run[1][k], base[1][k]), k


def test_retain_graph_second_backward(dev):
    from diff_gaussian_rasterization import GaussianRasterizer
    P, W, H = 1500, 100, 80
    g = random_gaussians(P, seed=68)
    cam = ring_camera(W, H, v=2)
    t = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in g.items()}
    m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
    col, _, _, alpha = GaussianRasterizer(_settings(cam, dev), return_alpha=True)(
        means3D=t["means3D"], means2D=m2, opacities=t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
        rotations=t["rotations"])
    loss = col.sum() + 0.7 * (alpha * alpha).sum()
    loss.backward(retain_graph=True)
    first = {k: v.grad.clone() for k, v in t.items()}
    for v in t.values():
        v.grad = None
    loss.backward()
    for k, v in t.items():
        assert torch.equal(first[k], v.grad), k


# ---------------------------------------------------------------------------------------------------------------- edges
def test_short_alpha_gradient_is_rejected(dev):
    """Both bindings check the size of an alpha gradient before anything is launched."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _hip
    P, W, H = 300, 64, 48
    g = random_gaussians(P, seed=2)
    rs = _settings(ring_camera(W, H, v=1), dev)
    t = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    _, radii, _, state = _hip.rasterize_forward(rs, t["means3D"], t["opacities"], t["colors_precomp"], None, t["scales"], t["rotations"], None)
    gc = torch.zeros((3, H, W), device=dev)
    short = torch.zeros((1, H, W - 1), device=dev)
    with pytest.raises(ValueError, match="grad_alpha"):
        _hip.rasterize_backward(state, gc, t["means3D"], radii, t["colors_precomp"], None, t["scales"], t["rotations"], None, grad_alpha=short)
    if dgr._C is not None:
        e = t["means3D"].new_empty(0)
        D, _, _, radii2, geom, binning, image = dgr._C.rasterize_gaussians(
            rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
            rs.tanfovx, rs.tanfovy, H, W, e, 0, rs.campos, False)
        with pytest.raises(RuntimeError, match="dL_dout_alpha"):
            dgr._C.rasterize_gaussians_backward(rs.bg, t["means3D"], radii2, t["colors_precomp"], t["scales"], t["rotations"], 1.0, e,
                                                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, gc, e, 0, rs.campos, geom, D, binning,
                                                image, dL_dout_alpha=short)


def test_full_size_mask_step(dev):
    """configs[2] shape (100 k Gaussians, four 800 x 800 views), a mask loss on alpha alone: finite, deterministic gradients, exactly zero
    colour gradients, and the alpha term present in every geometry gradient."""
    P, W, H, V = 100_000, 800, 800, 4
    g = random_gaussians(P, seed=81, scale_lo=0.005, scale_hi=0.05)
    cams = [ring_camera(W, H, v=v, V=V, bg=(0.0, 0.0, 0.0)) for v in range(V)]
    from diff_gaussian_rasterization import rasterize_gaussians_views
    rs = [_settings(c, dev) for c in cams]
    target = torch.tensor(np.random.default_rng(82).uniform(0, 1, (V, 1, H, W)).astype(np.float32) > 0.5, device=dev).float()

    def step():
        t = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in g.items()}
        m2 = torch.zeros((V, P, 3), device=dev, requires_grad=True)
        im, _, _, a = rasterize_gaussians_views(rs, t["means3D"], m2, t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                                                rotations=t["rotations"], return_alpha=True)
        (a - target).abs().mean().backward()
        torch.cuda.synchronize()
        return {k: v.grad.detach().cpu().numpy() for k, v in list(t.items()) + [("means2D", m2)]}
    a, b = step(), step()
    for k in a:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), f"{k}: not deterministic"
    assert not a["colors_precomp"].any()
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        assert np.abs(a[k]).max() > 0, k
