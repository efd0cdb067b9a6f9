"""gsdyn.depth_to_cloud / voxel_down_sample / observe_state on the device (csrc/gsr_voxel.hip) against the plain-torch statement of the same
definition on CPU tensors: ``points``, ``colors``, ``counts`` and ``first`` BIT-EQUAL in every case, no tolerance anywhere -- integer sums and
an fp64 mean leave one right answer.  Shapes: the smallest at which each part of the kernels can go wrong."""
import numpy as np
import pytest
import torch

import observe_ref as O
from test_observe_cpu import tabletop

pytestmark = pytest.mark.gpu

T = torch.from_numpy
FIELDS = ("points", "colors", "counts", "first")


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64) if t.is_floating_point() else t.cpu()


def _assert_same(got, want, what=""):
    for k in FIELDS:
        if want[k] is None:
            assert got[k] is None, f"{what}: {k} should be None"
            continue
        assert got[k].is_cuda and got[k].dtype == want[k].dtype and tuple(got[k].shape) == tuple(want[k].shape), \
            f"{what}: {k} {got[k].dtype} {tuple(got[k].shape)} against {want[k].dtype} {tuple(want[k].shape)}"
        a, b = _bits(got[k]), _bits(want[k])
        if a.numel() == 0:
            continue
        bad =torch.nonzero((a != b).reshape(a.shape[0], -1).any(1))[:, 0]
        assert bad.numel() == 0, f"{what}: {k}: {bad.numel()} of {a.shape[0]} rows differ, first row {int(bad[0])}: {got[k][bad[0]].tolist()} against {want[k][bad[0]].tolist()}"


def _depth_both(dev, d, K4, R, t, bbox, colors=None, masks=None, **kw):
    import gsdyn
    dv = lambda x: None if x is None else x.to(dev)  # noqa: E731
    want = gsdyn.depth_to_cloud(d, K4, R, t, bbox, colors=colors, masks=masks, **kw)
    got = gsdyn.depth_to_cloud(dv(d), dv(K4), dv(R), dv(t), bbox, colors=dv(colors), masks=dv(masks), **kw)
    torch.cuda.synchronize()
    return got, want


def _points_both(dev, pts, voxel_size, colors=None, bounds=None):
    import gsdyn
    want = gsdyn.voxel_down_sample(pts, voxel_size, colors=colors, bounds=bounds)
    got = gsdyn.voxel_down_sample(pts.to(dev), voxel_size, colors=None if colors is None else colors.to(dev), bounds=bounds)
    torch.cuda.synchronize()
    return got, want


@pytest.mark.parametrize("hw", [(1, 1), (3, 1), (5, 63), (5, 64), (7, 65), (48, 64)])
@pytest.mark.parametrize("V", [1, 2, 4])
def test_image_shapes(dev, V, hw):
    """Different intrinsics and poses per view, NaN / inf / 0 / negative depths, masks and colours; then without masks and colours."""
    d, K4, R, t, bbox, colors, masks = O.scene(V, hw[0], hw[1], seed=100 * V + hw[1])
    for vs in (0.005, 0.03):
        got, want = _depth_both(dev, T(d), T(K4), T(R), T(t), bbox, T(colors), T(masks), depth_range=(0.1, 2.0), voxel_size=vs)
        _assert_same(got, want, f"V = {V}, {hw}, voxel {vs}")
    got, want = _depth_both(dev, T(d), T(K4), T(R), T(t), bbox, None, T(masks).to(torch.uint8) * 3, voxel_size=0.03)
    _assert_same(got, want, f"V = {V}, {hw}, uint8 masks, no colours")
    got, want = _depth_both(dev, T(d), T(K4), T(R), T(t), bbox, T(colors), None, voxel_size=0.03)
    _assert_same(got, want, f"V = {V}, {hw}, no masks")


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_all_pixels_in_one_voxel(dev, N):
    """One row of N pixels, identity pose, a focal length so long that the row spans a tenth of a voxel: one voxel, its sums crossing the lanes of
    a wave (63 / 64 / 65) and workgroups (4097).  The expected sums are Python integers."""
    g = np.random.default_rng(N)
    f32 = np.float32
    d = g.uniform(0.9005, 0.9045, (1, 1, N)).astype(f32)
    colors = g.integers(0, 256, (1, 1, N, 3), dtype=np.uint8)
    fx, cx, cy = f32(1.0e7), f32(0.25), f32(-0.5)
    K4, R, t = torch.tensor([[fx, fx, cx, cy]]), torch.eye(3)[None], torch.zeros(1, 3)
    lo = np.array([-0.001, -0.001, 0.9], f32)
    bbox = np.stack([lo, lo + f32(0.1)], 1)
    got, want = _depth_both(dev, T(d), K4, R, t, bbox, T(colors), None, voxel_size=0.005)
    _assert_same(got, want, f"N = {N}")
    # the definition by hand: numpy fp32, one operation at a time (R = I: the products with 0 and 1 and the sums with 0 are exact)
    x = np.arange(N, dtype=f32)
    w = np.stack([((x - cx) * (f32(1) / fx)) * d[0, 0], ((f32(0) - cy) * (f32(1) / fx)) * d[0, 0], d[0, 0]], 1)
    inv_h = f32(1) / f32(0.005)
    u = ((w - lo).astype(f32) * inv_h).astype(f32)
    c = np.floor(u)
    assert (c == c[0]).all()
    S = [sum(int(float(v) * 2 ** 32) for v in (u - c)[:, a]) for a in range(3)]
    h64 = 1.0 / float(inv_h)
    mean = [f32((float(c[0, a]) + float(S[a]) / (float(N) * 4294967296.0)) * h64 + float(lo[a])) for a in range(3)]
    col = [f32(float(sum(int(v) for v in colors[0, 0, :, a])) / (255.0 * N)) for a in range(3)]
    assert got["counts"].tolist() == [N] and got["first"].tolist() == [0]
    assert got["points"].cpu().numpy().tolist() == [mean] and got["colors"].cpu().numpy().tolist() == [col]


def test_every_pixel_in_its_own_voxel_and_two_views_of_one_voxel(dev):
    """The tabletop of the CPU tests: 774 pixels, 774 voxels (M = number of kept pixels); then both views at one depth: every voxel has one
    member from each view and ``first`` comes from view 0."""
    d, K4, R, t, box = tabletop()
    got, want = _depth_both(dev, d, K4, R, t, box)
    _assert_same(got, want, "own voxels")
    assert got["counts"].max().item() == 1 and got["points"].shape[0] == int((d > 0).sum())
    d[1] = d[0]
    got, want = _depth_both(dev, d, K4, R, t, box)
    _assert_same(got, want, "two views")
    assert got["counts"].tolist() == [2] * int((d[0] > 0).sum()) and int(got["first"].max()) < d[0].numel()


def test_full_table(dev):
    """A 16 x 16 x 17 lattice in a box of exactly as many cells: M = N = the cells of the box, the table (2 N rounded up) at its fullest."""
    ijk = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(17), indexing="ij"), -1).reshape(-1, 3)
    pts = T((ijk * 0.25 + 0.125).astype(np.float32))
    got, want = _points_both(dev, pts[torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(1))], 0.25, bounds=([0, 0, 0], [3.875, 3.875, 4.125]))
    _assert_same(got, want, "lattice")
    assert got["points"].shape[0] == pts.shape[0]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_keys_that_differ_in_one_axis_high_bits(dev, axis):
    pts = np.full((64, 3), 0.5, np.float32)
    pts[:, axis] = np.arange(64) * 16384.0 + 0.5                 # cells 0, 2^14, .. 63 x 2^14: bits 14 .. 19 of one 21-bit field
    pts = np.concatenate([pts, pts + np.float32(0.25)])
    hi = [1.0, 1.0, 1.0]
    hi[axis] = 2.0 ** 21 - 3
    got, want = _points_both(dev, T(pts), 1.0, bounds=([0, 0, 0], hi))
    _assert_same(got, want, f"axis {axis}")
    assert got["counts"].tolist() == [2] * 64


def test_two_clusters_a_thousand_cells_apart(dev):
    g = torch.Generator().manual_seed(7)
    a = torch.rand(3000, 3, generator=g) * 0.05
    pts = torch.cat([a, a.flip(0) + 5.0])[torch.randperm(6000, generator=g)].contiguous()
    col = torch.randint(0, 256, (6000, 3), generator=g, dtype=torch.uint8)
    got, want = _points_both(dev, pts, 0.005, colors=col, bounds=([0, 0, 0], [6, 6, 6]))
    _assert_same(got, want, "clusters")


def test_box_and_cell_faces_with_dyadic_coordinates(dev):
    """Depths and pixels that give dyadic world coordinates exactly on cell faces and on both faces of the box."""
    H, W = 9, 9
    K4, R, t = torch.tensor([[4.0, 4.0, 4.0, 4.0]]), torch.eye(3)[None], torch.tensor([[0.0, 0.0, 0.0]])
    d = torch.full((1, H, W), 1.0)                               # x, y = (pixel - 4) / 4: -1, -0.75 .. 1;  z = 1
    d[0, 0] = 2.0                                                # y = -2: outside
    box = np.array([[-1.0, 1.0], [-1.0, 1.0], [1.0, 1.0]], np.float32)      # a box of zero height: z = 1 is on both faces
    got, want = _depth_both(dev, d, K4, R, t, box, depth_range=(0.5, 3.0), voxel_size=0.5)
    _assert_same(got, want, "faces")
    assert int(got["counts"].sum()) == 8 * 9                     # rows 1 .. 8 (y = -0.75 .. 1) of nine pixels; row 0 has d = 2: x = -2 .. 2, z = 2
    assert got["points"].shape[0] == 25                          # cells -1, -0.5, 0, 0.5 and the face x = 1 (a cell of its own), squared


def test_no_survivor_and_bad_depths(dev):
    K4, R, t = torch.tensor([[50.0, 50.0, 0.0, 0.0]]), torch.eye(3)[None], torch.zeros(1, 3)
    box = np.array([[-1, 1], [-1, 1], [0, 3]], np.float32)
    bad = torch.tensor([[[float("nan"), float("inf"), 0.0, -1.0, 2.0, 2.5, -float("inf")]]])
    got, want = _depth_both(dev, bad, K4, R, t, box, torch.zeros(1, 1, 7, 3, dtype=torch.uint8))
    _assert_same(got, want, "nothing kept")
    assert got["points"].shape == (0, 3) and got["colors"].shape == (0, 3)
    bad[0, 0, 3] = 1.0
    got, want = _depth_both(dev, bad, K4, R, t, box)
    _assert_same(got, want, "one kept")
    assert got["first"].tolist() == [3]
    got, want = _depth_both(dev, torch.full((1, 4, 5), 1.0), K4, R, t, box, None, torch.zeros(1, 4, 5, dtype=torch.bool))
    _assert_same(got, want, "mask all zero")


def test_voxel_down_sample(dev):
    g = torch.Generator().manual_seed(11)
    pts = torch.rand(5000, 3, generator=g) * torch.tensor([0.5, 0.4, 0.1]) - 0.2
    pts[17] = float("nan")
    pts[4000, 2] = float("inf")
    col = torch.randint(0, 256, (5000, 3), generator=g, dtype=torch.uint8)
    for bounds in (([-0.2, -0.2, -0.2], [0.3, 0.1, -0.12]), None):
        got, want = _points_both(dev, pts, 0.01, colors=col, bounds=bounds)
        _assert_same(got, want, f"random cloud, bounds {bounds}")
    got, want = _points_both(dev, pts[:1].clone(), 0.01)
    _assert_same(got, want, "N = 1")
    assert got["counts"].tolist() == [1]
    dup = pts[100:140].repeat(50, 1)                                  # every point fifty times
    got, want = _points_both(dev, dup, 0.002, colors=col[:2000].contiguous())
    _assert_same(got, want, "duplicates")
    assert int(got["counts"].min()) >= 50


def test_two_calls_and_a_permutation(dev):
    import gsdyn
    d, K4, R, t, bbox, colors, masks = O.scene(2, 48, 64, seed=5)
    args = [T(x).to(dev) for x in (d, K4, R, t)]
    one = gsdyn.depth_to_cloud(*args, bbox, colors=T(colors).to(dev), voxel_size=0.02)
    two = gsdyn.depth_to_cloud(*args, bbox, colors=T(colors).to(dev), voxel_size=0.02)
    assert all(torch.equal(_bits(one[k]), _bits(two[k])) for k in FIELDS)
    g = torch.Generator().manual_seed(2)
    pts = (torch.rand(4000, 3, generator=g) * 0.3).to(dev)
    col = torch.randint(0, 256, (4000, 3), generator=g, dtype=torch.uint8).to(dev)
    perm = torch.randperm(4000, generator=g).to(dev)
    a = gsdyn.voxel_down_sample(pts, 0.02, colors=col, bounds=([0, 0, 0], [0.3, 0.3, 0.3]))
    b = gsdyn.voxel_down_sample(pts[perm].contiguous(), 0.02, colors=col[perm].contiguous(), bounds=([0, 0, 0], [0.3, 0.3, 0.3]))

    def rows(o):
        p = _bits(o["points"]).numpy()
        order = np.lexsort(p.T[::-1])
        return p[order], _bits(o["colors"]).numpy()[order], o["counts"].cpu().numpy()[order]
    for x, y in zip(rows(a), rows(b)):
        assert np.array_equal(x, y)


def test_who_takes_the_kernels_and_who_the_fallback(dev, monkeypatch):
    import gsdyn
    from diff_gaussian_rasterization import _hip
    from gsdyn import observe as ob
    d, K4, R, t, bbox, colors, masks = [T(x) if i != 4 else x for i, x in enumerate(O.scene(2, 5, 64, seed=1))]
    pts = torch.rand(500, 3, generator=torch.Generator().manual_seed(0))

    def refuse(*a, **k):
        raise AssertionError("the wrong path ran")
    with monkeypatch.context() as m:                                  # device tensors of the kernels' kind: the fallback must not run
        m.setattr(ob, "_voxel_torch", refuse)
        gsdyn.depth_to_cloud(d.to(dev), K4, R, t, bbox, colors=colors.to(dev), masks=masks.to(dev))
        gsdyn.voxel_down_sample(pts.to(dev), 0.05)
    with monkeypatch.context() as m:                                  # everything else: the kernels must not run
        m.setattr(_hip, "voxel_points", refuse)
        m.setattr(_hip, "voxel_depth_views", refuse)
        gsdyn.depth_to_cloud(d, K4, R, t, bbox)                                                   # CPU tensors
        gsdyn.voxel_down_sample(pts, 0.05)
        assert gsdyn.voxel_down_sample(pts.double().to(dev), 0.05)["points"].dtype == torch.float64   # fp64
        wide = torch.rand(500, 6, generator=torch.Generator().manual_seed(0)).to(dev)
        gsdyn.voxel_down_sample(wide[:, ::2], 0.05)                                               # a strided view
        gsdyn.depth_to_cloud(d.to(dev).repeat(1, 1, 2)[:, :, ::2], K4, R, t, bbox)
        big = torch.rand((1 << 24) + 1, 3, device=dev)                                            # more points than the kernels take
        out = gsdyn.voxel_down_sample(big, 0.25, bounds=([0, 0, 0], [1, 1, 1]))
        assert int(out["counts"].sum()) == (1 << 24) + 1 and out["points"].shape[0] == 64
    strided = gsdyn.voxel_down_sample(wide[:, ::2], 0.05)
    _assert_same(gsdyn.voxel_down_sample(wide[:, ::2].contiguous(), 0.05), {k: (None if v is None else v.cpu()) for k, v in strided.items()}, "strided against kernels")


def test_wrapper_validation(dev):
    from diff_gaussian_rasterization import _hip
    pts = torch.rand(10, 3, device=dev)
    lo, hi = [0, 0, 0], [1, 1, 1]
    with pytest.raises(ValueError):
        _hip.voxel_points(pts.double(), lo, hi, 10.0, 10)
    with pytest.raises(ValueError):
        _hip.voxel_points(pts[:, :2], lo, hi, 10.0, 10)
    with pytest.raises(ValueError):
        _hip.voxel_points(pts, lo, hi, 10.0, 10, colors=torch.zeros(10, 3, device=dev))
    with pytest.raises(ValueError):
        _hip.voxel_points(pts, lo, hi, 2.0 ** 22, 10)                  # too many cells
    with pytest.raises(RuntimeError):
        _hip.voxel_points(pts, lo, hi, 10.0, 5)                        # outputs smaller than min(N, cells): refused by the library, no launch
    with pytest.raises(RuntimeError):
        _hip.voxel_points(pts.cpu(), lo, hi, 10.0, 10)
    d = torch.ones(1, 2, 3, device=dev)
    K4, R, t = torch.ones(1, 4, device=dev), torch.eye(3, device=dev)[None], torch.zeros(1, 3, device=dev)
    for bad in (dict(K4=K4.cpu()), dict(R=R[0]), dict(t=t.double()), dict(masks=torch.ones(1, 2, 3, device=dev)), dict(colors=torch.zeros(1, 2, 3, 3, device=dev))):
        kw = dict(K4=K4, R=R, t=t, colors=None, masks=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            _hip.voxel_depth_views(d, kw["K4"], kw["R"], kw["t"], lo, hi, 0.0, 2.0, 10.0, 6, colors=kw["colors"], masks=kw["masks"])


def test_observe_state_on_the_device_and_into_the_planner(dev):
    import gsdyn
    from test_plan_cost_cpu import BBOX, plan_case
    d, K4, R, t, box = tabletop()
    kw = dict(nb_neighbors=25, std_ratio0=1.5, fps_radius=0.02, max_nobj=100, start_idx=3)
    cpu = gsdyn.observe_state(d, K4, R, t, box, **kw)
    gpu = gsdyn.observe_state(d.to(dev), K4.to(dev), R.to(dev), t.to(dev), box, **kw)
    torch.cuda.synchronize()
    assert torch.equal(gpu["inlier_idx"].cpu(), cpu["inlier_idx"]) and torch.equal(gpu["state_idx"].cpu(), cpu["state_idx"])
    assert torch.equal(_bits(gpu["state"]), _bits(cpu["state"])) and torch.equal(_bits(gpu["points"]), _bits(cpu["points"]))
    model, _, target, seq0, pkw = plan_case(device=dev)
    pkw.update(n_sample=8, chunk=8)
    res = gsdyn.plan_actions(model, gpu["state"], target, BBOX, seq0, **pkw)
    torch.cuda.synchronize()
    assert res["act_seq"].shape == (2, 4) and res["state_seqs"].shape == (2, gpu["state"].shape[0], 3) and bool(torch.isfinite(res["reward"]))
