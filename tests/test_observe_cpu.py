"""gsdyn.voxel_down_sample / depth_to_cloud / observe_state without a GPU: the plain-torch statement of the definition (gsdyn/observe.py,
DESIGN.md section 3l) against the fp64 referee tests/observe_ref.py, its order and exactness properties, and its edges."""
import functools

import numpy as np
import pytest
import torch

import observe_ref as O

T = torch.from_numpy
EPS = 2.0 ** -24
RANGE = (0.1, 2.0)


@functools.lru_cache(maxsize=None)
def _proto():
    """The prototype input of the definition: V = 4, a 45 x 67 image; the fp64 world points once, for every test that needs them."""
    s = O.scene(4, 45, 67, seed=0)
    return s, O.world64(*s[:4])


def _cloud(s, voxel_size, **kw):
    import gsdyn
    d, K4, R, t, bbox, colors, masks = s
    return gsdyn.depth_to_cloud(T(d), T(K4), T(R), T(t), bbox, colors=T(colors), masks=T(masks), depth_range=RANGE, voxel_size=voxel_size, **kw)


def _members(s, voxel_size):
    """Per pixel: kept?, and the fallback's cell key -- from the module's own unprojection and the definition's fp32 cell expression; tied to the
    fallback's OUTPUT by the caller (first and counts of every voxel must agree)."""
    from gsdyn import observe as ob
    d, K4, R, t, bbox, colors, masks = s
    w = ob._world_torch(T(d), T(K4), T(R), T(t)).reshape(-1, 3).numpy()
    lo, hi = bbox[:, 0], bbox[:, 1]
    dd = d.reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = (dd > np.float32(RANGE[0])) & (dd < np.float32(RANGE[1])) & masks.reshape(-1) & ((w >= lo) & (w <= hi)).all(1)
        inv_h = np.float32(1.0) / np.float32(voxel_size)
        u = ((w - lo).astype(np.float32) * inv_h).astype(np.float32)
    c = np.floor(np.where(keep[:, None], u, 0)).astype(np.int64)
    return keep, (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], c, inv_h


@pytest.mark.parametrize("voxel_size", [0.005, 0.02])
def test_fp64_referee(voxel_size):
    """Voxel means of the fallback against the fp64 mean of the same members' fp64 world points (membership: the fallback's own, checked
    against its output's ``first`` and ``counts``, so no voxel is left out).

    The bound, from the roundings of the definition, with e = 2^-24, A = the largest of |coordinate|, |t| and the box extent:
      * xc = ((x - cx) * (1/fx)) * d is four roundings, 4 e |xc|; yc alike; zc = d is exact.
      * a = R[i,0] xc and b = R[i,1] yc carry 5 e each, c = R[i,2] d carries e; the three sums (a + b), (.. + c), (.. + t) add
        e |a + b|, e |a + b + c|, e |w|:  |dw| <= e (7 (|a| + |b|) + 2 |c| + |w|).
        A row of a rotation has norm 1, so |a| + |b| <= |p| and |c| <= |p| with p the camera-frame point, |p| = |w - t| <= 2 sqrt(3) A:
        |dw| <= e A (18 sqrt(3) + 1).
      * u = fl(fl(w - lo) * inv_h) is two roundings of a length <= A: 2 e A once mapped back through the EXACT 1 / inv_h (the rounding of
        inv_h itself cancels); f = u - c and q = int64(f 2^32) are exact (cell 0 truncates below h 2^-32); the integer mean is exact;
        a mean of members lies no further from the mean of their fp64 points than the worst member.
      * the final rounding to fp32 is e A; the fp64 evaluation and the referee's own roundings are below 2^-50 A.
    Total: (18 sqrt(3) + 4) e A + h 2^-32, times (1 + 2^-20) for the second-order terms.  The assertion is this bound, no fitted number; the
    measured worst ratio goes to profiles/observe_parity.txt."""
    s, w64 = _proto()
    out = _cloud(s, voxel_size)
    keep, key, _, _ = _members(s, voxel_size)
    idx = np.nonzero(keep)[0]
    uniq, inv = np.unique(key[idx], return_inverse=True)
    M = uniq.size
    first = np.full(M, key.size, np.int64)
    np.minimum.at(first, inv, idx)
    cnt = np.bincount(inv, minlength=M)
    order = np.argsort(first)
    assert np.array_equal(first[order], out["first"].numpy()) and np.array_equal(cnt[order], out["counts"].numpy())
    mean64 = np.stack([np.bincount(inv, weights=w64.reshape(-1, 3)[idx, a], minlength=M) for a in range(3)], 1)[order] / cnt[order][:, None]
    got = out["points"].numpy().astype(np.float64)
    A = max(np.abs(mean64).max(), np.abs(s[3]).max(), float((s[4][:, 1] - s[4][:, 0]).max()))
    bound = ((18 * np.sqrt(3) + 4) * EPS * A + voxel_size * 2.0 ** -32) * (1 + 2.0 ** -20)
    err = np.abs(got - mean64).max()
    print(f"observe parity: voxel {voxel_size}: M = {M}, kept {idx.size}, max |mean - fp64 mean| = {err:.3e} = {err / (EPS * A):.2f} x 2^-24 A "
          f"(A = {A:.3f}), bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound
    c64 = np.stack([np.bincount(inv, weights=s[5].reshape(-1, 3)[idx, a].astype(np.float64), minlength=M) for a in range(3)], 1)[order] / (255.0 * cnt[order][:, None])
    assert np.array_equal(out["colors"].numpy(), c64.astype(np.float32))      # one fp64 quotient, rounded once: the same number


@pytest.mark.parametrize("voxel_size", [0.005, 0.02])
def test_membership_against_fp64_floor(voxel_size):
    s, w64 = _proto()
    keep, _, c, inv_h = _members(s, voxel_size)
    idx = np.nonzero(keep)[0]
    u64 = (w64.reshape(-1, 3)[idx] - s[4][:, 0].astype(np.float64)) * float(inv_h)
    frac = u64 - np.floor(u64)
    near = ((frac < 2.0 ** -10) | (frac > 1 - 2.0 ** -10)).any(1)
    print(f"observe membership: voxel {voxel_size}: {near.sum()} of {idx.size} kept pixels within 2^-10 of a cell face ({100 * near.mean():.2f} %)")
    assert near.mean() <= 0.02
    assert np.array_equal(c[idx][~near], np.floor(u64[~near]).astype(np.int64))


def _sorted_rows(out):
    """Rows sorted by the mean's bits: a canonical order for comparing two results as sets."""
    p = out["points"].numpy()
    o = np.lexsort(O.bits(p).T[::-1])
    return [O.bits(p)[o], out["counts"].numpy()[o]] + ([O.bits(out["colors"].numpy())[o]] if out["colors"] is not None else [])


def test_order_counts_and_permutation():
    import gsdyn
    s, _ = _proto()
    out = _cloud(s, 0.02)
    keep, _, _, _ = _members(s, 0.02)
    f = out["first"].numpy()
    assert (np.diff(f) > 0).all() and keep[f].all()
    assert int(out["counts"].sum()) == int(keep.sum())
    assert out["points"].dtype == torch.float32 and out["colors"].dtype == torch.float32 and out["counts"].dtype == torch.int32 and out["first"].dtype == torch.int64
    again = _cloud(s, 0.02)
    assert all(torch.equal(out[k], again[k]) for k in out)
    # the same points through voxel_down_sample, in the module's own fp32 world coordinates, shuffled
    from gsdyn import observe as ob
    w = ob._world_torch(T(s[0]), T(s[1]), T(s[2]), T(s[3])).reshape(-1, 3)[T(keep)]
    col = T(s[5]).reshape(-1, 3)[T(keep)]
    bounds = (s[4][:, 0], s[4][:, 1])
    a = gsdyn.voxel_down_sample(w, 0.02, colors=col, bounds=bounds)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(w.shape[0]))
    b = gsdyn.voxel_down_sample(w[perm].contiguous(), 0.02, colors=col[perm].contiguous(), bounds=bounds)
    for x, y, z in zip(_sorted_rows(out), _sorted_rows(a), _sorted_rows(b)):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert (np.diff(b["first"].numpy()) > 0).all()


def test_dyadic_faces_land_where_the_definition_says():
    """h = 1/4, box [0, 2]^3: points on a cell face belong to the upper cell, both box faces are inside, the means are exact."""
    import gsdyn
    pts = torch.tensor([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.125, 0.0, 0.0], [2.0, 2.0, 2.0], [1.875, 2.0, 2.0], [0.5, 0.75, 1.0], [0.625, 0.875, 1.125],
                        [2.0000002, 0.0, 0.0], [-1e-9, 0.0, 0.0], [0.2499999, 0.0, 0.0]], dtype=torch.float32)
    out = gsdyn.voxel_down_sample(pts, 0.25, bounds=([0, 0, 0], [2, 2, 2]))
    assert out["first"].tolist() == [0, 1, 3, 4, 5]
    assert out["counts"].tolist() == [3, 1, 1, 1, 2]
    m = (np.float64(0.0) + np.float64(0.125) + np.float64(np.float32(0.2499999))) / 3
    want = np.array([[m, 0, 0], [0.25, 0, 0], [2, 2, 2], [1.875, 2, 2], [0.5625, 0.8125, 1.0625]])
    assert np.array_equal(out["points"].numpy(), want.astype(np.float32))
    # exact integer sums: q of every member, by hand
    q = [int(u * 2 ** 32) for u in (0.0, 0.5, float(np.float32(np.float32(0.2499999) * np.float32(4.0))))]      # u = w * inv_h, all in cell 0
    assert np.float32((0 + sum(q) / (3 * 2 ** 32)) * 0.25 + 0.0) == out["points"][0, 0].item()
    out64 = gsdyn.voxel_down_sample(pts.double(), 0.25, bounds=([0, 0, 0], [2, 2, 2]))
    assert out64["points"].dtype == torch.float64 and out64["first"].tolist() == [0, 1, 3, 4, 5]


def test_edges_of_the_images():
    import gsdyn
    K4, R, t = torch.tensor([[50.0, 50.0, 0.0, 0.0]]), torch.eye(3)[None], torch.zeros(1, 3)
    box = np.array([[-1, 1], [-1, 1], [0, 3]], np.float32)
    one = gsdyn.depth_to_cloud(torch.full((1, 1, 1), 1.5), K4, R, t, box)                     # one pixel
    assert one["points"].tolist() == [[0.0, 0.0, 1.5]] and one["counts"].tolist() == [1] and one["first"].tolist() == [0] and one["colors"] is None
    bad = torch.tensor([[[float("nan"), float("inf"), 0.0, -1.0, 2.0, 2.5]]])                # NaN, inf, 0, negative, the open upper bound, beyond
    none = gsdyn.depth_to_cloud(bad, K4, R, t, box, colors=torch.zeros(1, 1, 6, 3, dtype=torch.uint8))
    assert none["points"].shape == (0, 3) and none["colors"].shape == (0, 3) and none["counts"].shape == (0,) and none["first"].shape == (0,)
    assert none["counts"].dtype == torch.int32 and none["first"].dtype == torch.int64
    d = torch.full((1, 2, 3), 1.0)
    assert gsdyn.depth_to_cloud(d, K4, R, t, box, masks=torch.zeros(1, 2, 3, dtype=torch.bool))["points"].shape == (0, 3)
    m = torch.zeros(1, 2, 3, dtype=torch.uint8)
    m[0, 1, 2] = 7
    assert gsdyn.depth_to_cloud(d, K4, R, t, box, masks=m)["first"].tolist() == [5]
    K33 = torch.tensor([[[50.0, 0.0, 0.0], [0.0, 50.0, 0.0], [0.0, 0.0, 1.0]]])
    assert torch.equal(gsdyn.depth_to_cloud(d, K33, R, t, box)["points"], gsdyn.depth_to_cloud(d, K4, R, t, torch.from_numpy(box))["points"])
    K33[0, 0, 1] = 0.5
    with pytest.raises(ValueError):
        gsdyn.depth_to_cloud(d, K33, R, t, box)                                               # skew
    with pytest.raises(ValueError):
        gsdyn.depth_to_cloud(d, K4, R, t, box, voxel_size=2.0 / (2 ** 21 - 2))                # z spans 3 / h = 3.1 M cells: more than 2^21 - 2
    assert gsdyn.depth_to_cloud(d, K4, R, t, box, voxel_size=3.0 / (2 ** 21 - 2.5))["counts"].sum() == 6
    for wrong in (dict(depths=d.double()), dict(depths=d[0]), dict(K=K4[:, :3]), dict(R=R[0]), dict(t=t[0]), dict(bbox=box[:2]),
                  dict(colors=torch.zeros(1, 2, 3, 3)), dict(colors=torch.zeros(1, 2, 3, dtype=torch.uint8)), dict(masks=torch.zeros(1, 2, 3)),
                  dict(masks=torch.zeros(2, 3, dtype=torch.bool)), dict(voxel_size=0.0), dict(voxel_size=float("nan"))):
        args = dict(depths=d, K=K4, R=R, t=t, bbox=box)
        args.update(wrong)
        with pytest.raises(ValueError):
            gsdyn.depth_to_cloud(args.pop("depths"), args.pop("K"), args.pop("R"), args.pop("t"), args.pop("bbox"), **args)


def test_edges_of_the_points():
    import gsdyn
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(300, 3, generator=g)
    pts[5] = float("nan")
    pts[9, 1] = float("inf")
    auto = gsdyn.voxel_down_sample(pts, 0.1)                                                  # bounds=None: min / max of the finite rows
    fin = torch.isfinite(pts).all(1)
    given = gsdyn.voxel_down_sample(pts, 0.1, bounds=(pts[fin].amin(0), pts[fin].amax(0)))
    assert all(torch.equal(auto[k], given[k]) for k in ("points", "counts", "first")) and int(auto["counts"].sum()) == 298
    assert gsdyn.voxel_down_sample(torch.full((4, 3), float("nan")), 0.1)["points"].shape == (0, 3)
    assert gsdyn.voxel_down_sample(torch.zeros(0, 3), 0.1)["first"].shape == (0,)
    view = torch.rand(50, 6, generator=g)[:, ::2]                                             # a strided view
    assert torch.equal(gsdyn.voxel_down_sample(view, 0.2)["points"], gsdyn.voxel_down_sample(view.contiguous(), 0.2)["points"])
    for wrong in (dict(points=pts.half()), dict(points=pts[:, :2]), dict(points=pts[0]), dict(colors=torch.zeros(300, 3)), dict(colors=torch.zeros(299, 3, dtype=torch.uint8)),
                  dict(bounds=([0, 0, 0], [1, 1, float("inf")])), dict(bounds=([0, 0, 1], [1, 1, 0])), dict(voxel_size=-1.0), dict(voxel_size=1e-8)):
        args = dict(points=pts, voxel_size=0.1)
        args.update(wrong)
        with pytest.raises(ValueError):
            gsdyn.voxel_down_sample(args.pop("points"), args.pop("voxel_size"), **args)


def tabletop(dev="cpu"):
    """Two views straight down on a slab of 24 x 16 x 2 points (1 cm apart, centred in their 5 mm voxels) plus six far outliers inside the box."""
    H, W, f = 22, 24, 100.0
    K4 = torch.tensor([[f, f, 11.5, 7.5], [f, f, 11.5, 7.5]])
    R = torch.tensor([[[1.0, 0, 0], [0, -1, 0], [0, 0, -1]]] * 2)
    t = torch.tensor([[0.0, 0, 1.0], [0.0, 0, 1.0]])
    d = torch.zeros(2, H, W)
    d[0, :16], d[1, :16] = 0.9975, 0.9875                         # z = 0.0025 and 0.0125: x, y = (pixel - c) / f * d
    d[0, 18, 2], d[0, 19, 20], d[1, 18, 7], d[1, 20, 13], d[0, 21, 23], d[1, 21, 0] = 0.8, 0.75, 0.7, 0.85, 0.72, 0.78
    box = np.array([[-0.3, 0.3], [-0.3, 0.3], [0.0, 0.4]], np.float32)
    return d.to(dev), K4.to(dev), R.to(dev), t.to(dev), box


def test_observe_state_on_a_tabletop():
    import gsdyn
    d, K4, R, t, box = tabletop()
    out = gsdyn.observe_state(d, K4, R, t, box, nb_neighbors=25, std_ratio0=1.5, fps_radius=0.02, max_nobj=100, start_idx=0)
    pts, state, inl = out["points"], out["state"], out["inlier_idx"]
    assert pts.shape == (2 * 16 * 24 + 6, 3) and out["colors"] is None
    assert 1 <= state.shape[0] <= 100 and state.shape[1] == 3 and torch.equal(state, pts[out["state_idx"]])
    assert 2 * inl.numel() > 2 * 16 * 24 and bool((pts[inl][:, 2] < 0.02).all())       # the six outliers (z >= 0.15) are gone, most of the slab stays
    assert float(torch.cdist(pts[inl], state).min(1).values.max()) <= 0.02
    B, Tn = 3, 2
    seqs = state[None, None].expand(B, Tn, -1, -1).contiguous()
    cost = gsdyn.running_cost(seqs, torch.zeros(B, Tn, 4), state, state + 0.01, box)
    assert cost["reward_seqs"].shape == (B,) and bool(torch.isfinite(cost["reward_seqs"]).all())


def test_scratch_size_is_a_host_only_function():
    """gsr_voxel_scratch_bytes: O(min(N, cells)), 0 for arguments the calls reject (no GPU needed)."""
    import ctypes as C
    from diff_gaussian_rasterization import _hip
    lib = _hip.load_library()
    f3 = lambda *a: (C.c_float * 3)(*a)  # noqa: E731
    small = lib.gsr_voxel_scratch_bytes(1 << 24, f3(0, 0, 0), f3(0.01, 0.01, 0.01), 200.0)      # 27 cells: the table stays at its minimum
    big = lib.gsr_voxel_scratch_bytes(1 << 24, f3(0, 0, 0), f3(1, 1, 1), 1000.0)
    assert 0 < small < (1 << 24) * 4 + (1 << 20) < big < (1 << 25) * 56 + (1 << 24) * 4 + (1 << 20)
    assert lib.gsr_voxel_scratch_bytes((1 << 24) + 1, f3(0, 0, 0), f3(1, 1, 1), 200.0) == 0
    assert lib.gsr_voxel_scratch_bytes(100, f3(0, 0, 0), f3(1, 1, 1), 2.0 ** 21) == 0
    assert lib.gsr_voxel_scratch_bytes(100, f3(0, 0, 1), f3(1, 1, 0), 200.0) == 0
