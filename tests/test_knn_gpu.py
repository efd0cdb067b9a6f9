"""gsdyn.knn_points on the device against tests/knn_ref.py: indices EQUAL, squared distances BIT-EQUAL, no tolerance anywhere -- the
order (d2 ascending, index ascending) is total, so the answer is unique and depends on neither launch shape nor scheduling
(DESIGN.md section 3k).  Shapes: the smallest at which each part of csrc/gsr_knn.hip can go wrong."""
import functools

import numpy as np
import pytest
import torch

import knn_ref as R

pytestmark = pytest.mark.gpu

BRUTE_N = 2048      # csrc/gsr_knn.hip KNN_BRUTE_N: up to here every query takes the brute-force kernel, above it the grid


def _check(dev, pts, cases, rows=None, ref=None):
    """cases: (k, exclude_self) pairs, all cut from one reference of the cloud."""
    import gsdyn
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    ref = ref if ref is not None else R.KnnRef(pts, rows)
    t = torch.from_numpy(pts).to(dev)
    for k, ex in cases:
        idx, d2 = gsdyn.knn_points(t, k, exclude_self=ex)
        assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(idx.shape) == (pts.shape[0], k) == tuple(d2.shape)
        ri, rd = ref.top(k, ex)
        gi, gd = idx.cpu().numpy()[ref.rows], d2.cpu().numpy()[ref.rows]
        bad = np.nonzero((gi != ri).any(1) | (R.bits(gd) != R.bits(rd)).any(1))[0]
        assert bad.size == 0, f"k = {k}, exclude_self = {ex}: {bad.size} of {len(ref.rows)} rows differ, first row {ref.rows[bad[0]]}: " \
                              f"{gi[bad[0]]} / {gd[bad[0]]} against {ri[bad[0]]} / {rd[bad[0]]}"


@functools.lru_cache(maxsize=None)
def _uniform_ref(n):
    pts = np.random.default_rng(1000 + n).uniform(0, 1, (n, 3)).astype(np.float32)
    return pts, R.KnnRef(pts)


# wave edges (63 / 64 / 65), workgroup edges (257), k = N (64 of 64) and k = N - 1 (1 of 2, 64 of 65), the grid path (4099)
UNIFORM_CASES = [(n, k, ex) for n in (1, 2, 63, 64, 65, 257, 1000, 4099) for k in (1, 20, 21, 50, 64) for ex in (False, True) if k <= n - (1 if ex else 0)]


@pytest.mark.parametrize("n,k,exclude_self", UNIFORM_CASES)
def test_uniform_cube(dev, n, k, exclude_self):
    pts, ref = _uniform_ref(n)
    _check(dev, pts, [(k, exclude_self)], ref=ref)


@pytest.mark.parametrize("n", [BRUTE_N, BRUTE_N + 1])
def test_both_sides_of_the_brute_force_bound(dev, n):
    pts = np.random.default_rng(n).uniform(-1, 1, (n, 3)).astype(np.float32)
    _check(dev, pts, [(21, True), (50, False), (1, False), (64, True)])


# ---- the bound and its slack
def test_lattice_with_a_shuffled_copy(dev):
    """16^3 integer lattice + a shuffled copy: every distance is an exact integer, ties at every rank and across every cell face, every
    point has a duplicate.  The index order decides everywhere; a search that stopped at `<=` instead of `<` would miss ties."""
    a = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    b = a.copy()
    np.random.default_rng(5).shuffle(b)
    pts = np.concatenate([a, b])
    _check(dev, pts, [(21, True), (50, False), (7, True), (64, False)], rows=np.arange(0, pts.shape[0], 3))


def test_fine_cloud_at_a_large_offset(dev):
    """Spacing 1e-3 around (1000, -1000, 1000): an fp32 ulp there is 6e-5, the cell arithmetic rounds, coordinates collide.  A bound that
    trusts "p lies in cell c" exactly is not conservative here."""
    g = np.random.default_rng(11)
    lat = np.stack(np.meshgrid(*[np.arange(15)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    pts = (np.array([1000.0, -1000.0, 1000.0]) + 1e-3 * (lat + g.uniform(-0.3, 0.3, lat.shape))).astype(np.float32)
    _check(dev, pts, [(21, True), (50, False), (1, True)])


def test_sheet(dev):
    pts = np.random.default_rng(12).uniform(0, 1, (3000, 3)).astype(np.float32)
    pts[:, 2] = 0.25
    _check(dev, pts, [(21, True), (50, False)])


def test_line(dev):
    pts = np.full((3000, 3), 0.5, dtype=np.float32)
    pts[:, 0] = np.random.default_rng(13).uniform(-2, 2, 3000).astype(np.float32)
    _check(dev, pts, [(21, True), (50, False)])


@pytest.mark.parametrize("n", [500, 3000])     # the brute-force kernel; the grid with zero extent on all three axes (one cell)
def test_identical_points(dev, n):
    pts = np.tile(np.array([[0.3, -1.5, 2.0]], dtype=np.float32), (n, 1))
    _check(dev, pts, [(21, True), (50, False), (64, True)])


# ---- the shells and the brute-force pass
def _tabletop(n, seed):
    g = np.random.default_rng(seed)
    n_out = max(1, n // 100)
    a = g.uniform(0, 1, (n - n_out, 3)).astype(np.float32) * np.array((0.5, 0.5, 0.02), dtype=np.float32)
    b = g.uniform(-3, 3, (n_out, 3)).astype(np.float32)
    pts = np.concatenate([a, b])
    perm = g.permutation(n)
    return pts[perm], np.nonzero(perm >= n - n_out)[0]


def test_tabletop_with_far_outliers(dev):
    pts, _ = _tabletop(4099, 21)
    _check(dev, pts, [(21, True), (50, False)])


@pytest.mark.parametrize("gap", [100.0, 1.0e5])
def test_two_clusters_far_apart(dev, gap):
    """The box is almost empty: at gap 100 the grid has tens of thousands of cells per axis, at 1e5 the clamp to 2^20 cells per axis makes
    a cell larger than a cluster."""
    g = np.random.default_rng(22)
    pts = (g.normal(0, 0.01, (3000, 3)) + np.where(np.arange(3000)[:, None] % 2 == 0, 0.0, gap)).astype(np.float32)
    _check(dev, pts, [(21, True), (50, False)])


def test_larger_cloud_on_sampled_rows(dev):
    """N = 20 011: every 37th row plus every outlier's row (the rows the brute-force pass finishes); the reference covers those rows only."""
    pts, out_rows = _tabletop(20011, 23)
    rows = np.union1d(np.arange(0, 20011, 37), out_rows)
    assert np.isin(out_rows, rows).all() and out_rows.size == 200
    _check(dev, pts, [(21, True), (50, False)], rows=rows)


# ---- further properties
def test_two_calls_give_the_same_bits(dev):
    import gsdyn
    pts, _ = _tabletop(4099, 31)
    t = torch.from_numpy(pts).to(dev)
    a = gsdyn.knn_points(t, 21, exclude_self=True)
    b = gsdyn.knn_points(t, 21, exclude_self=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_a_permutation_gives_the_permuted_answer(dev):
    import gsdyn
    pts = np.random.default_rng(32).uniform(0, 1, (4099, 3)).astype(np.float32)
    ref = R.KnnRef(pts)
    d = ref.top(22, False)[1]
    assert (d[:, 1:] != d[:, :-1]).all(), "the cloud must be free of ties among each row's first 22"
    perm = np.random.default_rng(33).permutation(4099)
    i0, d0 = gsdyn.knn_points(torch.from_numpy(pts).to(dev), 21, exclude_self=True)
    i1, d1 = gsdyn.knn_points(torch.from_numpy(pts[perm]).to(dev), 21, exclude_self=True)       # row r of the permuted cloud is point perm[r]
    assert np.array_equal(perm[i1.cpu().numpy()], i0.cpu().numpy()[perm])
    assert np.array_equal(R.bits(d1.cpu().numpy()), R.bits(d0.cpu().numpy()[perm]))


def _rigidity_params(device):
    from gsdyn import synth_scene_params
    params = {k: v.detach() for k, v in synth_scene_params(3000, seed=3, device="cpu").items()}
    return {k: v.to(device) for k, v in params.items()}


def test_rigidity_variables_on_the_device_equal_the_cpu_call(dev):
    from gsdyn.step import make_rigidity_variables
    a = make_rigidity_variables(_rigidity_params(dev), num_knn=20, knn="grid")
    b = make_rigidity_variables(_rigidity_params("cpu"), num_knn=20, knn="grid")
    assert a["neighbor_indices"].shape[0] > BRUTE_N, "the scene must reach the grid path"
    for key in ("neighbor_indices", "rev_ptr", "rev_edge", "prev_offset"):
        assert torch.equal(a[key].cpu(), b[key]), key
    # the same d2 bits go into torch.sqrt and torch.exp on either side: correctly rounded on the host, within an ulp or two on the device,
    # which also flushes a subnormal weight (below 2^-126) to zero
    np.testing.assert_allclose(a["neighbor_dist"].cpu().numpy(), b["neighbor_dist"].numpy(), rtol=4 * 2.0 ** -24, atol=0)
    np.testing.assert_allclose(a["neighbor_weight"].cpu().numpy(), b["neighbor_weight"].numpy(), rtol=1e-6, atol=2.0 ** -126)


@pytest.mark.parametrize("seed", [1, 3])
def test_outlier_filter_on_the_device_equals_the_cpu_call(dev, seed):
    from gsdyn.dynamics import remove_statistical_outliers
    x = torch.from_numpy(R.tabletop_cloud(seed))
    keep64, passes, margin = R.outlier_loop_fp64(x.numpy())
    assert margin >= 2.9e-4 and passes == 6
    a = remove_statistical_outliers(x.to(dev), knn="grid")
    b = remove_statistical_outliers(x, knn="grid")
    assert torch.equal(a.cpu(), b) and np.array_equal(b.numpy(), keep64)


def test_predict_episode_grid_outlier_filter_picks_the_same_inliers(dev, monkeypatch):
    """predict_episode(outlier_knn="grid") on the small scene of tests/test_predict_shard_cpu.py: the filter is asked for the grid search and
    hands the rollout the inliers of the dense one."""
    from test_predict_shard_cpu import CAMS, H, ROLL, W, _episode_inputs
    import gsdyn.dynamics as D
    from gsdyn.predict import predict_episode, ring_poses
    model, params, eef = _episode_inputs()
    model = model.to(dev)
    params = {k: v.to(dev) for k, v in params.items()}
    seen = []
    real = D.remove_statistical_outliers

    def spy(xyz, *a, **kw):
        keep = real(xyz, *a, **kw)
        seen.append((kw.get("knn", "dense"), keep.cpu().clone()))
        return keep
    monkeypatch.setattr(D, "remove_statistical_outliers", spy)
    for mode in ("dense", "grid"):
        _, vis, tm = predict_episode(model, params, eef.to(dev), ring_poses(CAMS, W, H), W, H, rollout_cfg=ROLL, rank=0, world=1, outlier_knn=mode)
        assert len(vis) == eef.shape[0]
    assert [m for m, _ in seen] == ["dense", "grid"]
    assert torch.equal(seen[0][1], seen[1][1]) and 0 < seen[0][1].numel() <= params["means3D"].shape[0]
