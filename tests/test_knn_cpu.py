"""CPU tests of the exact k-nearest-neighbour search (gsdyn/knn.py, csrc/gsr_knn.hip): the exported symbols and their
argument checks, the plain-torch fallback -- the definition -- against tests/knn_ref.py bit for bit, and the two callers' ``knn="grid"``
switch against their dense form and against fp64."""
import os
import re

import numpy as np
import pytest
import torch

import knn_ref as R

SYMBOLS = ("gsr_knn_scratch_bytes", "gsr_knn")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared_and_the_abi_is_125():
    from diff_gaussian_rasterization import _hip
    import ctypes
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
        assert re.search(r"^(int|size_t) " + s + r"\(", header, re.M), s
    assert re.search(r"#define GSR_VERSION 125\b", header)
    lib = ctypes.CDLL(_hip.LIB_PATH)              # dlopen works without a GPU
    assert lib.gsr_version() == 125
    for s in SYMBOLS:
        getattr(lib, s)
    lib = _hip.load_library()
    sizes = [int(lib.gsr_knn_scratch_bytes(n)) for n in (1, 1000, 70_000, 500_000)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[3] <= 100 * 500_000               # O(N): below 100 bytes per point


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """N < 1, k < 1, k > 64, k > N - (exclude_self ? 1 : 0) and a NULL pointer come back as -2 with a text, before anything is launched.  Every
    pointer is a real buffer large enough for the refused call (on the device where there is one), so a check that regressed would launch
    on valid memory."""
    from diff_gaussian_rasterization import _hip
    import ctypes as C
    lib = _hip.load_library()
    where = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    N, K = 100, 65
    pts = torch.zeros(N * 3, dtype=torch.float32, device=where)
    scratch = torch.zeros(int(lib.gsr_knn_scratch_bytes(N)) + 256, dtype=torch.uint8, device=where)
    idx = torch.zeros(N * K, dtype=torch.int64, device=where)
    d2 = torch.zeros(N * K, dtype=torch.float32, device=where)
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda n, k, ex, a=p(pts), s=C.c_void_p(sp), i=p(idx), d=p(d2): lib.gsr_knn(n, a, k, ex, s, i, d, None)  # noqa: E731
    for n, k, ex in ((0, 1, 0), (-3, 1, 0), (N, 0, 0), (N, -1, 0), (N, 65, 0), (64, 64, 1), (20, 21, 0), (1, 1, 1)):
        assert call(n, k, ex) == -2, (n, k, ex)
        msg = lib.gsr_last_error()
        assert b"gsr_knn: bad argument" in msg and f"N = {n}, k = {k}, exclude_self = {ex}".encode() in msg, msg
    for null in ("a", "s", "i", "d"):
        assert call(N, 20, 1, **{null: None}) == -2 and b"gsr_knn: NULL pointer" in lib.gsr_last_error(), null
    if where.type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the fallback is the definition
def _equal(pts, k, exclude_self, **kw):
    from gsdyn import knn_points
    idx, d2 = knn_points(torch.from_numpy(pts), k, exclude_self=exclude_self)
    ri, rd = R.knn_ref(pts, k, exclude_self, **kw)
    assert idx.dtype == torch.int64 and d2.dtype == torch.from_numpy(pts).dtype and tuple(idx.shape) == (pts.shape[0], k)
    assert np.array_equal(idx.numpy(), ri), (k, exclude_self)
    assert np.array_equal(R.bits(d2.numpy()), R.bits(rd)), (k, exclude_self)


def _lattice(n):
    return np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def test_fallback_equals_the_reference_bit_for_bit():
    g = np.random.default_rng(0)
    uni = g.uniform(0, 1, (700, 3)).astype(np.float32)
    for k, ex in ((1, False), (21, True), (50, False), (64, True)):
        _equal(uni, k, ex)
    lat = _lattice(9)                                   # exact ties at every rank: the index order decides
    for k, ex in ((7, True), (21, True), (50, False)):
        _equal(lat, k, ex)
    dup = np.concatenate([uni[:200], uni[:200][g.permutation(200)], uni[:50]])     # every point two or three times
    for k, ex in ((1, True), (3, False), (21, True)):
        _equal(dup, k, ex)
    i1, _ = __import__("gsdyn").knn_points(torch.from_numpy(dup), 1, exclude_self=True)
    assert int(i1[400, 0]) == 0 and int(i1[0, 0]) != 0  # a duplicate of lower index IS the first neighbour; the point itself never is
    _equal(uni[:1], 1, False)                           # N = 1, k = 1
    _equal(uni[:40], 40, False)                         # k = N
    _equal(uni[:40], 39, True)                          # k = N - 1
    _equal(uni.astype(np.float64), 21, True)            # fp64: the same definition in the tensor's dtype
    _equal(uni, 65, False)                              # k = 65: beyond the kernel's list, the fallback only
    _equal(uni, 65, True)


def test_fallback_chunks_rows_without_changing_a_row(monkeypatch):
    from gsdyn import knn as K
    pts = torch.from_numpy(np.random.default_rng(1).uniform(0, 1, (5000, 3)).astype(np.float32))   # 5000 > 2^22 / 5000: several chunks
    whole = K.knn_points(pts, 21, exclude_self=True)
    rows = np.arange(0, 5000, 97)
    ri, rd = R.knn_ref(pts.numpy(), 21, True, rows=rows)
    assert np.array_equal(whole[0].numpy()[rows], ri) and np.array_equal(R.bits(whole[1].numpy()[rows]), R.bits(rd))


def test_knn_points_refuses_what_has_no_answer():
    from gsdyn import knn_points
    pts = torch.zeros(10, 3)
    for bad in (dict(k=0), dict(k=11), dict(k=10, exclude_self=True)):
        with pytest.raises(ValueError):
            knn_points(pts, **bad)
    with pytest.raises(ValueError):
        knn_points(torch.zeros(10, 2), 1)


# ------------------------------------------------------------------------------------------ the two callers
def _rigidity_params(P):
    from gsdyn import synth_scene_params
    return {k: v.detach() for k, v in synth_scene_params(P, seed=3, device="cpu").items()}


# cdist takes its matrix-product form (|a|^2 + |b|^2 - 2 a.b) from 26 rows on: its d2 carries an absolute error of about 2^-24 (|a|^2 + |b|^2),
# i.e. a relative error of about 2^-24 |p|^2 / d^2 in the distance.  The 1e-5 agreement between the two paths can therefore be asked only where
# d >~ 0.08 |p|: the 150-Gaussian scene (about 100 foreground points in the unit cube, nearest neighbours 0.1 apart).  At 3000 Gaussians the
# nearest neighbours are 0.011 apart and the dense path itself is 4.8e-4 away from fp64 (the grid path: 1.3e-7); there the lists must agree and
# the grid path must be the closer one.
@pytest.mark.parametrize("P,agree_1e5", [(150, True), (3000, False)])
def test_rigidity_variables_grid_equals_dense_and_is_closer_to_fp64(P, agree_1e5):
    from gsdyn.step import make_rigidity_variables
    params = _rigidity_params(P)
    dense = make_rigidity_variables(params, num_knn=20)
    grid = make_rigidity_variables(params, num_knn=20, knn="grid")
    assert set(dense) == set(grid)
    fg = params["means3D"][params["seg_colors"][:, 0] > 0.5]
    d = R.KnnRef(fg.numpy()).top(22, False)[1]
    assert (d[:, 1:] != d[:, :-1]).all(), "the scene must be free of ties among each row's first 22"
    for key in ("neighbor_indices", "rev_ptr", "rev_edge", "fg_idx", "bg_idx", "prev_offset"):
        assert torch.equal(dense[key], grid[key]), key
    nbr = grid["neighbor_indices"]
    assert tuple(nbr.shape) == (fg.shape[0], 20) and nbr.dtype == torch.int64
    exact = (fg.double()[nbr] - fg.double()[:, None]).norm(dim=-1)
    err_d = ((dense["neighbor_dist"].double() - exact).abs() / exact).max().item()
    err_g = ((grid["neighbor_dist"].double() - exact).abs() / exact).max().item()
    rel = ((dense["neighbor_dist"] - grid["neighbor_dist"]).abs() / grid["neighbor_dist"]).max().item()
    print(f"P = {P}: neighbor_dist against fp64: dense {err_d:.3e}, grid {err_g:.3e}; dense against grid {rel:.3e}")
    if agree_1e5:
        assert rel <= 1e-5
    assert err_g < err_d                                # cdist's matrix-product form is the inexact side
    assert err_g <= 4 * 2.0 ** -24                      # direct differences: five roundings and a root
    w = torch.exp(-2000 * exact ** 2)
    assert (grid["neighbor_weight"].double() - w).abs().max() <= (dense["neighbor_weight"].double() - w).abs().max()
    with pytest.raises(ValueError):
        make_rigidity_variables(params, knn="tree")


@pytest.mark.parametrize("seed", [1, 3])
def test_outlier_filter_grid_keeps_the_fp64_loops_points(seed):
    from gsdyn.dynamics import remove_statistical_outliers
    x = R.tabletop_cloud(seed)
    keep64, passes, margin = R.outlier_loop_fp64(x)
    # the comparison below cannot flip on fp32 rounding: no mean distance comes closer to a pass's threshold than thousands of ulp
    assert margin >= 2.9e-4, margin
    assert passes == 6 and keep64.size == {1: 2838, 3: 2863}[seed]
    grid = remove_statistical_outliers(torch.from_numpy(x), knn="grid")
    dense = remove_statistical_outliers(torch.from_numpy(x))
    assert grid.dtype == torch.int64 and np.array_equal(grid.numpy(), keep64)
    assert torch.equal(grid, dense)
    with pytest.raises(ValueError):
        remove_statistical_outliers(torch.from_numpy(x), knn="tree")


def test_switches_reach_train_and_predict():
    """train / initialize_post_first_timestep / predict_episode / collect_scene_data take the switch and default to the dense form."""
    import inspect
    import importlib
    T, Pr = importlib.import_module("gsdyn.train"), importlib.import_module("gsdyn.predict")   # (gsdyn.train the attribute is the function)
    for fn, name in ((T.train, "knn"), (T.initialize_post_first_timestep, "knn"), (Pr.predict_episode, "outlier_knn"), (Pr.collect_scene_data, "outlier_knn")):
        assert inspect.signature(fn).parameters[name].default == "dense", fn
