"""CPU tests of gsdyn.make_dynamics_batch's definition (gsdyn/dyn_data.py): bit for bit against the independent numpy referee
(tests/dyn_batch_ref.py), the overflow error, the graph against what ``_device_loss`` derives from the dense matrices, ``dynamics_loss`` on
a batch with and without them, ``draw_batch_randomness``, and the golden samples of the reference's ``DynDataset.__getitem__``
(tests/golden/dyn_batch_golden.npz, made by tests/golden/gen_dyn_batch_goldens.py)."""
import math
import os

import numpy as np
import pytest
import torch

import dyn_batch_ref as R

GRAPH_FIELDS = ("receivers", "senders", "row_start", "rev_ptr", "rev_edge")


def _build(arr, kw, **over):
    import gsdyn
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x  # noqa: E731
    k = {n: t(v) for n, v in kw.items()}
    k.update(over)
    return gsdyn.make_dynamics_batch(*(t(arr[n]) for n in ("particles", "eef", "pairs")), **k)


def _assert_matches_referee(got, ref, tag):
    assert set(got) == set(ref), (tag, set(got) ^ set(ref))
    for k, v in ref.items():
        if k == "graph":
            for f in GRAPH_FIELDS:
                g = getattr(got["graph"], f)
                assert g.dtype == torch.int64 and np.array_equal(g.numpy(), v[f]), (tag, f)
        elif k == "n_rel_rows":
            assert got[k] == v
        else:
            g = got[k].numpy()
            assert g.dtype == v.dtype and g.shape == v.shape, (tag, k, g.dtype, v.dtype, g.shape, v.shape)
            same = np.array_equal(g.view(np.int32), v.view(np.int32)) if v.dtype == np.float32 else np.array_equal(g, v)
            assert same, (tag, k)


# the edge list of the GPU tests (tests/test_dyn_batch_gpu.py), with the two large clouds once each
CASES = {
    "one_particle": dict(B=3, P=1, n_his=1, n_future=1, max_nobj=1, topk=1, connect_all=True, noise=None, mixed_counts=False),
    "row64": dict(B=3, P=63, n_his=3, n_future=3, max_nobj=63, topk=5, connect_all=False),
    "row65_lists_only": dict(B=3, P=64, n_his=3, n_future=2, max_nobj=64, topk=16, connect_all=True, dense=False),
    "row128_all_kept": dict(B=3, P=65, n_his=1, n_future=2, max_nobj=127, topk=5, connect_all=False, radius=(0.0, 0.0)),
    "row129_rope": dict(B=2, P=1000, n_his=3, n_future=3, max_nobj=128, topk=5, connect_all=False, radius=(0.01, 0.04)),
    "row151_cloth": dict(B=2, P=1024, n_his=3, n_future=3, max_nobj=150, topk=6, connect_all=True, radius=(0.0, 0.0)),
    "row256": dict(B=1, P=300, n_his=3, n_future=1, max_nobj=255, topk=16, connect_all=True, radius=(0.0, 0.0), mixed_counts=False),
    "one_object_topk_above": dict(B=3, P=65, n_his=3, n_future=3, max_nobj=20, topk=5, connect_all=False, radius=(1.0, 2.0)),
    "no_object_relations": dict(B=3, P=65, n_his=3, n_future=3, max_nobj=20, topk=5, connect_all=True, thresh=(0.0, 0.0)),
    "no_relations_at_all": dict(B=3, P=65, n_his=3, n_future=3, max_nobj=20, topk=5, connect_all=False, thresh=(0.0, 0.0)),
    "duplicates": dict(B=3, P=200, n_his=3, n_future=3, max_nobj=64, topk=5, connect_all=False, duplicates=True, radius=(0.0, 0.02)),
    "batch65": dict(B=65, P=65, n_his=1, n_future=2, max_nobj=20, topk=5, connect_all=True),
    "beyond_the_kernels": dict(B=2, P=1025, n_his=2, n_future=2, max_nobj=256, topk=17, connect_all=True, radius=(0.02, 0.05)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_definition_matches_the_referee_bit_for_bit(name):
    arr, kw = R.make_case(sorted(CASES).index(name) + 1, **CASES[name])
    _assert_matches_referee(_build(arr, kw), R.ref_batch(**arr, **kw), name)


def test_overflow_raises_value_error():
    arr, kw = R.make_case(23, B=3, P=200, n_his=3, n_future=3, max_nobj=40, topk=5, connect_all=True)
    n_rel = _build(arr, kw)["n_rel"].tolist()
    kw["max_nR"] = max(n_rel) - 1
    with pytest.raises(ValueError, match=rf"sample {n_rel.index(max(n_rel))} has {max(n_rel)} relations"):
        _build(arr, kw)
    with pytest.raises(ValueError):
        R.ref_batch(**arr, **kw)


def test_graph_is_what_the_trainer_derives_from_the_dense_matrices():
    """``_device_loss``'s list from Rr / Rs (argmax, nonzero, a stable sort by receiver) and ``split_graph`` of it."""
    from gsdyn.dynamics import DynamicsPredictor, split_graph
    arr, kw = R.make_case(5, B=3, P=200, n_his=3, n_future=3, max_nobj=40, topk=5, connect_all=True)
    batch = _build(arr, kw)
    B, _, N = batch["Rr"].shape
    recv, send, w = DynamicsPredictor._indices(batch["Rr"], batch["Rs"])
    b, r = torch.nonzero(w > 0, as_tuple=True)
    recv, order = torch.sort(recv[b, r] + b * N, stable=True)
    want = split_graph(recv, (send[b, r] + b * N)[order], B * N)
    assert want.receivers.numel() == int(batch["n_rel"].sum()) > 0
    for f in GRAPH_FIELDS:
        assert torch.equal(getattr(batch["graph"], f), getattr(want, f)), f


def test_dynamics_loss_is_the_same_with_and_without_the_dense_matrices():
    import gsdyn
    from gsdyn.dynamics import DynamicsPredictor
    arr, kw = R.make_case(6, B=3, P=100, n_his=3, n_future=2, max_nobj=20, topk=5, connect_all=True)
    torch.manual_seed(0)
    model = DynamicsPredictor(dict(nf_particle=16, nf_relation=16, nf_effect=16, attr_dim=2, state_dim=0, action_dim=3, pstep=2, rel_attr_dim=2,
                                   rel_group_dim=1, rel_distance_dim=3, n_his=3))
    results = []
    for dense in (True, False):
        batch = _build(arr, kw, dense=dense)
        assert ("Rr" in batch) == dense
        model.zero_grad()
        loss, info = gsdyn.dynamics_loss(model, batch, n_future=2)
        loss.backward()
        assert not info["device_path"]
        results.append((loss.detach().clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.isfinite(results[0][0]) and results[0][0] > 0
    assert torch.equal(results[0][0], results[1][0])
    for a, b in zip(results[0][1], results[1][1]):
        assert torch.equal(a, b)


def test_draw_batch_randomness():
    import gsdyn
    kw = dict(n_his=3, max_nobj=20, fps_radius_range=[0.03, 0.05], adj_radius_range=[0.06, 0.1], state_noise=0.004)
    n = torch.tensor([1, 5, 60, 1000] * 64)
    B = n.numel()
    d = gsdyn.draw_batch_randomness(B, n, generator=torch.Generator().manual_seed(3), **kw)
    assert set(d) == {"start_idx", "thin_start", "fps_radius", "adj_thresh", "rot", "noise"}
    assert d["start_idx"].dtype == d["thin_start"].dtype == torch.int64 and d["start_idx"].shape == d["thin_start"].shape == (B,)
    assert (d["start_idx"] >= 0).all() and (d["start_idx"] < n).all() and (d["thin_start"] >= 0).all() and (d["thin_start"] < n.clamp(max=20)).all()
    assert d["start_idx"][2::4].unique().numel() > 20 and d["thin_start"][3::4].max() > 10
    for k, (lo, hi) in (("fps_radius", (0.03, 0.05)), ("adj_thresh", (0.06, 0.1))):
        assert d[k].dtype == torch.float32 and d[k].shape == (B,) and (d[k] >= lo).all() and (d[k] <= hi).all() and d[k].std() > 0.1 * (hi - lo)
    rot = d["rot"]
    assert rot.dtype == torch.float32 and rot.shape == (B, 3, 3)
    ang = torch.atan2(rot[:, 1, 0], rot[:, 0, 0])
    assert ang.min() < -0.8 * math.pi and ang.max() > 0.8 * math.pi
    want = torch.stack([torch.cos(ang), -torch.sin(ang), 0 * ang, torch.sin(ang), torch.cos(ang), 0 * ang, 0 * ang, 0 * ang, 1 + 0 * ang], 1)
    assert torch.allclose(rot.reshape(B, 9), want, atol=1e-6)                  # a rotation about z
    assert d["noise"].dtype == torch.float32 and d["noise"].shape == (B, 3, 21, 3) and d["noise"].abs().max() <= 0.004
    assert d["noise"].abs().max() > 0.0039 and abs(float(d["noise"].mean())) < 1e-4
    again = gsdyn.draw_batch_randomness(B, n, generator=torch.Generator().manual_seed(3), **kw)
    other = gsdyn.draw_batch_randomness(B, n, generator=torch.Generator().manual_seed(4), **kw)
    assert all(torch.equal(d[k], again[k]) for k in d) and not torch.equal(d["noise"], other["noise"])
    # the draws are legal inputs of the builder
    arr, case = R.make_case(7, B=4, P=60, n_his=3, n_future=2, max_nobj=20, topk=5, connect_all=False, mixed_counts=False)
    mine = gsdyn.draw_batch_randomness(4, 60, generator=torch.Generator().manual_seed(5), **kw)
    batch = _build(arr, {k: v for k, v in case.items() if k not in mine}, **mine)
    assert (batch["n_obj"] >= 1).all() and batch["state"].shape == (4, 3, 21, 3)


@pytest.mark.parametrize("kind", ["rope", "cloth"])
def test_golden_samples_of_the_reference_dataset(golden_dir, kind):
    """The reference's ``DynDataset.__getitem__`` on recorded draws (the generator kept every decision of these samples at least 1e-5
    relative away from a tie, in fp64).  Integer and boolean outputs -- n_obj through obj_mask, attrs, p_instance, the relation lists
    through Rr / Rs -- are EQUAL.  Floats: the reference adds float64 noise into a float32 array (one rounding) and rotates with a BLAS
    product; the project rounds the noise to float32, adds, and rotates with three products and two sums.  With u = 2^-24, S >= |x| + |y| +
    |z| of an unrotated row and a the noise amplitude, each coordinate before the rotation differs by at most u a (the noise's rounding) +
    2 u (|x_i| + a) (one rounding of the sum on each side); the rotation's entries are at most 1 in magnitude, so that passes through as at
    most 2 u (S + 3 a) + 3 u a; each side's three-term product sum is within 3 u (S + 3 a) of the exact one (any order, fused or not).
    Total: at most 8 u (S + 3 a) + 3 u a <= 8 u (S + 4 a).  S is taken as the largest |x| + |y| + |z| over all input rows: the bound is
    one number per configuration (2.1e-7 and 2.4e-7 here), derived, not tuned."""
    g = np.load(os.path.join(golden_dir, "dyn_batch_golden.npz"))
    cfg = dict(zip(g[f"{kind}_cfg_keys"].tolist(), g[f"{kind}_cfg_vals"].tolist()))
    cfg["connect_all"] = bool(cfg["connect_all"])
    get = lambda k: g[f"{kind}_{k}"]  # noqa: E731
    arr = dict(particles=get("particles"), eef=get("eef"), pairs=get("pairs"))
    kw = dict(cfg, **{k: get(k) for k in ("start_idx", "thin_start", "fps_radius", "adj_thresh", "rot", "noise")})
    out = _build(arr, kw)
    S = max(float(np.abs(arr["particles"]).sum(-1).max()), float(np.abs(arr["eef"]).sum(-1).max()))
    bound = 8 * 2.0 ** -24 * (S + 4 * float(g[f"{kind}_state_noise"][0]))
    assert np.array_equal(out["n_obj"].numpy(), get("out_obj_mask").sum(1))
    for k in ("obj_mask", "attrs", "p_instance", "Rr", "Rs"):
        w = get("out_" + k)
        assert out[k].numpy().dtype == w.dtype and np.array_equal(out[k].numpy(), w), k
    assert np.array_equal(out["n_rel"].numpy(), (get("out_Rr").sum(-1) > 0).sum(1))
    for k in ("state", "action", "tool_future", "action_future", "state_future"):
        w = get("out_" + k)
        err = float(np.abs(out[k].numpy().astype(np.float64) - w).max())
        print(f"{kind} {k}: max abs difference {err:.3e}, bound {bound:.3e}")
        assert out[k].numpy().dtype == w.dtype == np.float32 and out[k].shape == w.shape and err <= bound, (k, err, bound)
