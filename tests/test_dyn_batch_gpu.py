"""GPU tests of the training-batch builder (csrc/gsr_dyn_batch.hip, gsdyn.make_dynamics_batch): the device path against the definition
(the plain-torch path on CPU tensors, itself checked against tests/dyn_batch_ref.py by test_dyn_batch_cpu.py) on the same seeded inputs,
BIT FOR BIT on every output, at the smallest shapes where the kernels can go wrong; then run-to-run identity, batch independence, the
overflow error, the trainer's seam and the fall-back beyond the kernels' limits.  Legal inputs only."""
import numpy as np
import pytest
import torch

import dyn_batch_ref as R

pytestmark = pytest.mark.gpu

GRAPH_FIELDS = ("receivers", "senders", "row_start", "rev_ptr", "rev_edge")


@pytest.fixture(autouse=True)
def _one_host_thread():
    """The definition is many small tensor ops on the host: one thread for the duration of a test (tests/test_gnn_train_gpu.py has the
    reason); the session's setting is put back."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def _tensors(arr, kw, dev):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev) if isinstance(x, np.ndarray) else x  # noqa: E731
    return [t(arr[k]) for k in ("particles", "eef", "pairs")], {k: t(v) for k, v in kw.items()}


def _build(arr, kw, dev, **over):
    import gsdyn
    a, k = _tensors(arr, kw, dev)
    k.update(over)
    return gsdyn.make_dynamics_batch(*a, **k)


def _bits(x):
    x = x.detach().cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _assert_same(got, want, tag=""):
    assert set(got) == set(want), (tag, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if k == "graph":
            for f in GRAPH_FIELDS:
                a, b = getattr(g, f), getattr(w, f)
                assert a.dtype == b.dtype == torch.int64 and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), (tag, k, f)
        elif k == "n_rel_rows":
            assert g == w, (tag, k)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, w.dtype, g.shape, w.shape)
            assert torch.equal(_bits(g), _bits(w)), (tag, k)


def _on_device(batch, dev):
    return all(v.device.type == dev.type for k, v in batch.items() if isinstance(v, torch.Tensor)) and batch["graph"].rev_edge.device.type == dev.type


# P in {1, 63, 64, 65, 1000, 1024}; max_nobj in {1, 63, 64, 127, 128, 150, 255} (N crosses every 64-lane boundary); topk in {1, 5, 16};
# B in {1, 3, 65}; n_his in {1, 3}; n_future = 1; noise None; dense off; per-sample radii and thresholds differ in every case
CASES = {
    "one_particle": dict(B=3, P=1, n_his=1, n_future=1, max_nobj=1, topk=1, connect_all=True, noise=None, mixed_counts=False),
    "row64": dict(B=3, P=63, n_his=3, n_future=3, max_nobj=63, topk=5, connect_all=False),
    "row65_lists_only": dict(B=3, P=64, n_his=3, n_future=2, max_nobj=64, topk=16, connect_all=True, dense=False),
    "row128_all_kept": dict(B=3, P=65, n_his=1, n_future=2, max_nobj=127, topk=5, connect_all=False, radius=(0.0, 0.0)),
    "row129_rope": dict(B=3, P=1000, n_his=3, n_future=3, max_nobj=128, topk=5, connect_all=False, radius=(0.01, 0.04)),
    "row151_cloth": dict(B=3, P=1024, n_his=3, n_future=3, max_nobj=150, topk=6, connect_all=True, radius=(0.0, 0.0)),
    "row256": dict(B=1, P=1024, n_his=3, n_future=1, max_nobj=255, topk=16, connect_all=True, radius=(0.0, 0.0), mixed_counts=False),
    "one_object_topk_above": dict(B=3, P=65, n_his=3, n_future=3, max_nobj=20, topk=5, connect_all=False, radius=(1.0, 2.0)),
    "no_object_relations": dict(B=3, P=65, n_his=3, n_future=3, max_nobj=20, topk=5, connect_all=True, thresh=(0.0, 0.0)),
    "no_relations_at_all": dict(B=3, P=65, n_his=3, n_future=3, max_nobj=20, topk=5, connect_all=False, thresh=(0.0, 0.0)),
    "duplicates": dict(B=3, P=200, n_his=3, n_future=3, max_nobj=64, topk=5, connect_all=False, duplicates=True, radius=(0.0, 0.02)),
    "batch65": dict(B=65, P=65, n_his=1, n_future=2, max_nobj=20, topk=5, connect_all=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_device_path_matches_the_definition_bit_for_bit(dev, name, monkeypatch):
    from diff_gaussian_rasterization import _hip
    arr, kw = R.make_case(sorted(CASES).index(name) + 1, **CASES[name])
    launches = []
    for fn in ("dyn_batch_sample", "dyn_batch_relations", "dyn_batch_graph"):
        monkeypatch.setattr(_hip, fn, lambda *a, _f=getattr(_hip, fn), _n=fn, **k: (launches.append(_n), _f(*a, **k))[1])
    want = _build(arr, kw, torch.device("cpu"))
    assert not launches                                                         # the definition launches none of the kernels
    got = _build(arr, kw, dev)
    assert launches == ["dyn_batch_sample", "dyn_batch_relations", "dyn_batch_graph"] and _on_device(got, dev)
    n_obj, n_rel = want["n_obj"].tolist(), want["n_rel"].tolist()
    print(f"{name}: n_obj {n_obj[:6]} n_rel {n_rel[:6]}")
    c = CASES[name]
    if c.get("radius") == (0.0, 0.0) and not c.get("duplicates"):
        n_p = kw["n_particles"] if kw["n_particles"] is not None else np.full(c["B"], c["P"])
        assert n_obj == np.minimum(n_p, c["max_nobj"]).tolist()                   # radius 0: every pick is kept
    if name == "one_object_topk_above":
        assert n_obj == [1] * c["B"]
    if name == "no_relations_at_all":
        assert n_rel == [0] * c["B"] and got["graph"].receivers.numel() == 0
    if name == "no_object_relations":
        assert n_rel == [2 * n for n in n_obj]
    _assert_same(got, want, name)


def test_two_runs_are_bit_identical(dev):
    arr, kw = R.make_case(21, **CASES["row129_rope"])
    _assert_same(_build(arr, kw, dev), _build(arr, kw, dev))


def test_a_sample_does_not_depend_on_its_batch(dev):
    arr, kw = R.make_case(22, B=3, P=200, n_his=3, n_future=3, max_nobj=70, topk=5, connect_all=True)
    whole = _build(arr, kw, dev)
    N = 71
    for b in range(3):
        one_kw = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        one = _build(dict(arr, pairs=arr["pairs"][b:b + 1]), one_kw, dev)
        for k, v in one.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(_bits(v[0]), _bits(whole[k][b])), (b, k)
        lo, hi = whole["graph"].row_start[b * N].item(), whole["graph"].row_start[(b + 1) * N].item()
        assert torch.equal(one["graph"].receivers + b * N, whole["graph"].receivers[lo:hi])
        assert torch.equal(one["graph"].senders + b * N, whole["graph"].senders[lo:hi])
        assert torch.equal(one["graph"].rev_edge + lo, whole["graph"].rev_edge[lo:hi])


def test_overflow_raises_and_launches_nothing_after_the_count(dev, monkeypatch):
    from diff_gaussian_rasterization import _hip
    arr, kw = R.make_case(23, B=3, P=200, n_his=3, n_future=3, max_nobj=40, topk=5, connect_all=True)
    n_rel = _build(arr, kw, torch.device("cpu"))["n_rel"].tolist()
    worst = int(np.argmax(n_rel))
    kw["max_nR"] = max(n_rel) - 1
    calls = []
    monkeypatch.setattr(_hip, "dyn_batch_graph", lambda *a, **k: calls.append(a))
    with pytest.raises(ValueError, match=rf"sample {n_rel.index(max(n_rel))} has {n_rel[worst]} relations"):
        _build(arr, kw, dev)
    assert not calls
    torch.cuda.synchronize()


MODEL = dict(nf_particle=32, nf_relation=32, nf_effect=32, attr_dim=2, state_dim=0, action_dim=3, pstep=3, rel_attr_dim=2, rel_group_dim=1,
             rel_distance_dim=3, n_his=3)


@pytest.mark.parametrize("name,case", [("rope", dict(B=3, P=300, n_his=3, n_future=3, max_nobj=40, topk=5, connect_all=False)),
                                       ("cloth151", dict(B=2, P=400, n_his=3, n_future=3, max_nobj=150, topk=6, connect_all=True,
                                                         radius=(0.0, 0.01)))])
def test_training_step_with_the_kernel_built_graph(dev, name, case):
    """train_dynamics_step on the builder's batch (graph from the kernel, the seam of dyn_train) against the same batch as the dense
    dictionary alone (the graph derived from Rr / Rs by nonzero and a stable sort, as before): the loss and every parameter gradient in
    the same bits; and the lists-only batch (dense off) the same again."""
    import gsdyn
    from gsdyn.dynamics import DynamicsPredictor
    arr, kw = R.make_case(31, **case)
    full = _build(arr, kw, dev)
    lists = _build(arr, kw, dev, dense=False)
    dense_only = {k: v for k, v in full.items() if k not in ("graph", "receivers", "senders", "n_rel", "n_rel_rows", "n_obj", "fps_idx")}
    assert full["state"].shape[2] == case["max_nobj"] + 1 and "Rr" not in lists
    torch.manual_seed(0)
    model = DynamicsPredictor(dict(MODEL), device=dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    results = []
    for batch in (dense_only, full, lists):
        loss = gsdyn.train_dynamics_step(model, opt, batch, n_future=case["n_future"], device_path=True)
        results.append((loss.clone(), [p.grad.clone() for p in model.parameters()]))
    assert gsdyn.dynamics_loss(model, lists, n_future=case["n_future"], device_path=True)[1]["device_path"]
    assert torch.isfinite(results[0][0]) and any(g.abs().max() > 0 for g in results[0][1])
    for loss, grads in results[1:]:
        assert torch.equal(_bits(loss), _bits(results[0][0])), name
        for g, w in zip(grads, results[0][1]):
            assert torch.equal(_bits(g), _bits(w)), name


@pytest.mark.parametrize("over", [dict(P=1025, max_nobj=20, topk=5), dict(P=300, max_nobj=256, topk=5), dict(P=65, max_nobj=20, topk=17)])
def test_beyond_a_limit_the_call_falls_back_to_the_definition(dev, monkeypatch, over):
    from diff_gaussian_rasterization import _hip
    arr, kw = R.make_case(41, B=2, n_his=2, n_future=2, connect_all=True, radius=(0.03, 0.06), **over)
    monkeypatch.setattr(_hip, "dyn_batch_sample", lambda *a, **k: pytest.fail("the kernels were launched beyond their limits"))
    got = _build(arr, kw, dev)
    assert _on_device(got, dev)
    _assert_same(got, _build(arr, kw, torch.device("cpu")))
