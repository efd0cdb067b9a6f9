"""CPU tests of the propagation network's training path: the fp32 statements of the two backward kernels (tests/gnn_bwd_ref.py) against
torch autograd of the eager formulas, ``gsdyn.dynamics_loss`` on CPU tensors (the fallback, which is also the definition) against the
dense fp64 referee, the exported symbols and the wrappers' argument checks."""
import os
import re

import numpy as np
import pytest
import torch

import gnn_bwd_ref as ref
import gnn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsr_gnn_aggregate_backward", "gsr_gnn_rel_inputs_backward")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _lists(N, E, rng):
    recv = np.sort(rng.integers(0, N, E)).astype(np.int64)
    send = rng.integers(0, N, E).astype(np.int64)
    row_start = np.searchsorted(recv, np.arange(N + 1)).astype(np.int64)
    return recv, send, row_start, ref.reverse_list(send, N)


def _torch_aggregate_grads(rew1, a23, send, recv, d_agg, n_sum):
    """autograd of agg = index_add(relu((rew1 + a2[recv]) + a3[send])) over the relations of receivers < n_sum, on the host."""
    r1, nb = torch.from_numpy(rew1).requires_grad_(), torch.from_numpy(a23).requires_grad_()
    H = r1.shape[1]
    rv, sd = torch.from_numpy(recv), torch.from_numpy(send)
    terms = torch.relu((r1 + nb[rv, :H]) + nb[sd, H:])
    keep = rv < n_sum
    agg = torch.zeros((nb.shape[0], H)).index_add(0, rv[keep], terms[keep])
    agg.backward(torch.from_numpy(d_agg))
    return r1.grad.numpy(), nb.grad.numpy()


@pytest.mark.parametrize("N,H,E", [(1, 4, 3), (7, 8, 40), (37, 12, 300)])
def test_aggregate_backward_statement_equals_torch_autograd(N, H, E):
    rng = np.random.default_rng(N * 100 + H)
    recv, send, row_start, (rev_ptr, rev_edge) = _lists(N, E, rng)
    rew1 = rng.standard_normal((E, H)).astype(np.float32)
    a23 = rng.standard_normal((N, 2 * H)).astype(np.float32)
    d_agg = rng.standard_normal((N, H)).astype(np.float32)
    # z exactly +0 and -0 (dyadic values that cancel), and a NaN
    a23[recv[0], 0], a23[send[0], H], rew1[0, 0] = 0.5, 0.25, -0.75
    a23[recv[1], 1], a23[send[1], H + 1], rew1[1, 1] = -0.0, -0.0, -0.0
    rew1[E - 1, 2] = np.nan
    for n_sum in sorted({N, N - 1}):
        d_r1, d_nb = ref.aggregate_backward(rew1, a23, send, row_start, rev_ptr, rev_edge, d_agg, n_sum)
        t_r1, t_nb = _torch_aggregate_grads(rew1, a23, send, recv, d_agg, n_sum)
        assert d_r1.dtype == np.float32 and d_nb.dtype == np.float32
        assert _same_bits(d_r1, t_r1) and _same_bits(d_nb, t_nb), (N, H, E, n_sum)
        if recv[0] < n_sum:
            assert d_r1[0, 0] == 0.0 and (recv[1] >= n_sum or d_r1[1, 1] == 0.0)
        if recv[E - 1] < n_sum:
            assert _bits(d_r1[E - 1, 2]) == _bits(d_agg[recv[E - 1], 2])          # a NaN z passes the gradient
        d64 = ref.aggregate_backward(rew1, a23, send, row_start, rev_ptr, rev_edge, d_agg, n_sum, dtype=np.float64)
        bound = ref.aggregate_backward_bound(rew1, a23, send, row_start, rev_ptr, rev_edge, d_agg, n_sum)
        assert np.array_equal(d64[0], d_r1.astype(np.float64)) and (np.abs(d_nb - d64[1]) <= bound).all()


@pytest.mark.parametrize("A,G,S", [(2, 1, 9), (0, 1, 3), (3, 2, 9), (2, 1, 0)])
def test_rel_inputs_backward_statement_equals_torch_autograd(A, G, S):
    rng = np.random.default_rng(10 * A + S)
    N, E, Dr = 11, 60, 2 * A + 1 + S
    recv, send, row_start, (rev_ptr, rev_edge) = _lists(N, E, rng)
    d_out = rng.standard_normal((E, Dr)).astype(np.float32)
    got = ref.rel_inputs_backward(d_out, row_start, rev_ptr, rev_edge, A, S)
    state = torch.zeros((N, S), requires_grad=True)
    (state[torch.from_numpy(recv)] - state[torch.from_numpy(send)]).backward(torch.from_numpy(d_out[:, 2 * A + 1:]).contiguous())
    assert got.shape == (N, S) and got.dtype == np.float32 and _same_bits(got, state.grad.numpy())
    want64 = ref.rel_inputs_backward(d_out, row_start, rev_ptr, rev_edge, A, S, dtype=np.float64)
    assert (np.abs(got - want64) <= ref.rel_inputs_backward_bound(d_out, row_start, rev_ptr, rev_edge, A, S)).all()


def test_symbols_are_exported_and_declared():
    from diff_gaussian_rasterization import _hip
    import ctypes
    import gsdyn
    from gsdyn.dynamics import DynamicsPredictor
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for s in SYMBOLS:
        assert s in _hip.EXPORTS and re.search(r"^int " + s + r"\(", header, re.M), s
        getattr(lib, s)
    assert re.search(r"#define GSR_VERSION 125\b", header) and lib.gsr_version() == 125
    assert callable(gsdyn.dynamics_loss) and callable(gsdyn.train_dynamics_step)
    assert callable(_hip.gnn_aggregate_backward) and callable(_hip.gnn_rel_inputs_backward)
    assert callable(DynamicsPredictor.propagate_split_grad)


def test_wrappers_refuse_what_the_kernels_would_misread():
    """Wrong dtypes and non-contiguous matrices are ValueErrors before anything else; tensors on the host are refused (no CPU fallback in
    the wrappers: the fallback of the training path is ``DynamicsPredictor.forward``)."""
    from diff_gaussian_rasterization import _hip
    N, H, E, A, S = 6, 8, 10, 2, 9
    rew1, a23, d_agg = torch.zeros((E, H)), torch.zeros((N, 2 * H)), torch.zeros((N, H))
    idx, ptr = torch.zeros(E, dtype=torch.int64), torch.zeros(N + 1, dtype=torch.int64)
    good = (rew1, a23, idx, idx, ptr, ptr, idx, d_agg)
    bad = {"rel_part float64": (0, rew1.double()), "rel_part not contiguous": (0, torch.zeros((E, 2 * H))[:, :H]),
           "node_parts float16": (1, a23.half()), "node_parts not contiguous": (1, torch.zeros((N, 4 * H))[:, :2 * H]),
           "d_agg float64": (7, d_agg.double()), "d_agg not contiguous": (7, torch.zeros((N, 2 * H))[:, :H])}
    for why, (k, t) in bad.items():
        with pytest.raises(ValueError):
            _hip.gnn_aggregate_backward(*(good[:k] + (t,) + good[k + 1:]))
            pytest.fail(f"accepted: {why}")
    with pytest.raises(RuntimeError, match="HIP device"):
        _hip.gnn_aggregate_backward(*good)
    d_out = torch.zeros((E, 2 * A + 1 + S))
    for t in (d_out.double(), torch.zeros((E, 2 * (2 * A + 1 + S)))[:, :2 * A + 1 + S]):
        with pytest.raises(ValueError):
            _hip.gnn_rel_inputs_backward(t, ptr, ptr, idx, A, S)
    with pytest.raises(RuntimeError, match="HIP device"):
        _hip.gnn_rel_inputs_backward(d_out, ptr, ptr, idx, A, S)


def _case(name, B, n_future, seed=5):
    kw = dict(gnn_ref.CONFIGS[name])
    instances = kw.pop("instances", 1)
    cfg = gnn_ref.base_cfg(**kw)
    return cfg, ref.make_batch(cfg, instances, B, 12, n_future, seed, dtype=torch.float64)


@pytest.mark.parametrize("name,B,n_future", [("C0", 2, 1), ("C0", 2, 3), ("C3", 3, 3), ("C9", 1, 3), ("C10", 2, 1)])
def test_dynamics_loss_on_the_host_equals_the_dense_referee(name, B, n_future):
    """fp64 on CPU tensors: the fallback path (index-form length term, denominator B n_rel with the padded rows) within 1e-12 of the dense
    referee, loss and gradients; the caller's batch is unchanged; ``device_path=True`` changes nothing on the host."""
    import gsdyn
    cfg, batch = _case(name, B, n_future)
    model = gnn_ref.make_model(cfg, 3).double()
    assert int((batch["Rr"].sum(-1) == 0).sum()) >= 7 * B                     # padded relation rows are present
    before = {k: v.clone() for k, v in batch.items()}
    want = ref.referee_loss(model, batch, n_future)
    g_want = torch.autograd.grad(want, list(model.parameters()))
    for path in (None, True, False):
        got, parts = gsdyn.dynamics_loss(model, batch, n_future=n_future, device_path=path)
        assert parts["device_path"] is False
        assert abs(got.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item())), (got.item(), want.item())
        assert abs(float(parts["mse"] + parts["length"]) - got.item()) <= 1e-15 and float(parts["length"]) > 0
        for a, b in zip(torch.autograd.grad(got, list(model.parameters())), g_want):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert all(torch.equal(batch[k], before[k]) for k in before)
    w = dict(mse_weight=0.5, length_weight=0.3)
    assert abs(float(gsdyn.dynamics_loss(model, batch, n_future=n_future, **w)[0]) - float(ref.referee_loss(model, batch, n_future, **w))) <= 1e-12


def test_train_dynamics_step_on_the_host_lowers_the_loss():
    import gsdyn
    cfg, batch = _case("C1", 2, 2)
    model = gnn_ref.make_model(cfg, 4).double()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = [float(gsdyn.train_dynamics_step(model, opt, batch, n_future=2)) for _ in range(3)]
    assert losses[2] < losses[0], losses
    with pytest.raises(ValueError):
        gsdyn.dynamics_loss(model, batch, n_future=0)


def test_propagate_split_grad_refuses_the_host():
    from gsdyn.dynamics import split_graph
    cfg, batch = _case("C0", 1, 1)
    model = gnn_ref.make_model(cfg, 3)
    N = batch["attrs"].shape[1]
    graph = split_graph(torch.zeros(4, dtype=torch.int64), torch.arange(4), N)
    assert graph.row_start.tolist() == [0] + [4] * N and graph.rev_ptr.tolist()[:6] == [0, 1, 2, 3, 4, 4] and graph.rev_edge.tolist() == [0, 1, 2, 3]
    with pytest.raises(RuntimeError):
        model.propagate_split_grad(torch.zeros((N, 9)), batch["attrs"][0].float(), torch.zeros((N, 1)), torch.zeros((N, 3)), graph)
