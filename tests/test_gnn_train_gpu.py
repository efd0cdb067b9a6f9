"""GPU tests of the propagation network's training path (csrc/gsr_gnn_bwd.hip, DynamicsPredictor.propagate_split_grad, gsdyn.dynamics_loss).

Part one: gsr_gnn_aggregate_backward and gsr_gnn_rel_inputs_backward bit for bit against their fp32 statements (tests/gnn_bwd_ref.py) and
within derived bounds of the fp64 sums, at every shape edge and segment layout of the forward's tests, and their special cases.
Part two: ``dynamics_loss`` on the device at every configuration of gnn_ref.CONFIGS against the dense fp64 referee on the host -- the loss,
the gradient of every parameter tensor and of ``state``.  The bound is norm-wise per tensor: 4 x the distance of the HOST fp32 eager
autograd (``DynamicsPredictor.forward``) from fp64 on the same input sets, the rule gnn_ref.yardstick applies to the forward: per tensor
the yardstick is the largest relative distance ||x32 - x64|| / ||x64|| over the configuration's input sets (B in {1, 3} x n_future in
{1, 2}), computed from the eager path, never from the code under test.  The measured distances are appended to gnn_train_parity.log next
to gnn_parity.log (``GSR_GNN_TRAIN_PARITY_LOG`` names another file); profiles/gnn_train_parity.txt is that log of one run."""
import functools
import os

import numpy as np
import pytest
import torch

import gnn_bwd_ref as ref
import gnn_ref
from hipcheck import _ROW_LOG
from test_gnn_kernels_gpu import PAD, _aggregate_case, _bits, _same_bits

pytestmark = pytest.mark.gpu

_LOG = os.environ.get("GSR_GNN_TRAIN_PARITY_LOG", os.path.join(os.path.dirname(_ROW_LOG), "gnn_train_parity.log"))


@pytest.fixture(autouse=True)
def _one_host_thread():
    """The host side of these tests is many small tensor ops (numpy statements, the fp64 referee under autograd).  The C oracle's OpenMP
    runtime is torch's too: once an earlier test of the session has run the oracle on every core of the machine, torch's intra-op pool has
    that many threads, and on a host that grants fewer cores each small op takes tens of milliseconds (tests/test_dynamics_gpu.py met the
    same).  One thread for the duration of a test; the session's setting is put back."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def _log(line):
    print(line)
    try:
        os.makedirs(os.path.dirname(_LOG), exist_ok=True)
        with open(_LOG, "a") as f:
            f.write(line + "\n")
    except OSError as e:
        print(f"(gnn_train_parity.log not written: {e})")


def _t(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrays)


# ========================================================================================== part one: gsr_gnn_aggregate_backward
def _run_aggregate_backward(dev, rew1, a23, send, row_start, d_agg, n_sum):
    from diff_gaussian_rasterization import _hip
    N = a23.shape[0]
    recv = ref.receivers_of(row_start)
    rev_ptr, rev_edge = ref.reverse_list(send, N)
    d_r1, d_nb = _hip.gnn_aggregate_backward(*_t(dev, rew1, a23, send, recv, row_start, rev_ptr, rev_edge, d_agg), n_sum)
    return d_r1.cpu().numpy(), d_nb.cpu().numpy(), (rev_ptr, rev_edge)


def _check_aggregate_backward(dev, rew1, a23, send, row_start, d_agg, n_sum, tag):
    d_r1, d_nb, (rev_ptr, rev_edge) = _run_aggregate_backward(dev, rew1, a23, send, row_start, d_agg, n_sum)
    args = (rew1, a23, send, row_start, rev_ptr, rev_edge, d_agg, n_sum)
    w_r1, w_nb = ref.aggregate_backward(*args)
    r64, nb64 = ref.aggregate_backward(*args, dtype=np.float64)
    assert w_r1.dtype == np.float32 and _same_bits(d_r1, w_r1) and _same_bits(d_nb, w_nb), tag
    assert np.array_equal(d_r1.astype(np.float64), r64), tag                                    # d_rew1: a selection, exact
    assert (np.abs(d_nb - nb64) <= ref.aggregate_backward_bound(*args)).all(), tag
    H = rew1.shape[1]
    assert not d_nb[n_sum:, :H].any() and not d_r1[int(row_start[n_sum]):].any(), tag          # rows >= n_sum: no segment, relations without gradient
    return d_r1, d_nb


@pytest.mark.parametrize("N,H", [(1, 4), (2, 4), (37, 4), (1, 8), (2, 8), (37, 8), (1, 64), (2, 64), (37, 64),
                                 (85, 12), (64, 16), (257, 4), (86, 12), (52, 20)])
def test_aggregate_backward_kernel_bit_for_bit(dev, N, H):
    """H in {4, 8, 64} x N in {1, 2, 37}; N H / 4 = 255, 256, 257 threads, and 258 / 260 with H / 4 = 3 / 5, where the last row's threads
    straddle two workgroups.  Every layout of the forward's test, with the dummy last row and n_sum = N - 1 (and N)."""
    rng = np.random.default_rng(N * 1000 + H + 1)
    for layout in ("none", "random", "alternate", "ends_empty", "first", "last"):
        rew1, a23, send, row_start, _, _ = _aggregate_case(N, H, layout, rng)
        d_agg = rng.standard_normal((N, H)).astype(np.float32)
        for n_sum in sorted({N, N - 1}):
            if row_start[-1] == 0:
                continue                                                                          # E = 0: test_backward_wrappers_without_relations
            _check_aggregate_backward(dev, rew1, a23, send, row_start, d_agg, n_sum, (N, H, layout, n_sum))


def _special_case(rng):
    """N = 9: row 3 sends 97 relations, row 5 sends none; recv == send entries; the dummy row's padding."""
    N, H = 9, 8
    deg = np.array([20, 11, 30, 9, 14, 12, 6, 10, PAD])
    row_start = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(row_start[-1])
    recv = ref.receivers_of(row_start)
    e0, e1 = int(row_start[2]) + 1, int(row_start[4]) + 2          # the two relations whose z the caller sets to +0 and -0
    send = rng.choice(np.array([0, 1, 2, 4, 6, 7]), E).astype(np.int64)
    free = np.setdiff1d(np.arange(E - PAD), [e0, e1])
    send[rng.choice(free, 97, replace=False)] = 3
    send[E - PAD:] = N - 1
    same = np.nonzero((send != 3) & (recv != 5) & (recv != N - 1))[0][::6]
    send[np.setdiff1d(same, [e0, e1])] = recv[np.setdiff1d(same, [e0, e1])]
    send[e0], send[e1] = 0, 1                                       # receivers 2 and 4
    assert int((send == 3).sum()) == 97 and not (send == 5).any() and int((send == recv).sum()) > 5
    rew1 = rng.standard_normal((E, H)).astype(np.float32)
    a23 = rng.standard_normal((N, 2 * H)).astype(np.float32)
    d_agg = rng.standard_normal((N, H)).astype(np.float32)
    return N, H, E, recv, send, row_start, rew1, a23, d_agg, e0, e1


def test_aggregate_backward_kernel_special_cases(dev):
    rng = np.random.default_rng(21)
    N, H, E, recv, send, row_start, rew1, a23, d_agg, e0, e1 = _special_case(rng)
    # z exactly +0 from dyadic values (relation e0, column 0), z exactly -0 (e1, column 1): both block
    a23[recv[e0], 0], a23[send[e0], H + 0], rew1[e0, 0] = 0.5, 0.25, -0.75
    a23[recv[e1], 1], a23[send[e1], H + 1], rew1[e1, 1] = -0.0, -0.0, -0.0
    assert send[e0] != recv[e0] and send[e1] != recv[e1]
    for n_sum in (N, N - 1):
        d_r1, d_nb = _check_aggregate_backward(dev, rew1, a23, send, row_start, d_agg, n_sum, ("special", n_sum))
        assert d_r1[e0, 0] == 0.0 and d_r1[e1, 1] == 0.0
        assert not d_nb[5, H:].any()                                                              # the row that sends nothing
        assert d_nb[3, H:].all()                                                                  # 97 terms: some gate is open in every column
    # one NaN in rew1 where the clean z is far below zero: the gate opens (threshold_backward passes the gradient at a NaN) for that
    # relation and column only -- its d_rew1 element, its receiver's row and its sender's row change, everything stays finite
    e, c = int(row_start[6]) + 3, 5
    clean = rew1.copy()
    clean[e, c] = -100.0
    dirty = clean.copy()
    dirty[e, c] = np.nan
    a_r1, a_nb, _ = _run_aggregate_backward(dev, clean, a23, send, row_start, d_agg, N)
    b_r1, b_nb = _check_aggregate_backward(dev, dirty, a23, send, row_start, d_agg, N, "nan")
    assert a_r1[e, c] == 0.0 and _bits(b_r1[e, c]) == _bits(d_agg[recv[e], c]) and np.isfinite(b_r1).all() and np.isfinite(b_nb).all()
    diff_r1, diff_nb = _bits(a_r1) != _bits(b_r1), _bits(a_nb) != _bits(b_nb)
    assert np.argwhere(diff_r1).tolist() == [[e, c]]
    assert sorted(np.argwhere(diff_nb).tolist()) == sorted([[int(recv[e]), c], [int(send[e]), H + c]])
    # two runs: identical bits
    c_r1, c_nb, _ = _run_aggregate_backward(dev, dirty, a23, send, row_start, d_agg, N)
    assert np.array_equal(_bits(b_r1), _bits(c_r1)) and np.array_equal(_bits(b_nb), _bits(c_nb))


def test_backward_wrappers_without_relations(dev):
    """E = 0 (and S = 0): zeros of the right shapes, no library call."""
    from diff_gaussian_rasterization import _hip
    N, H = 6, 8
    f = lambda *s: torch.randn(s, device=dev)  # noqa: E731
    none, ptr = torch.zeros((0,), dtype=torch.int64, device=dev), torch.zeros((N + 1,), dtype=torch.int64, device=dev)
    for n_sum in (None, N - 1):
        d_r1, d_nb = _hip.gnn_aggregate_backward(f(0, H), f(N, 2 * H), none, none, ptr, ptr, none, f(N, H), n_sum)
        assert d_r1.shape == (0, H) and d_nb.shape == (N, 2 * H) and d_nb.dtype == torch.float32 and not bool(d_nb.any())
    out = _hip.gnn_rel_inputs_backward(f(0, 14), ptr, ptr, none, 2, 9)
    assert out.shape == (N, 9) and out.dtype == torch.float32 and out.device == ptr.device and not bool(out.any())
    idx = torch.zeros((3,), dtype=torch.int64, device=dev)
    ptr3 = torch.tensor([0, 3, 3, 3, 3, 3, 3], dtype=torch.int64, device=dev)
    assert _hip.gnn_rel_inputs_backward(f(3, 5), ptr3, ptr3, torch.arange(3, device=dev), 2, 0).shape == (N, 0)
    for bad in ((f(3, 5).double(), ptr3, ptr3, idx), (f(3, 5), ptr3.int(), ptr3, idx), (f(3, 5), ptr3, ptr3.cpu(), idx), (f(3, 5), ptr3, ptr3, idx[:2])):
        with pytest.raises(ValueError):
            _hip.gnn_rel_inputs_backward(*bad, 2, 0)


# ========================================================================================== part one: gsr_gnn_rel_inputs_backward
@pytest.mark.parametrize("A,G,S", [(2, 1, 9), (0, 1, 3), (3, 2, 9), (2, 4, 3), (2, 1, 0)])
def test_rel_inputs_backward_kernel_bit_for_bit(dev, A, G, S):
    from diff_gaussian_rasterization import _hip
    Dr, N = 2 * A + 1 + S, 37
    rng = np.random.default_rng(1000 * A + 100 * G + S + 7)
    for E in (1, 256 // Dr, 256 // Dr + 1, 1000):
        recv = np.sort(rng.integers(0, N, E)).astype(np.int64)
        send = rng.integers(0, N, E).astype(np.int64)
        send[::5] = recv[::5]                                      # recv == send: the two sums cancel where they are alone
        send[send == 11] = 12                                      # a row that sends nothing
        row_start = np.searchsorted(recv, np.arange(N + 1)).astype(np.int64)
        rev_ptr, rev_edge = ref.reverse_list(send, N)
        d_out = rng.standard_normal((E, Dr)).astype(np.float32)
        runs = [_hip.gnn_rel_inputs_backward(*_t(dev, d_out, row_start, rev_ptr, rev_edge), A, S).cpu().numpy() for _ in range(2)]
        want32 = ref.rel_inputs_backward(d_out, row_start, rev_ptr, rev_edge, A, S)
        want64 = ref.rel_inputs_backward(d_out, row_start, rev_ptr, rev_edge, A, S, dtype=np.float64)
        tag = (A, G, S, E)
        assert runs[0].shape == (N, S) and want32.dtype == np.float32, tag
        assert np.array_equal(_bits(runs[0]), _bits(want32)) and np.array_equal(_bits(runs[0]), _bits(runs[1])), tag
        assert (np.abs(runs[0] - want64) <= ref.rel_inputs_backward_bound(d_out, row_start, rev_ptr, rev_edge, A, S)).all(), tag


# ========================================================================================== part two: the network
FACTOR = 4.0
N_OBJ = 39
SETS = [(1, 1), (1, 2), (3, 1), (3, 2)]          # (B, n_future)


def _grads(model, batch, loss):
    """dict: "loss", "state" and every parameter's name -> fp64 numpy arrays of the loss and its gradients."""
    names = [k for k, _ in model.named_parameters()]
    gs = torch.autograd.grad(loss, [batch["state"]] + [p for _, p in model.named_parameters()])
    out = {"loss": np.array([float(loss.detach())])}
    out.update({k: g.detach().cpu().double().numpy() for k, g in zip(["state"] + names, gs)})
    return out


def _distance(x, want):
    n = float(np.linalg.norm(want))
    d = float(np.linalg.norm(np.asarray(x, dtype=np.float64) - want))
    return d / n if n > 0 else d


def _with_state_grad(batch, device=None, dtype=None):
    b = ref.to(batch, device=device, dtype=dtype)
    b["state"].requires_grad_()
    return b


@functools.lru_cache(maxsize=None)
def _net_case(name):
    """One configuration, built once per process and left unchanged: the host fp32 model, its input sets, the fp64 referee's loss and
    gradients per set, and the yardstick per tensor (the host fp32 eager autograd's largest relative distance from fp64 over the sets)."""
    kw = dict(gnn_ref.CONFIGS[name])
    instances = kw.pop("instances", 1)
    cfg = gnn_ref.base_cfg(**kw)
    idx = int(name[1:])
    model = gnn_ref.make_model(cfg, 400 + idx)
    model64 = gnn_ref.make_model(cfg, 400 + idx).double()
    sets, refs, y = [], [], {}
    for k, (B, n_future) in enumerate(SETS):
        batch = ref.make_batch(cfg, instances, B, N_OBJ, n_future, 500 + 10 * idx + k)
        assert int((batch["Rr"].sum(-1) == 0).sum()) >= 7 * B
        b64 = _with_state_grad(batch, dtype=torch.float64)
        want = _grads(model64, b64, ref.referee_loss(model64, b64, n_future))
        b32 = _with_state_grad(batch)
        eager = _grads(model, b32, ref.referee_loss(model, b32, n_future))
        for t in want:
            y[t] = max(y.get(t, 0.0), _distance(eager[t], want[t]))
        sets.append((B, n_future, batch))
        refs.append(want)
    return dict(name=name, cfg=cfg, model=model, sets=sets, refs=refs, y=y)


def _fresh_model(c, dev):
    from gsdyn.dynamics import DynamicsPredictor
    m = DynamicsPredictor(c["cfg"]).eval()
    m.load_state_dict(c["model"].state_dict())
    return m.to(dev)


def _device_grads(model, batch, n_future, dev, **kw):
    import gsdyn
    b = _with_state_grad(batch, device=dev)
    loss, parts = gsdyn.dynamics_loss(model, b, n_future=n_future, **kw)
    return _grads(model, b, loss), parts, b


@pytest.mark.parametrize("name", list(gnn_ref.CONFIGS))
def test_dynamics_loss_on_the_device_against_fp64(dev, name):
    c = _net_case(name)
    model = _fresh_model(c, dev)
    assert model.split_grad_ok(torch.zeros((1, 1), device=dev))
    worst = {}
    for (B, n_future, batch), want in zip(c["sets"], c["refs"]):
        got, parts, _ = _device_grads(model, batch, n_future, dev, device_path=True)
        assert parts["device_path"] is True
        for t in want:
            e = _distance(got[t], want[t])
            worst[t] = max(worst.get(t, 0.0), e)
    for t in worst:
        _log(f"T1 {name:>3} {t:<40} device {worst[t]:.3e} = {worst[t] / c['y'][t] if c['y'][t] else float('inf'):.2f} y ({c['y'][t]:.3e})")
    bad = {t: (worst[t], c["y"][t]) for t in worst if not worst[t] <= FACTOR * c["y"][t]}
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ["C0", "C3"])
def test_device_gradients_are_bit_identical_from_run_to_run(dev, name):
    c = _net_case(name)
    model = _fresh_model(c, dev)
    B, n_future, batch = c["sets"][3]
    a, _, _ = _device_grads(model, batch, n_future, dev, device_path=True)
    b, parts, _ = _device_grads(model, batch, n_future, dev)                  # device_path=None: the kernels' path where it can run
    assert parts["device_path"] is True
    for t in a:
        assert np.array_equal(a[t].view(np.uint64), b[t].view(np.uint64)), t


def test_fallback_when_the_attributes_require_a_gradient(dev):
    """``attrs.requires_grad``: ``model.forward`` under autograd runs instead (the kernels have no gradient toward the attributes), the
    result is the referee's and the attributes receive their gradient."""
    import gsdyn
    c = _net_case("C6")
    model = _fresh_model(c, dev)
    B, n_future, batch = c["sets"][3]
    want = c["refs"][3]
    b = _with_state_grad(batch, device=dev)
    b["attrs"].requires_grad_()
    loss, parts = gsdyn.dynamics_loss(model, b, n_future=n_future, device_path=True)
    assert parts["device_path"] is False
    g_attrs, = torch.autograd.grad(loss, [b["attrs"]], retain_graph=True)
    got = _grads(model, b, loss)
    b64 = _with_state_grad(batch, dtype=torch.float64)
    b64["attrs"].requires_grad_()
    model64 = gnn_ref.make_model(c["cfg"], 400 + 6).double()
    w_attrs, = torch.autograd.grad(ref.referee_loss(model64, b64, n_future), [b64["attrs"]])
    b32 = _with_state_grad(batch)
    b32["attrs"].requires_grad_()
    h_attrs, = torch.autograd.grad(ref.referee_loss(c["model"], b32, n_future), [b32["attrs"]])
    y_attrs = _distance(h_attrs.double().numpy(), w_attrs.numpy())          # the host fp32 eager autograd's distance: the yardstick
    assert float(g_attrs.abs().max()) > 0 and _distance(g_attrs.cpu().double().numpy(), w_attrs.numpy()) <= FACTOR * y_attrs
    for t in want:
        assert _distance(got[t], want[t]) <= FACTOR * c["y"][t], t


def test_three_adam_steps_on_the_device_and_on_the_host(dev):
    """``train_dynamics_step`` x 3 from the same weights: the host in fp64 (the referee), the host in fp32 (the yardstick: its largest
    relative loss distance from fp64 over the steps) and the device path; the device's losses within 4 yardsticks at every step, and
    falling."""
    import gsdyn
    c = _net_case("C1")
    B, n_future, batch = c["sets"][3]

    def run(model, b, **kw):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        return [float(gsdyn.train_dynamics_step(model, opt, b, n_future=n_future, **kw)) for _ in range(3)]

    l64 = run(_fresh_model(c, "cpu").double(), ref.to(batch, dtype=torch.float64))
    l32 = run(_fresh_model(c, "cpu"), ref.to(batch))
    ldev = run(_fresh_model(c, dev), ref.to(batch, device=dev), device_path=True)
    y = max(abs(a - b) / abs(b) for a, b in zip(l32, l64))
    e = [abs(a - b) / abs(b) for a, b in zip(ldev, l64)]
    _log(f"T2 C1 three Adam steps: fp64 {l64}, host fp32 {l32}, device {ldev}; yardstick {y:.3e}, device distances {e}")
    assert all(x <= FACTOR * y for x in e), (e, y)
    assert ldev[2] < ldev[0] and l64[2] < l64[0]
