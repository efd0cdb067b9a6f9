"""GPU tests of the rigid-alignment loss (csrc/gsr_rigid_fit.hip, gsdyn.umeyama_fit, ``rigid_weight`` of gsdyn.dynamics_loss).

Part one: the kernel against the numpy fp64 referee (tests/rigid_fit_ref.py) at every lane-stride edge (N in {1, 2, 3, 63, 64, 65, 129,
257}; a lane walks rows lane, lane + 64, ...) and B in {1, 2, 65}, every cloud kind at each.  The bars are rigid_fit_ref.bars with
eps_store = 2^-24: one fp32 rounding of the stored value plus the referee's conditioning term, residual relative to max |Y|; ``code`` and
``count`` exact; every non-degenerate sample is asserted to have s1 / (s2 + s3) <= 1e4, so none escapes the bars.  Then the contract:
a NaN stays in its sample, a sample does not depend on its batch, two runs agree bit for bit, the wrapper's errors, empty shapes.
Part two: ``dynamics_loss(..., rigid_weight=0.05)`` on the device against the dense fp64 evaluation at two configurations of
gnn_ref.CONFIGS (C1: three history frames and the tool; C4: n_his = 1), B in {1, 3} x n_future in {1, 2}, under the rule of
tests/test_gnn_train_gpu.py: per tensor within 4 x the HOST fp32 eager path's distance from fp64, taken with the same term on.  The
measured distances are appended to rigid_loss_parity.log next to gnn_train_parity.log (``GSR_RIGID_PARITY_LOG`` names another file);
profiles/rigid_loss_parity.txt is that log of one run."""
import functools
import os

import numpy as np
import pytest
import torch

import gnn_bwd_ref
import gnn_ref
import rigid_fit_ref as ref
from hipcheck import _ROW_LOG
from test_gnn_train_gpu import FACTOR, N_OBJ, SETS, _distance, _fresh_model, _grads, _with_state_grad

pytestmark = pytest.mark.gpu

_LOG = os.environ.get("GSR_RIGID_PARITY_LOG", os.path.join(os.path.dirname(_ROW_LOG), "rigid_loss_parity.log"))
EPS32 = 2.0 ** -24


@pytest.fixture(autouse=True)
def _one_host_thread():
    """As in tests/test_gnn_train_gpu.py: the host side is many small tensor ops; one intra-op thread for the duration of a test."""
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
        print(f"(rigid_loss_parity.log not written: {e})")


def _run(dev, X, Y, mask):
    from diff_gaussian_rasterization import _hip
    out = _hip.rigid_fit(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), torch.from_numpy(mask).to(dev))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    return all(a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint32 if a[k].itemsize == 4 else np.uint8),
                                                           b[k].view(np.uint32 if b[k].itemsize == 4 else np.uint8)) for k in a)


# ========================================================================================== part one: the kernel
@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 129, 257])
def test_kernel_against_the_fp64_referee(dev, N, B):
    kinds_seen, worst = set(), {}
    for seed in range(-(-len(ref.KINDS) // B)):                     # enough batches for every kind to appear
        X, Y, mask, names = ref.make_batch(B, N, B * seed)
        want = ref.fit(X, Y, mask)
        got = _run(dev, X, Y, mask)
        assert got["R"].shape == (B, 3, 3) and got["t"].shape == (B, 1, 3) and got["aligned"].shape == (B, N, 3)
        assert all(got[k].dtype == np.float32 for k in ("R", "t", "aligned", "residual", "sse")) and got["code"].dtype == np.int32
        # bars: eps_store |value| (one fp32 rounding of the stored value; residual: eps_store max |Y|) + the conditioning term
        # (16 + 2 n) 2^-53 s1 / (s2 + s3) x the sample's scale -- rigid_fit_ref.bars; code and count exact; cond <= 1e4 asserted inside
        w = ref.check(got, want, X, Y, mask, EPS32, tag=(N, B, seed))
        worst = {k: max(worst.get(k, 0.0), v) for k, v in w.items()}
        kinds_seen |= set(names)
        for b, k in enumerate(names):
            assert want["code"][b] == (1 if (k in ref.DEGENERATE or N < 3) else 0), (k, N)
    assert kinds_seen == set(ref.KINDS)
    _log(f"K1 N {N:>3} B {B:>2}: worst error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_a_nan_stays_in_its_sample(dev):
    X, Y, mask, _ = ref.make_batch(5, 70, 2, kinds=("noised", "holes", "planar"))
    mask[1, 68], mask[3, 6] = True, False
    clean = _run(dev, X, Y, mask)
    Yn = Y.copy()
    Yn[1, 68, 2] = np.nan                    # a masked row behind the first lane stride: sample 1 is NaN
    Yn[3, 6, 0] = np.inf                     # an unmasked row: the fit does not see it
    got = _run(dev, X, Yn, mask)
    ref.check(got, ref.fit(X, Yn, mask), X, Yn, mask, EPS32, tag="nan")
    for k in ("R", "t", "aligned", "sse"):
        assert np.isnan(got[k][1]).all(), k
    assert np.isnan(got["residual"][1][mask[1]]).all() and not got["residual"][1][~mask[1]].any() and got["code"][1] == 1
    others = [0, 2, 3, 4]
    assert _same({k: v[others] for k, v in got.items()}, {k: v[others] for k, v in clean.items()})


def test_a_sample_does_not_depend_on_its_batch_and_runs_repeat(dev):
    X, Y, mask, _ = ref.make_batch(65, 129, 4)
    a, b = _run(dev, X, Y, mask), _run(dev, X, Y, mask)
    assert _same(a, b)                                                           # two runs: identical bits
    for s in (0, 7, 33, 64):
        alone = _run(dev, X[s:s + 1].copy(), Y[s:s + 1].copy(), mask[s:s + 1].copy())
        assert _same(alone, {k: v[s:s + 1] for k, v in a.items()}), s


def test_wrapper_errors_and_empty_shapes(dev):
    import gsdyn
    from diff_gaussian_rasterization import _hip
    X, Y, mask, _ = ref.make_batch(3, 10, 1)
    x, y, m = (torch.from_numpy(v).to(dev) for v in (X, Y, mask))
    wide = torch.cat([x, x], 2)
    for bad in ((x.double(), y.double(), m), (x, y, m.to(torch.uint8)), (x.cpu(), y.cpu(), m.cpu()), (x, y.cpu(), m), (wide[:, :, :3], y, m),
                (x, y[:, :5], m), (x, y, m[:, :5]), (x[0], y[0], m[0]), (x, y, None)):
        with pytest.raises(ValueError):
            _hip.rigid_fit(*bad)
    with pytest.raises(ValueError):
        gsdyn.umeyama_fit(wide[:, :, :3], y, m, kernel=True)
    # the public function routes: the view and fp64 take the torch statement, the contiguous fp32 tensors the kernel (same bits as the wrapper)
    via = gsdyn.umeyama_fit(x, y, m)
    assert _same({k: v.cpu().numpy() for k, v in via.items()}, _run(dev, X, Y, mask))
    want = ref.fit(X, Y, mask)
    for args in ((wide[:, :, :3], y, m), (x.double(), y.double(), m)):
        got = gsdyn.umeyama_fit(*args)
        assert got["R"].dtype == args[0].dtype and got["R"].device == x.device
        assert np.abs(got["R"].cpu().double().numpy() - want["R"]).max() <= 64 * EPS32 * ref.condition(want["sigma"]).max()
    for B, N in ((0, 5), (4, 0), (0, 0)):
        out = _hip.rigid_fit(torch.zeros((B, N, 3), device=dev), torch.zeros((B, N, 3), device=dev), torch.zeros((B, N), dtype=torch.bool, device=dev))
        assert out["aligned"].shape == (B, N, 3) and out["residual"].shape == (B, N, 3) and out["t"].shape == (B, 1, 3)
        assert torch.equal(out["R"], torch.eye(3, device=dev).expand(B, 3, 3)) and not out["t"].any() and not out["sse"].any()
        assert not out["count"].any() and bool((out["code"] == 1).all()) and out["code"].dtype == torch.int32 and out["sse"].shape == (B,)


# ========================================================================================== part two: the loss term
RIGID, LENGTH = 0.05, 0.05


def _referee_loss(model, batch, n_future):
    """gnn_bwd_ref.referee_loss's loop with the rigid term: per step also RIGID x mse(pred[mask], aligned[mask]), the alignment of the oldest
    history frame's object rows to the prediction by the numpy fp64 referee, held fixed."""
    state, action, mask = batch["state"], batch.get("action"), batch["obj_mask"]
    Rr, Rs = batch["Rr"], batch["Rs"]
    loss = 0.0
    for fi in range(n_future):
        gt = batch["state_future"][:, fi]
        n_p = gt.shape[1]
        pred = model(state=state, attrs=batch["attrs"], p_instance=batch["p_instance"], action=action, Rr=Rr, Rs=Rs)[0][:, :n_p]
        D = Rr[:, :, :n_p] - Rs[:, :, :n_p]
        len_pred = torch.norm(torch.matmul(D, pred), dim=-1)
        len_old = torch.norm(torch.matmul(D, state[:, 0, :n_p].detach()), dim=-1)
        fit = ref.fit(state[:, 0, :n_p].detach().numpy(), pred.detach().numpy(), mask.numpy())
        aligned = torch.from_numpy(fit["aligned"]).to(pred.dtype)
        loss = (loss + ((pred - gt) ** 2).mean() + LENGTH * ((len_pred - len_old) ** 2).mean()
                + RIGID * torch.nn.functional.mse_loss(pred[mask], aligned[mask]))
        if fi < n_future - 1:
            newest = torch.cat([pred, batch["tool_future"][:, fi, n_p:]], 1)
            state = torch.cat([state[:, 1:], newest[:, None]], 1)
            action = batch["action_future"][:, fi]
    return loss


def _with_mask(batch, k):
    """The dataset's ``obj_mask`` for a batch of gnn_bwd_ref.make_batch: every object row real but a few, holes included."""
    B = batch["state"].shape[0]
    mask = torch.ones((B, N_OBJ), dtype=torch.bool)
    mask[0, N_OBJ - 6:] = False
    for b in range(B):
        mask[b, [3 + b, 17, 30 - k]] = False
    return dict(batch, obj_mask=mask)


def _to(batch, device=None, dtype=None):
    out = _with_state_grad({k: v for k, v in batch.items() if k != "obj_mask"}, device=device, dtype=dtype)
    out["obj_mask"] = batch["obj_mask"].to(device=device)
    return out


@functools.lru_cache(maxsize=None)
def _net_case(name):
    """One configuration, built once per process and left unchanged: the host fp32 model, its input sets, the fp64 referee's loss and
    gradients per set, and per tensor the yardstick: the HOST fp32 eager path's (``dynamics_loss(device_path=False)`` on the CPU, the
    term on) largest relative distance from fp64 over the sets."""
    import gsdyn
    kw = dict(gnn_ref.CONFIGS[name])
    instances = kw.pop("instances", 1)
    cfg = gnn_ref.base_cfg(**kw)
    idx = int(name[1:])
    model = gnn_ref.make_model(cfg, 400 + idx)
    model64 = gnn_ref.make_model(cfg, 400 + idx).double()
    sets, refs, y = [], [], {}
    for k, (B, n_future) in enumerate(SETS):
        batch = _with_mask(gnn_bwd_ref.make_batch(cfg, instances, B, N_OBJ, n_future, 500 + 10 * idx + k), k)
        b64 = _to(batch, dtype=torch.float64)
        want = _grads(model64, b64, _referee_loss(model64, b64, n_future))
        b32 = _to(batch)
        loss32, parts = gsdyn.dynamics_loss(model, b32, n_future=n_future, length_weight=LENGTH, rigid_weight=RIGID, device_path=False)
        assert parts["device_path"] is False and float(parts["rigid"]) > 0
        eager = _grads(model, b32, loss32)
        for t in want:
            y[t] = max(y.get(t, 0.0), _distance(eager[t], want[t]))
        sets.append((B, n_future, batch))
        refs.append(want)
    return dict(name=name, cfg=cfg, model=model, sets=sets, refs=refs, y=y)


def _device_grads(model, batch, n_future, dev):
    import gsdyn
    b = _to(batch, device=dev)
    loss, parts = gsdyn.dynamics_loss(model, b, n_future=n_future, length_weight=LENGTH, rigid_weight=RIGID, device_path=True)
    assert parts["device_path"] is True and set(parts) == {"mse", "length", "rigid", "device_path"}
    return _grads(model, b, loss), parts


@pytest.mark.parametrize("name", ["C1", "C4"])
def test_rigid_loss_on_the_device_against_fp64(dev, name, monkeypatch):
    """Loss, d loss / d state and every parameter gradient within 4 yardsticks of the dense fp64 evaluation, the yardstick being the host
    fp32 eager path's distance with the same term on.  The models and input sets use the seeds of tests/test_gnn_train_gpu.py, at which
    that yardstick is 5e-8 .. 4e-7 for every tensor of both configurations (asserted below: no tensor's bar is looser than 4 x 1e-6; an input
    set on which the fp32 network itself sits at a ReLU edge would give a yardstick of 1e-4 .. 1e-3 and a bar that a wrong rigid gradient
    could pass).  Every alignment of the device path must come from the kernel, none from the torch statement: the calls are counted."""
    from diff_gaussian_rasterization import _hip
    import gsdyn.rigid_fit
    calls = {"kernel": 0, "torch": 0}
    real_kernel, real_torch = _hip.rigid_fit, gsdyn.rigid_fit.umeyama_fit_torch
    monkeypatch.setattr(_hip, "rigid_fit", lambda *a: (calls.__setitem__("kernel", calls["kernel"] + 1), real_kernel(*a))[1])
    monkeypatch.setattr(gsdyn.rigid_fit, "umeyama_fit_torch", lambda *a: (calls.__setitem__("torch", calls["torch"] + 1), real_torch(*a))[1])
    c = _net_case(name)
    model = _fresh_model(c, dev)
    calls.update(kernel=0, torch=0)                                   # (_net_case's eager yardstick runs the torch statement)
    assert max(c["y"].values()) <= 1e-6, c["y"]
    worst = {}
    for (B, n_future, batch), want in zip(c["sets"], c["refs"]):
        got, parts = _device_grads(model, batch, n_future, dev)
        again, _ = _device_grads(model, batch, n_future, dev)
        for t in want:
            worst[t] = max(worst.get(t, 0.0), _distance(got[t], want[t]))
            assert np.array_equal(got[t].view(np.uint64), again[t].view(np.uint64)), (t, B, n_future)      # two runs: identical bits
    assert calls == {"kernel": 2 * sum(n_future for _, n_future, _ in c["sets"]), "torch": 0}, calls
    for t in worst:
        _log(f"T1 {name:>3} {t:<40} device {worst[t]:.3e} = {worst[t] / c['y'][t] if c['y'][t] else float('inf'):.2f} y ({c['y'][t]:.3e})")
    bad = {t: (worst[t], c["y"][t]) for t in worst if not worst[t] <= FACTOR * c["y"][t]}
    assert not bad, (name, bad)


def test_train_step_with_all_three_weights(dev):
    import gsdyn
    c = _net_case("C1")
    B, n_future, batch = c["sets"][3]
    model = _fresh_model(c, dev)
    b = _to(batch, device=dev)
    b["state"] = b["state"].detach()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = [float(gsdyn.train_dynamics_step(model, opt, b, n_future=n_future, mse_weight=1.0, length_weight=LENGTH, rigid_weight=RIGID,
                                              device_path=True)) for _ in range(3)]
    _log(f"T2 C1 three Adam steps with mse 1, length {LENGTH}, rigid {RIGID} on the device: {losses}")
    assert all(np.isfinite(losses)) and losses[2] < losses[0]
