"""CPU tests of the rigid-alignment loss: the torch statement of gsdyn.umeyama_fit against the numpy fp64 referee (tests/rigid_fit_ref.py)
on every cloud kind, against the reference's own recorded numbers (tests/golden/rigid_loss_ref.npz: its ``rigid_loss`` and
``umeyama_algorithm`` run once on the CPU in fp32), the loss term of ``dynamics_loss`` against a direct autograd evaluation, and the
unchanged defaults."""
import os

import numpy as np
import pytest
import torch

import dyn_batch_ref
import rigid_fit_ref as ref


def _np(out):
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def _fit64(X, Y, mask, **kw):
    import gsdyn
    return _np(gsdyn.umeyama_fit(torch.from_numpy(X).double(), torch.from_numpy(Y).double(), torch.from_numpy(mask), **kw))


@pytest.mark.parametrize("N", [1, 2, 3, 12, 65, 257])
def test_torch_statement_against_the_referee(N):
    """Every kind of cloud (rotated + noised, planar, mirrored, nearly a half turn, X == Y, far from the origin, masks with holes, 0 - 3
    masked rows, collinear) in fp64: both sides compute in fp64, so the bars are rigid_fit_ref.bars with eps_store = 0."""
    X, Y, mask, names = ref.make_batch(2 * len(ref.KINDS), N, 3)
    want = ref.fit(X, Y, mask)
    worst = ref.check(_fit64(X, Y, mask), want, X, Y, mask, 0.0, tag=N)
    print(f"N = {N}: worst error / bar {worst}; codes {dict(zip(names, want['code'].tolist()))}")
    for b, k in enumerate(names):
        if k in ref.DEGENERATE or N < 3:
            assert want["code"][b] == 1, (k, N)
            if k == "n0":
                assert want["count"][b] == 0 and want["sse"][b] == 0 and np.array_equal(want["R"][b], np.eye(3)) and not want["t"][b].any()
            elif ref.DEGENERATE.get(k) is not None:
                assert want["count"][b] == min(ref.DEGENERATE[k], N)
        elif N >= 12:
            assert want["code"][b] == 0, (k, N)
        if want["code"][b] == 0:
            assert abs(np.linalg.det(want["R"][b]) - 1.0) < 1e-12           # a proper rotation, the mirrored cloud included
    if N >= 12:
        assert {"noised", "planar", "mirror", "near_pi", "same", "far", "holes", "n3"} <= {k for b, k in enumerate(names) if want["code"][b] == 0}


def test_float32_cpu_tensors_and_views_take_the_torch_statement():
    """fp32 on the CPU and a non-contiguous view: the torch statement in that dtype; within fp32 rounding x conditioning of the referee."""
    import gsdyn
    X, Y, mask, _ = ref.make_batch(4, 24, 11, kinds=("noised", "planar", "mirror", "holes"))
    want = ref.fit(X, Y, mask)
    wide = torch.from_numpy(np.concatenate([X, X], 2))
    for x in (torch.from_numpy(X), wide[:, :, :3]):
        got = gsdyn.umeyama_fit(x, torch.from_numpy(Y), torch.from_numpy(mask))
        assert got["R"].dtype == torch.float32 and got["code"].dtype == torch.int32 and got["count"].dtype == torch.int32
        assert got["t"].shape == (4, 1, 3) and not got["R"].requires_grad
        tol = 64 * 2.0 ** -24 * ref.condition(want["sigma"]).max()
        assert np.abs(got["R"].numpy() - want["R"]).max() <= tol
    with pytest.raises(ValueError):
        gsdyn.umeyama_fit(torch.from_numpy(X), torch.from_numpy(Y), torch.from_numpy(mask), kernel=True)       # CPU tensors: no kernel
    with pytest.raises(ValueError):
        gsdyn.umeyama_fit(torch.from_numpy(X), torch.from_numpy(Y)[:, :5], torch.from_numpy(mask))
    with pytest.raises(ValueError):
        gsdyn.umeyama_fit(torch.from_numpy(X), torch.from_numpy(Y), torch.from_numpy(mask).float())


def test_non_finite_sample_is_nan_and_alone():
    X, Y, mask, _ = ref.make_batch(5, 20, 2, kinds=("noised", "holes"))
    mask[1, 4], mask[3, 6] = True, False
    clean = _fit64(X, Y, mask)
    Yn = Y.copy()
    Yn[1, 4, 2] = np.nan                     # a masked row: sample 1 is NaN
    Yn[3, 6, 0] = np.inf                     # an unmasked row: nothing happens to the fit
    got = _fit64(X, Yn, mask)
    ref.check(got, ref.fit(X, Yn, mask), X, Yn, mask, 0.0, tag="nan")
    for k in ("R", "t", "aligned", "sse"):
        assert np.isnan(got[k][1]).all(), k
    assert np.isnan(got["residual"][1][mask[1]]).all() and not got["residual"][1][~mask[1]].any() and got["code"][1] == 1
    for b in (0, 2, 3, 4):
        for k in ("R", "t", "aligned", "residual", "sse", "count", "code"):
            assert np.array_equal(got[k][b], clean[k][b]), (b, k)


def test_reference_recording(golden_dir):
    """The reference's rigid_loss / umeyama_algorithm(fixed_scale=True), recorded once in fp32 on the CPU (B = 3, N = 12, full rank), against
    the torch statement in fp64.  Tolerance: 4 x the recording's own distance from the fp64 referee (the yardstick rule of
    tests/test_gnn_train_gpu.py) -- the recording is an fp32 computation, the statement an fp64 one."""
    g = np.load(os.path.join(golden_dir, "rigid_loss_ref.npz"))
    X, Y, mask = g["X"], g["Y"], g["mask"]
    assert X.shape == (3, 12, 3) and X.dtype == np.float32 and mask.dtype == bool
    want = ref.fit(X, Y, mask)
    assert not want["code"].any() and ref.condition(want["sigma"]).max() < 10
    want_loss = want["sse"].sum() / (3 * want["count"].sum())
    y = dict(R=np.abs(g["R"] - want["R"]).max(), t=np.abs(g["t"] - want["t"]).max(), loss=abs(float(g["loss"]) - want_loss))
    got = _fit64(X, Y, mask)
    e = dict(R=np.abs(got["R"] - g["R"]).max(), t=np.abs(got["t"] - g["t"]).max(),
             loss=abs(got["sse"].sum() / (3 * got["count"].sum()) - float(g["loss"])))
    print(f"recording's distance from the fp64 referee (yardstick) {y}; the fp64 statement's distance from the recording {e}")
    for k in y:
        assert y[k] > 0 and e[k] <= 4 * y[k], (k, e[k], y[k])


# ------------------------------------------------------------------------------------------------------------------- the loss term
def _model_and_batch(dense=True):
    import gsdyn
    from gsdyn.dynamics import DynamicsPredictor
    arr, kw = dyn_batch_ref.make_case(6, B=3, P=100, n_his=3, n_future=2, max_nobj=20, topk=5, connect_all=True)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x  # noqa: E731
    k = {n: t(v) for n, v in kw.items()}
    k["dense"] = dense
    batch = gsdyn.make_dynamics_batch(*(t(arr[n]) for n in ("particles", "eef", "pairs")), **k)
    torch.manual_seed(0)
    model = DynamicsPredictor(dict(nf_particle=16, nf_relation=16, nf_effect=16, attr_dim=2, state_dim=0, action_dim=3, pstep=2, rel_attr_dim=2,
                                   rel_group_dim=1, rel_distance_dim=3, n_his=3))
    return model, batch


def _direct_rigid(model, batch, n_future):
    """sum over the steps of mse(pred[mask], aligned.detach()[mask]), the alignment by the numpy referee: the reference's rigid_loss."""
    from gsdyn.dyn_train import _dense_relations, _next_history
    state, action, mask = batch["state"], batch["action"], batch["obj_mask"]
    Rr, Rs = _dense_relations(batch)
    total = 0.0
    for fi in range(n_future):
        n_p = batch["state_future"].shape[2]
        pred = model(state=state, attrs=batch["attrs"], p_instance=batch["p_instance"], action=action, Rr=Rr, Rs=Rs)[0][:, :n_p]
        fit = ref.fit(state[:, 0, :n_p].detach().numpy(), pred.detach().numpy(), mask.numpy())
        aligned = torch.from_numpy(fit["aligned"]).to(pred.dtype)
        total = total + torch.nn.functional.mse_loss(pred[mask], aligned[mask])
        if fi < n_future - 1:
            state, action = _next_history(state, pred, batch["tool_future"][:, fi]), batch["action_future"][:, fi]
    return total


def test_loss_term_against_a_direct_autograd_evaluation():
    """In fp64 (model and batch), so that the two evaluations of the same term agree to rounding: loss, the term, parameter gradients."""
    import gsdyn
    model, batch = _model_and_batch()
    model = model.double()
    batch = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}
    assert batch["obj_mask"].dtype == torch.bool and 0 < int(batch["obj_mask"].sum()) < batch["obj_mask"].numel()
    params = list(model.parameters())
    base, _ = gsdyn.dynamics_loss(model, batch, n_future=2, length_weight=0.05, device_path=False)
    g_base = torch.autograd.grad(base, params)
    loss, parts = gsdyn.dynamics_loss(model, batch, n_future=2, length_weight=0.05, rigid_weight=0.05, device_path=False)
    g_loss = torch.autograd.grad(loss, params)
    direct = 0.05 * _direct_rigid(model, batch, 2)
    g_direct = torch.autograd.grad(direct, params)
    assert set(parts) == {"mse", "length", "rigid", "device_path"} and float(parts["rigid"]) > 0 and not parts["rigid"].requires_grad
    assert abs(float(parts["rigid"]) - float(direct.detach())) <= 1e-9 * float(direct.detach())
    assert abs(float(loss.detach()) - float(base.detach()) - float(direct.detach())) <= 1e-12 * abs(float(loss.detach()))
    num = sum(float(((a - b - c) ** 2).sum()) for a, b, c in zip(g_loss, g_base, g_direct))
    den = sum(float((c ** 2).sum()) for c in g_direct)
    print(f"rigid term {float(direct.detach()):.6e}, gradient distance {(num / den) ** 0.5:.3e}")
    assert den > 0 and (num / den) ** 0.5 <= 1e-9, (num, den)


def test_train_step_takes_the_three_weights_and_missing_mask_raises():
    import gsdyn
    model, batch = _model_and_batch(dense=False)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = [float(gsdyn.train_dynamics_step(model, opt, batch, n_future=2, mse_weight=1.0, length_weight=0.05, rigid_weight=0.05)) for _ in range(3)]
    assert all(np.isfinite(losses)) and losses[2] < losses[0]
    del batch["obj_mask"]
    with pytest.raises(ValueError):
        gsdyn.dynamics_loss(model, batch, n_future=2, rigid_weight=0.05)
    gsdyn.dynamics_loss(model, batch, n_future=2)                       # without the term the mask is not needed


def test_default_weight_changes_nothing():
    import gsdyn
    model, batch = _model_and_batch()
    a, pa = gsdyn.dynamics_loss(model, batch, n_future=2)
    b, pb = gsdyn.dynamics_loss(model, batch, n_future=2, rigid_weight=0.0)
    assert torch.equal(a, b) and set(pa) == set(pb) == {"mse", "length", "device_path"}
    ga, gb = torch.autograd.grad(a, list(model.parameters())), torch.autograd.grad(b, list(model.parameters()))
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))
    want = a.detach()
    # the two-term loss restated: what the call returned before the term existed
    from gsdyn.dyn_train import _eager_loss
    mse, length = _eager_loss(model, batch, 2, 1.0, 0.01)[:2]
    assert torch.equal(want, (mse + length).detach())
