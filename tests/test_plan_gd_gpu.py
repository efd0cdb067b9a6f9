"""GPU tests of the gradient planner (csrc/gsr_plan_cost_grad.hip through gsdyn.running_cost_grad; gsdyn.rollout_actions_grad;
gsdyn.plan_actions_gd).

The cost kernel.  Its four values are compared BIT FOR BIT with gsr_plan_cost's.  Its gradients are compared with the numpy fp64 statement
of tests/gd_ref.py on the same fp32 inputs, on inputs where that statement itself decides every minimum, gate and wall with a relative
margin of 1e-5 (asserted; ~40 x the 4 ulp of an fp32 squared distance).  The bound is per element and derived, not tuned:
  chamfer part     a fixed-order fp32 sum of k unit-vector terms is within (k + 8) 2^-24 sum|terms| of the exact sum (k - 1 additions, and
                   8 ulp for a term's own subtraction, root, division and the final scaling); sum|terms| and k come from the fp64 statement;
  collision, box   the forward's stated 1e-5 absolute on their values times the factor sharpness pw / T that multiplies them (gd_ref's
                   ``coef``): the unit vector's few ulp and the last additions vanish beside it;
  an element that receives no term must be exactly zero.
The rollout.  One batched differentiable model call against an fp64 host ``_propagate`` under autograd on the same relations, with the
per-sample ``propagate_split_grad`` as the yardstick (the batched path may be twice as far: test_plan_gpu's own factor); the whole rollout
against the fp64 definition -- relation lists equal, states within test_plan_gpu's rollout bound, gradients within 4 y per tensor, y the
CPU fp32 definition's own relative distance from fp64 on the same case (test_gnn_train_gpu's rule).
The measured distances are appended to plan_gd_parity.log next to the other GPU logs (``GSR_PLAN_GD_PARITY_LOG`` names another file);
profiles/plan_gd_parity.txt is that log of one run."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gd_ref  # noqa: E402
from hipcheck import _ROW_LOG  # noqa: E402
from test_plan_cost_gpu import BOX, _case  # noqa: E402
from test_plan_gd_cpu import BBOX, HAND_CASES, KW, assert_margins, roll_gd_case, roll_margins, still_case  # noqa: E402

_LOG = os.environ.get("GSR_PLAN_GD_PARITY_LOG", os.path.join(os.path.dirname(_ROW_LOG), "plan_gd_parity.log"))
ULP = 2.0 ** -24
FACTOR = 4.0


@pytest.fixture(autouse=True)
def _one_host_thread():
    """The host side of these tests is many small tensor ops (the numpy statement, fp64 referees under autograd); once an earlier test of the
    session has run the C oracle on every core, torch's intra-op pool has that many threads and each small op takes tens of milliseconds on
    a host that grants fewer cores (tests/test_gnn_train_gpu.py explains).  One thread for the duration of a test."""
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
        print(f"(plan_gd_parity.log not written: {e})")


# every value of every axis: n_obj {1, 2, 63, 64, 65, 127, 128, 129, 1024}, M {1, 2, 63, 64, 65, 255, 256, 257, 1025, 4096}, T {1, 2, 3}, B {1, 3, 257}
# -- a subset of test_plan_cost_gpu.COST_CASES; the slice rule changes at 64 / 65 and 128 / 129 particles, the tile at 1024 / 1025 targets.
# Seed 0 (the forward test's inputs) keeps the margins at every one of them: the first seed of a host-side search.
GD_CASES = [(1, 1, 1, 1), (1, 4096, 2, 3), (2, 2, 3, 3), (2, 257, 1, 1), (2, 65, 1, 257), (63, 63, 2, 3), (63, 256, 3, 1), (64, 64, 1, 3), (64, 1, 3, 257),
            (65, 65, 2, 1), (65, 255, 3, 3), (127, 256, 1, 3), (127, 2, 2, 1), (128, 257, 2, 3), (128, 4096, 3, 1), (129, 1025, 2, 3), (1024, 4096, 1, 1),
            (1024, 63, 2, 3), (100, 1000, 3, 3)]

for _axis, _values in enumerate(((1, 2, 63, 64, 65, 127, 128, 129, 1024), (1, 2, 63, 64, 65, 255, 256, 257, 1025, 4096), (1, 2, 3), (1, 3, 257))):
    assert set(_values) <= {c[_axis] for c in GD_CASES}, "GD_CASES must hold every value of every axis"


def _kernel(dev, case, bbox=BOX):
    from diff_gaussian_rasterization import _hip
    from gsdyn import plan
    d = [t.to(dev).contiguous() for t in case]
    out = _hip.plan_cost_grad(*d, plan._box4(bbox, dev, torch.float32), KW["pusher_size"], KW["sharpness"], KW["penalty_weight"])
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _reference(shape, seed=0):
    """The fp64 statement of one case, computed once per process and left unchanged."""
    case = _case(*shape, seed=seed)
    want = gd_ref.cost_grad_ref(*case, BOX.reshape(4), **KW)
    assert_margins(want["margins"], shape)
    return case, want


def _bounds(want):
    k = np.zeros(want["g_state"].shape[:3])
    k[:, -1] = want["terms"]
    b_state = (k[..., None] + 8) * ULP * want["abs_state"] + 1e-5 * want["coef_state"]
    return b_state, 1e-5 * want["coef_act"]


def _in_bounds(got, want, bound):
    """The largest |got - want| as a multiple of the element's bound; an element whose bound is zero must be exactly equal."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    free = bound > 0
    assert (err[~free] == 0).all(), "an element that receives no term is not exactly zero"
    return float((err[free] / bound[free]).max()) if free.any() else 0.0


@pytest.mark.parametrize("n_obj,M,T,B", GD_CASES)
def test_kernel_values_are_the_bits_of_gsr_plan_cost(dev, n_obj, M, T, B):
    from diff_gaussian_rasterization import _hip
    from gsdyn import plan
    case = _case(n_obj, M, T, B)
    r, ch, co, bp, gs, ga = _kernel(dev, case)
    d = [t.to(dev) for t in case]
    w = _hip.plan_cost(*d, plan._box4(BOX, dev, torch.float32), KW["pusher_size"], KW["sharpness"], KW["penalty_weight"])
    for name, a, b in zip(("reward", "chamfer", "collision", "box_pen"), (r, ch, co, bp), w):
        assert torch.equal(a, b), name
    assert gs.shape == (B, T, n_obj, 3) and ga.shape == (B, T, 4)


@pytest.mark.parametrize("n_obj,M,T,B", GD_CASES)
def test_kernel_gradients_against_fp64(dev, n_obj, M, T, B):
    """Per element |g - g64| <= (k + 8) 2^-24 sum|chamfer terms| + 1e-5 sharpness pw / T [where a collision or box gate is open]; exactly zero
    where no term arrives (module docstring)."""
    case, want = _reference((n_obj, M, T, B))
    _, _, _, _, gs, ga = _kernel(dev, case)
    b_state, b_act = _bounds(want)
    e_s = _in_bounds(gs.cpu().numpy(), want["g_state"], b_state)
    e_a = _in_bounds(ga.cpu().numpy(), want["g_actions"], b_act)
    m = want["margins"]
    _log(f"cost grad n_obj={n_obj:4d} M={M:4d} T={T} B={B:3d}: g_state {e_s:.3f}, g_actions {e_a:.3f} of the bound; margins nn {m['nn']:.1e} gate {m['gate']:.1e} "
         f"wall {m['wall']:.1e}; largest |g_state| {np.abs(want['g_state']).max():.3e}")
    assert e_s <= 1.0 and e_a <= 1.0, (e_s, e_a)
    assert np.abs(want["g_state"]).max() > 0


def test_kernel_is_bit_identical_from_run_to_run_and_independent_of_the_batch(dev):
    case = _case(100, 1500, 3, 257, seed=2)
    a, b = _kernel(dev, case), _kernel(dev, case)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.isfinite(a[4]).all() and a[4].abs().max() > 0
    for row in (0, 100, 256):                                   # row b of the B = 257 call = the B = 1 call on sample b, bit for bit
        one = _kernel(dev, (case[0][row:row + 1], case[1][row:row + 1], case[2], case[3]))
        for x, y in zip(a, one):
            assert torch.equal(x[row:row + 1], y), row


@pytest.mark.parametrize("case", HAND_CASES, ids=lambda f: f.__name__)
def test_hand_cases_on_the_device(dev, case, monkeypatch):
    """tests/test_plan_gd_cpu.py's hand cases -- the tie, the coincidence, the gates, the NaN sample -- through the kernel (the torch
    statement is made to raise)."""
    from gsdyn import plan

    def refuse(*a, **k):
        raise AssertionError("the torch statement ran on the device path")
    monkeypatch.setattr(plan, "_running_cost_grad_reference", refuse)
    case(device=dev, dtype=torch.float32)


@pytest.mark.parametrize("n_obj,M,T,B", [(100, 1000, 3, 3), (65, 255, 3, 3), (1024, 63, 2, 3)])
def test_device_path_against_the_torch_statement_on_the_device(dev, n_obj, M, T, B):
    """Both in fp32 on the device; each within the bounds of the fp64 statement, so within twice the bound of each other."""
    from gsdyn import plan
    case, want = _reference((n_obj, M, T, B))
    _, _, _, _, gs, ga = _kernel(dev, case)
    s, a, c, t = [x.to(dev) for x in case]
    s.requires_grad_(True)
    a.requires_grad_(True)
    r, _, _, _ = plan._running_cost_grad_reference(s, a, c, t, plan._box4(BOX, dev, torch.float32), **KW)
    ts, ta = torch.autograd.grad(r.sum(), (s, a))
    b_state, b_act = _bounds(want)
    e_s = _in_bounds(ts.cpu().numpy(), gs.double().cpu().numpy(), 2 * b_state)
    e_a = _in_bounds(ta.cpu().numpy(), ga.double().cpu().numpy(), 2 * b_act)
    _log(f"cost grad vs torch statement on the device n_obj={n_obj} M={M} T={T} B={B}: g_state {e_s:.3f}, g_actions {e_a:.3f} of twice the bound")
    assert e_s <= 1.0 and e_a <= 1.0


def test_the_dispatch_takes_the_kernel_and_the_statement_where_it_must(dev, monkeypatch):
    from diff_gaussian_rasterization import _hip
    from gsdyn import plan, running_cost_grad
    calls = {"kernel": 0, "statement": 0}
    kernel, statement = _hip.plan_cost_grad, plan._running_cost_grad_reference
    monkeypatch.setattr(_hip, "plan_cost_grad", lambda *a, **k: (calls.__setitem__("kernel", calls["kernel"] + 1), kernel(*a, **k))[1])
    monkeypatch.setattr(plan, "_running_cost_grad_reference", lambda *a, **k: (calls.__setitem__("statement", calls["statement"] + 1), statement(*a, **k))[1])

    def run(case, where, dtype, **extra):
        s, a, c, t = [x.to(device=where, dtype=dtype) for x in case]
        s.requires_grad_(True)
        a.requires_grad_(True)
        if extra.get("target_grad"):
            t.requires_grad_(True)
        out = running_cost_grad(s, a, c, t, BOX)
        g = torch.autograd.grad(out["reward_seqs"].sum(), (s, a))
        assert all(torch.isfinite(x).all() for x in g)
        return out
    case = _case(20, 30, 2, 3, seed=4)
    out = run(case, dev, torch.float32)
    assert calls == {"kernel": 1, "statement": 0} and out["reward_seqs"].is_cuda
    direct = _kernel(dev, case)
    assert torch.equal(out["reward_seqs"].detach(), direct[0]) and torch.equal(out["collision"], direct[2])
    calls["kernel"] = 0
    run(case, "cpu", torch.float32)
    run(case, dev, torch.float64)
    run(_case(1025, 3, 1, 1, seed=4), dev, torch.float32)
    run(case, dev, torch.float32, target_grad=True)
    assert calls == {"kernel": 0, "statement": 4}


# ------------------------------------------------------------------------------------------ one batched differentiable model call
def _call_case(B, n_obj, n_his, g):
    hist = torch.rand((B, n_his, n_obj, 3), generator=g) * torch.tensor([0.4, 0.4, 0.05])
    eef = torch.rand((B, n_his, 3), generator=g) * torch.tensor([0.4, 0.4, 0.05])
    delta = torch.cat([(torch.rand((B, 2), generator=g) - 0.5) * 0.05, torch.zeros((B, 1))], 1)
    w = torch.rand((B, n_obj, 3), generator=g) - 0.5
    return hist, eef, delta, w


def _rel(x, want):
    return float((x.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("width", [16, 64])
@pytest.mark.parametrize("B", [1, 2, 65])
def test_one_batched_differentiable_model_call_against_fp64(dev, B, width):
    """The gradient of sum w pred toward the history, the tool rows and the tool's motion.  Referee: ``_propagate`` in fp64 on the host under
    autograd, sample by sample, on the relations the batched call built.  Yardstick: ``propagate_split_grad`` sample by sample on the same
    relations; the batched call -- the same kernels on one block-diagonal graph, other GEMM shapes -- may be twice as far
    (test_plan_gpu.test_one_batched_model_call_against_fp64's factor).  Distances: max |x - x64| / max |x64| per tensor."""
    from gsdyn import plan
    from gsdyn.dynamics import split_graph
    from test_plan_gpu import _model
    n_obj, n_his, thr, topk = 20, 3, 0.15, 5
    R = n_obj + 1
    model = _model(width, seed=width).to(dev)
    m64 = copy.deepcopy(model).double().cpu()
    hist, eef, delta, w = _call_case(B, n_obj, n_his, torch.Generator().manual_seed(B + width))

    def leaves(where, dtype):
        return [x.to(device=where, dtype=dtype).requires_grad_(True) for x in (hist, eef, delta)]
    h, e, d = leaves(dev, torch.float32)
    a, g, n_valid, e_cap = plan._batched_constants(model, B, n_obj, topk, dev)
    states = [torch.cat([h[:, k], e[:, k, None]], 1) for k in range(n_his)]
    pos, (recv, send, cnt, rows) = plan._batched_call_grad(model, states, d, a, g, n_valid, thr, topk, e_cap)
    got = torch.autograd.grad((pos[:, :n_obj] * w.to(dev)).sum(), (h, e, d))
    assert int(cnt.item()) > B * n_obj
    a1, g1, _, _ = plan._sample_constants(model, n_obj, dev, torch.float32)
    rows_h, recv_h, send_h = rows.cpu(), recv.cpu(), send.cpu()
    h64, e64, d64 = leaves("cpu", torch.float64)
    hy, ey, dy = leaves(dev, torch.float32)
    loss64, lossy = 0.0, 0.0
    for b in range(B):
        lo, hi = int(rows_h[b * R]), int(rows_h[(b + 1) * R])
        r_b, s_b = recv_h[lo:hi] - b * R, send_h[lo:hi] - b * R

        def one(hh, ee, dd, where, dtype):
            st = torch.cat([torch.cat([hh[b, k], ee[b, k, None]], 0) for k in range(n_his)], 1)            # [R, 3 n_his]
            act = torch.cat([torch.zeros((n_obj, 3), device=where, dtype=dtype), dd[b, None]], 0)
            return st, act
        st, act = one(h64, e64, d64, "cpu", torch.float64)
        p64, _ = m64._propagate(st, a1.double().cpu(), g1.double().cpu(), act, r_b, s_b)
        loss64 = loss64 + (p64[:n_obj] * w[b].double()).sum()
        st, act = one(hy, ey, dy, dev, torch.float32)
        py, _ = model.propagate_split_grad(st, a1, g1, act, split_graph(r_b.to(dev), s_b.to(dev), R))
        lossy = lossy + (py[:n_obj] * w[b].to(dev)).sum()
    want = torch.autograd.grad(loss64, (h64, e64, d64))
    yard = torch.autograd.grad(lossy, (hy, ey, dy))
    for name, x, y, w64 in zip(("history", "tool rows", "tool motion"), got, yard, want):
        e_b, e_y = _rel(x, w64), _rel(y, w64)
        _log(f"one differentiable call B={B:3d} width={width:3d} {name:<11}: per-sample {e_y:.3e}, batched {e_b:.3e} of the largest gradient (fp64 host referee)")
        assert float(w64.abs().max()) > 0 and e_b <= 2.0 * e_y, (name, e_b, e_y)


# ------------------------------------------------------------------------------------------ the whole rollout
def _distance(x, want):
    n = float(torch.linalg.vector_norm(want))
    d = float(torch.linalg.vector_norm(x.double().cpu() - want))
    return d / n if n > 0 else d


def _roll_grads(model, state, actions, w, kw, **extra):
    from gsdyn import rollout_actions_grad
    a = actions.clone().requires_grad_(True)
    trace = []
    out = rollout_actions_grad(model, state, a, _trace=trace, **extra, **kw)["state_seqs"]
    names = [k for k, _ in model.named_parameters()]
    gs = torch.autograd.grad((out * w).sum(), [a] + [p for _, p in model.named_parameters()])
    return out.detach(), dict(zip(["actions"] + names, gs)), trace


@functools.lru_cache(maxsize=None)
def _roll_reference(detach_steps):
    """The fp64 definition on the host (referee) and the fp32 definition on the host (yardstick), once per process."""
    m64, s64, a64, w64, kw = roll_gd_case(torch.float64)
    m_thr, m_k, m_z, trace = roll_margins(m64, s64, a64, kw)
    assert m_thr >= 1e-3 and m_k >= 1e-3 and m_z >= 1e-3, (m_thr, m_k, m_z)      # the definition ITSELF decides every relation and every lowest z with a margin
    out64, g64, _ = _roll_grads(m64, s64, a64, w64, kw, detach_steps=detach_steps)
    m32, s32, a32, w32, _ = roll_gd_case(torch.float32)
    _, g32, _ = _roll_grads(m32, s32, a32, w32, kw, detach_steps=detach_steps)
    y = {k: _distance(g32[k], g64[k]) for k in g64}
    calls = {(b, li, ai): (recv, send) for b, li, ai, _, recv, send in trace}
    return out64, g64, y, calls, (m_thr, m_k, m_z)


@pytest.mark.parametrize("detach_steps", [False, True])
def test_whole_differentiable_rollout_against_the_fp64_definition(dev, detach_steps):
    from gsdyn import rollout_actions
    from test_plan_gpu import ROLL, ROLL_REPEATS, _one_call_errors
    out64, g64, y, calls, margins = _roll_reference(detach_steps)
    model, state, actions, w, kw = roll_gd_case(torch.float32, dev)
    assert model.split_grad_ok(state)
    out, got, trace = _roll_grads(model, state, actions, w, kw, detach_steps=detach_steps)
    R, seen = ROLL["n_obj"] + 1, 0
    for li, ai, newest, recv, send, cnt in trace:                       # the batched lists, cut per sample, against the definition's
        m = int(cnt.item())
        recv, send = recv[:m].cpu(), send[:m].cpu()
        for b in range(ROLL["B"]):
            if (b, li, ai) not in calls:
                continue                                                # (a call beyond the sample's repeat count: discarded)
            sel = (recv >= b * R) & (recv < (b + 1) * R)
            assert torch.equal(recv[sel] - b * R, calls[(b, li, ai)][0]) and torch.equal(send[sel] - b * R, calls[(b, li, ai)][1]), (b, li, ai)
            seen += 1
    assert seen == sum(sum(r) for r in ROLL_REPEATS)
    # the states: test_plan_gpu's rollout bound -- the per-sample device path's own distance from fp64 for this model, doubled, per model call
    _, _, p_y, _ = _one_call_errors(model, ROLL["B"], ROLL["n_obj"], dev, torch.Generator().manual_seed(11), thr=ROLL["thr"])
    depth = max(sum(r) for r in ROLL_REPEATS)
    err = float((out.double().cpu() - out64).abs().max())
    with torch.no_grad():
        same = torch.equal(out, rollout_actions(model, state, actions, **kw)["state_seqs"])
    _log(f"differentiable rollout detach_steps={detach_steps}: margins thr {margins[0]:.2e} k {margins[1]:.2e} z {margins[2]:.2e}; states max abs error "
         f"{err:.3e}, bound {2.0 * p_y * depth:.3e}; bit-equal to rollout_actions: {same}")
    assert err <= 2.0 * p_y * depth
    bad = {}
    for k in g64:
        e = _distance(got[k], g64[k])
        _log(f"differentiable rollout detach_steps={detach_steps} {k:<40} device {e:.3e} = {e / y[k] if y[k] else float('inf'):.2f} y ({y[k]:.3e})")
        if not e <= FACTOR * y[k]:
            bad[k] = (e, y[k])
    assert float(g64["actions"].abs().max()) > 0 and not bad, bad
    if detach_steps:
        assert float(got["actions"][:, 0].abs().max()) > 0              # the first push still moves the first state


def test_rollout_gradients_are_bit_identical_from_run_to_run(dev):
    """The two GNN kernels' backward sums run in a fixed order; the GEMM library's reductions are observed, not guaranteed, to repeat."""
    model, state, actions, w, kw = roll_gd_case(torch.float32, dev)
    out_a, a, _ = _roll_grads(model, state, actions, w, kw)
    out_b, b, _ = _roll_grads(model, state, actions, w, kw)
    assert torch.equal(out_a, out_b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_refused_models_and_sizes_take_the_definition(dev, monkeypatch):
    from gsdyn import plan
    from test_plan_gpu import ROLL, _model
    model, state, actions, w, kw = roll_gd_case(torch.float32, dev)
    taken = []
    ref_fn, dev_fn = plan._rollout_reference, plan._rollout_device_grad
    monkeypatch.setattr(plan, "_rollout_reference", lambda *a, **k: (taken.append("definition"), ref_fn(*a, **k))[1])
    monkeypatch.setattr(plan, "_rollout_device_grad", lambda *a, **k: (taken.append("device"), dev_fn(*a, **k))[1])
    a = actions.clone().requires_grad_(True)
    odd = _model(18, seed=1, motion_scale=ROLL["motion_scale"]).to(dev)              # nf_effect = 18: the split path refuses
    out = plan.rollout_actions_grad(odd, state, a, **kw)["state_seqs"]
    (g,) = torch.autograd.grad((out * w).sum(), a)
    assert taken == ["definition"] and out.is_cuda and torch.isfinite(g).all() and float(g.abs().max()) > 0
    with pytest.raises(RuntimeError, match="device path"):
        plan.rollout_actions_grad(odd, state, a, device_path=True, **kw)
    big = (torch.rand((128, 3), generator=torch.Generator().manual_seed(2)) * 0.5).to(dev)
    out = plan.rollout_actions_grad(model, big, a[:1, :1], **kw)["state_seqs"]
    assert taken == ["definition", "definition"] and out.shape == (1, 1, 128, 3) and out.requires_grad
    plan.rollout_actions_grad(model, state, a, **kw)
    plan.rollout_actions_grad(model, state, a, device_path=False, **kw)
    assert taken == ["definition", "definition", "device", "definition"]


# ------------------------------------------------------------------------------------------ plan_actions_gd
def test_plan_actions_gd_on_the_device_picks_what_the_cpu_picks(dev):
    """Width-16 model, 12 particles, 8 candidates from ONE CPU generator (the sampler draws on the generator's device), T = 2.  The referee is
    the same call on CPU tensors in fp64; its top two iteration-0 rewards differ by more than 1e-2 (asserted), ten times the 1e-3 within
    which the device's rewards must lie (test_plan_cost_gpu's end-to-end bound: rollout error times the chamfer's slope, cost bounds)."""
    from gsdyn import plan_actions_gd, rollout_actions, running_cost, sample_action_seq
    from test_plan_cost_cpu import LOWER, UPPER, plan_case
    model, state, target, seq0, kw = plan_case()
    kw.pop("chunk")
    seed = kw["generator"].initial_seed()
    drawn = sample_action_seq(seq0, LOWER, UPPER, 8, iter_index=0, noise_level=1.0, push_length=0.05, generator=torch.Generator().manual_seed(seed))
    m64 = copy.deepcopy(model).double()
    out64 = rollout_actions(m64, state.double(), drawn.double(), push_length=0.05, adj_thresh=0.12)["state_seqs"]
    r64 = running_cost(out64, drawn.double(), state.double(), target.double(), BBOX)["reward_seqs"]
    top = r64.sort(descending=True).values
    assert float(top[0] - top[1]) > 1e-2, "the seed has a near-tie"
    best = int(torch.argmax(r64))
    model_d, state_d, target_d, seq0_d, kw_d = plan_case(device=dev)
    kw_d.pop("chunk")
    one = plan_actions_gd(model_d, state_d, target_d, BBOX, seq0_d, n_update_iter=1, rollout_best=False, **kw_d)
    torch.cuda.synchronize()
    assert torch.equal(one["act_seq"].cpu(), drawn[best])                            # the initial samples are the CPU call's, and the same one wins
    assert abs(float(one["reward_history"][0]) - float(r64[best])) <= 1e-3
    kw_d["generator"] = torch.Generator().manual_seed(seed)
    res = plan_actions_gd(model_d, state_d, target_d, BBOX, seq0_d, n_update_iter=3, lr=1e-4, **kw_d)
    _log(f"plan_actions_gd: fp64 best initial reward {float(r64[best]):.6f}, device {float(one['reward_history'][0]):.6f}; three iterations {res['reward_history'].tolist()}")
    h = res["reward_history"]
    assert res["act_seq"].is_cuda and h.shape == (3,) and (h[1:] >= h[:-1]).all()
    fresh = rollout_actions(model_d, state_d, res["act_seq"][None], push_length=0.05, adj_thresh=0.12)["state_seqs"]
    assert torch.equal(fresh[0], res["state_seqs"])
    assert float(running_cost(fresh, res["act_seq"][None], state_d, target_d, BBOX)["reward_seqs"][0]) == float(res["reward"])


def test_plan_actions_gd_on_the_device_lowers_the_collision_term(dev):
    from gsdyn import plan_actions_gd, running_cost
    model, state, target, seq0, init, kw = still_case(device=dev)
    for b in range(3):
        res = plan_actions_gd(model, state, target, BBOX, seq0, n_update_iter=11, lr=1e-3, init=init[b:b + 1], **kw)
        h = res["reward_history"]
        assert h.shape == (11,) and (h[1:] > h[:-1]).all(), h
        assert torch.equal(res["act_seq"][:, 3], init[b, :, 3])
        frames = state[None, None].expand(1, 2, -1, -1).contiguous()
        before = running_cost(frames, init[b:b + 1], state, target, BBOX)
        after = running_cost(res["state_seqs"][None], res["act_seq"][None], state, target, BBOX)
        assert float(after["collision"].mean()) < float(before["collision"].mean())
