"""CPU tests of the gradient planner (gsdyn/plan.py ``running_cost_grad``, ``rollout_actions_grad``, ``plan_actions_gd``;
csrc/gsr_plan_cost_grad.hip): the exported symbol and its argument checks; the torch statement of the cost's gradient against the numpy fp64
statement of tests/gd_ref.py, against central differences and against hand-computed cases (which tests/test_plan_gd_gpu.py runs again on the
device); the differentiable rollout against central differences; and the planner's loop."""
import math
import os
import re

import numpy as np
import pytest
import torch

import gd_ref
from test_plan_cost_cpu import BBOX, LOWER, UPPER, _model, plan_case
from test_plan_cost_gpu import BOX, _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(pusher_size=0.01, sharpness=100.0, penalty_weight=5.0)
MARGIN = 1e-5        # every discrete decision of the fp64 statement keeps this (relative): ~40 x the 4 ulp of an fp32 squared distance


def test_symbol_is_exported_and_declared_and_the_abi_is_125():
    from diff_gaussian_rasterization import _hip
    import ctypes
    import gsdyn
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_plan_cost_grad" in _hip.EXPORTS and re.search(r"^int gsr_plan_cost_grad\(", header, re.M)
    assert re.search(r"#define GSR_VERSION 125\b", header)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert lib.gsr_version() == 125
    getattr(lib, "gsr_plan_cost_grad")
    for name in ("running_cost_grad", "rollout_actions_grad", "plan_actions_gd"):
        assert callable(getattr(gsdyn, name))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """gsr_plan_cost's refusals: -2 with a text, nothing launched.  Every pointer is a real buffer large enough for the refused call."""
    from diff_gaussian_rasterization import _hip
    import ctypes as C
    lib = _hip.load_library()
    where = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    B, T, n_obj, big, M = 3, 2, 12, 1025, 7
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=where)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    seqs, acts, cur, tgt, box = f32(B * T * big * 3), f32(B * T * 4), f32(big * 3), f32(M * 3), f32(4)
    rew, ch, co, bp, gs, ga = f32(B), f32(B), f32(B * T), f32(B * T), f32(B * T * big * 3), f32(B * T * 4)

    def call(b, t, n, m, s=seqs, g=gs):
        return lib.gsr_plan_cost_grad(b, t, n, m, p(s), p(acts), p(cur), p(tgt), p(box), 0.01, 100.0, 5.0, p(rew), p(ch), p(co), p(bp), p(g), p(ga), None)
    assert call(0, T, n_obj, M) == -2 and b"B, T, M >= 1" in lib.gsr_last_error()
    assert call(B, 0, n_obj, M) == -2 and b"T = 0" in lib.gsr_last_error()
    assert call(B, T, n_obj, 0) == -2 and b"M = 0" in lib.gsr_last_error()
    assert call(B, T, big, M) == -2 and b"n_obj <= 1024" in lib.gsr_last_error()
    assert call(B, T, 0, M) == -2
    assert call(B, T, n_obj, M, None) == -2 and b"NULL" in lib.gsr_last_error()
    assert call(B, T, n_obj, M, seqs, None) == -2 and b"NULL" in lib.gsr_last_error()
    assert call(1 << 20, 1 << 10, n_obj, M) == -2 and b"2^31" in lib.gsr_last_error()
    assert call(B, T, n_obj, 1 << 30) == -2 and b"2^31" in lib.gsr_last_error()
    if where.type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the torch statement
def _grads(case, bbox=BOX, device="cpu", dtype=torch.float64, **kw):
    """running_cost_grad on ``case`` -> (dict of values, g_state, g_actions) with d_reward = 1 for every sample."""
    from gsdyn import running_cost_grad
    s, a, c, t = [x.to(device=device, dtype=dtype) for x in case]
    s.requires_grad_(True)
    a.requires_grad_(True)
    out = running_cost_grad(s, a, c, t, bbox, **{**KW, **kw})
    gs, ga = torch.autograd.grad(out["reward_seqs"].sum(), (s, a))
    return out, gs, ga


def test_values_on_cpu_equal_running_cost():
    from gsdyn import running_cost
    for shape in ((17, 23, 3, 5), (1, 1, 1, 2), (40, 5, 2, 3)):
        for dtype in (torch.float64, torch.float32):
            case = [x.to(dtype) for x in _case(*shape, seed=1)]
            out, _, _ = _grads(case, dtype=dtype)
            want = running_cost(*case, BOX)
            for k in want:
                assert torch.equal(out[k].detach(), want[k]), (shape, dtype, k)
            assert out["reward_seqs"].requires_grad and not out["chamfer"].requires_grad and not out["collision"].requires_grad and not out["box"].requires_grad


# (n_obj, M, T, B, seed): every value of n_obj {1, 2, 65}, M {1, 2, 257}, T {1, 3}, B {1, 3}; the seeds are the first of a host-side search whose
# fp64 statement decides every minimum, gate and wall with the margin the test asserts
CPU_CASES = [(1, 1, 1, 1, 0), (1, 257, 3, 3, 0), (2, 2, 3, 3, 0), (2, 257, 1, 1, 0), (65, 1, 3, 1, 0), (65, 2, 1, 3, 1), (65, 257, 3, 3, 0)]


def assert_margins(m, what):
    assert m["nn"] >= MARGIN and m["gate"] >= MARGIN and m["wall"] >= MARGIN and m["extreme_ties"] == 0 and m["zero"] == 0, (what, m)


@pytest.mark.parametrize("n_obj,M,T,B,seed", CPU_CASES)
def test_fp64_gradients_equal_the_numpy_statement_and_central_differences(n_obj, M, T, B, seed):
    from gsdyn import running_cost
    case = [x.double() for x in _case(n_obj, M, T, B, seed=seed)]
    want = gd_ref.cost_grad_ref(*case, BOX.reshape(4), **KW)
    assert_margins(want["margins"], (n_obj, M, T, B, seed))
    out, gs, ga = _grads(case)
    assert np.abs(out["reward_seqs"].detach().numpy() - want["reward"]).max() <= 1e-12
    scale_s, scale_a = max(np.abs(want["g_state"]).max(), 1e-300), max(np.abs(want["g_actions"]).max(), 1e-300)
    assert np.abs(gs.numpy() - want["g_state"]).max() <= 1e-12 * scale_s
    assert np.abs(ga.numpy() - want["g_actions"]).max() <= 1e-12 * scale_a
    assert np.abs(want["g_state"]).max() > 0 and (T == 1 or np.abs(want["g_state"][:, 0]).max() > 0)      # the comparison is not of zeros
    s, a, c, t = case
    rng = np.random.default_rng(n_obj + M)
    pick_s = rng.choice(s.numel(), size=min(40, s.numel()), replace=False)
    fd_s = gd_ref.torch_central_differences(lambda v: running_cost(v, a, c, t, BOX, **KW)["reward_seqs"].sum(), s, 1e-7, pick_s)
    fd_a = gd_ref.torch_central_differences(lambda v: running_cost(s, v, c, t, BOX, **KW)["reward_seqs"].sum(), a, 1e-7)
    # central differences of step 1e-7 on values of size 1: truncation h^2 f''' and rounding 1e-16 / h -- 1e-6 of the largest gradient with room
    assert np.abs(fd_s - gs.numpy().reshape(-1)[pick_s]).max() <= 1e-6 * max(scale_s, 1.0)
    assert np.abs(fd_a - ga.numpy().reshape(-1)).max() <= 1e-6 * max(scale_a, 1.0)


def test_the_statement_slices_B_without_changing_a_sample(monkeypatch):
    from gsdyn import plan
    case = [x.double() for x in _case(64, 64, 2, 6, seed=2)]
    whole = _grads(case)
    monkeypatch.setattr(plan, "COST_TABLE_ENTRIES", 2 * 64 * 64)
    sliced = _grads(case)
    assert torch.equal(whole[1], sliced[1]) and torch.equal(whole[2], sliced[2]) and torch.equal(whole[0]["reward_seqs"], sliced[0]["reward_seqs"])


# ------------------------------------------------------------------------------------------ hand cases (run again on the device by the GPU file)
FAR = np.array([[-10.0, 10.0], [-10.0, 10.0]])        # walls whose exp(-100 margin) is exactly zero in fp32 and fp64


def _hand(frames, target, starts, cur=None, bbox=FAR, device="cpu", dtype=torch.float64, **kw):
    """One sample: frames [T][n_obj][3], starts [T][2] -> (values, g_state [T, n_obj, 3], g_actions [T, 4])."""
    s = torch.tensor([frames], dtype=dtype)
    a = torch.tensor([[[x, y, 0.0, 1.0] for x, y in starts]], dtype=dtype)
    cur = s[0, 0].clone() if cur is None else torch.tensor(cur, dtype=dtype)
    out, gs, ga = _grads((s, a, cur, torch.tensor(target, dtype=dtype)), bbox=bbox, device=device, dtype=dtype, **kw)
    return out, gs[0].cpu(), ga[0].cpu()


def hand_tie_between_two_targets(device="cpu", dtype=torch.float64):
    """One particle exactly midway between two targets (coordinates exact in fp32): the LOWER target index takes the particle's term,
    -(P - q_0) / |.| = (-1, 0, 0); the two targets' own terms cancel exactly.  The higher index would give (+1, 0, 0)."""
    _, gs, ga = _hand([[[0.5, 0.0, 0.0]]], [[0.25, 0.0, 0.0], [0.75, 0.0, 0.0]], [(50.0, 50.0)], device=device, dtype=dtype)
    assert gs.tolist() == [[[-1.0, 0.0, 0.0]]] and ga.tolist() == [[0.0, 0.0, 0.0, 0.0]]
    # one target exactly midway between two particles: the LOWER particle index takes the target's term, +1; the particles' own terms are -+ 1/2
    _, gs, _ = _hand([[[0.25, 0.0, 0.0], [0.75, 0.0, 0.0]]], [[0.5, 0.0, 0.0]], [(50.0, 50.0)], device=device, dtype=dtype)
    assert gs.tolist() == [[[1.5, 0.0, 0.0], [-0.5, 0.0, 0.0]]]


def hand_target_on_a_particle(device="cpu", dtype=torch.float64):
    """A target coincident with particle 0: both of its terms are the zero vector, finite; particle 1 is pulled toward the target."""
    out, gs, _ = _hand([[[0.5, 0.5, 0.0], [0.25, 0.5, 0.0]]], [[0.5, 0.5, 0.0]], [(50.0, 50.0)], device=device, dtype=dtype)
    assert gs.tolist() == [[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]] and float(out["chamfer"][0]) == 0.125


def hand_collision_gate(device="cpu", dtype=torch.float64):
    """T = 2.  Push 1 starts 2^-5 to the right of particle 0 of frame 0 with pusher_size = 2^-7: the gate is open, c = exp(-100 (2^-5 -
    2^-7)); d reward / d a_x = (5 / 2) 100 c and the particle's x receives the opposite.  Inside the pusher (2^-8 away): zero, both."""
    frames = [[[0.5, 0.5, 0.0], [0.0, 0.0, 0.0]], [[0.5, 0.5, 0.0], [0.0, 0.0, 0.0]]]
    p = 2.0 ** -7
    for off, open_ in ((2.0 ** -5, True), (2.0 ** -8, False)):
        out, gs, ga = _hand(frames, [[0.5, 0.5, 0.0]], [(50.0, 50.0), (0.5 + off, 0.5)], device=device, dtype=dtype, pusher_size=p)
        c = math.exp(-100 * (off - p)) if open_ else 1.0
        want = 2.5 * 100 * c if open_ else 0.0
        assert abs(float(out["collision"][0, 1]) - c) <= 1e-6
        assert abs(float(ga[1, 0]) - want) <= 1e-5 * max(want, 1.0) and float(ga[1, 1]) == 0.0 and ga[:, 2:].abs().max() == 0
        assert abs(float(gs[0, 0, 0]) + want) <= 1e-5 * max(want, 1.0) and gs[0, 1].abs().max() == 0 and gs[0, :, 1:].abs().max() == 0
        assert ga[0].abs().max() == 0                                              # push 0 meets state_cur from far away: c = 0


def hand_box_walls(device="cpu", dtype=torch.float64):
    """T = 2, frame 0 (no chamfer there; the next push starts far away).  Walls at [0, 1]^2."""
    unit = np.array([[0.0, 1.0], [0.0, 1.0]])
    g = 2.5 * 100 * math.exp(-12.5)
    last = [[0.5, 0.5, 0.0], [0.5, 0.5, 0.0]]
    for frame0, want in (([[0.125, 0.5, 0.0], [0.5, 0.5, 0.0]], [[g, 0.0, 0.0], [0.0, 0.0, 0.0]]),         # x_lo: + to the leftmost x
                         ([[0.5, 0.5, 0.0], [0.875, 0.5, 0.0]], [[0.0, 0.0, 0.0], [-g, 0.0, 0.0]]),        # x_hi: - to the rightmost x
                         ([[0.5, 0.5, 0.0], [0.5, 0.125, 0.0]], [[0.0, 0.0, 0.0], [0.0, g, 0.0]]),         # y_lo
                         ([[0.5, 0.875, 0.0], [0.5, 0.5, 0.0]], [[0.0, -g, 0.0], [0.0, 0.0, 0.0]]),        # y_hi
                         ([[0.125, 0.125, 0.0], [0.5, 0.5, 0.0]], [[g, 0.0, 0.0], [0.0, 0.0, 0.0]]),       # x_lo and y_lo equal: the lower wall index
                         ([[-0.125, 0.5, 0.0], [0.5, 0.5, 0.0]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]),      # beyond a wall: box = 1, no gradient
                         ([[0.0, 0.5, 0.0], [0.5, 0.5, 0.0]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])):        # on a wall: margin 0, no gradient
        out, gs, ga = _hand([frame0, last], [[0.5, 0.5, 0.0]], [(50.0, 50.0), (50.0, 50.0)], cur=last, bbox=unit, device=device, dtype=dtype)
        assert (gs[0] - torch.tensor(want, dtype=dtype)).abs().max() <= 1e-5 * g, (frame0, gs[0])
        assert ga.abs().max() == 0
        assert (float(out["box"][0, 0]) == 1.0) == (frame0[0][0] <= 0.0)


def hand_nan_sample(device="cpu", dtype=torch.float64):
    """One NaN coordinate in the FIRST frame of sample 1: all of that sample's gradient rows are NaN -- also the last frame's and the action
    rows the NaN never reached --, the other samples' are bit-equal to the call without it.  Columns 2 and 3 of the others are zero."""
    case = [x.to(dtype) for x in _case(5, 7, 3, 3, seed=8)]
    _, gs0, ga0 = _grads(case, device=device, dtype=dtype)
    case[0] = case[0].clone()
    case[0][1, 0, 2, 1] = math.nan
    out, gs, ga = _grads(case, device=device, dtype=dtype)
    assert math.isnan(float(out["reward_seqs"][1].detach())) and torch.isnan(gs[1]).all() and torch.isnan(ga[1]).all()
    for b in (0, 2):
        assert torch.equal(gs[b], gs0[b]) and torch.equal(ga[b], ga0[b]) and torch.isfinite(gs[b]).all()
        assert ga[b][:, 2:].abs().max() == 0 and ga[b][:, :2].abs().max() > 0


HAND_CASES = [hand_tie_between_two_targets, hand_target_on_a_particle, hand_collision_gate, hand_box_walls, hand_nan_sample]


@pytest.mark.parametrize("case", HAND_CASES, ids=lambda f: f.__name__)
def test_hand_cases(case):
    case()
    case(dtype=torch.float32)


# ------------------------------------------------------------------------------------------ the differentiable rollout
def z_margin(trace_points):
    """The smallest relative lead of the lowest object z over the second lowest among the frames a tool height is taken from."""
    m = math.inf
    for pts in trace_points:
        z = torch.sort(pts[:-1, 2].double()).values
        m = min(m, float((z[1] - z[0]) / max(abs(float(z[0])), abs(float(z[1])), 1e-300)))
    return m


def roll_gd_case(dtype=torch.float64, device="cpu"):
    """tests/test_plan_gpu.py's rollout case (grid of spacing 0.1, threshold 0.135, mixed repeat counts) and a fixed weight tensor."""
    from test_plan_gpu import ROLL, _roll_case
    model, state, actions = _roll_case()
    w = torch.rand((ROLL["B"], ROLL["T"], ROLL["n_obj"], 3), generator=torch.Generator().manual_seed(5), dtype=torch.float64) - 0.5
    kw = dict(push_length=ROLL["push"], adj_thresh=ROLL["thr"], topk=ROLL["topk"], n_his=3)
    return model.to(device=device, dtype=dtype), state.to(device=device, dtype=dtype), actions.to(device=device, dtype=dtype), w.to(device=device, dtype=dtype), kw


def roll_margins(model, state, actions, kw):
    """(relation threshold margin, k-th neighbour margin, lowest-z margin) of the definition's own decisions, and its trace."""
    from gsdyn import rollout_actions_grad
    from test_plan_gpu import _relation_margins
    trace = []
    with torch.no_grad():
        out = rollout_actions_grad(model, state, actions, device_path=False, _trace=trace, **kw)["state_seqs"]
    ms = [_relation_margins(pts.double(), kw["adj_thresh"], kw["topk"]) for _, _, _, pts, _, _ in trace]
    pts = [p for _, _, _, p, _, _ in trace] + [torch.cat([o, o[:1]], 0) for o in out.reshape(-1, out.shape[2], 3)]
    return min(m[0] for m in ms), min(m[1] for m in ms), z_margin(pts), trace


def test_rollout_grad_values_equal_rollout_actions_and_margins_hold():
    from gsdyn import rollout_actions, rollout_actions_grad
    model, state, actions, w, kw = roll_gd_case()
    m_thr, m_k, m_z, _ = roll_margins(model, state, actions, kw)
    assert m_thr >= 1e-3 and m_k >= 1e-3 and m_z >= 1e-3, (m_thr, m_k, m_z)
    a = actions.clone().requires_grad_(True)
    got = rollout_actions_grad(model, state, a, **kw)
    want = rollout_actions(model, state, actions, **kw)
    assert torch.equal(got["state_seqs"].detach(), want["state_seqs"]) and torch.equal(got["action_seqs"].detach(), want["action_seqs"])
    assert got["state_seqs"].requires_grad
    det = rollout_actions_grad(model, state, a, detach_steps=True, **kw)["state_seqs"]
    assert torch.equal(det.detach(), want["state_seqs"])
    with pytest.raises(RuntimeError, match="device path"):
        rollout_actions_grad(model, state, a, device_path=True, **kw)
    with pytest.raises(ValueError, match="at least once"):
        rollout_actions_grad(model, state, torch.zeros((1, 1, 4), dtype=torch.float64), **kw)


def test_rollout_grad_against_central_differences():
    """d(sum w state_seqs) / d actions (columns 0 - 2; the length column has no gradient) with mixed repeat counts, and toward the model's
    parameters for a few entries of the first and the last layer.  Step 1e-6 in fp64 (torch.autograd.gradcheck's): rounding 1e-16 |f| / h
    ~ 1e-10, truncation h^2 f''' / 6, and a ReLU whose pre-activation lies within the step of zero adds up to its whole contribution times
    h / |pre-activation range| -- 1e-5 of the largest gradient covers them (gradcheck itself asks 1e-3 relative)."""
    from gsdyn import rollout_actions, rollout_actions_grad
    model, state, actions, w, kw = roll_gd_case()
    a = actions.clone().requires_grad_(True)
    loss = (rollout_actions_grad(model, state, a, **kw)["state_seqs"] * w).sum()
    params = [model.particle_encoder.model[0].weight, model.non_rigid_predictor.linear_2.weight]
    grads = torch.autograd.grad(loss, [a] + params)
    f = lambda v: (rollout_actions(model, state, v, **kw)["state_seqs"] * w).sum()  # noqa: E731
    cols = [i for i in range(actions.numel()) if i % 4 != 3]
    fd = gd_ref.torch_central_differences(f, actions, 1e-6, cols)
    g = grads[0].numpy().reshape(-1)
    scale = np.abs(fd).max()
    assert scale > 1e-4 and np.abs(fd - g[cols]).max() <= 1e-5 * scale, (scale, np.abs(fd - g[cols]).max())
    assert np.abs(g[3::4]).max() == 0.0
    for p, gp in zip(params, grads[1:]):
        keep = p.detach().clone()
        idx = list(range(0, p.numel(), max(1, p.numel() // 7)))

        def fp(v, p=p):
            with torch.no_grad():
                p.copy_(v)
            return (rollout_actions(model, state, actions, **kw)["state_seqs"] * w).sum()
        fd_p = gd_ref.torch_central_differences(fp, keep, 1e-6, idx)
        with torch.no_grad():
            p.copy_(keep)
        sc = float(gp.abs().max())
        assert sc > 0 and np.abs(fd_p - gp.numpy().reshape(-1)[idx]).max() <= 1e-5 * sc


def test_rollout_grad_detach_steps_cuts_the_path_between_look_ahead_steps():
    from gsdyn import rollout_actions_grad
    model, state, actions, w, kw = roll_gd_case()
    a = actions.clone().requires_grad_(True)
    last = (rollout_actions_grad(model, state, a, detach_steps=True, **kw)["state_seqs"][:, -1] * w[:, -1]).sum()
    (g,) = torch.autograd.grad(last, a)
    assert g[:, 0].abs().max() == 0.0 and g[:, 1, :3].abs().max() > 0
    a2 = actions.clone().requires_grad_(True)
    last2 = (rollout_actions_grad(model, state, a2, **kw)["state_seqs"][:, -1] * w[:, -1]).sum()
    (g2,) = torch.autograd.grad(last2, a2)
    assert g2[:, 0, :3].abs().max() > 0                                             # attached: the first push moves the last state


# ------------------------------------------------------------------------------------------ the planner's loop
def test_plan_actions_gd_one_iteration_returns_the_best_initial_sample():
    from gsdyn import plan_actions_gd, rollout_actions, running_cost, sample_action_seq
    model, state, target, seq0, kw = plan_case()
    kw.pop("chunk")
    res = plan_actions_gd(model, state, target, BBOX, seq0, n_update_iter=1, **kw)
    drawn = sample_action_seq(seq0, LOWER, UPPER, 8, iter_index=0, noise_level=1.0, push_length=0.05, generator=torch.Generator().manual_seed(kw["generator"].initial_seed()))
    out = rollout_actions(model, state, drawn, push_length=0.05, adj_thresh=0.12)["state_seqs"]
    rewards = running_cost(out, drawn, state, target, BBOX)["reward_seqs"]
    best = int(torch.argmax(rewards))
    assert torch.equal(res["act_seq"], drawn[best]) and res["reward_history"].shape == (1,)
    assert float(res["reward_history"][0]) == float(rewards[best])
    one = rollout_actions(model, state, drawn[best:best + 1], push_length=0.05, adj_thresh=0.12)["state_seqs"]
    assert torch.equal(res["state_seqs"], one[0])
    assert float(res["reward"]) == float(running_cost(one, drawn[best:best + 1], state, target, BBOX)["reward_seqs"][0])
    assert all(p.grad is None for p in model.parameters())                         # the model's parameters accumulate nothing
    # init is honoured: the winner is one of ITS rows
    init = drawn[[5, 2, 7]].clone()
    res = plan_actions_gd(model, state, target, BBOX, seq0, n_update_iter=1, init=init, **kw)
    assert torch.equal(res["act_seq"], init[int(torch.argmax(rewards[[5, 2, 7]]))])


def still_model(device="cpu"):
    """A model whose predictor's last layer is zero: the particles never move, the reward depends on the pushes through the collision
    term only."""
    model = _model().to(device)
    with torch.no_grad():
        model.non_rigid_predictor.linear_2.weight.zero_()
        model.non_rigid_predictor.linear_2.bias.zero_()
    return model


def still_case(device="cpu"):
    """12 particles on a 3 x 4 grid of spacing 0.2 (ten steps of 1e-3 away from a particle approach no other one), start points 0.03 - 0.05
    away from one of them (outside the pusher: the gate is open), T = 2."""
    _, _, target, seq0, kw = plan_case(device=device)
    kw.pop("chunk"), kw.pop("n_sample")
    ix = torch.arange(12, dtype=torch.float32)
    state = torch.stack([(ix % 3) * 0.2, torch.div(ix, 3, rounding_mode="floor") * 0.2 - 0.15, 0.001 * ix], 1).to(device)
    off = torch.tensor([[[0.03, 0.0], [0.0, 0.04]], [[-0.03, 0.02], [0.05, 0.0]], [[0.0, -0.03], [0.02, 0.03]]], device=device)
    near = state[[0, 5, 9]][:, None, :2] + off
    init = torch.cat([near, torch.tensor([0.3, 1.4], device=device).expand(3, 2, 2)], 2)
    return still_model(device), state, target, seq0, init, kw


def test_plan_actions_gd_lowers_the_collision_term_and_leaves_the_lengths():
    from gsdyn import plan_actions_gd, running_cost
    model, state, target, seq0, init, kw = still_case()
    for b in range(3):
        res = plan_actions_gd(model, state, target, BBOX, seq0, n_update_iter=11, lr=1e-3, init=init[b:b + 1], **kw)
        h = res["reward_history"]
        assert h.shape == (11,) and (h[1:] > h[:-1]).all(), h                      # B = 1: the history IS the reward of each iteration
        assert torch.equal(res["act_seq"][:, 3], init[b, :, 3])                    # zero gradient: Adam leaves the lengths alone
        assert not torch.equal(res["act_seq"][:, :2], init[b, :, :2])
        frames = state[None, None].expand(1, 2, -1, -1)                            # the particles never move
        before = running_cost(frames, init[b:b + 1], state, target, BBOX)
        after = running_cost(res["state_seqs"][None], res["act_seq"][None], state, target, BBOX)
        assert float(after["collision"].mean()) < float(before["collision"].mean())
        assert float(after["chamfer"][0]) == float(before["chamfer"][0]) and torch.equal(after["box"], before["box"])
    res = plan_actions_gd(model, state, target, BBOX, seq0, n_update_iter=6, lr=1e-3, init=init, **kw)
    h = res["reward_history"]
    assert (h[1:] >= h[:-1]).all() and torch.isfinite(res["act_seq"]).all() and res["state_seqs"].shape == (2, 12, 3)
