"""CPU tests of the planner's rollout (gsdyn/plan.py): the exported symbols, ``decode_action``, and the torch fallback of
``rollout_actions`` -- the semantic definition of the batched HIP path -- against a literal restatement of the reference's loop
(``dynamics`` of the reference's real_world/plan.py) on the dense ``Rr / Rs`` form of the model."""
import math
import os
import re

import pytest
import torch

SYMBOLS = ("gsr_construct_edges_batch", "gsr_plan_step_head", "gsr_plan_step_tail")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(width=16, **kw):
    c = dict(nf_particle=width, nf_relation=width, nf_effect=width, attr_dim=2, state_dim=0, action_dim=3, pstep=3, rel_attr_dim=2,
             rel_group_dim=1, rel_distance_dim=3, n_his=3)
    c.update(kw)
    return c


def _model(width=16, seed=0, dtype=torch.float32, **kw):
    from gsdyn.dynamics import DynamicsPredictor
    torch.manual_seed(seed)
    return DynamicsPredictor(_cfg(width, **kw)).eval().to(dtype)


def _case(B=3, T=2, n_obj=12, repeats=((1, 2), (3, 1), (2, 2)), seed=3, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    state = (torch.rand((n_obj, 3), generator=g, dtype=torch.float64) * torch.tensor([0.3, 0.3, 0.02], dtype=torch.float64)).to(dtype)
    xy = torch.rand((B, T, 2), generator=g, dtype=torch.float64) * 0.3
    theta = (torch.rand((B, T, 1), generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    length = torch.tensor(repeats, dtype=torch.float64)[:, :, None] + 0.4          # int() truncates: 1.4 -> 1
    return state, torch.cat([xy, theta, length], 2).to(dtype)


def _reference_loop(model, state, actions, push_length, adj_thresh, topk, n_his):
    """The reference's ``dynamics`` loop, line for line where it bears on the result: every sample runs through the batched dense-form
    ``forward`` up to the largest repeat count of the step, relations from per-sample ``construct_edges`` turned into one-hot matrices
    and zero-padded to a common count (the reference's ``pad_torch``)."""
    from gsdyn.dynamics import construct_edges, edges_to_dense
    from gsdyn.plan import decode_action
    dtype = state.dtype
    bsz, n_look = actions.shape[0], actions.shape[1]
    decoded, repeat = decode_action(actions, push_length=push_length)
    n_obj = state.shape[0]
    obj_kp = state[None, None].repeat(bsz, n_his, 1, 1)
    out = torch.zeros((bsz, n_look, n_obj, 3), dtype=dtype)
    mask = torch.ones(n_obj + 1, dtype=torch.bool)
    tool = torch.zeros(n_obj + 1, dtype=torch.bool)
    tool[n_obj] = True

    def relations(last):                # [bsz, n_obj + 1, 3] -> Rr, Rs [bsz, n_rel_max, n_obj + 1]
        pairs = [edges_to_dense(*construct_edges(last[b], adj_thresh, mask, tool, topk=topk), n_obj + 1, dtype=dtype) for b in range(bsz)]
        n_rel = max(p[0].shape[0] for p in pairs)
        pad = lambda m: torch.cat([m, torch.zeros((n_rel - m.shape[0], n_obj + 1), dtype=dtype)], 0)  # noqa: E731
        return torch.stack([pad(p[0]) for p in pairs]), torch.stack([pad(p[1]) for p in pairs])

    with torch.no_grad():
        for li in range(n_look):
            if li > 0:
                obj_kp = out[:, li - 1:li].clone().repeat(1, n_his, 1, 1)
            z = obj_kp[:, -1, :, 2].min(dim=1).values
            eef_kp = torch.zeros((bsz, 1, 3), dtype=dtype)
            eef_kp[:, 0, 0] = decoded[:, li, 0]
            eef_kp[:, 0, 1] = decoded[:, li, 1]
            eef_kp[:, 0, 2] = z
            eef_delta = torch.zeros((bsz, 1, 3), dtype=dtype)
            eef_delta[:, 0, 0] = decoded[:, li, 2] - decoded[:, li, 0]
            eef_delta[:, 0, 1] = decoded[:, li, 3] - decoded[:, li, 1]
            states = torch.zeros((bsz, n_his, n_obj + 1, 3), dtype=dtype)
            states[:, :, :n_obj] = obj_kp
            states[:, :, n_obj:] = eef_kp[:, None]
            states_delta = torch.zeros((bsz, n_obj + 1, 3), dtype=dtype)
            states_delta[:, n_obj:] = eef_delta
            attrs = torch.zeros((bsz, n_obj + 1, 2), dtype=dtype)
            attrs[:, :n_obj, 0] = 1.0
            attrs[:, n_obj:, 1] = 1.0
            p_instance = torch.ones((bsz, n_obj, 1), dtype=dtype)
            Rr, Rs = relations(states[:, -1])
            for ai in range(1, 1 + int(repeat[:, li].max())):
                pred_state, _ = model(state=states, attrs=attrs, p_instance=p_instance, action=states_delta, Rr=Rr, Rs=Rs)
                keep = repeat[:, li] == ai
                out[keep, li] = pred_state[keep].clone()
                z_cur = pred_state[:, :, 2].min(dim=1).values
                eef_cur = states[:, -1, n_obj:] + states_delta[:, n_obj:]
                eef_cur[:, 0, 2] = z_cur
                states_cur = torch.cat([pred_state, eef_cur], dim=1)
                Rr, Rs = relations(states_cur)
                states = torch.cat([states[:, 1:], states_cur[:, None]], dim=1)
    return out, decoded


def test_symbols_are_exported_and_declared_and_the_abi_is_125():
    from diff_gaussian_rasterization import _hip
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
        assert re.search(r"^int " + s + r"\(", header, re.M), s
    assert re.search(r"#define GSR_VERSION 125\b", header)
    import ctypes
    lib = ctypes.CDLL(_hip.LIB_PATH)              # dlopen works without a GPU
    assert lib.gsr_version() == 125
    for s in SYMBOLS:
        getattr(lib, s)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The argument checks run on the host before anything is launched: a capacity one below the bound, no sample and too many particles
    come back as error codes with a text.  Every pointer is a real buffer large enough for the refused call (on the device where there is
    one), so a check that regressed would launch on valid memory instead of faulting."""
    from diff_gaussian_rasterization import _hip
    import ctypes as C
    lib = _hip.load_library()
    where = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    B, n_obj, topk, big = 3, 12, 5, 128
    bound = _hip.plan_edge_capacity(B, n_obj, topk)
    big_cap = _hip.plan_edge_capacity(B, big, topk)
    assert bound == 3 * (12 * 5 + 24)
    assert _hip.plan_edge_capacity(2, 3, 5) == 2 * (3 * 3 + 6)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=where)  # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=where)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    R = big + 1
    pos, nv, cnt = f32(B * R * 3), torch.full((1,), n_obj, dtype=torch.int32, device=where), torch.zeros(1, dtype=torch.int32, device=where)
    recv, send, rows, scratch = i64(big_cap), i64(big_cap), i64(B * R + 2), i64(B * (2 * R + 1))
    call = lambda b, n, cap: lib.gsr_construct_edges_batch(b, p(pos), n, p(nv), 0.01, topk, cap, p(recv), p(send), p(cnt), p(rows), p(scratch), None)  # noqa: E731
    assert call(B, n_obj, bound - 1) != 0 and b"bound" in lib.gsr_last_error()
    assert call(0, n_obj, bound) != 0 and b"B >= 1" in lib.gsr_last_error()
    assert call(B, big, big_cap) != 0 and b"n_obj_cap <= 127" in lib.gsr_last_error()
    n_his, T = 3, 2
    hist, eef, delta, mot = f32(B * n_his * big * 3), f32(B * n_his * 3), f32(B * 3), f32((B * R + 1) * 3)
    rep, out = torch.ones(B * T, dtype=torch.int32, device=where), f32(B * T * big * 3)
    assert lib.gsr_plan_step_tail(B, n_his, big, T, 1, 0, 100.0, p(mot), p(delta), p(rep), p(hist), p(eef), p(out), None) != 0
    assert b"gsr_plan_step_tail" in lib.gsr_last_error()
    attrs, inst, st, p_in, nodes, last = f32((B * R + 1) * 2), f32(B * R + 1), f32((B * R + 1) * 9), f32((B * R + 1) * 14), f32((B * R + 1) * 12), f32(B * R * 3)
    assert lib.gsr_plan_step_head(0, n_his, n_obj, 2, 0, p(hist), p(eef), p(delta), p(attrs), p(inst), p(st), p(p_in), p(nodes), p(last), None) != 0
    assert b"gsr_plan_step_head" in lib.gsr_last_error()
    if where.type == "cuda":
        torch.cuda.synchronize()


def test_decode_action_hand_values():
    from gsdyn import decode_action
    a = torch.tensor([[[0.5, -0.25, 0.0, 3.9], [1.0, 2.0, math.pi / 2, 1.0]],
                      [[0.0, 0.0, math.pi, 2.5], [-1.0, 0.5, -math.pi / 2, 0.99]]], dtype=torch.float64)
    dec, rep = decode_action(a, push_length=0.5)
    expect = torch.tensor([[[0.5, -0.25, 0.0, -0.25], [1.0, 2.0, 1.0, 1.5]],
                           [[0.0, 0.0, 0.5, 0.0], [-1.0, 0.5, -1.0, 1.0]]], dtype=torch.float64)
    assert torch.allclose(dec, expect, atol=1e-15, rtol=0)
    assert rep.dtype == torch.int32 and rep.tolist() == [[3, 1], [2, 0]]          # truncation towards zero, as .to(int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rollout_actions_equals_the_reference_loop(dtype):
    """B = 3, T = 2, 12 particles, repeats [[1, 2], [3, 1], [2, 2]], a seeded 16-wide model: fp32 within 1e-5 of the largest displacement,
    fp64 bit for bit."""
    from gsdyn import rollout_actions
    model = _model(dtype=dtype)
    state, actions = _case(dtype=dtype)
    got = rollout_actions(model, state, actions, push_length=0.05, adj_thresh=0.12, topk=5, n_his=3)
    ref, dec = _reference_loop(model, state, actions, 0.05, 0.12, 5, 3)
    assert got["state_seqs"].shape == (3, 2, 12, 3) and got["state_seqs"].dtype == dtype
    assert torch.equal(got["action_seqs"], dec)
    disp = (ref - state[None, None]).abs().max().item()
    assert disp > 1e-4                                    # the model moves the particles: the comparison is not of the input with itself
    assert not torch.equal(ref[:, 0], ref[:, 1])
    err = (got["state_seqs"] - ref).abs().max().item()
    print(f"{dtype}: largest displacement {disp:.3e}, max abs difference {err:.3e}")
    if dtype == torch.float64:
        assert torch.equal(got["state_seqs"], ref)
    else:
        assert err <= 1e-5 * disp


def test_repeat_below_one_is_refused():
    from gsdyn import rollout_actions
    model = _model()
    state, actions = _case(repeats=((1, 2), (0, 1), (2, 2)))
    with pytest.raises(ValueError, match="repeat"):
        rollout_actions(model, state, actions, push_length=0.05, adj_thresh=0.12)


def test_chunking_does_not_change_a_sample():
    from gsdyn import rollout_actions
    model = _model()
    state, actions = _case()
    kw = dict(push_length=0.05, adj_thresh=0.12, topk=5, n_his=3)
    a = rollout_actions(model, state, actions, chunk=2, **kw)["state_seqs"]
    b = rollout_actions(model, state, actions, chunk=3, **kw)["state_seqs"]
    assert torch.equal(a, b)


def test_more_than_127_particles_take_the_fallback(monkeypatch):
    """The device kernels hold a sample in two 64-lane ballots: 128 particles are served by the torch fallback, not refused.  The decision
    is a pure function of the model and the particle count (``_split_ok`` stands in for "a HIP device" here)."""
    from gsdyn import plan, rollout_actions
    model = _model()
    probe = torch.zeros((1, 3))
    assert not plan._device_path_ok(model, probe, 12)                   # a CPU tensor: the split path refuses
    monkeypatch.setattr(model, "_split_ok", lambda a: True)
    assert plan._device_path_ok(model, probe, 127) and plan._device_path_ok(model, probe, 1)
    assert not plan._device_path_ok(model, probe, 128) and not plan._device_path_ok(model, probe, 0)
    monkeypatch.undo()
    state, actions = _case(B=1, T=1, n_obj=128, repeats=((2,),))
    out = rollout_actions(model, state, actions, push_length=0.05, adj_thresh=0.12)["state_seqs"]
    assert out.shape == (1, 1, 128, 3) and torch.isfinite(out).all()
