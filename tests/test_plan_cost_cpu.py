"""CPU tests of the planner's cost, MPPI update, sampler and ``plan_actions`` (gsdyn/plan.py, csrc/gsr_plan_cost.hip): the exported symbols
and their argument checks, the torch fallbacks -- the semantic definitions of the two kernels -- against the fp64 statements of
tests/plan_cost_ref.py and against hand-computed cases, the sampler's rules, and one whole planning step on CPU tensors."""
import math
import os
import re

import numpy as np
import torch

import plan_cost_ref as ref

SYMBOLS = ("gsr_plan_cost", "gsr_plan_mppi_update")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BBOX = np.array([[-0.1, 0.6], [-0.2, 0.5], [0.0, 0.1]])           # the reference's [3, 2] array; rows x, y are used
LOWER, UPPER = [-0.1, -0.2, -math.pi, 1.0], [0.6, 0.5, math.pi, 3.0]


def _box(bbox=BBOX):
    return np.asarray(bbox)[:2, :2].reshape(4)


def _cost_case(B=5, T=3, n_obj=17, M=23, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.5, 0.5, 0.02], dtype=torch.float64)
    r = lambda *sh: torch.rand(sh, generator=g, dtype=torch.float64)  # noqa: E731
    state_seqs, state_cur, target = r(B, T, n_obj, 3) * scale, r(n_obj, 3) * scale, r(M, 3) * scale
    actions = torch.cat([r(B, T, 2) * 0.5, (r(B, T, 1) * 2 - 1) * math.pi, r(B, T, 1) * 10 + 10], 2)
    return tuple(t.to(dtype) for t in (state_seqs, actions, state_cur, target))


def _cfg(width=16, **kw):
    c = dict(nf_particle=width, nf_relation=width, nf_effect=width, attr_dim=2, state_dim=0, action_dim=3, pstep=3, rel_attr_dim=2,
             rel_group_dim=1, rel_distance_dim=3, n_his=3)
    c.update(kw)
    return c


def _model(width=16, seed=0):
    from gsdyn.dynamics import DynamicsPredictor
    torch.manual_seed(seed)
    return DynamicsPredictor(_cfg(width)).eval()


def test_symbols_are_exported_and_declared_and_the_abi_is_125():
    from diff_gaussian_rasterization import _hip
    import ctypes
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
        assert re.search(r"^int " + s + r"\(", header, re.M), s
    assert re.search(r"#define GSR_VERSION 125\b", header)
    lib = ctypes.CDLL(_hip.LIB_PATH)              # dlopen works without a GPU
    assert lib.gsr_version() == 125
    for s in SYMBOLS:
        getattr(lib, s)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """B = 0, M = 0, n_obj = 1025 and a NULL pointer come back as -2 with a text, before anything is launched.  Every pointer is a real buffer
    large enough for the refused call (on the device where there is one), so a check that regressed would launch on valid memory."""
    from diff_gaussian_rasterization import _hip
    import ctypes as C
    lib = _hip.load_library()
    where = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    B, T, n_obj, big, M = 3, 2, 12, 1025, 7
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=where)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    seqs, acts, cur, tgt, box = f32(B * T * big * 3), f32(B * T * 4), f32(big * 3), f32(M * 3), f32(4)
    rew, ch, co, bp = f32(B), f32(B), f32(B * T), f32(B * T)
    cost = lambda b, n, m, s=seqs: lib.gsr_plan_cost(b, T, n, m, p(s) if s is not None else None, p(acts), p(cur), p(tgt), p(box),  # noqa: E731
                                                     0.01, 100.0, 5.0, p(rew), p(ch), p(co), p(bp), None)
    assert cost(0, n_obj, M) == -2 and b"B, T, M >= 1" in lib.gsr_last_error()
    assert cost(B, n_obj, 0) == -2 and b"M = 0" in lib.gsr_last_error()
    assert cost(B, big, M) == -2 and b"n_obj <= 1024" in lib.gsr_last_error()
    assert cost(B, n_obj, M, None) == -2 and b"NULL" in lib.gsr_last_error()
    lo, hi, seq, idx, best = f32(4), f32(4), f32(T * 4), torch.zeros(1, dtype=torch.int64, device=where), f32(1)
    upd = lambda b, t, r=rew: lib.gsr_plan_mppi_update(b, t, p(acts), p(r) if r is not None else None, 500.0, 0.01, p(lo), p(hi), p(seq), p(idx),  # noqa: E731
                                                       p(best), None)
    assert upd(0, T) == -2 and b"B, T >= 1" in lib.gsr_last_error()
    assert upd(B, 0) == -2 and b"T = 0" in lib.gsr_last_error()
    assert upd(B, T, None) == -2 and b"NULL" in lib.gsr_last_error()
    if where.type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the fallbacks against the fp64 statements
def test_running_cost_fallback_equals_the_fp64_statement():
    from gsdyn import running_cost
    for shape in (dict(), dict(B=2, T=1, n_obj=1, M=1), dict(B=3, T=2, n_obj=40, M=5, seed=4)):
        s, a, c, t = _cost_case(**shape)
        got = running_cost(s, a, c, t, BBOX)
        want = ref.cost_ref(s, a, c, t, _box())
        for k_got, k_ref in (("reward_seqs", "reward"), ("chamfer", "chamfer"), ("collision", "collision"), ("box", "box")):
            assert got[k_got].dtype == torch.float64 and tuple(got[k_got].shape) == want[k_ref].shape
            err = np.abs(got[k_got].numpy() - want[k_ref]).max()
            assert err <= 1e-12, (shape, k_got, err)
    assert got["collision"].min() < 0.9 and got["box"].max() < 1.0        # the terms vary: the comparison is not of constants


def test_running_cost_fallback_slices_B_without_changing_a_sample(monkeypatch):
    """The [b, M, n_obj] table is built for slices of B; a sample's result does not depend on the slicing."""
    from gsdyn import plan
    s, a, c, t = _cost_case(B=6, n_obj=64, M=64)
    monkeypatch.setattr(plan, "COST_TABLE_ENTRIES", 2 * 64 * 64)                 # two samples per slice
    whole = plan.running_cost(s, a, c, t, BBOX)
    one = [plan.running_cost(s[b:b + 1], a[b:b + 1], c, t, BBOX) for b in range(6)]
    for k in whole:
        assert torch.equal(whole[k], torch.cat([o[k] for o in one], 0))


def test_mppi_update_fallback_equals_the_fp64_statement():
    """The displacement form of the fallback against the differenced form of the fp64 statement."""
    from gsdyn import mppi_update
    g = torch.Generator().manual_seed(1)
    for B, T, spread in ((1, 1, 0.0), (7, 3, 0.01), (50, 2, 0.1)):
        _, acts, _, _ = _cost_case(B=B, T=T, seed=B)
        rewards = -torch.rand(B, generator=g, dtype=torch.float64) * spread
        got = mppi_update(acts, rewards, reward_weight=500.0, lower=[-1, -1, -4, 0], upper=[1, 1, 4, 100], push_length=0.01)
        seq, best, rmax = ref.update_ref(acts, rewards, 500.0, [-1, -1, -4, 0], [1, 1, 4, 100], 0.01)
        assert np.abs(got["act_seq"].numpy() - seq).max() <= 1e-12
        assert int(got["best_index"]) == best and float(got["best_reward"]) == rmax


# ------------------------------------------------------------------------------------------ hand-computed cases
def _hand(state_last, target, start=(5.0, 5.0), cur=None, bbox=((-10.0, 10.0), (-10.0, 10.0))):
    from gsdyn import running_cost
    s = torch.tensor([[state_last]], dtype=torch.float64)
    cur = s[0, 0] if cur is None else torch.tensor(cur, dtype=torch.float64)
    a = torch.tensor([[[start[0], start[1], 0.0, 1.0]]], dtype=torch.float64)
    return running_cost(s, a, cur, torch.tensor(target, dtype=torch.float64), np.array(bbox))


def test_hand_chamfer_two_particles_two_targets():
    """Particles (0,0,0), (1,0,0); targets (0,1,0), (3,0,0): target -> particle 1 and 2, particle -> target 1 and sqrt 2."""
    out = _hand([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0], [3.0, 0.0, 0.0]])
    assert abs(float(out["chamfer"][0]) - ((1 + 2) / 2 + (1 + math.sqrt(2)) / 2)) < 1e-15


def test_hand_start_point_inside_the_pusher_gives_collision_exactly_one():
    out = _hand([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], start=(1.004, 0.003), cur=[[0.0, 0.0, 0.5], [1.0, 0.0, 0.5]])
    assert float(out["collision"][0, 0]) == 1.0                      # 5 mm from the second particle, z not counted
    far = _hand([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], start=(1.0, 0.03))
    assert abs(float(far["collision"][0, 0]) - math.exp(-100 * 0.02)) < 1e-12


def test_hand_particle_on_a_wall_gives_box_exactly_one():
    on = _hand([[0.25, 0.5, 0.0], [1.0, 0.75, 0.0]], [[0.0, 0.0, 0.0]], bbox=((0.25, 2.0), (0.0, 2.0)))
    assert float(on["box"][0, 0]) == 1.0
    inside = _hand([[0.25, 0.5, 0.0], [1.0, 0.75, 0.0]], [[0.0, 0.0, 0.0]], bbox=((0.0, 2.0), (0.0, 2.0)))
    assert abs(float(inside["box"][0, 0]) - math.exp(-100 * 0.25)) < 1e-15         # the nearest wall: x_lo, 0.25 away
    r = -float(inside["chamfer"][0]) - 5 * float(inside["collision"][0, 0]) - 5 * float(inside["box"][0, 0])
    assert abs(float(inside["reward_seqs"][0]) - r) < 1e-15


def test_hand_equal_rewards_give_the_plain_mean():
    from gsdyn import mppi_update
    acts = torch.tensor([[[0.1, 0.2, 0.0, 10.0]], [[0.3, 0.4, 0.0, 20.0]], [[0.2, 0.6, 0.0, 12.0]]], dtype=torch.float64)
    out = mppi_update(acts, torch.full((3,), -0.25, dtype=torch.float64), reward_weight=500.0, lower=[-1, -1, -4, 0], upper=[1, 1, 4, 100], push_length=0.01)
    assert torch.allclose(out["act_seq"], torch.tensor([[0.2, 0.4, 0.0, 14.0]], dtype=torch.float64), atol=1e-14, rtol=0)
    assert int(out["best_index"]) == 0 and float(out["best_reward"]) == -0.25            # a tie: the lowest index


def test_hand_one_dominant_reward_returns_that_sample_after_the_clip():
    from gsdyn import mppi_update
    acts = torch.tensor([[[0.1, 0.2, 0.5, 10.0]], [[0.3, 0.9, -2.0, 25.0]], [[0.2, 0.6, 1.0, 12.0]]], dtype=torch.float64)
    out = mppi_update(acts, torch.tensor([-5.0, -1.0, -3.0], dtype=torch.float64), reward_weight=500.0, lower=[-1, -0.5, -4, 0], upper=[1, 0.5, 4, 20],
                      push_length=0.01)
    assert torch.allclose(out["act_seq"], torch.tensor([[0.3, 0.5, -2.0, 20.0]], dtype=torch.float64), atol=1e-13, rtol=0)   # y and length clamped
    assert int(out["best_index"]) == 1
    inf = mppi_update(acts, torch.tensor([-math.inf, -1.0, -math.inf], dtype=torch.float64), reward_weight=1.0, lower=[-1, -1, -4, 0], upper=[1, 1, 4, 100],
                      push_length=0.01)
    assert torch.allclose(inf["act_seq"], acts[1], atol=1e-13, rtol=0)                    # -inf: weight 0
    nan = mppi_update(acts, torch.tensor([-1.0, math.nan, -3.0], dtype=torch.float64), reward_weight=1.0, lower=[-1, -1, -4, 0], upper=[1, 1, 4, 100],
                      push_length=0.01)
    assert torch.isnan(nan["act_seq"]).all() and int(nan["best_index"]) == 1


def test_clip_actions_wraps_column_zero_and_clamps():
    from gsdyn import clip_actions
    a = torch.tensor([[4.0, 0.7, 5.0, 30.0], [0.25, -0.9, -5.0, 0.5]], dtype=torch.float64)
    got = clip_actions(a, [-5, -0.5, -math.pi, 1], [5, 0.5, math.pi, 20])
    want = torch.tensor([[4.0 - 2 * math.pi, 0.5, math.pi, 20.0], [0.25, -0.5, -math.pi, 1.0]], dtype=torch.float64)
    assert torch.allclose(got, want, atol=1e-15, rtol=0)


# ------------------------------------------------------------------------------------------ the sampler
def test_sample_action_seq_rules():
    from gsdyn import sample_action_seq
    seed = torch.tensor([[0.2, 0.1, 0.3, 2.0], [0.3, 0.2, -1.0, 1.5]], dtype=torch.float64)
    kw = dict(noise_level=0.02, push_length=0.05)
    first = sample_action_seq(seed, LOWER, UPPER, 64, iter_index=0, generator=torch.Generator().manual_seed(5), **kw)
    assert first.shape == (64, 2, 4)
    lo, hi = torch.tensor(LOWER, dtype=torch.float64), torch.tensor(UPPER, dtype=torch.float64)
    assert (first >= lo).all() and (first <= hi).all() and first.std(0).min() > 0
    later = sample_action_seq(seed, LOWER, UPPER, 64, iter_index=1, generator=torch.Generator().manual_seed(5), **kw)
    assert torch.equal(later[0], seed)                                              # sample 0 stays unperturbed
    assert not torch.equal(later[1], seed) and (later >= lo).all() and (later <= hi).all()
    d0, d1 = (later[1:, 0, :2] - seed[0, :2]).std(), (later[1:, 1, :2] - seed[1, :2]).std()
    assert 0.5 * 0.1 * 0.02 < d0 < 2 * 0.1 * 0.02 and d1 > 3 * d0                   # 0.1 * 10^i * N(0, noise_level)
    again = sample_action_seq(seed, LOWER, UPPER, 64, iter_index=1, generator=torch.Generator().manual_seed(5), **kw)
    assert torch.equal(later, again)                                                # seeded: reproducible
    other = sample_action_seq(seed, LOWER, UPPER, 64, iter_index=1, generator=torch.Generator().manual_seed(6), **kw)
    assert not torch.equal(later, other)


# ------------------------------------------------------------------------------------------ one planning step
SEED = 9          # a seed whose top two rewards differ by more than 1e-2 within either chunk and between the chunks' winners (the GPU test asserts it)


def plan_case(device="cpu", seed=SEED, n_obj=12):
    """The end-to-end case shared with tests/test_plan_cost_gpu.py: a width-16 model, 12 particles, n_sample = 8, chunk = 4, T = 2."""
    g = torch.Generator().manual_seed(3)
    state = (torch.rand((n_obj, 3), generator=g) * torch.tensor([0.3, 0.3, 0.02])).to(device)
    target = (torch.rand((20, 3), generator=g) * torch.tensor([0.3, 0.3, 0.02]) + torch.tensor([0.1, 0.05, 0.0])).to(device)
    model = _model().to(device)
    kw = dict(lower=LOWER, upper=UPPER, push_length=0.05, adj_thresh=0.12, n_sample=8, chunk=4, generator=torch.Generator().manual_seed(seed))
    return model, state, target, torch.zeros((2, 4), device=device), kw


def test_plan_actions_on_cpu():
    from gsdyn import plan, plan_actions, rollout_actions, running_cost, sample_action_seq
    model, state, target, seq0, kw = plan_case()
    kw.update(n_sample=6)
    res = plan_actions(model, state, target, BBOX, seq0, **kw)
    assert res["act_seq"].shape == (2, 4) and res["state_seqs"].shape == (2, 12, 3) and res["reward"].dim() == 0
    assert res["chunk_rewards"].shape == (2,)                                        # ceil(6 / 4)
    g = torch.Generator().manual_seed(SEED)                                            # the samples the call drew: 4, then 2
    drawn = [sample_action_seq(seq0, LOWER, UPPER, n, iter_index=0, noise_level=1.0, push_length=0.05, generator=g) for n in (4, 2)]
    win = int(torch.argmax(res["chunk_rewards"]))
    assert float(res["reward"]) == float(res["chunk_rewards"][win])                  # the winner is the arg-max chunk
    assert any(torch.equal(res["act_seq"], a) for a in drawn[win])                   # one of the sampled sequences, of the winning chunk
    roll = rollout_actions(model, state, res["act_seq"][None], push_length=0.05, adj_thresh=0.12)["state_seqs"]
    assert torch.equal(roll[0], res["state_seqs"])
    own = running_cost(roll, res["act_seq"][None], state, target, BBOX)["reward_seqs"][0]
    assert float(own) == float(res["reward"])                                        # its reward is the cost of its own B = 1 rollout
    for c, acts in enumerate(drawn):                                                 # every chunk kept its best sample
        out = rollout_actions(model, state, acts, push_length=0.05, adj_thresh=0.12)["state_seqs"]
        best = int(torch.argmax(running_cost(out, acts, state, target, BBOX)["reward_seqs"]))
        one = rollout_actions(model, state, acts[best:best + 1], push_length=0.05, adj_thresh=0.12)["state_seqs"]
        assert float(running_cost(one, acts[best:best + 1], state, target, BBOX)["reward_seqs"][0]) == float(res["chunk_rewards"][c])
    assert plan.MAX_COST_PARTICLES == 1024


def test_plan_actions_more_iterations_keep_the_best_sample_seen():
    """With n_update_iter = 2 and rollout_best off, a chunk's reward is the largest sample reward of either iteration."""
    from gsdyn import plan_actions
    model, state, target, seq0, kw = plan_case()
    kw.update(n_sample=4)                                                            # one chunk: both calls draw the same first samples
    one = plan_actions(model, state, target, BBOX, seq0, rollout_best=False, n_update_iter=1, noise_level=0.02, **kw)
    kw["generator"] = torch.Generator().manual_seed(SEED)
    two = plan_actions(model, state, target, BBOX, seq0, rollout_best=False, n_update_iter=2, noise_level=0.02, **kw)
    assert (two["chunk_rewards"] >= one["chunk_rewards"]).all()
    assert torch.isfinite(two["act_seq"]).all() and two["state_seqs"].shape == (2, 12, 3) and two["chunk_rewards"].shape == (1,)
