"""GPU tests of the planner's cost and MPPI update kernels (csrc/gsr_plan_cost.hip through gsdyn.running_cost / gsdyn.mppi_update) against the
fp64 statements of tests/plan_cost_ref.py on the same fp32 inputs, and of ``gsdyn.plan_actions`` on the device against the same call on CPU
tensors.  The bounds are derived, not tuned:
  chamfer     relative 1e-5: each term within 4 ulp; a sum of M <= 4096 positive terms kept in 256 partial sums (thread i adds the terms i,
              i + 256, ..; then an 8-level tree) is within (M / 256 + 8) ulp, below the (M / 64 + 10) ulp ~ 4.4e-6 a 64-sum order would give;
  collision,  absolute 1e-5: values in [0, 1]; the argument error 100 * 4 ulp * d weighted by exp(-100 d) peaks near 2e-7, the rest is the
  box         exponential's own error;
  reward      the sum of its parts' bounds;
  update      x, y within 2e-5 max|column|, theta within 1e-4 rad (modulo 2 pi), length within relative 1e-4: the weight error 30 * 2 ulp +
              exp ~ 5e-6 on every term that is not negligible, with a margin of about 3.
The measured distances are appended to plan_cost_parity.log next to the other GPU logs (hipcheck's row-margins log; ``GSR_PLAN_COST_PARITY_LOG``
names another file); profiles/plan_cost_parity.txt is that log of one run, copied by hand under a one-line header."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import plan_cost_ref as ref  # noqa: E402
from hipcheck import _ROW_LOG  # noqa: E402

_LOG = os.environ.get("GSR_PLAN_COST_PARITY_LOG", os.path.join(os.path.dirname(_ROW_LOG), "plan_cost_parity.log"))
BOX = np.array([[-0.05, 1.03], [-0.02, 1.1]])
PW = 5.0


def _log(line):
    print(line)
    try:
        os.makedirs(os.path.dirname(_LOG), exist_ok=True)
        with open(_LOG, "a") as f:
            f.write(line + "\n")
    except OSError as e:
        print(f"(plan_cost_parity.log not written: {e})")


def _case(n_obj, M, T, B, seed=0):
    """Coordinates in [0, 1]^3 with z scaled by 0.02, as the tabletop is; fp32 on the host."""
    g = torch.Generator().manual_seed(seed * 1000003 + n_obj * 7919 + M * 31 + T * 5 + B)
    scale = torch.tensor([1.0, 1.0, 0.02])
    r = lambda *sh: torch.rand(sh, generator=g)  # noqa: E731
    actions = torch.cat([r(B, T, 2), (r(B, T, 1) * 2 - 1) * math.pi, r(B, T, 1) * 10 + 10], 2)
    return r(B, T, n_obj, 3) * scale, actions, r(n_obj, 3) * scale, r(M, 3) * scale


def _run(dev, case, bbox=BOX, **kw):
    from gsdyn import running_cost
    out = running_cost(*[t.to(dev) for t in case], bbox, **kw)
    torch.cuda.synchronize()
    return out


def _distances(got, want):
    c = lambda t: t.double().cpu().numpy()  # noqa: E731
    with np.errstate(invalid="ignore"):
        e_ch = np.max(np.abs(c(got["chamfer"]) - want["chamfer"]) / np.abs(want["chamfer"]).clip(1e-300))
        e_co = np.max(np.abs(c(got["collision"]) - want["collision"]))
        e_bx = np.max(np.abs(c(got["box"]) - want["box"]))
        e_rw = np.max(np.abs(c(got["reward_seqs"]) - want["reward"]) / (1e-5 * np.abs(want["chamfer"]) + 2 * PW * 1e-5))
    return e_ch, e_co, e_bx, e_rw


def _assert_within(got, want):
    e_ch, e_co, e_bx, e_rw = _distances(got, want)
    assert e_ch <= 1e-5 and e_co <= 1e-5 and e_bx <= 1e-5 and e_rw <= 1.0, (e_ch, e_co, e_bx, e_rw)
    return e_ch, e_co, e_bx, e_rw


# every value of every axis at least once: n_obj {1, 2, 63, 64, 65, 127, 128, 1024}, M {1, 2, 63, 64, 65, 255, 256, 257, 4096}, T {1, 2, 3},
# B {1, 3, 257}; the slice rule of the particle -> target direction changes at 64 / 65 and 128 / 129 particles, the LDS tile at 1024 targets
COST_CASES = [(1, 1, 1, 1), (1, 4096, 2, 3), (2, 2, 3, 3), (2, 257, 1, 1), (2, 65, 1, 257), (63, 63, 2, 3), (63, 256, 3, 1), (64, 64, 1, 3),
              (64, 1, 3, 257), (64, 4096, 2, 1), (65, 65, 2, 1), (65, 255, 3, 3), (65, 64, 3, 257), (127, 256, 1, 3), (127, 2, 2, 1),
              (128, 257, 2, 3), (128, 4096, 3, 1), (128, 255, 2, 257), (129, 1025, 2, 3), (1024, 4096, 1, 1), (1024, 63, 2, 3), (1024, 1, 1, 1),
              (1024, 257, 3, 3), (100, 1000, 3, 3)]


for _axis, _values in enumerate(((1, 2, 63, 64, 65, 127, 128, 1024), (1, 2, 63, 64, 65, 255, 256, 257, 4096), (1, 2, 3), (1, 3, 257))):
    assert set(_values) <= {c[_axis] for c in COST_CASES}, "COST_CASES must hold every value of every axis"


@pytest.mark.parametrize("n_obj,M,T,B", COST_CASES)
def test_cost_against_fp64(dev, n_obj, M, T, B):
    case = _case(n_obj, M, T, B)
    got = _run(dev, case)
    want = ref.cost_ref(*case, BOX.reshape(4))
    e = _distances(got, want)
    _log(f"cost   n_obj={n_obj:4d} M={M:4d} T={T} B={B:3d}: chamfer rel {e[0]:.2e}, collision abs {e[1]:.2e}, box abs {e[2]:.2e}, reward {e[3]:.3f} of its bound")
    assert got["reward_seqs"].shape == (B,) and got["collision"].shape == (B, T) and got["box"].shape == (B, T)
    _assert_within(got, want)


def test_cost_is_bit_identical_from_run_to_run_and_independent_of_the_batch(dev):
    case = _case(100, 1500, 3, 257, seed=2)
    a, b = _run(dev, case), _run(dev, case)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for row in (0, 100, 256):                                   # row b of the B = 257 call = the B = 1 call on sample b, bit for bit
        one = _run(dev, (case[0][row:row + 1], case[1][row:row + 1], case[2], case[3]))
        for k in a:
            assert torch.equal(a[k][row:row + 1], one[k]), (k, row)


@pytest.mark.parametrize("n_obj,M,T,B", [(100, 1000, 3, 3), (65, 257, 2, 3), (1024, 64, 1, 1)])
def test_cost_device_path_against_the_torch_fallback_on_the_device(dev, n_obj, M, T, B):
    """Both in fp32 on the device, within the same bounds as against the fp64 statement."""
    from gsdyn import plan
    case = _case(n_obj, M, T, B, seed=3)
    got = _run(dev, case)
    d = [t.to(dev) for t in case]
    r, ch, co, bp = plan._running_cost_reference(*d, plan._box4(BOX, dev, torch.float32), 0.01, 100.0, PW)
    want = {"reward": r.double().cpu().numpy(), "chamfer": ch.double().cpu().numpy(), "collision": co.double().cpu().numpy(), "box": bp.double().cpu().numpy()}
    e = _distances(got, want)
    _log(f"cost vs torch fallback on the device n_obj={n_obj} M={M} T={T} B={B}: chamfer rel {e[0]:.2e}, collision {e[1]:.2e}, box {e[2]:.2e}, reward {e[3]:.3f}")
    _assert_within(got, want)


def test_the_dispatch_takes_the_kernels_and_they_answer_directly(dev, monkeypatch):
    """``running_cost`` / ``mppi_update`` reach gsr_plan_cost / gsr_plan_mppi_update for float32 device tensors (with the torch fallbacks
    made to raise, the calls still succeed), and the wrappers called directly give the same bits and meet the fp64 bounds."""
    from diff_gaussian_rasterization import _hip
    from gsdyn import mppi_update, plan, running_cost

    def refuse(*a, **k):
        raise AssertionError("the torch fallback ran on the device path")
    case = _case(100, 300, 2, 5, seed=9)
    d = [t.to(dev) for t in case]
    box = plan._box4(BOX, dev, torch.float32)
    r, ch, co, bp = _hip.plan_cost(*d, box, 0.01, 100.0, PW)
    acts, rewards = _update_case(130, 2, 1.0, 0.0, seed=9)
    lo, hi = torch.tensor(LOWER, device=dev), torch.tensor(UPPER, device=dev)
    seq, best, rmax = _hip.plan_mppi_update(acts.to(dev), rewards.to(dev), RW, PUSH, lo, hi)
    monkeypatch.setattr(plan, "_running_cost_reference", refuse)
    monkeypatch.setattr(plan, "_mppi_update_reference", refuse)
    got = running_cost(*d, BOX)
    upd = mppi_update(acts.to(dev), rewards.to(dev), reward_weight=RW, lower=LOWER, upper=UPPER, push_length=PUSH)
    torch.cuda.synchronize()
    assert torch.equal(got["reward_seqs"], r) and torch.equal(got["chamfer"], ch) and torch.equal(got["collision"], co) and torch.equal(got["box"], bp)
    assert torch.equal(upd["act_seq"], seq) and int(upd["best_index"]) == int(best) and float(upd["best_reward"]) == float(rmax)
    _assert_within({"reward_seqs": r, "chamfer": ch, "collision": co, "box": bp}, ref.cost_ref(*case, BOX.reshape(4)))
    want, w_best, _ = ref.update_ref(acts, rewards, RW, LOWER, UPPER, PUSH)
    ex, ey, et, el = _update_distances(seq.double().cpu().numpy(), want, acts)
    assert int(best) == w_best and ex <= 2e-5 and ey <= 2e-5 and et <= 1e-4 and el <= 1e-4


# ------------------------------------------------------------------------------------------ edge cases, each at the smallest shape
def test_edge_target_on_the_particles_gives_zero_not_nan(dev):
    s, a, c, _ = _case(2, 2, 1, 1, seed=5)
    got = _run(dev, (s, a, c, s[0, 0].clone()))
    assert float(got["chamfer"][0]) == 0.0
    s, a, c, t = _case(3, 2, 2, 1, seed=5)
    t[1] = s[0, 1, 2]                                            # one target point on one particle of the last step
    got = _run(dev, (s, a, c, t))
    assert torch.isfinite(got["chamfer"]).all()
    _assert_within(got, ref.cost_ref(s, a, c, t, BOX.reshape(4)))


def test_edge_all_particles_identical(dev):
    s, a, c, t = _case(65, 3, 2, 1, seed=6)
    s[:] = s[0, 0, 0]
    c[:] = c[0]
    got = _run(dev, (s, a, c, t))
    _assert_within(got, ref.cost_ref(s, a, c, t, BOX.reshape(4)))


def test_edge_start_point_exactly_at_the_pusher_size(dev):
    """pusher_size = 2^-7 and a start point 2^-7 right of the only near particle: the distance, its root and the difference are exact, d = 0."""
    p = 2.0 ** -7
    s = torch.tensor([[[[0.5, 0.5, 0.01], [0.9, 0.1, 0.0]]]])
    a = torch.tensor([[[0.5 + p, 0.5, 0.0, 10.0]]])
    t = torch.tensor([[0.3, 0.3, 0.0]])
    got = _run(dev, (s, a, s[0, 0].clone(), t), pusher_size=p)
    assert float(got["collision"][0, 0]) == 1.0
    a[0, 0, 0] = 0.5 + 2 * p                                     # one pusher size further out: exp(-100 * 2^-7)
    got = _run(dev, (s, a, s[0, 0].clone(), t), pusher_size=p)
    assert abs(float(got["collision"][0, 0]) - math.exp(-100 * p)) <= 1e-5


def test_edge_particles_outside_every_wall(dev):
    s, a, c, t = _case(2, 1, 2, 1, seed=7)
    s[0, :, 0, :2] = torch.tensor([-1.0, -1.0])
    s[0, :, 1, :2] = torch.tensor([2.0, 2.0])
    got = _run(dev, (s, a, c, t), bbox=np.array([[0.4, 0.6], [0.4, 0.6]]))
    assert (got["box"] == 1.0).all()
    _assert_within(got, ref.cost_ref(s, a, c, t, np.array([0.4, 0.6, 0.4, 0.6])))


def test_edge_a_nan_coordinate_poisons_its_sample_only(dev):
    s, a, c, t = _case(2, 2, 2, 3, seed=8)
    clean = _run(dev, (s, a, c, t))
    s2 = s.clone()
    s2[1, 1, 0, 0] = math.nan                                   # sample 1, last step
    got = _run(dev, (s2, a, c, t))
    assert math.isnan(float(got["reward_seqs"][1])) and math.isnan(float(got["chamfer"][1])) and math.isnan(float(got["box"][1, 1]))
    for k in got:
        assert torch.equal(got[k][0], clean[k][0]) and torch.equal(got[k][2], clean[k][2]), k
    s3 = s.clone()
    s3[1, 0, 1, 1] = math.nan                                   # sample 1, first step: its box term and the next push's collision term
    got = _run(dev, (s3, a, c, t))
    assert math.isnan(float(got["reward_seqs"][1])) and math.isnan(float(got["collision"][1, 1])) and math.isnan(float(got["box"][1, 0]))
    assert torch.isfinite(got["chamfer"]).all() and torch.isfinite(got["reward_seqs"][[0, 2]]).all()
    want = ref.cost_ref(s3, a, c, t, BOX.reshape(4))
    assert np.isnan(want["reward"][1]) and np.isnan(want["collision"][1, 1])          # the fp64 statement agrees on where the NaN goes


# ------------------------------------------------------------------------------------------ the update
RW, PUSH = 500.0, 0.01
LOWER, UPPER = [0.0, 0.0, -math.pi, 5.0], [1.0, 1.0, math.pi, 20.0]     # the length's lower limit sits below the 7 push lengths every combination keeps: no clamp hides a length error
THETA0 = (0.0, math.pi / 2, -2.0, math.pi)
SPREADS = (0.0, 1.0, 50.0, 5.0e6)                                 # reward_weight * (largest - smallest reward)
UPDATE_CASES = [(B, (1, 3)[(i + j) % 2], SPREADS[j], THETA0[(i + j) % 4]) for i, B in enumerate((1, 2, 63, 64, 65, 1000, 1025)) for j in range(4)]


def _update_case(B, T, spread, theta0, seed=0):
    """Lengths in [10, 20], angles within +-pi/4 of theta0: every convex combination keeps a displacement of at least 7 push lengths."""
    g = torch.Generator().manual_seed(seed * 7919 + B * 13 + T)
    r = lambda *sh: torch.rand(sh, generator=g)  # noqa: E731
    acts = torch.cat([r(B, T, 2), theta0 + (r(B, T, 1) * 2 - 1) * (math.pi / 4), r(B, T, 1) * 10 + 10], 2)
    u = r(B)
    if B > 1:
        u[0], u[B - 1] = 1.0, 0.0
    return acts, -6.0 - u * (spread / RW)


def _update(dev, acts, rewards, rw=RW):
    from gsdyn import mppi_update
    out = mppi_update(acts.to(dev), rewards.to(dev), reward_weight=rw, lower=LOWER, upper=UPPER, push_length=PUSH)
    torch.cuda.synchronize()
    return out["act_seq"].double().cpu().numpy(), int(out["best_index"]), float(out["best_reward"])


def _wrapped(d):
    return np.abs(np.mod(d + math.pi, 2 * math.pi) - math.pi)


def _update_distances(seq, want, acts):
    col = acts.double().abs().amax((0, 1)).numpy()
    return (np.max(np.abs(seq[:, 0] - want[:, 0])) / col[0], np.max(np.abs(seq[:, 1] - want[:, 1])) / col[1], np.max(_wrapped(seq[:, 2] - want[:, 2])),
            np.max(np.abs(seq[:, 3] - want[:, 3]) / want[:, 3]))


@pytest.mark.parametrize("B,T,spread,theta0", UPDATE_CASES)
def test_update_against_fp64(dev, B, T, spread, theta0):
    acts, rewards = _update_case(B, T, spread, theta0)
    seq, best, rmax = _update(dev, acts, rewards)
    want, w_best, w_rmax = ref.update_ref(acts, rewards, RW, LOWER, UPPER, PUSH)
    ex, ey, et, el = _update_distances(seq, want, acts)
    _log(f"update B={B:4d} T={T} rw*spread={spread:9.1f} theta0={theta0:+.3f}: x {ex:.2e}, y {ey:.2e} of the column, theta {et:.2e} rad, length rel {el:.2e}")
    assert best == w_best and rmax == w_rmax
    assert ex <= 2e-5 and ey <= 2e-5 and et <= 1e-4 and el <= 1e-4


def test_update_best_index_ties_go_to_the_lowest_index(dev):
    acts, rewards = _update_case(1025, 1, 1.0, 0.0, seed=1)
    top = float(rewards.max()) + 0.5
    for places, expect in (((1024, 3), 3), ((700, 64, 65), 64), ((1024,), 1024), ((1, 1000), 1)):       # one thread, two waves, the last sample
        r = rewards.clone()
        r[list(places)] = top
        assert _update(dev, acts, r)[1:] == (expect, top)
    assert _update(dev, acts, torch.full((1025,), -6.0))[1] == 0


def test_update_minus_infinity_gets_weight_zero(dev):
    acts, rewards = _update_case(65, 3, 1.0, -2.0, seed=2)
    r = torch.full((130,), -math.inf)
    r[::2] = rewards                                              # every second sample is dead
    a = torch.zeros((130, 3, 4))
    a[::2] = acts
    a[1::2] = torch.tensor([0.9, 0.9, 3.0, 20.0])
    with_dead, live = _update(dev, a, r), _update(dev, acts, rewards)
    assert with_dead[1] == 2 * live[1] and with_dead[2] == live[2]
    assert max(_update_distances(with_dead[0], live[0], acts)) <= 1e-6            # the same terms in another partition of the sums


def test_update_nan_reward(dev):
    acts, rewards = _update_case(65, 3, 1.0, 0.0, seed=3)
    rewards[40] = math.nan
    rewards[64] = math.nan
    seq, best, rmax = _update(dev, acts, rewards)
    assert np.isnan(seq).all() and best == 40 and math.isnan(rmax)


def test_update_is_bit_identical_from_run_to_run(dev):
    from gsdyn import mppi_update
    acts, rewards = _update_case(1000, 3, 50.0, math.pi, seed=4)
    a, r = acts.to(dev), rewards.to(dev)
    one = mppi_update(a, r, reward_weight=RW, lower=LOWER, upper=UPPER, push_length=PUSH)
    two = mppi_update(a, r, reward_weight=RW, lower=LOWER, upper=UPPER, push_length=PUSH)
    for k in one:
        assert torch.equal(one[k], two[k]), k


def test_update_device_path_against_the_torch_fallback_on_the_device(dev):
    from gsdyn import plan
    acts, rewards = _update_case(1000, 3, 50.0, math.pi / 2, seed=5)
    seq, best, rmax = _update(dev, acts, rewards)
    lo, hi = torch.tensor(LOWER, device=dev), torch.tensor(UPPER, device=dev)
    f_seq, f_best, f_rmax = plan._mppi_update_reference(acts.to(dev), rewards.to(dev), RW, lo, hi, PUSH)
    e = _update_distances(seq, f_seq.double().cpu().numpy(), acts)
    assert best == int(f_best) and rmax == float(f_rmax)
    assert e[0] <= 2e-5 and e[1] <= 2e-5 and e[2] <= 1e-4 and e[3] <= 1e-4


# ------------------------------------------------------------------------------------------ end to end
def test_plan_actions_on_the_device_picks_what_the_cpu_picks(dev):
    """Width-16 model, 12 particles, n_sample = 8, chunk = 4, T = 2, one CPU generator for both calls (the sampler draws on the generator's
    device).  The seed is one whose top two rewards differ by more than 1e-2 within either chunk and between the chunks' winners on the CPU,
    checked here first; if the two rollouts' fp32 differences flipped a choice all the same, both rewards are printed and the test fails."""
    from gsdyn import plan_actions, rollout_actions, running_cost, sample_action_seq
    from test_plan_cost_cpu import BBOX, LOWER as LO, UPPER as UP, plan_case
    model, state, target, seq0, kw = plan_case()
    g, tops = torch.Generator().manual_seed(kw["generator"].initial_seed()), []
    for n in (4, 4):
        acts = sample_action_seq(seq0, LO, UP, n, iter_index=0, noise_level=1.0, push_length=0.05, generator=g)
        out = rollout_actions(model, state, acts, push_length=0.05, adj_thresh=0.12)["state_seqs"]
        r = running_cost(out, acts, state, target, BBOX)["reward_seqs"].sort(descending=True).values
        assert float(r[0] - r[1]) > 1e-2, "the seed has a near-tie within a chunk"
        tops.append(float(r[0]))
    assert abs(tops[0] - tops[1]) > 1e-2, "the seed has a near-tie between the chunks"
    cpu = plan_actions(model, state, target, BBOX, seq0, **kw)
    model_d, state_d, target_d, seq0_d, kw_d = plan_case(device=dev)
    gpu = plan_actions(model_d, state_d, target_d, BBOX, seq0_d, **kw_d)
    torch.cuda.synchronize()
    _log(f"plan_actions: chunk rewards cpu {cpu['chunk_rewards'].tolist()}, device {gpu['chunk_rewards'].tolist()}; reward cpu {float(cpu['reward']):.6f}, "
         f"device {float(gpu['reward']):.6f}")
    assert gpu["act_seq"].is_cuda and gpu["state_seqs"].shape == (2, 12, 3) and gpu["chunk_rewards"].shape == (2,)
    assert int(torch.argmax(gpu["chunk_rewards"])) == int(torch.argmax(cpu["chunk_rewards"]))
    assert torch.equal(gpu["act_seq"].cpu(), cpu["act_seq"])                         # the same sample of the same chunk
    assert abs(float(gpu["reward"]) - float(cpu["reward"])) <= 1e-3
    assert (gpu["chunk_rewards"].cpu() - cpu["chunk_rewards"]).abs().max() <= 1e-3
