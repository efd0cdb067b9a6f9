"""GPU tests of the planner's rollout (gsdyn/plan.py, csrc/gsr_plan.hip): the batched relations against the single-graph kernel and
against torch, the glue kernels against their torch statements (bit for bit), one batched model call and a whole rollout against fp64
evaluations on the host.  The measured distances are appended to plan_rollout_parity.log next to the other GPU logs (hipcheck's row-margins
log; ``GSR_PLAN_PARITY_LOG`` names another file); profiles/plan_rollout_parity.txt is that log of one run, copied by hand under a
one-line header -- the tests do not rewrite a committed file on every run."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from hipcheck import _ROW_LOG  # noqa: E402

_LOG = os.environ.get("GSR_PLAN_PARITY_LOG", os.path.join(os.path.dirname(_ROW_LOG), "plan_rollout_parity.log"))      # next to hipcheck's row-margins log


def _log(line):
    print(line)
    try:
        os.makedirs(os.path.dirname(_LOG), exist_ok=True)
        with open(_LOG, "a") as f:
            f.write(line + "\n")
    except OSError as e:
        print(f"(plan_rollout_parity.log not written: {e})")


def _cfg(width=16, **kw):
    c = dict(nf_particle=width, nf_relation=width, nf_effect=width, attr_dim=2, state_dim=0, action_dim=3, pstep=3, rel_attr_dim=2,
             rel_group_dim=1, rel_distance_dim=3, n_his=3)
    c.update(kw)
    return c


def _model(width, seed=0, motion_scale=1.0, **kw):
    from gsdyn.dynamics import DynamicsPredictor
    torch.manual_seed(seed)
    m = DynamicsPredictor(_cfg(width, **kw)).eval()
    with torch.no_grad():
        m.non_rigid_predictor.linear_2.weight.mul_(motion_scale)
        m.non_rigid_predictor.linear_2.bias.mul_(motion_scale)
    return m


# ------------------------------------------------------------------------------------------ relations
def _bound(n_obj, topk):
    return n_obj * min(topk, n_obj) + 2 * n_obj


def _expected_from_single_graph_kernel(pos, nv, thr, topk, e_cap):
    """Per-sample gsr_construct_edges_rows (the existing kernel), shifted by b R and concatenated: what the batch kernel must give."""
    from diff_gaussian_rasterization import _hip
    B, R = pos.shape[0], pos.shape[1]
    dev = pos.device
    recv, send, rows, base = [], [], [], 0
    for b in range(B):
        r, s, c, _, rs = _hip.construct_edges_padded(pos[b], nv, thr, topk, _bound(R - 1, topk), R, dense_n=R + 1, row_start=True)
        m = int(c.item())
        recv.append(r[:m] + b * R)
        send.append(s[:m] + b * R)
        rows.append(rs[:R] + base)
        base += m
    pad = torch.full((e_cap - base,), B * R, dtype=torch.int64, device=dev)
    tail = torch.tensor([base, e_cap], dtype=torch.int64, device=dev)
    return torch.cat(recv + [pad]), torch.cat(send + [pad]), base, torch.cat(rows + [tail])


def _positions(kind, B, R, g):
    if kind == "lattice":                        # a quarter-unit lattice: many exactly equal distances
        return torch.randint(0, 4, (B, R, 3), generator=g).float() * 0.25
    return torch.rand((B, R, 3), generator=g)


@pytest.mark.parametrize("n_obj_cap", [1, 5, 63, 64, 65, 127])
def test_batched_relations_equal_the_single_graph_kernel(dev, n_obj_cap):
    from diff_gaussian_rasterization import _hip
    g = torch.Generator().manual_seed(100 + n_obj_cap)
    R = n_obj_cap + 1
    met_bound = only_self = False
    for B in (1, 2, 3, 65):
        for n_valid in sorted({0, 1, n_obj_cap - 1, n_obj_cap}):
            nv = torch.tensor([n_valid], dtype=torch.int32, device=dev)
            for topk in (1, 5, 16):
                e_cap = B * _bound(n_obj_cap, topk)
                assert e_cap == _hip.plan_edge_capacity(B, n_obj_cap, topk)
                for kind, thr in (("random", 0.3), ("lattice", 0.3), ("random", 1e-6), ("random", 1e3)):
                    pos = _positions(kind, B, R, g).to(dev)
                    recv, send, cnt, rows = _hip.construct_edges_batch(pos, nv, thr, topk, e_cap)
                    w_recv, w_send, w_cnt, w_rows = _expected_from_single_graph_kernel(pos, nv, thr, topk, e_cap)
                    tag = (B, n_obj_cap, n_valid, topk, kind, thr)
                    assert int(cnt.item()) == w_cnt, tag
                    assert rows.shape == (B * R + 2,) and torch.equal(rows, w_rows), tag
                    assert torch.equal(recv, w_recv) and torch.equal(send, w_send), tag
                    if thr == 1e-6:               # only self-relations, none with the tool
                        assert w_cnt == B * n_valid and torch.equal(recv[:w_cnt], send[:w_cnt]), tag
                        only_self = only_self or n_valid > 0
                    if thr == 1e3 and n_valid == n_obj_cap:
                        assert w_cnt == e_cap, tag      # the bound is met exactly: no padding at all
                        met_bound = True
    assert met_bound and only_self


def test_batched_relations_equal_torch_for_tie_free_positions(dev):
    from diff_gaussian_rasterization import _hip
    from gsdyn.dynamics import construct_edges
    g = torch.Generator().manual_seed(5)
    for B, cap, n_valid, topk, thr in ((3, 20, 20, 5, 0.4), (2, 65, 40, 5, 0.3), (65, 12, 12, 3, 0.5), (1, 127, 127, 16, 0.25)):
        R = cap + 1
        pos = torch.rand((B, R, 3), generator=g)
        recv, send, cnt, rows = _hip.construct_edges_batch(pos.to(dev), torch.tensor([n_valid], dtype=torch.int32, device=dev), thr, topk)
        m = int(cnt.item())
        mask = torch.ones(n_valid + 1, dtype=torch.bool); tool = torch.zeros(n_valid + 1, dtype=torch.bool); tool[n_valid] = True    # noqa: E702
        remap = torch.cat([torch.arange(n_valid), torch.tensor([cap])])
        want = []
        for b in range(B):
            comp = torch.cat([pos[b, :n_valid], pos[b, cap:]], 0)
            r, s = construct_edges(comp, thr, mask, tool, topk=topk)
            want.append(torch.stack([remap[r], remap[s]], 1) + b * R)
        want = torch.cat(want)
        assert m == want.shape[0] and torch.equal(torch.stack([recv[:m], send[:m]], 1).cpu(), want), (B, cap, n_valid, topk)
        assert bool((recv[m:] == B * R).all()) and bool((send[m:] == B * R).all())
        assert torch.equal(rows[:B * R + 1].cpu(), torch.searchsorted(recv[:m].cpu(), torch.arange(B * R + 1)))


def test_capacity_below_the_bound_is_refused(dev):
    from diff_gaussian_rasterization import _hip
    pos = torch.rand((3, 13, 3)).to(dev)
    nv = torch.tensor([12], dtype=torch.int32, device=dev)
    bound = _hip.plan_edge_capacity(3, 12, 5)
    with pytest.raises(RuntimeError, match="bound"):
        _hip.construct_edges_batch(pos, nv, 0.3, 5, bound - 1)
    recv, _, cnt, _ = _hip.construct_edges_batch(pos, nv, 0.3, 5, bound)
    assert recv.shape == (bound,) and 0 < int(cnt.item()) <= bound


# ------------------------------------------------------------------------------------------ glue
def _head_statement(hist, eef_hist, delta, a, inst, with_state):
    B, n_his, n_obj = hist.shape[0], hist.shape[1], hist.shape[2]
    R = n_obj + 1
    states = torch.cat([hist, eef_hist[:, :, None]], 2)                                   # [B, n_his, R, 3]
    st = torch.cat([states.transpose(1, 2).reshape(B * R, 3 * n_his), torch.zeros((1, 3 * n_his), device=hist.device)], 0)
    act = torch.zeros((B, R, 3), device=hist.device)
    act[:, n_obj] = delta
    act = torch.cat([act.reshape(B * R, 3), torch.zeros((1, 3), device=hist.device)], 0)
    p_in = torch.cat([a] + ([st] if with_state else []) + [act], 1)
    nodes = torch.cat([a, inst[:, None], st], 1)
    return st, p_in, nodes, states[:, -1].contiguous()


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("n_his", [1, 3])
def test_glue_kernels_equal_their_torch_statements(dev, B, n_his):
    from diff_gaussian_rasterization import _hip
    g = torch.Generator().manual_seed(7 * B + n_his)
    for n_obj, T in ((20, 2), (127, 3), (1, 1)):
        R = n_obj + 1
        rnd = lambda *sh: torch.rand(sh, generator=g).to(dev)  # noqa: E731
        hist, eef_hist, delta = rnd(B, n_his, n_obj, 3), rnd(B, n_his, 3), rnd(B, 3) - 0.5
        a, inst = rnd(B * R + 1, 2), rnd(B * R + 1)
        if n_obj >= 2:
            hist[0, -1, 0:2, 2] = -4.0                    # two particles of sample 0 end at exactly -5: a shared lowest z
        for with_state in (False, True):
            got = _hip.plan_step_head(hist, eef_hist, delta, a, inst, with_state)
            want = _head_statement(hist, eef_hist, delta, a, inst, with_state)
            for x, y, name in zip(got, want, ("state_rows", "particle_inputs", "rel_nodes", "states_last")):
                assert x.shape == y.shape and torch.equal(x, y), (name, B, n_his, n_obj, with_state)
        # tail: motions beyond the clamp on both sides, two particles sharing the lowest predicted z in sample 0
        mot = (torch.rand((B * R + 1, 3), generator=g) * 4 - 2).to(dev)
        clampv = 1.0
        if n_obj >= 2:
            mot[0:2, 2] = -7.0                            # clamped to -1: predicted z = -4 - 1, every other particle stays above -1
        for repeat_kind in ("none", "some", "all"):
            ai, li = 2, T - 1
            rep = torch.full((B, T), 7, dtype=torch.int32)
            if repeat_kind == "all":
                rep[:, li] = ai
            elif repeat_kind == "some":
                rep[::2, li] = ai
            rep = rep.to(dev)
            h2, e2 = hist.clone(), eef_hist.clone()
            out = torch.full((B, T, n_obj, 3), -3.0, device=dev)
            want_out = out.clone()
            _hip.plan_step_tail(mot, delta, rep, h2, e2, out, ai, li, clampv)
            pred = hist[:, -1] + torch.clamp(mot[:B * R].view(B, R, 3)[:, :n_obj], -clampv, clampv)
            zmin = pred[:, :, 2].min(dim=1).values
            eef_new = torch.cat([eef_hist[:, -1, :2] + delta[:, :2], zmin[:, None]], 1)
            keep = rep[:, li] == ai
            want_out[keep, li] = pred[keep]
            assert torch.equal(h2, torch.cat([hist[:, 1:], pred[:, None]], 1)), (B, n_his, n_obj, repeat_kind)
            assert torch.equal(e2, torch.cat([eef_hist[:, 1:], eef_new[:, None]], 1)), (B, n_his, n_obj, repeat_kind)
            assert torch.equal(out, want_out), (B, n_his, n_obj, repeat_kind)
            assert int(keep.sum()) == {"none": 0, "some": (B + 1) // 2, "all": B}[repeat_kind]
            if n_obj >= 2:
                p0 = pred[0, :, 2]
                assert float(p0[0]) == float(p0[1]) == float(zmin[0]) and int((p0 == zmin[0]).sum()) >= 2      # a shared minimum


# ------------------------------------------------------------------------------------------ one model call
def _one_call_inputs(B, n_obj, n_his, g, dev):
    hist = torch.rand((B, n_his, n_obj, 3), generator=g) * torch.tensor([0.4, 0.4, 0.05])
    eef_hist = torch.rand((B, n_his, 3), generator=g) * torch.tensor([0.4, 0.4, 0.05])
    delta = torch.cat([(torch.rand((B, 2), generator=g) - 0.5) * 0.05, torch.zeros((B, 1))], 1)
    return hist.to(dev), eef_hist.to(dev), delta.to(dev)


def _one_call_errors(model, B, n_obj, dev, g, thr=0.15, topk=5):
    """(yardstick, batched, yardstick_pos, batched_pos): the largest distance of the per-sample split path and of the batched path from an
    fp64 host evaluation of ``_propagate`` on the same relations -- of the motions, relative to the largest motion, and of the predicted
    positions (last + clamp(motion), the fp32 addition's rounding included), absolute."""
    from diff_gaussian_rasterization import _hip
    from gsdyn.plan import _sample_constants
    import copy
    n_his, R = model.model_config["n_his"], n_obj + 1
    hist, eef_hist, delta = _one_call_inputs(B, n_obj, n_his, g, dev)
    a1, g1, _, _ = _sample_constants(model, n_obj, dev, torch.float32)
    a = torch.cat([a1.repeat(B, 1), torch.zeros((1, 2), device=dev)], 0).contiguous()
    gi = torch.cat([g1.repeat(B, 1), torch.zeros((1, 1), device=dev)], 0).contiguous()
    with torch.no_grad():
        st, p_in, nodes, last = _hip.plan_step_head(hist, eef_hist, delta, a, gi.view(-1), False)
        recv, send, cnt, rows = _hip.construct_edges_batch(last, torch.tensor([n_obj], dtype=torch.int32, device=dev), thr, topk)
        _, mot = model._propagate_split(None, a, gi, None, recv, send, dummy_last_row=True, p_in=p_in, nodes=nodes, row_start=rows, motion_only=True)
        m64 = copy.deepcopy(model).double().cpu()
        rows_h, recv_h, send_h = rows.cpu(), recv.cpu(), send.cpu()
        e_y = e_b = p_y = p_b = scale = 0.0
        for b in range(B):
            lo, hi = int(rows_h[b * R]), int(rows_h[(b + 1) * R])
            r_b, s_b = recv_h[lo:hi] - b * R, send_h[lo:hi] - b * R
            st_b = st[b * R:(b + 1) * R]
            act = torch.zeros((R, 3), device=dev)
            act[n_obj] = delta[b]
            ref_pos, ref = m64._propagate(st_b.double().cpu(), a1.double().cpu(), g1.double().cpu(), act.double().cpu(), r_b, s_b)
            assert model._split_ok(a1)
            one_pos, one = model._propagate_split(st_b, a1, g1, act, r_b.to(dev), s_b.to(dev))    # the existing per-sample device path
            ref, ref_pos = ref[:n_obj], ref_pos[:n_obj]
            mot_b = mot[b * R:b * R + n_obj]
            pos_b = st_b[:n_obj, -3:] + torch.clamp(mot_b, -model.motion_clamp, model.motion_clamp)      # gsr_plan_step_tail's arithmetic
            scale = max(scale, float(ref.abs().max()))
            e_y = max(e_y, float((one[:n_obj].double().cpu() - ref).abs().max()))
            e_b = max(e_b, float((mot_b.double().cpu() - ref).abs().max()))
            p_y = max(p_y, float((one_pos[:n_obj].double().cpu() - ref_pos).abs().max()))
            p_b = max(p_b, float((pos_b.double().cpu() - ref_pos).abs().max()))
    assert int(cnt.item()) > B * n_obj                     # more than the self-relations: the graphs are connected
    return e_y / scale, e_b / scale, p_y, p_b


@pytest.mark.parametrize("width", [16, 64])
@pytest.mark.parametrize("B", [1, 2, 65])
def test_one_batched_model_call_against_fp64(dev, B, width):
    """The bound is measured: the existing per-sample device path's distance from fp64 on the same inputs; the batched path may be twice
    as far off (both are fp32 and differ in GEMM tiling and row count only; the 2 covers another library kernel at the larger M)."""
    model = _model(width, seed=width).to(dev)
    g = torch.Generator().manual_seed(B + width)
    e_y, e_b, p_y, p_b = _one_call_errors(model, B, 20, dev, g)
    _log(f"one model call  B={B:3d} width={width:3d}: per-sample split path {e_y:.3e}, batched {e_b:.3e} of the largest motion; "
         f"positions {p_y:.3e} / {p_b:.3e} absolute (fp64 host reference)")
    assert e_b <= 2.0 * e_y and p_b <= 2.0 * p_y, (B, width, e_y, e_b, p_y, p_b)


# ------------------------------------------------------------------------------------------ whole rollout
ROLL = dict(B=5, T=2, n_obj=20, width=16, seed=13, thr=0.135, topk=5, push=0.02, motion_scale=0.02)
ROLL_REPEATS = ((1, 3), (2, 1), (3, 2), (1, 1), (2, 3))


def _roll_case(seed=None):
    """20 particles on a jittered 5 x 4 grid of spacing 0.1 (the threshold 0.135 lies between the grid's 0.1 and its diagonal 0.141), small
    motions: the relation decisions of the fp64 reference keep a margin (asserted by the test), found by a seed search on the host."""
    seed = ROLL["seed"] if seed is None else seed
    g = torch.Generator().manual_seed(1000 + seed)
    B, T, n_obj = ROLL["B"], ROLL["T"], ROLL["n_obj"]
    ix = torch.arange(n_obj, dtype=torch.float64)
    grid = torch.stack([(ix % 5) * 0.1, torch.div(ix, 5, rounding_mode="floor") * 0.1, torch.zeros(n_obj, dtype=torch.float64)], 1)
    state = grid + (torch.rand((n_obj, 3), generator=g, dtype=torch.float64) - 0.5) * torch.tensor([0.012, 0.012, 0.01], dtype=torch.float64)
    xy = torch.rand((B, T, 2), generator=g, dtype=torch.float64) * torch.tensor([0.4, 0.3], dtype=torch.float64)
    theta = (torch.rand((B, T, 1), generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    length = torch.tensor(ROLL_REPEATS, dtype=torch.float64)[:, :, None] + 0.5
    model = _model(ROLL["width"], seed=seed, motion_scale=ROLL["motion_scale"])
    return model, state.float(), torch.cat([xy, theta, length], 2).float()          # fp32: the reference starts from the same numbers


def _relation_margins(points, thr, topk):
    """points [R, 3] fp64, the tool last -> (the smallest relative distance of a squared pair distance from thr^2 over the pairs the rule
    looks at, the smallest relative gap between a receiver's k-th and (k + 1)-th nearest object)."""
    n_obj = points.shape[0] - 1
    d = ((points[:, None] - points[None]) ** 2).sum(-1)
    t2 = thr * thr
    m_thr = float(((d - t2).abs() / t2).min())
    k = min(topk, n_obj)
    m_k = float("inf")
    if k < n_obj:
        s = torch.sort(d[:n_obj, :n_obj], dim=1).values
        m_k = float(((s[:, k] - s[:, k - 1]) / s[:, k]).min())
    return m_thr, m_k


def _fp64_reference_rollout():
    from gsdyn.plan import rollout_actions
    model, state, actions = _roll_case()
    trace = []
    out = rollout_actions(model.double(), state.double(), actions.double(), push_length=ROLL["push"], adj_thresh=ROLL["thr"], topk=ROLL["topk"], n_his=3, _trace=trace)
    calls = {}
    for s, e, tr in trace:
        for b, li, ai, pts, recv, send in tr:
            calls[(s + b, li, ai)] = (pts, recv, send)
    return out["state_seqs"], calls


@pytest.fixture(scope="module")
def roll_reference():
    return _fp64_reference_rollout()


def test_whole_rollout_against_the_fp64_fallback(dev, roll_reference):
    from gsdyn.plan import rollout_actions
    ref, calls = roll_reference
    n_calls = sum(sum(r) for r in ROLL_REPEATS)
    assert len(calls) == n_calls
    margins = [_relation_margins(p, ROLL["thr"], ROLL["topk"]) for p, _, _ in calls.values()]
    m_thr, m_k = min(m[0] for m in margins), min(m[1] for m in margins)
    assert m_thr >= 1e-3 and m_k >= 1e-3, (m_thr, m_k)                 # the reference ITSELF decides every relation with a margin
    model, state, actions = _roll_case()
    model = model.to(dev)
    trace = []
    got = rollout_actions(model, state.to(dev), actions.to(dev), push_length=ROLL["push"], adj_thresh=ROLL["thr"], topk=ROLL["topk"], n_his=3,
                          _trace=trace)["state_seqs"]
    (s, e, tr), = trace
    R = ROLL["n_obj"] + 1
    seen = 0
    for li, ai, last, recv, send, cnt in tr:                            # the batched lists, cut per sample, against the reference's
        m = int(cnt.item())
        recv, send = recv[:m].cpu(), send[:m].cpu()
        for b in range(ROLL["B"]):
            if (b, li, ai) not in calls:
                continue                                                # (a call beyond the sample's repeat count: discarded)
            sel = (recv >= b * R) & (recv < (b + 1) * R)
            _, w_recv, w_send = calls[(b, li, ai)]
            assert torch.equal(recv[sel] - b * R, w_recv) and torch.equal(send[sel] - b * R, w_send), (b, li, ai)
            seen += 1
    assert seen == n_calls
    # positions: the one-call bound -- the per-sample device path's own distance from fp64 for THIS model at this position scale (the
    # predicted positions: motion error + the rounding of the fp32 addition), doubled -- times the model calls behind a state
    # (the yardstick is taken on fresh random inputs in a 0.4 box, not on the rollout's own states: it is tied to the case under test by the
    # model, the threshold, the particle count and the position scale only)
    g = torch.Generator().manual_seed(11)
    _, _, p_y, _ = _one_call_errors(model, ROLL["B"], ROLL["n_obj"], dev, g, thr=ROLL["thr"])
    disp = float((ref - state.double()[None, None]).abs().max())
    err = float((got.double().cpu() - ref).abs().max())
    depth = max(sum(r) for r in ROLL_REPEATS)
    bound = 2.0 * p_y * depth
    _log(f"whole rollout   B={ROLL['B']} T={ROLL['T']} n_obj={ROLL['n_obj']}: margins thr {m_thr:.2e} k {m_k:.2e}; largest displacement {disp:.3e}, "
         f"max abs error {err:.3e}, bound {bound:.3e} (= 2 x {p_y:.3e} x {depth} calls)")
    assert disp > 1e-3 and err <= bound, (err, bound)


def test_rollout_is_deterministic_and_chunking_stays_within_the_one_call_bound(dev):
    from gsdyn.plan import rollout_actions
    model, state, actions = _roll_case()
    model, state, actions = model.to(dev), state.to(dev), actions.to(dev)
    kw = dict(push_length=ROLL["push"], adj_thresh=ROLL["thr"], topk=ROLL["topk"], n_his=3)
    a = rollout_actions(model, state, actions, **kw)["state_seqs"]
    b = rollout_actions(model, state, actions, **kw)["state_seqs"]
    assert torch.equal(a, b)
    c2 = rollout_actions(model, state, actions, chunk=2, **kw)["state_seqs"]
    c5 = rollout_actions(model, state, actions, chunk=5, **kw)["state_seqs"]
    assert torch.equal(c5, a)
    g = torch.Generator().manual_seed(11)
    _, _, p_y, _ = _one_call_errors(model, ROLL["B"], ROLL["n_obj"], dev, g, thr=ROLL["thr"])
    err = float((c2 - c5).abs().max())
    _log(f"chunk 2 vs 5: max abs difference {err:.3e}, one-call bound {2.0 * p_y:.3e}")
    assert err <= 2.0 * p_y


def test_refused_models_and_sizes_take_the_fallback(dev, monkeypatch):
    """nf_effect = 18 is no multiple of 4 (the split path refuses), 128 particles exceed the kernels' 127: both run the torch fallback on the
    device -- seen by wrapping the two paths -- and agree with a direct call of it.  The fallback's ``index_add_`` sums with atomics on a
    device, so two runs differ in the order of fp32 additions: a few units of 6e-8 per sum, some tens of summands, five calls in a row --
    1e-5 of the largest displacement bounds it with room.  A model the kernels serve does take them."""
    from gsdyn import plan
    model, state, actions = _roll_case()
    model, state, actions = model.to(dev), state.to(dev), actions.to(dev)
    kw = dict(push_length=ROLL["push"], adj_thresh=ROLL["thr"], topk=ROLL["topk"], n_his=3)
    taken = []
    ref_fn, dev_fn = plan._rollout_reference, plan._rollout_device
    monkeypatch.setattr(plan, "_rollout_reference", lambda *a, **k: (taken.append("fallback"), ref_fn(*a, **k))[1])
    monkeypatch.setattr(plan, "_rollout_device", lambda *a, **k: (taken.append("kernels"), dev_fn(*a, **k))[1])
    odd = _model(18, seed=1, motion_scale=ROLL["motion_scale"]).to(dev)
    got = plan.rollout_actions(odd, state, actions, **kw)["state_seqs"]
    assert taken == ["fallback"] and got.is_cuda
    with torch.no_grad():
        dec, rep = plan.decode_action(actions, ROLL["push"])
        want = ref_fn(odd, state, dec, rep.cpu().tolist(), ROLL["thr"], ROLL["topk"], 3)
    disp = float((want - state[None, None]).abs().max())
    assert disp > 1e-3 and float((got - want).abs().max()) <= 1e-5 * disp
    big = (torch.rand((128, 3), generator=torch.Generator().manual_seed(2)) * 0.5).to(dev)
    out = plan.rollout_actions(model, big, actions[:1, :1], **kw)["state_seqs"]
    assert taken == ["fallback", "fallback"] and out.shape == (1, 1, 128, 3) and torch.isfinite(out).all()
    plan.rollout_actions(model, state, actions, chunk=3, **kw)
    assert taken == ["fallback", "fallback", "kernels", "kernels"]
