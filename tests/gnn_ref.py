"""The propagation network (gsdyn.dynamics.DynamicsPredictor) and the two kernels between its matrix products (csrc/gsr_gnn.hip), restated
in plain numpy -- the reference of tests/test_gnn_ref_cpu.py (which checks THIS file against the torch module in fp64 and the committed
goldens) and tests/test_gnn_kernels_gpu.py (which checks the device paths against it).  Nothing here imports the torch modules: the weights
arrive as a dict of arrays under the names of the module's ``state_dict``.

The second half is the test matrix both files share: the eleven model configurations, the case shape (20 object particles + one tool, 8 seeded
input sets per configuration) and the yardstick ``y_c`` -- the distance of the HOST fp32 ``_propagate`` from the fp64 reference, the unit in
which the device paths' distance is bounded.  Those helpers use torch (for the module under test and ``construct_edges``), imported lazily."""
import functools

import numpy as np

U24 = 2.0 ** -24          # the unit roundoff of fp32 (round to nearest)


# ------------------------------------------------------------------------------------------ the two kernels
def rel_inputs(nodes, recv, send, A, G, dtype=np.float64):
    """nodes [N, A + G + S] = (attributes | instance columns | state) -> the relation encoder's input rows [E, 2 A + 1 + S] =
    (attributes[recv], attributes[send], sum_k |instance[recv, k] - instance[send, k]|, state[recv] - state[send]), evaluated in ``dtype``.
    With ``dtype=np.float32`` this is the kernel's own arithmetic: gathers, one subtraction per difference column, the group column summed
    over ascending k from 0."""
    x = np.asarray(nodes, dtype=dtype)
    recv, send = np.asarray(recv, dtype=np.int64), np.asarray(send, dtype=np.int64)
    xr, xs = x[recv], x[send]
    grp = np.zeros((recv.shape[0],), dtype=dtype)
    for k in range(G):
        grp = grp + np.abs(xr[:, A + k] - xs[:, A + k])
    return np.concatenate([xr[:, :A], xs[:, :A], grp[:, None], xr[:, A + G:] - xs[:, A + G:]], 1).astype(dtype)


def _relu(x):
    return np.where(x < 0, np.zeros_like(x), x)          # as torch.relu: a NaN stays a NaN


def _aggregate(rew1, a23, send, row_start, n_sum, dtype):
    r1, nb = np.asarray(rew1, dtype=dtype), np.asarray(a23, dtype=dtype)
    send, rs = np.asarray(send, dtype=np.int64), np.asarray(row_start, dtype=np.int64)
    N, H = nb.shape[0], nb.shape[1] // 2
    a2, a3 = nb[:, :H], nb[:, H:]
    out = np.zeros((N, H), dtype=dtype)
    if n_sum == 0 or r1.shape[0] == 0:
        return out
    lo = rs[:n_sum]
    deg = rs[1:n_sum + 1] - lo
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(deg.max(initial=0))):          # the j-th entry of every segment that has one: list order per row
            rows = np.nonzero(deg > j)[0]
            e = lo[rows] + j
            out[rows] = out[rows] + _relu((r1[e] + a2[rows]) + a3[send[e]])
    return out


def aggregate(rew1, a23, send, row_start, n_sum):
    """agg[i] = sum over e in [row_start[i], row_start[i + 1]) of relu(rew1[e] + a23[i, :H] + a23[send[e], H:]) for i < n_sum, zero for the
    rows behind; fp64.  rew1 [E, H], a23 [N, 2 H], row_start [N + 1]."""
    return _aggregate(rew1, a23, send, row_start, n_sum, np.float64)


def aggregate_f32(rew1, a23, send, row_start, n_sum):
    """The same in fp32, in list order: each term relu((r1 + a2) + a3) added to a running sum that starts at zero.  Only additions occur
    (nothing a compiler could contract), so this is the kernel's bit-exact statement.  A NaN term stays NaN."""
    return _aggregate(rew1, a23, send, row_start, n_sum, np.float32)


def aggregate_bound(rew1, a23, send, row_start, n_sum):
    """The derived bound of |aggregate_f32 - aggregate| per element: (n_e + 2) 2^-24 sum_e(|r1_e| + |a2| + |a3_e|), n_e = the row's segment
    length, the sum in fp64.  Two roundings per term (both at most 2^-24 of |r1| + |a2| + |a3|; ReLU is 1-Lipschitz, so it does not grow
    them), n_e - 1 roundings of the running sum (each at most 2^-24 of the final sum of magnitudes, to first order; the + 2 in place of + 1
    covers the second-order terms)."""
    r1, nb = np.abs(np.asarray(rew1, dtype=np.float64)), np.abs(np.asarray(a23, dtype=np.float64))
    send, rs = np.asarray(send, dtype=np.int64), np.asarray(row_start, dtype=np.int64)
    N, H = nb.shape[0], nb.shape[1] // 2
    mag = np.zeros((N, H))
    n_e = np.zeros((N,))
    for i in range(n_sum):
        e = np.arange(rs[i], rs[i + 1])
        n_e[i] = e.size
        mag[i] = (r1[e] + nb[i, :H][None] + nb[send[e], H:]).sum(0)
    return (n_e[:, None] + 2) * U24 * mag


# ------------------------------------------------------------------------------------------ the network
def _lin(w, name, x):
    return x @ w[name + ".weight"].T + w[name + ".bias"]


def _mlp3(w, name, x):
    for k in (0, 2, 4):
        x = _relu(_lin(w, f"{name}.model.{k}", x))
    return x


def propagate(weights, cfg, state_t, a, g, act, recv, send, motion_clamp=100.0):
    """The network as ``DynamicsPredictor._propagate`` writes it, fp64: state_t [N, 3 n_his] (oldest first), attributes a [N, attr_dim],
    instance columns g [N, G], action act [N, action_dim] (ignored for action_dim = 0), relations as index vectors [E] -> (predicted
    positions, motions) of all N rows."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    f = lambda x: np.asarray(x, dtype=np.float64)  # noqa: E731
    state_t, a, g = f(state_t), f(a), f(g)
    recv, send = np.asarray(recv, dtype=np.int64), np.asarray(send, dtype=np.int64)
    N, n_his = a.shape[0], int(cfg["n_his"])
    s4 = state_t.reshape(N, n_his, 3)
    parts = [a]
    if cfg["state_dim"] == 3:
        parts.append(state_t)
    elif cfg["state_dim"] == 1:
        parts.append(s4[:, :, 2])
    if int(cfg.get("motion_dim", 0)) > 0:
        parts.append((s4[:, 1:] - s4[:, :-1]).reshape(N, (n_his - 1) * 3))
    if cfg["action_dim"] > 0:
        parts.append(f(act))
    p_inputs = np.concatenate(parts, 1)
    r_inputs = rel_inputs(np.concatenate([a, g, state_t], 1), recv, send, a.shape[1], g.shape[1])
    particle_encode = _mlp3(w, "particle_encoder", p_inputs)
    relation_encode = _mlp3(w, "relation_encoder", r_inputs)
    effect = particle_encode
    for _ in range(int(cfg["pstep"])):
        e_rel = _relu(_lin(w, "relation_propagator.linear", np.concatenate([relation_encode, effect[recv], effect[send]], 1)))
        agg = np.zeros_like(effect)
        np.add.at(agg, recv, e_rel)
        effect = _relu(_lin(w, "particle_propagator.linear", np.concatenate([particle_encode, agg], 1)) + effect)
    x = _relu(_lin(w, "non_rigid_predictor.linear_0", effect))
    x = _relu(_lin(w, "non_rigid_predictor.linear_1", x))
    motion = _lin(w, "non_rigid_predictor.linear_2", x)
    return state_t[:, -3:] + np.clip(motion, -motion_clamp, motion_clamp), motion


# ------------------------------------------------------------------------------------------ the test matrix
def base_cfg(width=16, **kw):
    c = dict(nf_particle=width, nf_relation=width, nf_effect=width, attr_dim=2, state_dim=0, motion_dim=0, action_dim=3, pstep=3, rel_attr_dim=2,
             rel_group_dim=1, rel_distance_dim=3, n_his=3)
    c.update(kw)
    return c


# every configuration differs from the suite's default (C0) in one respect; "instances": the width of p_instance
CONFIGS = {
    "C0": dict(),
    "C1": dict(state_dim=3),
    "C2": dict(state_dim=1),
    "C3": dict(state_dim=3, motion_dim=3),
    "C4": dict(n_his=1, state_dim=3),
    "C5": dict(pstep=1),
    "C6": dict(attr_dim=3, rel_attr_dim=3),
    "C7": dict(nf_particle=8, nf_relation=24, nf_effect=12),
    "C8": dict(nf_particle=4, nf_relation=4, nf_effect=4),
    "C9": dict(action_dim=0),
    "C10": dict(instances=2),
}
N_OBJ, N_SETS, THR, TOPK = 20, 8, 0.15, 5


def weights_of(model):
    return {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()}


def make_model(cfg, seed):
    import torch
    from gsdyn.dynamics import DynamicsPredictor
    torch.manual_seed(seed)
    return DynamicsPredictor(cfg).eval()


def input_sets(cfg, instances, seed, n_sets=N_SETS, n_obj=N_OBJ, thr=THR, topk=TOPK):
    """``n_sets`` seeded inputs of the case shape: ``n_obj`` object particles and one tool (the last row) in a 0.4 x 0.4 x 0.05 box with a
    history of small steps behind the newest positions, the relations of ``construct_edges`` on the host (ascending in the receiver), the
    tool's action in its row.  The attributes (object / tool flag, a random third column where attr_dim = 3) and the instance columns are
    the same in every set of a configuration.  Each set: dict of CPU tensors state_t, a, g, act, recv, send (fp32 / int64) and ``state``
    [n_his, N, 3]."""
    import torch
    from gsdyn.dynamics import construct_edges
    gen = torch.Generator().manual_seed(seed)
    N, n_his, A = n_obj + 1, int(cfg["n_his"]), int(cfg["attr_dim"])
    box = torch.tensor([0.4, 0.4, 0.05])
    a = torch.zeros((N, A))
    a[:n_obj, 0] = 1.0
    a[n_obj, 1] = 1.0
    if A > 2:
        a[:, 2:] = torch.rand((N, A - 2), generator=gen)
    g = torch.zeros((N, instances))
    if instances == 1:
        g[:n_obj] = 1.0
    else:                                               # one-hot instance membership, the objects split evenly
        g[torch.arange(n_obj), torch.arange(n_obj) * instances // n_obj] = 1.0
    mask = torch.ones(N, dtype=torch.bool)
    tool = torch.zeros(N, dtype=torch.bool)
    tool[n_obj] = True
    sets = []
    for _ in range(n_sets):
        last = torch.rand((N, 3), generator=gen) * box
        steps = (torch.rand((n_his, N, 3), generator=gen) - 0.5) * 0.02
        steps[-1] = 0.0
        state = last[None] + torch.flip(torch.cumsum(torch.flip(steps, [0]), 0), [0])       # state[-1] = last
        act = torch.zeros((N, 3))
        act[n_obj, :2] = (torch.rand((2,), generator=gen) - 0.5) * 0.05
        recv, send = construct_edges(state[-1], thr, mask, tool, topk=topk, n_tool=1)
        assert recv.shape[0] > N and bool((recv[1:] >= recv[:-1]).all())
        sets.append(dict(state=state, state_t=state.transpose(0, 1).reshape(N, n_his * 3).contiguous(), a=a, g=g,
                         act=act[:, :int(cfg["action_dim"])].contiguous(), recv=recv, send=send))
    return sets


def errors(pos, mot, ref_pos, ref_mot, n_obj=N_OBJ):
    """(the largest motion error of the object rows relative to the largest fp64 motion, the largest absolute position error)."""
    ref_pos, ref_mot = ref_pos[:n_obj], ref_mot[:n_obj]
    e_m = float(np.abs(np.asarray(mot, dtype=np.float64)[:n_obj] - ref_mot).max() / np.abs(ref_mot).max())
    e_p = float(np.abs(np.asarray(pos, dtype=np.float64)[:n_obj] - ref_pos).max())
    return e_m, e_p


def yardstick(model, sets):
    """(y, p_y, refs): the host fp32 ``_propagate``'s distance from ``propagate`` over the input sets -- motions relative to the largest
    fp64 motion of the set, positions absolute -- and the fp64 (positions, motions) of every set."""
    import torch
    w, cfg = weights_of(model), model.model_config
    y = p_y = 0.0
    refs = []
    with torch.no_grad():
        for s in sets:
            ref = propagate(w, cfg, s["state_t"].numpy(), s["a"].numpy(), s["g"].numpy(), s["act"].numpy(), s["recv"].numpy(), s["send"].numpy())
            pos, mot = model._propagate(s["state_t"], s["a"], s["g"], s["act"], s["recv"], s["send"])
            e_m, e_p = errors(pos.numpy(), mot.numpy(), *ref)
            y, p_y = max(y, e_m), max(p_y, e_p)
            refs.append(ref)
    return y, p_y, refs


@functools.lru_cache(maxsize=None)
def case(name):
    """One configuration of the matrix, built once per process and left unchanged: dict(cfg, instances, model (host, fp32), weights (fp64
    arrays), sets, refs (fp64 positions / motions per set), y (the motion yardstick y_c), p_y (the position yardstick))."""
    kw = dict(CONFIGS[name])
    instances = kw.pop("instances", 1)
    cfg = base_cfg(**kw)
    idx = int(name[1:])
    model = make_model(cfg, 100 + idx)
    sets = input_sets(cfg, instances, 200 + idx)
    y, p_y, refs = yardstick(model, sets)
    return dict(name=name, cfg=cfg, instances=instances, model=model, weights=weights_of(model), sets=sets, refs=refs, y=y, p_y=p_y)
