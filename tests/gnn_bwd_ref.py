"""The backward of the propagation network's two kernels (csrc/gsr_gnn_bwd.hip) restated in numpy, and the training loss of
gsdyn.dynamics_loss restated densely -- the references of tests/test_gnn_train_cpu.py and tests/test_gnn_train_gpu.py.

Part one, the kernels.  ``aggregate_backward`` / ``rel_inputs_backward`` with ``dtype=np.float32`` are the kernels' bit-exact statements:
every output element is a running sum that starts at zero and takes its terms in a stated order (a node's receiver segment in list order,
its sender-side reverse list in ascending relation id); only additions and one subtraction occur.  With ``dtype=np.float64`` the same sums
are taken in fp64.  The ReLU gate m[e] = (z[e] <= 0) ? 0 : d_agg[recv_e] is part of the DEFINITION in both: z is the forward's fp32
pre-activation (rew1[e] + a2[recv_e]) + a3[send_e], so the fp64 form differs from the fp32 one by the roundings of the sums alone
(``sum_bound``: deg 2^-24 sum |terms| for deg terms) and not by a gate that an fp64 z would open or close differently at a cancellation.

Part two, the loss.  ``referee_loss`` is the loop of the reference's training step on the dataset's dense Rr / Rs, written with matrix
products as the reference's length term is, around ``DynamicsPredictor.forward`` -- run in fp64 on the host under autograd it is the
referee of every path of ``dynamics_loss``.  ``make_batch`` builds a seeded batch of the dataset's dictionary with padded relation rows."""
import numpy as np

U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------ lists
def reverse_list(send, N):
    """The sender-side reverse list: (rev_ptr [N + 1], rev_edge [E]) = the relation ids stably sorted by sender."""
    send = np.asarray(send, dtype=np.int64)
    rev_edge = np.argsort(send, kind="stable").astype(np.int64)
    rev_ptr = np.concatenate([[0], np.cumsum(np.bincount(send, minlength=N))]).astype(np.int64)
    return rev_ptr, rev_edge


def receivers_of(row_start):
    rs = np.asarray(row_start, dtype=np.int64)
    return np.repeat(np.arange(rs.shape[0] - 1, dtype=np.int64), np.diff(rs))


def _ordered_sums(vals, ptr, dtype):
    """out[i] = ((0 + vals[ptr[i]]) + vals[ptr[i] + 1]) + ... in ``dtype``; vals [L, C] in list position order."""
    ptr = np.asarray(ptr, dtype=np.int64)
    lo, deg = ptr[:-1], np.diff(ptr)
    out = np.zeros((lo.shape[0], vals.shape[1]), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(deg.max(initial=0))):
            rows = np.nonzero(deg > j)[0]
            out[rows] = out[rows] + vals[lo[rows] + j].astype(dtype)
    return out


def sum_bound(vals, ptr):
    """deg 2^-24 sum |terms| per output element of ``_ordered_sums`` (deg - 1 roundings, each at most 2^-24 of the sum of magnitudes to
    first order; the spare one covers the second-order terms)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    return np.diff(ptr)[:, None] * U24 * _ordered_sums(np.abs(np.asarray(vals, dtype=np.float64)), ptr, np.float64)


# ------------------------------------------------------------------------------------------ gsr_gnn_aggregate_backward
def gate(rew1, a23, send, recv, d_agg, n_sum):
    """m [E, H] (fp32): d_agg[recv_e] where the forward's fp32 z[e] = (rew1[e] + a2[recv_e]) + a3[send_e] is not <= 0 (a NaN z passes,
    z = +-0 blocks: threshold_backward) and recv_e < n_sum, +0 elsewhere."""
    r1, nb, g = np.asarray(rew1, dtype=np.float32), np.asarray(a23, dtype=np.float32), np.asarray(d_agg, dtype=np.float32)
    H = r1.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        z = (r1 + nb[recv, :H]) + nb[send, H:]
        blocked = (z <= 0) | (np.asarray(recv) >= n_sum)[:, None]
    return np.where(blocked, np.float32(0), g[recv]).astype(np.float32)


def aggregate_backward(rew1, a23, send, row_start, rev_ptr, rev_edge, d_agg, n_sum, dtype=np.float32):
    """-> (d_rew1 [E, H] = m, d_a23 [N, 2 H] = (segment sums of m in list order | reverse-list sums of m in ascending e)) in ``dtype``."""
    recv = receivers_of(row_start)
    m = gate(rew1, a23, send, recv, d_agg, n_sum)
    seg = _ordered_sums(m, row_start, dtype)
    seg[n_sum:] = 0                                           # rows the forward did not sum own no segment (their m is 0 anyway)
    rev = _ordered_sums(m[np.asarray(rev_edge, dtype=np.int64)], rev_ptr, dtype)
    return m.astype(dtype), np.concatenate([seg, rev], 1)


def aggregate_backward_bound(rew1, a23, send, row_start, rev_ptr, rev_edge, d_agg, n_sum):
    recv = receivers_of(row_start)
    m = gate(rew1, a23, send, recv, d_agg, n_sum)
    m = np.where(np.isnan(m), 0, m)
    return np.concatenate([sum_bound(m, row_start), sum_bound(m[np.asarray(rev_edge, dtype=np.int64)], rev_ptr)], 1)


# ------------------------------------------------------------------------------------------ gsr_gnn_rel_inputs_backward
def rel_inputs_backward(d_out, row_start, rev_ptr, rev_edge, A, S, dtype=np.float32):
    """d_state [N, S] = (list-order sum over the segment) - (ascending-e sum over the reverse list) of d_out's state columns."""
    d = np.asarray(d_out, dtype=np.float32)[:, 2 * A + 1:2 * A + 1 + S]
    return _ordered_sums(d, row_start, dtype) - _ordered_sums(d[np.asarray(rev_edge, dtype=np.int64)], rev_ptr, dtype)


def rel_inputs_backward_bound(d_out, row_start, rev_ptr, rev_edge, A, S):
    """One chain of deg_r + deg_s terms (two running sums and the subtraction: deg_r + deg_s - 1 roundings)."""
    d = np.abs(np.asarray(d_out, dtype=np.float64))[:, 2 * A + 1:2 * A + 1 + S]
    mags = _ordered_sums(d, row_start, np.float64) + _ordered_sums(d[np.asarray(rev_edge, dtype=np.int64)], rev_ptr, np.float64)
    deg = np.diff(np.asarray(row_start, dtype=np.int64)) + np.diff(np.asarray(rev_ptr, dtype=np.int64))
    return deg[:, None] * U24 * mags


# ------------------------------------------------------------------------------------------ the loss
def referee_loss(model, batch, n_future, mse_weight=1.0, length_weight=0.01):
    """The training loss on the dense relation matrices: per step, mse(prediction, future state) and the mse between the relations'
    lengths in the prediction and in the OLDEST history frame -- relation ends taken with Rr / Rs restricted to the object columns (an end
    at a tool row is the origin), the mean over all B n_rel rows, padding included.  The prediction becomes the newest history frame of
    the next step.  Runs ``model.forward`` in the model's dtype under autograd; nothing of the caller's is modified."""
    import torch
    state, action = batch["state"], batch.get("action")
    Rr, Rs = batch["Rr"], batch["Rs"]
    loss = 0.0
    for fi in range(n_future):
        gt = batch["state_future"][:, fi]
        n_p = gt.shape[1]
        pred = model(state=state, attrs=batch["attrs"], p_instance=batch["p_instance"], action=action, Rr=Rr, Rs=Rs)[0][:, :n_p]
        D = Rr[:, :, :n_p] - Rs[:, :, :n_p]                                   # [B, n_rel, n_p]: one matrix gives the difference vectors
        len_pred = torch.norm(torch.matmul(D, pred), dim=-1)                  # (a padded row: length 0, and torch.norm's slope there is 0)
        len_old = torch.norm(torch.matmul(D, state[:, 0, :n_p].detach()), dim=-1)
        loss = loss + mse_weight * ((pred - gt) ** 2).mean() + length_weight * ((len_pred - len_old) ** 2).mean()
        if fi < n_future - 1:
            newest = torch.cat([pred, batch["tool_future"][:, fi, n_p:]], 1)
            state = torch.cat([state[:, 1:], newest[:, None]], 1)
            action = batch["action_future"][:, fi]
    return loss


def make_batch(cfg, instances, B, n_obj, n_future, seed, pad_rows=7, thr=0.15, topk=5, dtype=None):
    """A seeded batch of the dataset's dictionary (CPU, fp32 unless ``dtype``): ``n_obj`` object particles and one tool (the last row) per
    graph, relations of ``construct_edges`` on the newest frame as dense one-hot rows, every graph padded with all-zero rows up to the
    longest list + ``pad_rows``; futures a few small steps on."""
    import torch
    from gsdyn.dynamics import construct_edges, edges_to_dense
    gen = torch.Generator().manual_seed(seed)
    N, n_his, A = n_obj + 1, int(cfg["n_his"]), int(cfg["attr_dim"])
    box = torch.tensor([0.4, 0.4, 0.05])
    a = torch.zeros((N, A))
    a[:n_obj, 0] = 1.0
    a[n_obj, 1] = 1.0
    if A > 2:
        a[:, 2:] = torch.rand((N, A - 2), generator=gen)
    g = torch.zeros((n_obj, instances))
    if instances == 1:
        g[:] = 1.0
    else:
        g[torch.arange(n_obj), torch.arange(n_obj) * instances // n_obj] = 1.0
    mask = torch.ones(N, dtype=torch.bool)
    tool = torch.zeros(N, dtype=torch.bool)
    tool[n_obj] = True
    states, lists, futures, tools, actions = [], [], [], [], []
    for _ in range(B):
        last = torch.rand((N, 3), generator=gen) * box
        steps = (torch.rand((n_his, N, 3), generator=gen) - 0.5) * 0.02
        steps[-1] = 0.0
        states.append(last[None] + torch.flip(torch.cumsum(torch.flip(steps, [0]), 0), [0]))
        lists.append(construct_edges(last, thr, mask, tool, topk=topk, n_tool=1))
        walk = torch.cumsum((torch.rand((n_future, N, 3), generator=gen) - 0.5) * 0.02, 0) + last[None]
        futures.append(walk[:, :n_obj])
        tools.append(walk[:max(n_future - 1, 0)])
        act = torch.zeros((n_future, N, 3))
        act[:, n_obj, :2] = (torch.rand((n_future, 2), generator=gen) - 0.5) * 0.05
        actions.append(act)
    n_rel = max(r.shape[0] for r, _ in lists) + pad_rows
    Rr, Rs = torch.zeros((B, n_rel, N)), torch.zeros((B, n_rel, N))
    for b, (r, s) in enumerate(lists):
        Rr[b, :r.shape[0]], Rs[b, :r.shape[0]] = edges_to_dense(r, s, N)
    acts = torch.stack(actions)
    batch = dict(state=torch.stack(states), attrs=a[None].repeat(B, 1, 1), p_instance=g[None].repeat(B, 1, 1), action=acts[:, 0].contiguous(),
                 Rr=Rr, Rs=Rs, state_future=torch.stack(futures), tool_future=torch.stack(tools), action_future=acts[:, 1:].contiguous())
    if dtype is not None:
        batch = {k: v.to(dtype) for k, v in batch.items()}
    return batch


def to(batch, device=None, dtype=None):
    return {k: v.detach().to(device=device, dtype=dtype).clone() for k, v in batch.items()}
