"""Fitting the propagation network -- the training loop body of the reference's third program (its src/train.py:171-220) as two
functions: ``dynamics_loss`` (the ``n_future`` predictions of one batch, each written into the next step's history, with the mse and
relation-length terms) and ``train_dynamics_step`` (zero_grad, loss, backward, optimiser step).

Two paths compute the same loss.  The DEFINITION is ``DynamicsPredictor.forward`` under autograd on the dataset's dense ``Rr`` / ``Rs``.
The DEVICE path (float32 on a HIP device) turns the B graphs of a batch into one block-diagonal index-form graph -- node ids offset by
b N, padded relations dropped, relations stably sorted by receiver, built ONCE per batch -- and runs ``propagate_split_grad``: the split
propagation with kernels for the two steps between the matrix products, forward and backward.  Its gradients are sums in a fixed order
(no atomics) and bit-identical from run to run; the eager path's scatter_add / index backward are not.

A batch of ``gsdyn.make_dynamics_batch`` carries that graph already (key ``graph``, built by a kernel from the relation lists): the device
path then uses it as it is -- no ``nonzero``, no sort, no host read -- and the dense ``Rr`` / ``Rs`` may be absent (``dense=False``): the
length term divides by B x ``n_rel_rows``, the eager path builds the matrices from the padded lists ``receivers`` / ``senders``.

``rigid_weight`` adds the reference's third term, its ``rigid_loss`` (src/train.py:32-40): the prediction's distance from the rigidly
aligned oldest history frame (``gsdyn.rigid_fit.umeyama_fit``).  The reference's ``train_config['rigid_loss']``
configuration is ``length_weight=0.05, rigid_weight=0.05``.

``DEVICE_PATH_DEFAULT`` is what ``device_path=None`` means; DESIGN.md section 3m has the measurement that decided it.
Out of scope here: l1_loss and local_rigid_loss (the reference's train() selects neither; the second needs a per-end gather whose backward
is an atomic index_add), a whole-batch scale of the alignment, graph capture of the step, reading episode files (the batches themselves:
``gsdyn.dyn_data``), checkpoints, plots."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .dynamics import DynamicsPredictor, _GnnRelInputs, split_graph
from .rigid_fit import umeyama_fit

DEVICE_PATH_DEFAULT = True          # measured 1.3 - 3.6 x faster per training step than the eager path (profiles/gnn_train_cost.txt)


def _device_path_ok(model: DynamicsPredictor, batch: Dict) -> bool:
    state, attrs, inst = batch["state"], batch["attrs"], batch["p_instance"]
    if not (state.is_cuda and state.dtype == torch.float32 and attrs.dtype == torch.float32 and model.split_grad_ok(attrs)):
        return False
    if attrs.requires_grad or inst.requires_grad or ("Rr" in batch and batch["Rr"].dtype != torch.float32):
        return False
    if "Rr" not in batch and "graph" not in batch:
        return False
    return all(p.device == state.device and p.dtype == torch.float32 for p in model.parameters())


def _length_term(d_pred, d_pos, denom):
    """mse between the relations' lengths after and before the step; ``denom`` = B n_rel, the padded rows included (their lengths are 0
    on both sides), as the dense formula divides."""
    return ((d_pred.norm(dim=-1) - d_pos.norm(dim=-1)) ** 2).sum() / denom


class _RigidTerm(torch.autograd.Function):
    """sum_b sse_b / (3 sum_b count_b) as a function of the prediction, the alignment held fixed: the reference's
    ``F.mse_loss(pred[obj_mask], aligned.detach()[obj_mask])``.  The forward saves 2 residual / (3 sum count); the backward is one
    elementwise multiply (no reduction, no atomics: bit-identical from run to run)."""

    @staticmethod
    def forward(ctx, pred, residual, sse, count):
        denom = 3.0 * count.sum().to(sse.dtype)
        ctx.save_for_backward(residual * (2.0 / denom))
        return sse.sum() / denom

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None, None


def _rigid_term(pred, x0, mask, kernel):
    """The rigid term of one step: ``x0`` = the oldest history frame's object rows, ``pred`` the prediction, ``mask`` the real rows.
    A batch without a real object row gives 0 / 0 = NaN, as the reference's mse over an empty selection does."""
    fit = umeyama_fit(x0.detach().contiguous(), pred.detach().contiguous(), mask.contiguous(), kernel=kernel)
    return _RigidTerm.apply(pred, fit["residual"], fit["sse"], fit["count"])


def _obj_mask(batch, rigid_weight):
    if rigid_weight == 0.0:
        return None
    if "obj_mask" not in batch:
        raise ValueError("dynamics_loss: rigid_weight needs batch['obj_mask'] ([B, n_p] bool; gsdyn.make_dynamics_batch returns it)")
    return batch["obj_mask"].to(torch.bool)


def _next_history(state, pred, tool_next):
    """The history one step on: the prediction for the object particles, the recorded rows for the tools (a new tensor)."""
    n_p = pred.shape[1]
    return torch.cat([state[:, 1:], torch.cat([pred, tool_next[:, n_p:]], 1)[:, None]], 1)


def _dense_relations(batch):
    """The batch's one-hot ``Rr`` / ``Rs`` [B, n_rel_rows, N]: its own, or built from the padded lists (padding = N: an all-zero row)."""
    if "Rr" in batch:
        return batch["Rr"], batch["Rs"]
    N, dt = batch["state"].shape[2], batch["state"].dtype
    hot = lambda idx: torch.nn.functional.one_hot(idx, N + 1)[..., :N].to(dt)  # noqa: E731
    return hot(batch["receivers"]), hot(batch["senders"])


def _eager_loss(model, batch, n_future, mse_weight, length_weight, rigid_weight=0.0, rigid_kernel=None):
    state, action = batch["state"], batch.get("action")
    Rr, Rs = _dense_relations(batch)
    B, n_rel, N = Rr.shape
    recv, send, w = model._indices(Rr, Rs)
    bidx = torch.arange(B, device=state.device)[:, None]
    mask = _obj_mask(batch, rigid_weight)
    terms = [0.0, 0.0, 0.0]
    for fi in range(n_future):
        gt = batch["state_future"][:, fi]
        n_p = gt.shape[1]
        pred = model(state=state, attrs=batch["attrs"], p_instance=batch["p_instance"], action=action, Rr=Rr, Rs=Rs)[0][:, :n_p]
        # a relation's end at a tool row (>= n_p) counts as the origin, as in the dense product with Rr[:, :, :n_p]
        ext = lambda x: torch.cat([x, x.new_zeros((B, N - n_p, 3))], 1)  # noqa: E731
        diff = lambda x: (x[bidx, recv] - x[bidx, send]) * w[..., None]  # noqa: E731
        terms[0] = terms[0] + mse_weight * torch.nn.functional.mse_loss(pred, gt)
        terms[1] = terms[1] + length_weight * _length_term(diff(ext(pred)), diff(ext(state[:, 0, :n_p].detach())), B * n_rel)
        if mask is not None:
            terms[2] = terms[2] + rigid_weight * _rigid_term(pred, state[:, 0, :n_p], mask, False)
        if fi < n_future - 1:
            state, action = _next_history(state, pred, batch["tool_future"][:, fi]), batch["action_future"][:, fi]
    return terms


def _device_loss(model, batch, n_future, mse_weight, length_weight, rigid_weight=0.0, rigid_kernel=None):
    c = model.model_config
    state, action, attrs, inst = batch["state"], batch.get("action"), batch["attrs"], batch["p_instance"]
    dev, n_his = state.device, state.shape[1]
    # ---- the batch's graphs as one block-diagonal graph, once (the relations do not change over the n_future steps)
    if "graph" in batch:                                             # gsdyn.make_dynamics_batch built it: nothing to derive, no host read
        graph = batch["graph"]
        B, N = state.shape[0], state.shape[2]
        n_rel = batch["Rr"].shape[1] if "Rr" in batch else int(batch["n_rel_rows"])
    else:
        Rr, Rs = batch["Rr"], batch["Rs"]
        B, n_rel, N = Rr.shape
        recv, send, w = model._indices(Rr, Rs)
        b, r = torch.nonzero(w > 0, as_tuple=True)                   # the one host read of the batch: the relation count
        recv, order = torch.sort(recv[b, r] + b * N, stable=True)    # batch-major already; within a receiver the dataset's row order stays
        graph = split_graph(recv, (send[b, r] + b * N)[order], B * N)
    a = attrs.reshape(B * N, attrs.shape[2]).contiguous()
    g = torch.cat([inst, inst.new_zeros((B, N - inst.shape[1], inst.shape[2]))], 1).reshape(B * N, inst.shape[2]).contiguous()
    none = a.new_zeros((B * N, 0))
    mask = _obj_mask(batch, rigid_weight)
    terms = [0.0, 0.0, 0.0]
    for fi in range(n_future):
        gt = batch["state_future"][:, fi]
        n_p = gt.shape[1]
        state_t = state.transpose(1, 2).reshape(B * N, n_his * 3)
        act = action.reshape(B * N, action.shape[2]).contiguous() if c["action_dim"] > 0 else none
        pos = model.propagate_split_grad(state_t, a, g, act, graph)[0].view(B, N, 3)
        pred = pos[:, :n_p]
        obj = torch.zeros((1, N, 1), dtype=pos.dtype, device=dev)
        obj[:, :n_p] = 1.0
        # the relations' difference vectors through the relation-input kernel (no attributes, no instances, three "state" columns): its
        # backward is the fixed-order walk, where a row gather's would be an index_add with atomics
        d_pred = _GnnRelInputs.apply(none, none, (pos * obj).reshape(B * N, 3), graph)[:, 1:]
        pos0 = (state[:, 0].detach() * obj).reshape(B * N, 3)
        terms[0] = terms[0] + mse_weight * torch.nn.functional.mse_loss(pred, gt)
        terms[1] = terms[1] + length_weight * _length_term(d_pred, pos0[graph.receivers] - pos0[graph.senders], B * n_rel)
        if mask is not None:
            terms[2] = terms[2] + rigid_weight * _rigid_term(pred, state[:, 0, :n_p], mask, rigid_kernel)
        if fi < n_future - 1:
            state, action = _next_history(state, pred, batch["tool_future"][:, fi]), batch["action_future"][:, fi]
    return terms


def dynamics_loss(model: DynamicsPredictor, batch: Dict, *, n_future: int, mse_weight: float = 1.0, length_weight: float = 0.01,
                  rigid_weight: float = 0.0, device_path: Optional[bool] = None, _rigid_kernel: Optional[bool] = None
                  ) -> Tuple[torch.Tensor, Dict]:
    """The training loss of one batch of the reference's dataset dictionary: ``state`` [B, n_his, N, 3], ``attrs`` [B, N, attr_dim],
    ``p_instance`` [B, n_p, G], ``action`` [B, N, 3], dense ``Rr`` / ``Rs`` [B, n_rel, N] (all-zero rows are padding; a batch of
    ``gsdyn.make_dynamics_batch`` may carry ``graph``, ``receivers`` / ``senders`` and ``n_rel_rows`` instead), ``state_future``
    [B, >= n_future, n_p, 3], ``tool_future`` / ``action_future`` [B, >= n_future - 1, N, 3].  ``n_future`` predictions; each becomes the
    newest frame of the next step's history (the tools' rows from ``tool_future``, the action from ``action_future``); every step adds
    mse_weight x mse(prediction, state_future) + length_weight x mse of the relations' lengths against the oldest history frame.  The
    caller's tensors are not modified.  -> (loss, dict(mse=, length= the weighted sums over the steps, detached; device_path= bool)).

    ``rigid_weight`` (default 0: the term is absent, the graph and the returned dict are those of the two-term loss): when non-zero, every
    step also adds rigid_weight x sum_b sse_b / (3 sum_b count_b), where ``gsdyn.umeyama_fit`` aligns the oldest history frame's object rows
    ``state[:, 0, :n_p]`` rigidly to the prediction over ``batch["obj_mask"]`` ([B, n_p] bool; ``ValueError`` when missing) and sse /
    count are its squared residual and row count per sample -- the reference's ``mse(pred[obj_mask], aligned.detach()[obj_mask])``.  The
    alignment is held fixed: the gradient toward the prediction is rigid_weight x 2 residual / (3 sum count).  The dict then also has
    ``rigid``.  The kernels' path aligns with the kernel ``gsr_rigid_fit``, ``model.forward``'s path with the torch statement
    (``_rigid_kernel=False``, private, makes the kernels' path use the torch statement too: tools/rigid_loss_cost.py's comparison).  Not here:
    l1_loss, local_rigid_loss, a whole-batch scale, graph capture.

    ``device_path``: True asks for the kernels' path, False for plain ``model.forward`` under autograd, None for ``DEVICE_PATH_DEFAULT``.
    The kernels' path is taken only for float32 tensors on a HIP device with a configuration the split propagation accepts and attributes
    / instances that need no gradient; everything else runs ``model.forward``, which is also the definition."""
    n_future = int(n_future)
    if n_future < 1:
        raise ValueError("dynamics_loss: n_future must be at least 1")
    want = DEVICE_PATH_DEFAULT if device_path is None else bool(device_path)
    use = want and _device_path_ok(model, batch)
    rigid_weight = float(rigid_weight)
    mse, length, rigid = (_device_loss if use else _eager_loss)(model, batch, n_future, float(mse_weight), float(length_weight), rigid_weight,
                                                                        _rigid_kernel)
    if rigid_weight == 0.0:
        return mse + length, dict(mse=mse.detach(), length=length.detach(), device_path=use)
    return mse + length + rigid, dict(mse=mse.detach(), length=length.detach(), rigid=rigid.detach(), device_path=use)


def train_dynamics_step(model: DynamicsPredictor, optimizer, batch: Dict, **kw) -> torch.Tensor:
    """One optimisation step on one batch: zero_grad, ``dynamics_loss(model, batch, **kw)``, backward, step.  -> the loss (detached)."""
    optimizer.zero_grad()
    loss, _ = dynamics_loss(model, batch, **kw)
    loss.backward()
    optimizer.step()
    return loss.detach()
