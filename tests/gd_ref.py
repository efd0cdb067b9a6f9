"""fp64 statement of the gradient of the planner's cost (gsdyn.running_cost_grad, csrc/gsr_plan_cost_grad.hip), written with numpy from the
formulas of include/gsr.h one sample and one step at a time, with the MARGIN of every discrete decision it takes, and helpers for central
finite differences.  Inputs of any float dtype are taken to float64 first: "the same fp32 inputs" of the GPU tests.

``cost_grad_ref`` returns, beside the values and the two gradients:
  abs_state [B, T, n_obj, 3] : per element, the sum of the absolute values of the chamfer terms that were added into it (the bound of a
                               fixed-order fp32 sum is a multiple of it), and terms [B, n_obj]: how many such terms the last frame's row has;
  coef_state, coef_act       : per element, the absolute factor d reward / d (collision or box value) that multiplies a unit vector there
                               (sharpness * pw / T where a gate is open, else 0): the collision / box part of the bound;
  margins                    : dict of the smallest margins met, each relative --
      "nn"    best against second-best SQUARED distance of every nearest-neighbour decision (chamfer both ways, collision), (d2_2 - d2_1) / d2_2;
      "gate"  |d - pusher| / max(d, pusher) of every collision term;
      "wall"  of every box term: the active wall's lead over the next wall in exp(-s max(margin, 0)), relative, where the active margin is
              positive; and |margin| of the active wall relative to the larger of the coordinate and the wall;
      "extreme_ties" : how many of the box extremes (x min, x max, y min, y max of a frame) are attained more than once;
      "zero"  how many nearest-neighbour distances are exactly zero (their contribution is the zero vector; they carry no margin)."""
import math

import numpy as np


def _np(a):
    return a.detach().cpu().double().numpy() if hasattr(a, "detach") else np.asarray(a, dtype=np.float64)


def _gap(d2):
    """Relative gap of the two smallest entries of a 1-D array of squared distances (inf for a single entry, nan for a zero best: excluded)."""
    if d2.shape[0] < 2:
        return math.inf
    two = np.partition(d2, 1)[:2]
    if two[0] == 0.0:
        return math.nan
    return (two[1] - two[0]) / two[1]


def cost_grad_ref(state_seqs, actions, state_cur, target, box, pusher_size=0.01, sharpness=100.0, penalty_weight=5.0):
    S, A, C, G, bx = _np(state_seqs), _np(actions), _np(state_cur), _np(target), _np(box).reshape(4)
    B, T, n_obj, M = S.shape[0], S.shape[1], S.shape[2], G.shape[0]
    reward, chamfer, coll, boxp = np.zeros(B), np.zeros(B), np.zeros((B, T)), np.zeros((B, T))
    g_state, g_act = np.zeros_like(S), np.zeros_like(A)
    abs_state, coef_state, coef_act = np.zeros_like(S), np.zeros_like(S), np.zeros_like(A)
    terms = np.zeros((B, n_obj), dtype=np.int64)
    nn, gate, wall, ties, zero = [], [], [], 0, 0
    w = penalty_weight / T
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(B):
            P = S[b, T - 1]
            diff = P[None, :, :] - G[:, None, :]                                     # [M, n_obj, 3]: P_n - q_m
            d2 = (diff ** 2).sum(-1)
            for m in range(M):                                                       # target m -> its nearest particle (ascending m)
                n = int(np.argmin(d2[m]))                                            # the first among equals
                d = math.sqrt(d2[m, n])
                chamfer[b] += d / M
                nn.append(_gap(d2[m]))
                if d > 0.0:
                    term = -(1.0 / M) * diff[m, n] / d
                    g_state[b, T - 1, n] += term
                    abs_state[b, T - 1, n] += np.abs(term)
                    terms[b, n] += 1
                else:
                    zero += 1
            for n in range(n_obj):                                                   # particle n -> its nearest target
                m = int(np.argmin(d2[:, n]))
                d = math.sqrt(d2[m, n])
                chamfer[b] += d / n_obj
                nn.append(_gap(d2[:, n]))
                if d > 0.0:
                    term = -(1.0 / n_obj) * diff[m, n] / d
                    g_state[b, T - 1, n] += term
                    abs_state[b, T - 1, n] += np.abs(term)
                    terms[b, n] += 1
                else:
                    zero += 1
            for t in range(T):
                Q = C[:, :2] if t == 0 else S[b, t - 1, :, :2]
                q2 = ((A[b, t, :2][None] - Q) ** 2).sum(-1)
                n = int(np.argmin(q2))
                d = math.sqrt(q2[n])
                nn.append(_gap(q2))
                gate.append(abs(d - pusher_size) / max(d, pusher_size))
                c = math.exp(-sharpness * max(d - pusher_size, 0.0)) if not math.isnan(d) else math.nan
                coll[b, t] = c
                if d - pusher_size > 0.0 and d > 0.0:
                    u = (A[b, t, :2] - Q[n]) / d
                    g_act[b, t, :2] += w * sharpness * c * u
                    coef_act[b, t, :2] = w * sharpness
                    if t > 0:
                        g_state[b, t - 1, n, :2] -= w * sharpness * c * u
                        coef_state[b, t - 1, n, :2] += w * sharpness
                x, y = S[b, t, :, 0], S[b, t, :, 1]
                idx = [int(np.argmin(x)), int(np.argmax(x)), int(np.argmin(y)), int(np.argmax(y))]
                ties += sum(int((v == v[i]).sum() > 1) for v, i in ((x, idx[0]), (x, idx[1]), (y, idx[2]), (y, idx[3])))
                margins = np.array([x[idx[0]] - bx[0], bx[1] - x[idx[1]], y[idx[2]] - bx[2], bx[3] - y[idx[3]]])
                e = np.exp(-sharpness * np.maximum(margins, 0.0))
                k = int(np.argmax(e)) if not np.isnan(e).any() else int(np.argmax(np.isnan(e)))      # the first among equals; a NaN is the largest
                boxp[b, t] = e[k]
                coord = (x[idx[0]], x[idx[1]], y[idx[2]], y[idx[3]])[k]
                wall.append(abs(margins[k]) / max(abs(coord), abs(bx[k]), 1e-300))
                if margins[k] > 0.0:
                    others = np.delete(e, k)
                    wall.append((e[k] - others.max()) / e[k])
                    g = w * sharpness * e[k]
                    g_state[b, t, idx[k], k >> 1] += g if k % 2 == 0 else -g
                    coef_state[b, t, idx[k], k >> 1] += w * sharpness
            reward[b] = -chamfer[b] - penalty_weight * coll[b].mean() - penalty_weight * boxp[b].mean()
            if not np.isfinite(reward[b]):
                g_state[b], g_act[b] = math.nan, math.nan
    fin = lambda v: np.nanmin(np.array(v + [math.inf], dtype=np.float64))  # noqa: E731
    margins = {"nn": fin(nn), "gate": fin(gate), "wall": fin(wall), "extreme_ties": ties, "zero": zero}
    return {"reward": reward, "chamfer": chamfer, "collision": coll, "box": boxp, "g_state": g_state, "g_actions": g_act, "abs_state": abs_state,
            "terms": terms, "coef_state": coef_state, "coef_act": coef_act, "margins": margins}


def central_differences(f, x, h=1e-6, index=None):
    """d f / d x of a scalar function of one float64 numpy array by central differences: the whole array, or the flat indices ``index``."""
    x = np.array(x, dtype=np.float64)
    flat = x.reshape(-1)
    index = range(flat.shape[0]) if index is None else index
    out = np.zeros(len(index))
    for k, i in enumerate(index):
        keep = flat[i]
        flat[i] = keep + h
        up = float(f(x))
        flat[i] = keep - h
        down = float(f(x))
        flat[i] = keep
        out[k] = (up - down) / (2 * h)
    return out


def torch_central_differences(f, x, h=1e-6, index=None):
    """The same for a function of one float64 torch tensor."""
    import torch
    return central_differences(lambda a: f(torch.from_numpy(a.copy())), x.detach().cpu().numpy(), h, index)
