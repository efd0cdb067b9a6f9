"""fp64 statements of the planner's cost and MPPI update (gsdyn.running_cost / gsdyn.mppi_update, csrc/gsr_plan_cost.hip), written from their
formulas with numpy, one sample and one step at a time.  The update is written in the reference's DIFFERENCED form -- the weighted means of
the start points and of the end points, then their difference -- so that the displacement form of the code under test is checked against
it.  Inputs of any float dtype are taken to float64 first: "the same fp32 inputs" of the GPU tests."""
import math

import numpy as np


def _np(a):
    return a.detach().cpu().double().numpy() if hasattr(a, "detach") else np.asarray(a, dtype=np.float64)


def _min(a, axis=None):
    return np.min(a, axis=axis)                  # numpy's min propagates a NaN, as torch.min does


def cost_ref(state_seqs, actions, state_cur, target, box, pusher_size=0.01, sharpness=100.0, penalty_weight=5.0):
    """-> dict of float64 arrays: reward [B], chamfer [B], collision [B, T], box [B, T].  ``box`` = (x_lo, x_hi, y_lo, y_hi)."""
    S, A, C, G, bx = _np(state_seqs), _np(actions), _np(state_cur), _np(target), _np(box).reshape(4)
    B, T = S.shape[0], S.shape[1]
    chamfer, coll, boxp = np.zeros(B), np.zeros((B, T)), np.zeros((B, T))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            P = S[b, T - 1]
            dist = np.sqrt(((G[:, None, :] - P[None, :, :]) ** 2).sum(-1))          # [M, n_obj]
            chamfer[b] = _min(dist, axis=1).mean() + _min(dist, axis=0).mean()
            for t in range(T):
                Q = C[:, :2] if t == 0 else S[b, t - 1, :, :2]
                d = _min(np.sqrt(((A[b, t, :2][None] - Q) ** 2).sum(-1))) - pusher_size
                coll[b, t] = math.exp(-sharpness * np.maximum(d, 0.0))
                x, y = S[b, t, :, 0], S[b, t, :, 1]
                margins = np.array([x.min() - bx[0], bx[1] - x.max(), y.min() - bx[2], bx[3] - y.max()])
                boxp[b, t] = np.max(np.exp(-sharpness * np.maximum(margins, 0.0)))
    reward = -chamfer - penalty_weight * coll.mean(1) - penalty_weight * boxp.mean(1)
    return {"reward": reward, "chamfer": chamfer, "collision": coll, "box": boxp}


def clip_ref(seq, lower, upper):
    out = np.array(seq, dtype=np.float64)
    out[..., 0] = np.mod(out[..., 0] + math.pi, 2 * math.pi) - math.pi              # column 0: the reference's rule, kept
    return np.minimum(np.maximum(out, _np(lower)), _np(upper))


def update_ref(act_seqs, rewards, reward_weight, lower, upper, push_length, clip=True):
    """-> (act_seq [T, 4], best_index, best_reward) in float64, the reference's differenced form.  ``clip=False`` leaves the clip out (for
    comparing angles modulo 2 pi)."""
    A, r = _np(act_seqs), _np(rewards)
    nan = np.isnan(r)
    best = int(np.argmax(nan)) if nan.any() else int(np.flatnonzero(r == r.max())[0])
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(reward_weight * (r - r[best]))
        w = (e / e.sum())[:, None]
        xs, ys, th, ln = A[:, :, 0], A[:, :, 1], A[:, :, 2], A[:, :, 3]
        x_ends, y_ends = xs - ln * push_length * np.cos(th), ys - ln * push_length * np.sin(th)
        x, y, x_end, y_end = (w * xs).sum(0), (w * ys).sum(0), (w * x_ends).sum(0), (w * y_ends).sum(0)
        theta = np.arctan2(y - y_end, x - x_end)
        length = np.sqrt((x_end - x) ** 2 + (y_end - y) ** 2) / push_length
    seq = np.stack([x, y, theta, length], -1)
    return (clip_ref(seq, lower, upper) if clip else seq), best, r[best]
