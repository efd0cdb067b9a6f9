"""Plain fp64 references and scene builders for the kernels that move the Gaussians during a rollout (gsr_dynamics.hip: fit_bones_kernel,
fit_rotations_kernel, mat2quat_unit, lbs_kernel): tests/test_rollout_geometry_gpu.py compares the device with them, and
tests/test_dynamics_ref_cpu.py pins them, without a GPU, to the host path of gsdyn/dynamics.py that the reference's goldens pin.

Nothing here imports the library: numpy in fp64 on the fp32 inputs, written from the definitions.  Scenes are CPU fp32 tensors.
Degenerate neighbourhoods are EXACTLY degenerate in fp32 (dyadic coordinates with few bits -- every product and sum of the moment matrix is
exact --, or an exactly zero coordinate), so no rank decision hangs on rounding: ``bone_scene`` asserts it."""
from __future__ import annotations

import math

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
# a singular-value ratio below this is a zero that LAPACK's fp64 SVD could not return as 0 (its backward error is a few eps_fp64 of the
# largest value); everything that decides a rank in a scene of this file is either that or above RANK_CLEAR
SVD_ZERO = 1e-12
RANK_CLEAR = 1e-3


# ------------------------------------------------------------------------------------------ references
def moments_ref64(bones, motions, rel):
    """F_b = sum over the bones j with rel[b][j] != 0 of (new_j - new_b)(old_j - old_b)^T, old = bones, new = bones + motions, summed in
    fp64 from the fp32 inputs -> (F [nb,3,3] float64, neighbour counts [nb] int64)."""
    b = np.asarray(bones, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    m = np.asarray(motions, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    r = np.asarray(rel) != 0
    nb = b.shape[0]
    new = b + m
    F = np.zeros((nb, 3, 3))
    for i in range(nb):
        j = np.nonzero(r[i])[0]
        if j.size:
            F[i] = (new[j] - new[i]).T @ (b[j] - b[i])
    return F, r.sum(1).astype(np.int64)


def singular_values64(F32):
    """Descending singular values [nb,3] of fp32 moment matrices by numpy's fp64 SVD."""
    return np.linalg.svd(np.asarray(F32, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3), compute_uv=False)


def classify_ref(F32, n):
    """The code gsr_fit_rotations / gsr_fit_bones must return for the moment matrices F32 [nb,3,3] (fp32) with n [nb] neighbours:
      0 = identity by rule (no neighbour, F = 0, or full rank with det F < 0), 2 = Kabsch rotation, 3 = rank 1 resolved on the device,
      1 = rank 1 with a vanishing first column (left to the caller's LAPACK).
    Rank: the reference's rule S > S.max * 3 eps_fp32 on the fp64 singular values of the fp32 matrix; sign of det in fp64."""
    F = np.asarray(F32, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)
    n = np.asarray(n).reshape(-1)
    S = np.linalg.svd(F, compute_uv=False)
    rank = (S > S.max(axis=1, keepdims=True) * 3 * EPS32).sum(1)
    det = np.linalg.det(F)
    code = np.full(F.shape[0], 2, dtype=np.int32)
    for i in range(F.shape[0]):
        if n[i] <= 0 or not F[i].any() or rank[i] == 0:
            code[i] = 0
        elif rank[i] == 1:
            code[i] = 1 if not F[i][:, 0].any() else 3
        elif rank[i] == 3 and det[i] < 0:
            code[i] = 0
    return code


def lbs_ref64(bones, R, t, bq, xyz, quat, n_valid=None):
    """Linear blend skinning in fp64 with direct distances: weights 1 / max(|x - bone|, 1e-4) normalised over the bones; positions = the
    weighted sum of the rigid images R_b (x - bone_b) + t_b + bone_b; orientations = normalise(weighted sum of the bones' quaternions) x the
    Gaussian's quaternion, (w, x, y, z).  The SAME R, t, bq as the kernel gets: the skinning alone, not the fit.  n_valid: only the first
    n_valid bones (clamped to their number).  -> (xyz_new [P,3], quat_new [P,4] or None), float64."""
    f = lambda a, *sh: np.asarray(a, dtype=np.float32).astype(np.float64).reshape(*sh)   # noqa: E731
    B, Rm, T, Q, X = f(bones, -1, 3), f(R, -1, 3, 3), f(t, -1, 3), f(bq, -1, 4), f(xyz, -1, 3)
    if n_valid is not None:
        k = min(int(n_valid), B.shape[0])
        B, Rm, T, Q = B[:k], Rm[:k], T[:k], Q[:k]
    P = X.shape[0]
    out_x = np.zeros((P, 3))
    out_q = None if quat is None else np.zeros((P, 4))
    G = None if quat is None else f(quat, -1, 4)
    for s in range(0, P, 4096):
        x = X[s:s + 4096]
        diff = x[:, None, :] - B[None]
        d = np.sqrt((diff * diff).sum(-1))
        w = 1.0 / np.maximum(d, 1e-4)
        w = w / w.sum(1, keepdims=True)
        moved = np.einsum("bjk,pbk->pbj", Rm, diff) + T[None] + B[None]
        out_x[s:s + 4096] = (moved * w[..., None]).sum(1)
        if quat is not None:
            a = (Q[None] * w[..., None]).sum(1)
            a = a / np.maximum(np.sqrt((a * a).sum(-1, keepdims=True)), 1e-12)
            g = G[s:s + 4096]
            a0, a1, a2, a3 = a.T
            g0, g1, g2, g3 = g.T
            out_q[s:s + 4096] = np.stack([a0 * g0 - a1 * g1 - a2 * g2 - a3 * g3, a0 * g1 + a1 * g0 + a2 * g3 - a3 * g2,
                                          a0 * g2 - a1 * g3 + a2 * g0 + a3 * g1, a0 * g3 + a1 * g2 - a2 * g1 + a3 * g0], 1)
    return out_x, out_q


def quat_to_mat64(q):
    """Unit-normalised (w, x, y, z) -> rotation matrices [.., 3, 3] in fp64."""
    q = np.asarray(q).astype(np.float64)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = np.moveaxis(q, -1, 0)
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def axis_angle64(axis, angle):
    """Rodrigues' rotation matrix in fp64."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


# ------------------------------------------------------------------------------------------ bone scenes
# the classes of bone_scene: name -> bones per group.  A group is closed: its bones are related to bones of the group only.
_GROUPS = (("one_neighbour", 2), ("isolated", 1), ("coincident", 2), ("code1", 2), ("collinear", 4), ("coplanar", 6), ("mirrored", 6))
_BLOCK = sum(s for _, s in _GROUPS)        # 23 bones: one group of every degenerate class
_GENERIC_MIN = 8
# what fit_bone_rotations must return per class ("identity", or None = whatever the literal form gives) and the device code
CLASS_CODE = {"generic": 2, "one_neighbour": 3, "collinear": 3, "coplanar": 2, "mirrored": 0, "isolated": 0, "coincident": 0, "code1": 1}
IDENTITY_CLASSES = ("mirrored", "isolated", "coincident")


def _dyadic(rng, n, bits, lo=0.125, hi=0.875):
    """n x 3 coordinates k / 2^bits in [lo, hi]."""
    q = 1 << bits
    return rng.integers(int(lo * q), int(hi * q) + 1, size=(n, 3)).astype(np.float64) / q


def _fill_group(name, idx, bones, new, rel, rng):
    """Positions before / after the step and relations of one closed group at the bone indices idx."""
    k = len(idx)
    all_pairs = lambda: rel.__setitem__((np.repeat(idx, k), np.tile(idx, k)), 1)   # noqa: E731   (itself included: its offset is 0)
    if name == "isolated":
        bones[idx] = _dyadic(rng, k, 6)
        new[idx] = bones[idx] + 1.0 / 64
    elif name == "one_neighbour":                 # a <-> b: F = w o^T, every product exact (6-bit offsets before and after)
        bones[idx] = _dyadic(rng, k, 5)
        bones[idx[1]] = bones[idx[0]] + np.array([3, -2, 5]) / 32.0 / 4
        new[idx[0]] = bones[idx[0]]
        new[idx[1]] = bones[idx[0]] + np.array([2, 4, -3]) / 32.0 / 4
        rel[idx[0], idx[1]] = rel[idx[1], idx[0]] = 1
    elif name == "coincident":                    # related bones at the same place: F = 0 with n > 0
        bones[idx] = _dyadic(rng, 1, 6)
        new[idx[0]] = bones[idx[0]] + np.array([1, 0, 2]) / 64.0
        new[idx[1]] = bones[idx[1]] + np.array([0, 3, 1]) / 64.0
        all_pairs()
    elif name == "code1":                         # one neighbour whose old offset has x exactly 0: F's first column vanishes
        bones[idx] = _dyadic(rng, k, 5)
        bones[idx[1]] = bones[idx[0]] + np.array([0, 3, -2]) / 128.0
        new[idx[0]] = bones[idx[0]]
        new[idx[1]] = bones[idx[0]] + np.array([1, 2, 3]) / 128.0
        rel[idx[0], idx[1]] = rel[idx[1], idx[0]] = 1
    elif name == "collinear":                     # a line onto a line: F = (sum a_j^2) d' d^T exactly
        c, c2 = _dyadic(rng, 1, 4, 0.25, 0.75)[0], _dyadic(rng, 1, 4, 0.25, 0.75)[0]
        a = np.arange(k) - 1.0                    # -1, 0, 1, 2, ...
        bones[idx] = c + a[:, None] * np.array([2, 1, -1]) / 64.0
        new[idx] = c2 + a[:, None] * np.array([1, -2, 2]) / 64.0
        all_pairs()
    elif name == "coplanar":                      # a patch in z = 0.5 that only sees itself and stays planar (tilted): F's third column is 0
        bones[idx, :2] = 0.3 + 0.4 * rng.random((k, 2))
        bones[idx, 2] = 0.5
        ang = 0.3
        xy = (bones[idx, :2] - 0.5) @ np.array([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]]).T + 0.5
        new[idx, :2] = xy
        new[idx, 2] = 0.5 + 0.1 * (bones[idx, 0] - 0.5)
        all_pairs()
    elif name == "mirrored":                      # the group reflected in z: det F < 0 at full rank -> the reference's identity fallback
        bones[idx] = 0.3 + 0.4 * rng.random((k, 3))
        new[idx] = (bones[idx] - 0.5) * np.array([1.0, 1.0, -1.0]) + 0.5
        all_pairs()
    else:
        raise KeyError(name)


def bone_scene(nb, seed=0):
    """A bone set of nb bones with as many neighbourhood classes as nb allows, laid out by index range:
      generic (rank 3, det > 0), one_neighbour and collinear (rank 1), coplanar (rank 2), mirrored (det F < 0 -> identity), isolated
      (identity), coincident (F = 0 with n > 0 -> identity), code1 (one neighbour whose old offset has x exactly 0).
    From 54 bones on there are TWO groups of every degenerate class: one at the lowest indices, one at the highest (wholly beyond 64 from 87 bones
    on; the last bone of all is always a degenerate one), the generic bones -- each related to its 8 nearest generic bones, itself included --
    between them.  -> dict(bones, motions, rel [nb,nb] int64 as CPU tensors, ranges = {class: [(start, stop), ...]}).
    Asserts that every singular-value ratio that decides a rank is below SVD_ZERO (an exact zero) or above RANK_CLEAR."""
    rng = np.random.default_rng(1000 * nb + seed)
    bones, new = np.zeros((nb, 3)), np.zeros((nb, 3))
    rel = np.zeros((nb, nb), dtype=np.int64)
    ranges = {}

    def place(names, start):
        for name, size in names:
            idx = np.arange(start, start + size)
            _fill_group(name, idx, bones, new, rel, rng)
            ranges.setdefault(name, []).append((start, start + size))
            start += size
        return start

    if nb >= 2 * _BLOCK + _GENERIC_MIN:
        lo = place(_GROUPS, 0)
        place(_GROUPS[::-1], nb - _BLOCK)        # (mirrored, ..., one_neighbour): other lanes than the low block's
        generic = np.arange(lo, nb - _BLOCK)
    else:
        chosen, left = [], nb
        for name, size in _GROUPS:               # greedy, in this order
            if size <= left:
                chosen.append((name, size))
                left -= size
        if 0 < left < _GENERIC_MIN:
            chosen += [("isolated", 1)] * left
            left = 0
        lo = place(chosen, 0)
        generic = np.arange(lo, nb)
    if generic.size:
        g = generic
        bones[g] = rng.random((g.size, 3))
        R = axis_angle64([0.3, -0.5, 0.8], 0.3)
        new[g] = (bones[g] - 0.5) @ R.T + 0.5 + 0.002 * rng.standard_normal((g.size, 3))
        d = np.linalg.norm(bones[g][:, None] - bones[g][None], axis=-1)
        near = np.argsort(d, axis=1, kind="stable")[:, :8]
        rel[np.repeat(g, near.shape[1]), g[near].reshape(-1)] = 1
        ranges["generic"] = [(int(g[0]), int(g[-1]) + 1)]
    b32 = bones.astype(np.float32)
    m32 = (new.astype(np.float32) - b32).astype(np.float32)
    scene = dict(bones=torch.from_numpy(b32), motions=torch.from_numpy(m32), rel=torch.from_numpy(rel), ranges=ranges)
    # no rank decision hangs on rounding
    F, n = moments_ref64(b32, m32, rel)
    S = singular_values64(F.astype(np.float32))
    for i in range(nb):
        if n[i] == 0 or S[i, 0] == 0.0:
            continue
        for ratio in S[i, 1:] / S[i, 0]:
            assert ratio < SVD_ZERO or ratio > RANK_CLEAR, ("bone_scene: a rank decision near rounding", nb, seed, i, S[i])
    return scene


def class_indices(scene, name):
    return [i for a, b in scene["ranges"].get(name, []) for i in range(a, b)]


# ------------------------------------------------------------------------------------------ half-turns
HALF_TURN_DIAGS = ((1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))
HALF_TURN_QUATS = ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
NEAR_HALF_TURN_AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.6, -0.3, 0.74), (-0.2, 0.9, 0.4))
NEAR_HALF_TURN_GAPS = (1e-1, 1e-2, 1e-3, 3e-4)


def _stars(rotations, arms):
    """One star per rotation: a bone at (.5, .5, .5) that does not move and is related to its neighbours at 0.25 * arm, which turn about it
    by the rotation; the neighbours are related to nobody.  -> scene dict with ``stars`` = the centre bones' indices."""
    k = len(arms)
    nb = len(rotations) * (k + 1)
    bones = np.full((nb, 3), 0.5)
    new = bones.copy()
    rel = np.zeros((nb, nb), dtype=np.int64)
    stars = []
    for s, R in enumerate(rotations):
        c = s * (k + 1)
        stars.append(c)
        for a, arm in enumerate(arms):
            o = 0.25 * np.asarray(arm, dtype=np.float64)
            bones[c + 1 + a] = 0.5 + o
            new[c + 1 + a] = 0.5 + np.asarray(R, dtype=np.float64) @ o
            rel[c, c + 1 + a] = 1
    b32 = bones.astype(np.float32)
    m32 = (new.astype(np.float32) - b32).astype(np.float32)
    return dict(bones=torch.from_numpy(b32), motions=torch.from_numpy(m32), rel=torch.from_numpy(rel), stars=stars)


def _tilted_axes():
    """Half-turn axes off the coordinate axes: three whose rotation matrix is exact in fp32 (a signed permutation: (1,1,0), (0,1,1),
    (1,0,1)), then nine per dominant coordinate: 30 stars of 4 bones."""
    rng = np.random.default_rng(314)
    axes = [(1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0)]
    for k in range(3):
        for _ in range(9):
            a = rng.uniform(-0.6, 0.6, 3)
            a[k] = 1.0
            axes.append(tuple(a / np.linalg.norm(a)))
    return axes


def half_turn_stars():
    """(exact, near, tilted).
    exact: three stars with six neighbours at +- 0.25 e_k moved by exactly diag(1,-1,-1), diag(-1,1,-1), diag(-1,-1,1): F is exactly
      +- 0.125 on the diagonal, the Jacobi loop makes no rotation, the fit must return the diagonal matrix EXACTLY and mat2quat takes its
      second, third and fourth branch (trace = -1): unit quaternions (0,1,0,0), (0,0,1,0), (0,0,0,1).  ``rotations`` / ``quats`` = those.
    near: one star (three neighbours at + 0.25 e_k, F = R / 16) per (axis, gap) of NEAR_HALF_TURN_AXES x NEAR_HALF_TURN_GAPS turned by
      pi - gap: the trace branch with a tiny w (or, once trace + 1 drowns in fp32 rounding, whichever branch the rounded matrix picks).
    tilted: such stars turned by pi exactly (gap 0) about _tilted_axes(): the fitted matrix's trace is -1 up to fp32 rounding, so
      about half of them take a half-turn branch WITH non-zero off-diagonal sums (on a coordinate axis those sums are all zero, and a
      wrong sign on one of them would not show).
    near / tilted: ``rotations`` = the fp64 rotations, ``labels`` = (axis, gap)."""
    e = np.eye(3)
    exact = _stars([np.diag(d) for d in HALF_TURN_DIAGS], [s * e[k] for k in range(3) for s in (1.0, -1.0)])
    exact["rotations"] = torch.tensor(np.stack([np.diag(d) for d in HALF_TURN_DIAGS]), dtype=torch.float32)
    exact["quats"] = torch.tensor(HALF_TURN_QUATS, dtype=torch.float32)

    def family(labels):
        rots = [axis_angle64(ax, math.pi - gap) for ax, gap in labels]
        sc = _stars(rots, [e[k] for k in range(3)])
        sc["rotations"] = torch.tensor(np.stack(rots))
        sc["labels"] = labels
        return sc
    near = family([(ax, gap) for ax in NEAR_HALF_TURN_AXES for gap in NEAR_HALF_TURN_GAPS])
    tilted = family([(ax, 0.0) for ax in _tilted_axes()])
    return exact, near, tilted


def mat2quat_branch(R):
    """Which branch of mat2quat (0 = trace, 1 / 2 / 3 = largest diagonal element x / y / z) fp32 matrices [n,3,3] take: the reference's
    comparisons on the fp32 sums, as the host path and the kernel evaluate them."""
    R = np.asarray(R, dtype=np.float32)
    m00, m11, m22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    t = np.maximum((m00 + m11) + m22, np.float32(-1))
    b0 = t > -1
    b1 = ~b0 & (m00 >= m11) & (m00 >= m22)
    b2 = ~b0 & (m11 >= m22) & (m11 > m00)
    return np.where(b0, 0, np.where(b1, 1, np.where(b2, 2, 3)))


# ------------------------------------------------------------------------------------------ Gaussians around bones
GAUSSIAN_GROUPS = ("on_bone", "inside_clamp", "across_clamp", "underflow", "free")


def gaussians_around(bones, P, seed=0):
    """P Gaussians (xyz [P,3], unit quaternions [P,4], CPU fp32) around the bones, rows in this order:
      on_bone      exactly on a bone (distance 0: the clamp of the inverse distance at its far end);
      inside_clamp 3e-5 from a bone;
      across_clamp 1e-4 (1 +- 1e-3) from a bone, alternating;
      underflow    1e-25 from a bone along an axis on which the bone's coordinate is exactly 0 (the squared distance underflows in fp32;
                   only bones with such a coordinate can have one: the group is empty without them);
      free         uniform in the unit cube.
    Up to 8 rows per special group, fewer when P or the number of bones is small (P = 1: one Gaussian on a bone).
    -> (xyz, quat, ranges = {group: (start, stop)})."""
    rng = np.random.default_rng(77 + 131 * P + seed)
    b = np.asarray(bones, dtype=np.float32).reshape(-1, 3)
    nb = b.shape[0]
    per = max(1, min(8, nb, P // 5))
    xyz = np.zeros((P, 3), dtype=np.float32)
    ranges, row = {}, 0

    def take(name, rows):
        nonlocal row
        rows = rows[:max(0, P - row)]
        xyz[row:row + len(rows)] = rows
        ranges[name] = (row, row + len(rows))
        row += len(rows)

    pick = lambda: b[rng.permutation(nb)[:per]].astype(np.float64)      # noqa: E731
    unit = lambda n: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.standard_normal((n, 3)))   # noqa: E731
    take("on_bone", pick().astype(np.float32))
    take("inside_clamp", (pick() + 3e-5 * unit(per)).astype(np.float32))
    sign = np.where(np.arange(per) % 2 == 0, 1.0, -1.0)[:, None]
    take("across_clamp", (pick() + 1e-4 * (1 + 1e-3 * sign) * unit(per)).astype(np.float32))
    zero = [(i, int(np.nonzero(b[i] == 0)[0][0])) for i in range(nb) if (b[i] == 0).any()][:per]
    under = np.array([b[i] for i, _ in zero], dtype=np.float32).reshape(-1, 3)
    for r, (_, ax) in enumerate(zero):
        under[r, ax] = np.float32(1e-25)
    take("underflow", under)
    take("free", rng.random((P - row, 3)).astype(np.float32))
    q = rng.standard_normal((P, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return torch.from_numpy(xyz), torch.from_numpy(q), ranges


def skinning_case(P, nb, seed=0):
    """Inputs of one skinning call: nb bones in the unit cube (bone 0 with x exactly 0, so that the underflow rows exist), orthonormal R
    (QR of random matrices), small t, unit bone quaternions with w >= 0, and gaussians_around them.  CPU fp32 tensors."""
    rng = np.random.default_rng(5 + 17 * P + 1009 * nb + seed)
    bones = rng.random((nb, 3)).astype(np.float32)
    bones[0, 0] = 0.0
    R = np.linalg.qr(rng.standard_normal((nb, 3, 3)))[0].astype(np.float32)
    t = (0.02 * rng.standard_normal((nb, 3))).astype(np.float32)
    bq = rng.standard_normal((nb, 4))
    bq[:, 0] = np.abs(bq[:, 0])
    bq = (bq / np.linalg.norm(bq, axis=1, keepdims=True)).astype(np.float32)
    xyz, quat, ranges = gaussians_around(bones, P, seed)
    return dict(bones=torch.from_numpy(bones), R=torch.from_numpy(R), t=torch.from_numpy(t), bq=torch.from_numpy(bq), xyz=xyz, quat=quat,
                ranges=ranges)


# the sizes tests/test_rollout_geometry_gpu.py uses (tests/test_dynamics_ref_cpu.py pins the builders at the same ones)
FIT_SIZES_MASK = (1, 2, 63, 64, 65, 100, 127, 128)      # bit-mask path of fit_bones_kernel: one and two workgroups, both ballot halves
FIT_SIZES_ROWS = (129, 160, 257)                         # its row walk
SKIN_SIZES = ((1, 1), (255, 2), (256, 85), (257, 100), (511, 255), (512, 256), (513, 257), (1025, 513))     # (P, nb)
