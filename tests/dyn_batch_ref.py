"""Referee of gsdyn.make_dynamics_batch: a numpy restatement of its definition (gsdyn/dyn_data.py's docstring),
written independently of that module -- sample by sample, row by row, every operation a separately rounded float32 one -- plus the
fp64 margins the golden generator checks (how far each decision of a sample sits from flipping).  No torch, no kernels."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def fma32(a, b, c):
    """float32 fma(a, b, c), exactly: the product of two float32 is exact in float64; the float64 sum is turned into a round-to-odd sum
    (TwoSum gives its error), which rounds to float32 as the exact sum does (53 >= 2 x 24 + 2)."""
    a, b, c = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def sqdist32(p, q):
    """(dx dx + dy dy) + dz dz in float32, rows of p against the point (or rows) q."""
    d = (p - q).astype(F32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F32) + d[..., 2] * d[..., 2]).astype(F32)


def norm32(p, q):
    """sqrt(fma(dz, dz, fma(dy, dy, dx dx))) in float32: the thinning's distance."""
    d = (p - q).astype(F32)
    return np.sqrt(fma32(d[..., 2], d[..., 2], fma32(d[..., 1], d[..., 1], (d[..., 0] * d[..., 0]).astype(F32)))).astype(F32)


def fps_picks(cloud, npoints, start):
    mind = np.full(cloud.shape[0], np.inf, F32)
    picks, cur = [], int(start)
    for _ in range(npoints):
        picks.append(cur)
        mind = np.minimum(mind, sqdist32(cloud, cloud[cur]))
        cur = int(np.argmax(mind))                      # the first maximum
    return np.array(picks, np.int64)


def thin_picks(pts, radius, start):
    kept = [int(start)]
    dist = norm32(pts, pts[kept[0]])
    while dist.max() > F32(radius):
        kept.append(int(np.argmax(dist)))
        dist = np.minimum(dist, norm32(pts, pts[kept[-1]]))
    return np.array(kept, np.int64)


def rotate32(x, r):
    """x [..., 3] times r [3, 3]: out[c] = (x0 r[0][c] + x1 r[1][c]) + x2 r[2][c], one float32 rounding per operation."""
    x, r = np.asarray(x, F32), np.asarray(r, F32)
    out = np.empty(x.shape, F32)
    for c in range(3):
        out[..., c] = ((x[..., 0] * r[0, c]).astype(F32) + (x[..., 1] * r[1, c]).astype(F32)).astype(F32) + (x[..., 2] * r[2, c]).astype(F32)
    return out


def relations(last, n_obj, adj_thresh, topk, connect_all):
    """last [N, 3] (tool in the last row) -> the relation list [(receiver, sender)] in row-major order."""
    N = last.shape[0]
    tool = N - 1
    thr2 = F32(F32(adj_thresh) * F32(adj_thresh))
    k = min(int(topk), int(n_obj))
    rel = []
    for i in range(N):
        if not (i < n_obj or i == tool):
            continue
        dis = sqdist32(last, last[i])
        if i < n_obj:
            nearest = set(np.lexsort((np.arange(n_obj), dis[:n_obj]))[:k].tolist())      # by distance, then by index
            for j in range(n_obj):
                if dis[j] < thr2 and j in nearest:
                    rel.append((i, j))
            if dis[tool] < thr2 or connect_all:
                rel.append((i, tool))
        else:
            for j in range(n_obj):
                if dis[j] < thr2 or connect_all:
                    rel.append((i, j))
    return rel


def ref_batch(particles, eef, pairs, *, n_his, n_future, max_nobj, max_nR, topk, connect_all, start_idx, thin_start, fps_radius, adj_thresh,
              rot, noise=None, n_particles=None, dense=True):
    """numpy arrays in, dict of numpy arrays out (graph: a dict of its five int64 lists).  Raises ValueError on overflow."""
    particles, eef, pairs = np.asarray(particles, F32), np.asarray(eef, F32), np.asarray(pairs, np.int64)
    B, T = pairs.shape
    P, N = particles.shape[1], max_nobj + 1
    o = dict(state=np.zeros((B, n_his, N, 3), F32), action=np.zeros((B, N, 3), F32), tool_future=np.zeros((B, n_future - 1, N, 3), F32),
             action_future=np.zeros((B, n_future - 1, N, 3), F32), state_future=np.zeros((B, n_future, max_nobj, 3), F32),
             attrs=np.zeros((B, N, 2), F32), p_instance=np.zeros((B, max_nobj, 1), F32), obj_mask=np.zeros((B, max_nobj), bool),
             n_obj=np.zeros((B,), np.int32), fps_idx=np.full((B, max_nobj), -1, np.int64), receivers=np.full((B, max_nR), N, np.int64),
             senders=np.full((B, max_nR), N, np.int64), n_rel=np.zeros((B,), np.int32), n_rel_rows=max_nR)
    if dense:
        o["Rr"], o["Rs"] = np.zeros((B, max_nR, N), F32), np.zeros((B, max_nR, N), F32)
    g_recv, g_send = [], []
    for b in range(B):
        n_p = P if n_particles is None else int(n_particles[b])
        r = np.asarray(rot[b], F32)
        cloud = particles[pairs[b, n_his - 1], :n_p]
        picks = fps_picks(cloud, min(max_nobj, n_p), int(start_idx[b]))
        idx = picks[thin_picks(cloud[picks], fps_radius[b], int(thin_start[b]))]
        n = len(idx)
        o["n_obj"][b], o["fps_idx"][b, :n] = n, idx
        o["obj_mask"][b, :n], o["p_instance"][b, :n, 0], o["attrs"][b, :n, 0], o["attrs"][b, max_nobj, 1] = True, 1, 1, 1
        hist = np.zeros((n_his, N, 3), F32)
        for fi in range(n_his):
            hist[fi, :n], hist[fi, max_nobj] = particles[pairs[b, fi], idx], eef[pairs[b, fi]]
        if noise is not None:
            hist = (hist + np.asarray(noise[b], F32)).astype(F32)
        o["state"][b] = rotate32(hist, r)
        act = np.zeros((N, 3), F32)
        act[max_nobj] = (eef[pairs[b, n_his]] - eef[pairs[b, n_his - 1]]).astype(F32)
        o["action"][b] = rotate32(act, r)
        for fi in range(n_future - 1):
            tf, af = np.zeros((N, 3), F32), np.zeros((N, 3), F32)
            tf[max_nobj] = eef[pairs[b, n_his + fi]]
            af[max_nobj] = (eef[pairs[b, n_his + fi + 1]] - eef[pairs[b, n_his + fi]]).astype(F32)
            o["tool_future"][b, fi], o["action_future"][b, fi] = rotate32(tf, r), rotate32(af, r)
        for fi in range(n_future):
            fut = np.zeros((max_nobj, 3), F32)
            fut[:n] = particles[pairs[b, n_his + fi], idx]
            o["state_future"][b, fi] = rotate32(fut, r)
        rel = relations(o["state"][b, n_his - 1], n, adj_thresh[b], topk, connect_all)
        o["n_rel"][b] = len(rel)
        if len(rel) > max_nR:
            raise ValueError(f"sample {b} has {len(rel)} relations, more than max_nR = {max_nR}")
        for e, (i, j) in enumerate(rel):
            o["receivers"][b, e], o["senders"][b, e] = i, j
            if dense:
                o["Rr"][b, e, i], o["Rs"][b, e, j] = 1, 1
            g_recv.append(b * N + i)
            g_send.append(b * N + j)
    o["graph"] = graph_lists(g_recv, g_send, B * N)
    return o


def graph_lists(recv, send, n_rows):
    """The five lists of gsdyn.dynamics.SplitGraph from a relation list that ascends in the receiver, by counting."""
    E = len(recv)
    row_start, rev_ptr = np.zeros(n_rows + 1, np.int64), np.zeros(n_rows + 1, np.int64)
    cnt_r, cnt_s = np.bincount(np.asarray(recv, np.int64), minlength=n_rows), np.bincount(np.asarray(send, np.int64), minlength=n_rows)
    row_start[1:], rev_ptr[1:] = np.cumsum(cnt_r), np.cumsum(cnt_s)
    by_sender = [[] for _ in range(n_rows)]
    for e in range(E):
        by_sender[send[e]].append(e)
    rev_edge = np.array([e for lst in by_sender for e in lst], np.int64)
    return dict(receivers=np.asarray(recv, np.int64).reshape(-1), senders=np.asarray(send, np.int64).reshape(-1), row_start=row_start,
                rev_ptr=rev_ptr, rev_edge=rev_edge.reshape(-1))


# ------------------------------------------------------------------------------------------ fp64 margins (the golden generator's checks)
def decision_margins(particles, eef, pairs, b, *, n_his, max_nobj, topk, start_idx, thin_start, fps_radius, adj_thresh, last):
    """How far sample b's decisions sit from flipping, in float64 on the float32 inputs: dict of the smallest RELATIVE gaps --
    fps_tie (best against second-best running minimum at a pick), thin_tie (the same at a thinning round), thin_radius (a thinning maximum
    against the radius), threshold (a pair distance of `last` against the threshold), kth (the k-th against the (k + 1)-th nearest object).
    `last` = the noised, rotated last history frame [N, 3] the relations are built from; its first n_obj rows are the real objects."""
    cloud = np.asarray(particles, np.float64)[int(pairs[b, n_his - 1])]
    rel_gap = lambda a, c: abs(a - c) / max(abs(a), abs(c), 1e-300)  # noqa: E731
    out = dict(fps_tie=np.inf, thin_tie=np.inf, thin_radius=np.inf, threshold=np.inf, kth=np.inf)
    mind = np.full(cloud.shape[0], np.inf)
    picks, cur = [], int(start_idx[b])
    for k in range(min(max_nobj, cloud.shape[0])):
        picks.append(cur)
        mind = np.minimum(mind, ((cloud - cloud[cur]) ** 2).sum(-1))
        order = np.argsort(-mind, kind="stable")
        if k + 1 < min(max_nobj, cloud.shape[0]) and len(order) > 1:
            out["fps_tie"] = min(out["fps_tie"], rel_gap(mind[order[0]], mind[order[1]]))
        cur = int(order[0])
    pts = cloud[picks]
    kept = [int(thin_start[b])]
    dist = np.sqrt(((pts - pts[kept[0]]) ** 2).sum(-1))
    while True:
        order = np.argsort(-dist, kind="stable")
        out["thin_radius"] = min(out["thin_radius"], rel_gap(dist[order[0]], float(fps_radius[b])))
        if not dist[order[0]] > float(fps_radius[b]):
            break
        if len(order) > 1:
            out["thin_tie"] = min(out["thin_tie"], rel_gap(dist[order[0]], dist[order[1]]))
        kept.append(int(order[0]))
        dist = np.minimum(dist, np.sqrt(((pts - pts[kept[-1]]) ** 2).sum(-1)))
    n = len(kept)
    last = np.asarray(last, np.float64)
    thr2 = float(adj_thresh[b]) ** 2
    real = list(range(n)) + [last.shape[0] - 1]
    for i in real:
        d = ((last[real] - last[i]) ** 2).sum(-1)
        out["threshold"] = min(out["threshold"], min(rel_gap(x, thr2) for x in d))
        if i < n and n > topk:
            s = np.sort(d[:n])
            out["kth"] = min(out["kth"], rel_gap(s[topk - 1], s[topk]))
    out["n_obj"] = n
    return out


# ------------------------------------------------------------------------------------------ seeded inputs for the tests
def make_case(seed, *, B, P, n_his, n_future, max_nobj, topk, connect_all, F=7, radius=(0.02, 0.06), thresh=(0.04, 0.1), noise=0.003,
              mixed_counts=True, duplicates=False, max_nR=None, dense=True):
    """-> (arrays, kwargs) of numpy inputs for make_dynamics_batch / ref_batch: a thin sheet of P particles that drifts over F frames, a
    tool path, per-sample frame rows, particle counts (mixed within the batch, at least 1), and every random draw.  ``radius`` / ``thresh``:
    the per-sample ranges (they differ within a batch); ``duplicates``: every particle appears twice or more (ties go to the lower index).
    ``max_nR`` defaults to the exact upper bound max_nobj min(topk, max_nobj) + 2 max_nobj."""
    rng = np.random.RandomState(seed)
    base = rng.uniform(0, 1, (P, 3)) * np.array([0.3, 0.2, 0.02])
    if duplicates:
        base = base[rng.randint(0, max(P // 3, 1), P)]
    t = np.arange(F)[:, None, None]
    particles = (base[None] + 0.003 * t * np.array([1.0, -0.5, 0.2])).astype(F32)
    eef = (np.array([0.1, 0.08, 0.03]) + 0.01 * rng.uniform(-1, 1, (F, 3))).astype(F32)
    T = n_his + n_future
    pairs = rng.randint(0, F, (B, T)).astype(np.int64)
    n_particles = rng.randint(max(P // 2, 1), P + 1, B).astype(np.int32) if mixed_counts else None
    n_p = np.full(B, P) if n_particles is None else n_particles
    npick = np.minimum(n_p, max_nobj)
    ang = rng.uniform(-np.pi, np.pi, B)
    c, s, z, o = np.cos(ang), np.sin(ang), np.zeros(B), np.ones(B)
    kw = dict(n_his=n_his, n_future=n_future, max_nobj=max_nobj, topk=topk, connect_all=connect_all, dense=dense,
              max_nR=max_nobj * min(topk, max_nobj) + 2 * max_nobj if max_nR is None else max_nR,
              start_idx=(rng.uniform(0, 1, B) * n_p).astype(np.int64), thin_start=(rng.uniform(0, 1, B) * npick).astype(np.int64),
              fps_radius=rng.uniform(radius[0], radius[1], B).astype(F32), adj_thresh=rng.uniform(thresh[0], thresh[1], B).astype(F32),
              rot=np.stack([c, -s, z, s, c, z, z, z, o], 1).reshape(B, 3, 3).astype(F32),
              noise=None if noise is None else rng.uniform(-noise, noise, (B, n_his, max_nobj + 1, 3)).astype(F32), n_particles=n_particles)
    return dict(particles=particles, eef=eef, pairs=pairs), kw
