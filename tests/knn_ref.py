"""Reference for gsdyn.knn_points in numpy, and an fp64 statement of the outlier loop.

The definition, for fp32 points [N, 3]: d2(i, j) = (dx*dx + dy*dy) + dz*dz with dx = p[i].x - p[j].x and so on, every operation fp32 in
that order (numpy float32 arrays: one rounding per operation, nothing fused); row i = the k smallest under the total order (d2
ascending, then j ascending).  With exclude_self, j = i is left out by identity."""
import numpy as np

MAX_K = 66   # entries of the order kept per row: enough for every k <= 65, with or without the query itself


class KnnRef:
    """The head of every checked row's total order, computed once per cloud; ``top(k, exclude_self)`` cuts the answers out of it.
    ``rows``: the query rows to compute (default: all)."""

    def __init__(self, points, rows=None):
        p = np.ascontiguousarray(points)
        assert p.ndim == 2 and p.shape[1] == 3
        self.dtype = p.dtype
        self.N = p.shape[0]
        self.rows = np.arange(self.N) if rows is None else np.asarray(rows, dtype=np.int64)
        take = min(self.N, MAX_K)
        self.order = np.empty((len(self.rows), take), dtype=np.int64)
        self.d2 = np.empty((len(self.rows), take), dtype=p.dtype)
        x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
        chunk = max(1, (1 << 22) // self.N)
        for s in range(0, len(self.rows), chunk):
            r = self.rows[s:s + chunk]
            dx, dy, dz = x[r, None] - x[None], y[r, None] - y[None], z[r, None] - z[None]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == p.dtype
            # everything up to the take-th smallest VALUE (ties with it included), then a stable sort of those few: the stable order's head
            kth = np.partition(d2, take - 1, axis=1)[:, take - 1]
            for a in range(len(r)):
                cand = np.nonzero(d2[a] <= kth[a])[0]                       # ascending j
                o = cand[np.argsort(d2[a, cand], kind="stable")][:take]     # stable: equal d2 keep ascending j
                self.order[s + a] = o
                self.d2[s + a] = d2[a, o]

    def top(self, k, exclude_self=False):
        """(idx [R, k] int64, d2 [R, k]) of the checked rows."""
        assert 1 <= k <= self.N - (1 if exclude_self else 0) and k + (1 if exclude_self else 0) <= self.order.shape[1]
        if not exclude_self:
            return self.order[:, :k].copy(), self.d2[:, :k].copy()
        idx = np.empty((len(self.rows), k), dtype=np.int64)
        d2 = np.empty((len(self.rows), k), dtype=self.dtype)
        for a, i in enumerate(self.rows):
            keep = self.order[a] != i
            idx[a] = self.order[a][keep][:k]
            d2[a] = self.d2[a][keep][:k]
        return idx, d2


def knn_ref(points, k, exclude_self=False, rows=None):
    return KnnRef(points, rows).top(k, exclude_self)


def bits(a):
    """The bit patterns of a float array (so that equality means bit equality, and NaN / -0 cannot hide)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def outlier_loop_fp64(xyz, nb_neighbors=50, std_ratio0=2.0, step=0.5):
    """gsdyn.dynamics.remove_statistical_outliers in fp64: (surviving indices, passes run, the smallest relative distance of any
    point's mean neighbour distance to a pass's threshold)."""
    x = np.asarray(xyz, dtype=np.float64)
    keep = np.arange(x.shape[0])
    it, margin = 0, np.inf
    while True:
        p = x[keep]
        k = min(nb_neighbors, p.shape[0])
        d2 = sum((p[:, None, c] - p[None, :, c]) ** 2 for c in range(3))
        md = np.sqrt(np.partition(d2, k - 1, axis=1)[:, :k]).mean(1)
        thr = md.mean() + (std_ratio0 + step * it) * md.std(ddof=1)
        margin = min(margin, float(np.abs(md - thr).min() / thr))
        ok = md < thr
        it += 1
        if ok.all():
            return keep, it, margin
        keep = keep[ok]


def tabletop_cloud(seed, n=3000, n_out=30):
    """The outlier tests' cloud: a thin slab plus 1 % far points, shuffled; handed out as fp32."""
    g = np.random.default_rng(seed)
    a = g.uniform(0, 1, (n, 3)).astype(np.float32) * (0.5, 0.5, 0.02)
    b = (g.uniform(-1, 1, (n_out, 3)) * 3).astype(np.float32)
    x = np.concatenate([a, b])
    g.shuffle(x)
    return x.astype(np.float32)
