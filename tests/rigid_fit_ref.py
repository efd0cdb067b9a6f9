"""The referee of gsdyn.umeyama_fit / gsr_rigid_fit: the rule set of gsdyn/rigid_fit.py restated in numpy fp64
-- ``numpy.linalg.svd`` per sample with the cross-product formula on top -- and the seeded clouds the CPU and GPU tests share.

Rule set, per sample with n masked rows, mu_x / mu_y the masked means, C = (1 / n) sum (Y - mu_y)(X - mu_x)^T, s1 >= s2 >= s3:
  n >= 3 and s2 > 3 * 2^-23 * s1 : R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T, t = mu_y - R mu_x     code 0
  rank <= 1 or n < 3              : R = I, t = mu_y - mu_x                                              code 1
  n = 0                           : R = I, t = 0, sse = 0                                               code 1
  a non-finite masked value       : R, t, aligned, residual's masked rows, sse = NaN                    code 1"""
import numpy as np

RANK_TOL = 3.0 * 2.0 ** -23


def fit(X, Y, mask):
    """X, Y [B, N, 3] (any float dtype; taken to fp64), mask [B, N] bool -> dict of fp64 / int32 arrays with the keys of
    gsdyn.umeyama_fit plus ``sigma`` [B, 3] (C's singular values, descending; NaN for a non-finite sample)."""
    X, Y, mask = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64), np.asarray(mask, dtype=bool)
    B, N = mask.shape
    out = dict(R=np.zeros((B, 3, 3)), t=np.zeros((B, 1, 3)), aligned=np.zeros((B, N, 3)), residual=np.zeros((B, N, 3)), sse=np.zeros(B),
               count=np.zeros(B, dtype=np.int32), code=np.ones(B, dtype=np.int32), sigma=np.zeros((B, 3)))
    for b in range(B):
        m = mask[b]
        n = int(m.sum())
        out["count"][b] = n
        R, t = np.eye(3), np.zeros(3)
        if n > 0:
            x, y = X[b][m], Y[b][m]
            if not (np.isfinite(x).all() and np.isfinite(y).all()):
                R, t = np.full((3, 3), np.nan), np.full(3, np.nan)
                out["sigma"][b] = np.nan
            else:
                mu_x, mu_y = x.mean(0), y.mean(0)
                C = (y - mu_y).T @ (x - mu_x) / n
                U, S, Vh = np.linalg.svd(C)
                out["sigma"][b] = S
                if n >= 3 and S[1] > RANK_TOL * S[0]:
                    u1, u2, v1, v2 = U[:, 0], U[:, 1], Vh[0], Vh[1]
                    R = np.outer(u1, v1) + np.outer(u2, v2) + np.outer(np.cross(u1, u2), np.cross(v1, v2))
                    out["code"][b] = 0
                t = mu_y - R @ mu_x
        with np.errstate(invalid="ignore"):
            aligned = X[b] @ R.T + t
            res = np.where(m[:, None], Y[b] - aligned, 0.0)
        out["R"][b], out["t"][b, 0], out["aligned"][b], out["residual"][b], out["sse"][b] = R, t, aligned, res, (res * res).sum()
    return out


def condition(sigma):
    """s1 / (s2 + s3): how strongly the fitted rotation moves with a perturbation of C, relative to C's size."""
    return sigma[..., 0] / (sigma[..., 1] + sigma[..., 2])


COND_MAX = 1e4          # the bars below are stated for samples with s1 / (s2 + s3) <= COND_MAX; the seeded clouds all satisfy it


def bars(want, X, Y, eps_store):
    """Per-sample bars for an implementation that computes in fp64 and stores with unit roundoff ``eps_store`` (2^-24 for fp32 outputs, 0
    for fp64 ones), against ``want`` = fit(X, Y, mask).  With e = 2^-53:
      dR  = (16 + 2 n) e cond   -- the rotation's distance between two fp64 evaluations: C is a sum of n products per entry, summed in
                                    another order ((n + 2) e relative each, both sides), each SVD adds a few e, and the fitted rotation
                                    moves by cond = s1 / (s2 + s3) times the relative perturbation of C (code 1: no SVD enters, cond := 1);
      R        : eps_store |R| + dR
      t        : eps_store |t| + 2 dR scale          (t = mu_y - R mu_x; scale = max |X| + max |Y| over the sample's finite values)
      aligned  : eps_store |aligned| + 4 dR scale    (X R^T + t: the two errors add)
      residual : eps_store max |Y| + 4 dR scale      (relative to max |Y|, not to itself)
      sse      : eps_store sse + 2 sqrt(3 n sse) d + 3 n d^2 with d = 4 dR scale  (3 n squares, each residual within d).
    -> dict of arrays that broadcast against the outputs."""
    e = 2.0 ** -53
    n = want["count"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = np.where(want["code"] == 0, condition(want["sigma"]), 1.0)
    dR = (16.0 + 2.0 * n) * e * cond
    fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0).reshape(a.shape[0], -1).max(1, initial=0.0)  # noqa: E731
    scale = fin(np.asarray(X, dtype=np.float64)) + fin(np.asarray(Y, dtype=np.float64))
    d = 4.0 * dR * scale
    return dict(R=eps_store * np.abs(want["R"]) + dR[:, None, None],
                t=eps_store * np.abs(want["t"]) + (2.0 * dR * scale)[:, None, None],
                aligned=eps_store * np.abs(want["aligned"]) + d[:, None, None],
                residual=(eps_store * fin(np.asarray(Y, dtype=np.float64)) + d)[:, None, None],
                sse=eps_store * want["sse"] + 2.0 * np.sqrt(3.0 * n * want["sse"]) * d + 3.0 * n * d * d)


def check(got, want, X, Y, mask, eps_store, tag=""):
    """Assert ``got`` (dict of numpy arrays) against ``want`` = fit(...): code and count exact, NaN exactly where the referee has NaN, every
    float within its bar, residual exactly 0 outside the mask; every code-0 sample must be inside COND_MAX, so that no sample escapes.
    -> the worst error / bar per key."""
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["code"], want["code"]), (tag, got["code"], want["code"])
    assert not np.asarray(got["residual"])[~np.asarray(mask, dtype=bool)].any(), (tag, "residual outside the mask")          # exactly 0
    ok = want["code"] == 0
    assert (condition(want["sigma"][ok]) <= COND_MAX).all(), (tag, condition(want["sigma"][ok]).max())
    b = bars(want, X, Y, eps_store)
    worst = {}
    for k in ("R", "t", "aligned", "residual", "sse"):
        g, w = np.asarray(got[k], dtype=np.float64), want[k]
        assert g.shape == w.shape, (tag, k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, k)
        with np.errstate(invalid="ignore"):
            err, bar = np.abs(g - w), np.broadcast_to(b[k], w.shape)
        live = ~np.isnan(w)
        assert (err[live] <= bar[live]).all(), (tag, k, float((err[live] / np.maximum(bar[live], 1e-300)).max()))
        worst[k] = float((err[live] / np.maximum(bar[live], 1e-300)).max()) if live.any() else 0.0
    return worst


# ---------------------------------------------------------------------------------------------------------------- the seeded clouds
def _rotation(rng, angle=None):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(0.2, 2.5) if angle is None else angle
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def _cloud(rng, N, centre=(0.2, 0.2, 0.02), spread=(0.2, 0.12, 0.05)):
    """An anisotropic box of N points: its three extents differ, so the singular values of C stay well apart."""
    return (rng.uniform(-1, 1, (N, 3)) * np.asarray(spread) + np.asarray(centre)).astype(np.float32)


KINDS = ("noised", "planar", "mirror", "near_pi", "same", "far", "holes", "n0", "n1", "n2", "n3", "collinear")
DEGENERATE = {"n0": 0, "n1": 1, "n2": 2, "collinear": None}          # kind -> its masked row count (None: whatever the mask has); code 1


def make_case(kind, N, seed):
    """One sample of a kind: (X [N, 3] fp32, Y [N, 3] fp32, mask [N] bool).  The masks of "holes" and of every kind at N >= 8 have holes,
    not only a prefix; the n-kinds mask exactly min(n, N) rows."""
    rng = np.random.default_rng(seed)
    X = _cloud(rng, N)
    mask = np.ones(N, dtype=bool)
    if N >= 8:
        mask[rng.choice(N, N // 5, replace=False)] = False
    Rt, tt = _rotation(rng), rng.uniform(-0.1, 0.1, 3)
    noise = 0.002 * rng.standard_normal((N, 3))
    if kind == "planar":
        X[:, 2] = 0.02
        noise[:, 2] = 0.0
    elif kind == "near_pi":
        Rt = _rotation(rng, angle=np.pi - 1e-3)
    elif kind == "far":
        X = _cloud(rng, N, centre=(10.0 / np.sqrt(3),) * 3, spread=(0.05, 0.03, 0.0125))
    elif kind == "holes":
        mask = rng.uniform(size=N) < 0.5
        mask[rng.choice(N, min(N, 4), replace=False)] = True
    elif kind in ("n0", "n1", "n2", "n3"):
        mask[:] = False
        mask[rng.choice(N, min(int(kind[1]), N), replace=False)] = True
    elif kind == "collinear":
        X = (np.asarray([0.2, 0.1, 0.02]) + rng.uniform(-1, 1, (N, 1)) * np.asarray([0.3, -0.2, 0.1])).astype(np.float32)
        noise[:] = 0.0
    Y = X.astype(np.float64) @ Rt.T + tt + noise
    if kind == "mirror":
        Y = X.astype(np.float64) * np.asarray([1.0, 1.0, -1.0]) + tt + noise
    elif kind == "same":
        Y = X.astype(np.float64)
    elif kind == "collinear":
        Y = X.astype(np.float64) + tt          # (a pure shift keeps the fp32 rows on one line: C has rank 1 up to fp32 rounding)
    return X, Y.astype(np.float32), mask


def make_batch(B, N, seed, kinds=KINDS):
    """B samples cycling through ``kinds`` (shifted by the seed): (X [B, N, 3], Y [B, N, 3] fp32, mask [B, N] bool, the kinds' names)."""
    names = [kinds[(seed + b) % len(kinds)] for b in range(B)]
    cases = [make_case(k, N, 7919 * seed + 31 * b + N) for b, k in enumerate(names)]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), names
