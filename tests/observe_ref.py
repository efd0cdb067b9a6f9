"""fp64 referee and shared scenes of the perception tests (tests/test_observe_cpu.py, tests/test_observe_gpu.py).

The referee restates the reference's formulas in numpy fp64, independently of gsdyn/observe.py: ``depth2fgpcd`` with a general inverse of
the 3x3 intrinsics, ``R @ p + t``, the per-voxel mean of the fp64 points.  It never rounds to fp32."""
import numpy as np


def look_at(pos, target=(0.0, 0.0, 0.0)):
    """Camera-to-board rotation of a camera at ``pos`` that looks at ``target``: columns = the camera's x (right), y (down), z (forward)."""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    z = (target - pos) / np.linalg.norm(target - pos)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], 1)


CAM_POS = [(0.55, 0.45, 0.6), (-0.5, 0.5, 0.7), (-0.45, -0.55, 0.65), (0.6, -0.4, 0.55)]
BBOX = np.array([[-0.25, 0.25], [-0.2, 0.2], [-0.02, 0.12]], np.float32)


def scene(V, H, W, seed=0, bad_depths=True):
    """A tabletop seen by V cameras with different intrinsics and poses: every pixel's ray is cut at a random height in [-0.04, 0.14] over
    the board, so the kept points fill a slab and some fall outside the box on every side.  With ``bad_depths`` a few pixels are NaN, inf,
    0 and negative.  Returns float32 depths [V, H, W], K4 [V, 4], R [V, 3, 3], t [V, 3], BBOX, uint8 colors [V, H, W, 3], bool masks."""
    g = np.random.default_rng(seed)
    depths = np.zeros((V, H, W), np.float32)
    K4 = np.zeros((V, 4), np.float32)
    R = np.zeros((V, 3, 3), np.float32)
    t = np.zeros((V, 3), np.float32)
    for v in range(V):
        pos = np.asarray(CAM_POS[v % 4]) * (1.0 + 0.05 * (v // 4))
        Rv = look_at(pos, (0.02 * v, -0.01 * v, 0.03))
        f = 0.9 * max(H, W) * (1.0 + 0.1 * v)
        K4[v] = (f, f * 1.03, 0.5 * W - 0.3 + 0.2 * v, 0.5 * H + 0.4 - 0.1 * v)
        R[v], t[v] = Rv, pos
        x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        ray = np.stack([(x - K4[v, 2]) / K4[v, 0], (y - K4[v, 3]) / K4[v, 1], np.ones_like(x)], -1)
        z0 = g.uniform(-0.04, 0.14, (H, W))
        depths[v] = ((z0 - pos[2]) / (ray @ Rv[2])).astype(np.float32)
    if bad_depths and depths.size >= 8:
        flat = depths.reshape(-1)
        where = g.choice(flat.size, size=min(8, flat.size // 2), replace=False)
        flat[where] = np.resize(np.array([np.nan, np.inf, 0.0, -0.5, -np.inf, 5.0], np.float32), where.size)
    colors = g.integers(0, 256, (V, H, W, 3), dtype=np.uint8)
    masks = g.uniform(size=(V, H, W)) < 0.9
    return depths, K4, R, t, BBOX.copy(), colors, masks


def world64(depths, K4, R, t):
    """The reference's unprojection in fp64: p_cam = inv(K) @ (x, y, 1) * d with a general 3x3 inverse, w = R @ p_cam + t.  [V, H, W, 3]."""
    V, H, W = depths.shape
    out = np.zeros((V, H, W, 3), np.float64)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    pix = np.stack([x, y, np.ones_like(x)], -1)
    for v in range(V):
        fx, fy, cx, cy = (float(a) for a in K4[v])
        Kinv = np.linalg.inv(np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64))
        with np.errstate(invalid="ignore"):                     # NaN / inf depths stay NaN / inf
            p = (pix @ Kinv.T) * depths[v].astype(np.float64)[..., None]
            out[v] = p @ R[v].astype(np.float64).T + t[v].astype(np.float64)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)
