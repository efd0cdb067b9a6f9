"""tile_sort by list-length class (gsr_binning.hip): one wave with 1 / 2 / 4 / 8 keys per lane up to 64 / 128 / 256 / 512 entries, a PAIR
of waves of one workgroup for 513 .. 1016 entries (the first 512 and the rest in registers, the 1024-merge's first step crosses through LDS), the
4096-entry block above.  Lists whose length sits on each side of every class edge, with many equal-depth ties, in a two-view call,
synchronous and capacity mode: point_list, ranges and n_contrib against the oracle bit for bit.  And one launch that mixes several
513 .. 1016 lists with short ones -- an odd number of them, an even number, none -- for the block -> ticket mapping."""
import functools

import numpy as np
import pytest
import torch

from hipcheck import *  # noqa: F401,F403
from hipcheck import _check_lists, _settings

pytestmark = pytest.mark.gpu


def _oracles(g, cams):
    return [TiledOracle(c, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"], rotations=g["rotations"],
                        nthreads=8) for c in cams]


def _lens(o2):
    return o2.ranges[:, 1].astype(np.int64) - o2.ranges[:, 0].astype(np.int64)


@functools.lru_cache(maxsize=None)
def edge_scene(P, W, H):
    """P Gaussians far wider than the image and faint (as in test_tile_sort_paths): every one lands in every tile, so every list has P
    entries.  Half of them are duplicated in position (equal depth bits) and 150 share one depth (test_tile_row_binning_lists_vs_oracle)."""
    g = random_gaussians(P, seed=170 + P, scale_lo=5.0, scale_hi=9.0, spread=0.5)
    g["opacities"][:] = 0.03
    half = P // 2
    g["means3D"][half:2 * half] = g["means3D"][:half]
    g["means3D"][:150] = g["means3D"][0]
    cams = (ring_camera(W, H, v=1), ring_camera(W, H, v=3))
    return g, cams, _oracles(g, cams)


MIXED_TILES = ((0, 0), (2, 1), (3, 3))      # (tile column, tile row) of the clusters of the mixed scene, in view 0


@functools.lru_cache(maxsize=None)
def mixed_scene(k):
    """64 x 64 (16 tiles): 400 small Gaussians (short lists) and k clusters of 600 tiny ones, each strung along view 0's ray through the
    centre of one tile: k lists of 513 .. 1016 entries in view 0; in view 1, a quarter turn on, the clusters are streaks over several tiles."""
    W = H = 64
    cams = (ring_camera(W, H, v=1), ring_camera(W, H, v=2))
    g = random_gaussians(400, seed=181, scale_lo=0.01, scale_hi=0.04)
    eye = np.array([4.0 * np.cos(2 * np.pi / 4 + 0.3), 0.8, 4.0 * np.sin(2 * np.pi / 4 + 0.3)])      # ring_camera(v=1)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0]); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    # pixels per world unit at the origin's depth, from the oracle's own projection of two points
    probe = random_gaussians(2, seed=1, scale_lo=0.01, scale_hi=0.02)
    probe["means3D"] = np.stack([np.zeros(3), 0.1 * right]).astype(np.float32)
    m2 = _oracles(probe, cams[:1])[0].means2D
    ppu = (m2[1] - m2[0]) / 0.1                                    # pixel step per unit along `right` (x, y)
    sx = ppu[0]
    sy = -abs(sx)                                                  # `up` moves the image point towards smaller y by the same scale
    rng = np.random.default_rng(182)
    parts = [g]
    for i, (tx, ty) in enumerate(MIXED_TILES[:k]):
        c = random_gaussians(600, seed=190 + i, scale_lo=0.0015, scale_hi=0.003)
        dx, dy = (16 * tx + 8 - m2[0][0]) / sx, (16 * ty + 8 - m2[0][1]) / sy
        t = rng.uniform(-0.5, 0.5, (600, 1))
        c["means3D"] = (t * fwd[None] + dx * right[None] + dy * up[None] + rng.normal(0, 0.003, (600, 3))).astype(np.float32)
        c["means3D"][300:] = c["means3D"][:300]                    # equal-depth pairs inside the long lists too
        c["opacities"][:] = 0.02
        parts.append(c)
    g = {key: np.concatenate([p[key] for p in parts]) for key in g}
    return g, cams, _oracles(g, cams)


def n_pair_lists(o2s):
    return sum(int(((_lens(o) > 512) & (_lens(o) <= 1016)).sum()) for o in o2s)


def _run_and_check(g, cams, o2s, dev):
    from diff_gaussian_rasterization import _hip
    P, (H, W) = len(g["means3D"]), (cams[0].image_height, cams[0].image_width)
    t = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    rss = [_settings(c, dev) for c in cams]
    _hip._entries_capacity.pop((dev.index, P, H, W), None)
    for no_sync in (False, True):          # the second call runs in capacity mode (the first one left the capacity behind)
        im, radii, depth, states = _hip.rasterize_forward_batch(rss, t["means3D"], t["opacities"], t["colors_precomp"], None, t["scales"],
                                                                t["rotations"], None, no_host_sync=no_sync)
        assert (states[0].pending is not None) == no_sync and _hip.forward_counts_ok(states)
        torch.cuda.synchronize()
        for v, o2 in enumerate(o2s):
            views = _hip.debug_views(states[v])
            D = int(views["offsets"][-1])
            views["point_list"] = views["point_list"][:D]
            ok = ~o2.ambiguous
            assert np.array_equal(radii[v].cpu().numpy(), o2.radii)
            _check_lists(views, H, W, o2.point_list, o2.ranges, o2.n_contrib, ok, o2.means2D, o2.conic_opacity, o2.tiles_touched, o2.offsets)
            assert mixed_err(im[v].cpu().numpy()[:, ok], o2.color[:, ok]) < TOL
            assert mixed_err(depth[v].cpu().numpy()[:, ok], o2.depth[:, ok]) < TOL


EDGE_CASES = [(256, 32, 32), (257, 48, 32), (512, 48, 32), (513, 32, 32), (600, 48, 32), (1016, 32, 32), (1017, 48, 32),
              # the upper wave of a pair holds 1, 2, 4 or 8 keys per lane: n - 512 on each side of 64, 128 and 256
              (576, 48, 32), (577, 32, 32), (640, 32, 32), (641, 48, 32), (768, 48, 32), (769, 32, 32)]


@pytest.mark.parametrize("P,W,H", EDGE_CASES)
def test_list_length_on_each_side_of_every_class_edge(dev, P, W, H):
    g, cams, o2s = edge_scene(P, W, H)
    for o2 in o2s:                         # the case sits in its class: every tile's list holds all P Gaussians
        assert _lens(o2).min() == _lens(o2).max() == P, (_lens(o2).min(), _lens(o2).max())
    _run_and_check(g, cams, o2s, dev)


@pytest.mark.parametrize("k,n_pair", [(2, 3), (3, 4), (0, 0)])
def test_pair_tickets_next_to_short_lists_in_one_launch(dev, k, n_pair):
    """n_pair lists of 513 .. 1016 entries in a launch of short ones (k clusters: one such list each in view 0, and their streaks pile up
    to one more in view 1): an odd count leaves the last workgroup's second pair of waves without a ticket, none leaves no paired
    workgroup at all; the wave tickets start right behind them."""
    g, cams, o2s = mixed_scene(k)
    lens = np.concatenate([_lens(o) for o in o2s])
    assert n_pair_lists(o2s) == n_pair, sorted(lens)[-6:]
    assert lens.max() <= 1016 and ((lens > 0) & (lens <= 512)).sum() >= 16
    _run_and_check(g, cams, o2s, dev)
