"""Generate ``dyn_batch_golden.npz``: samples of the reference's ``DynDataset.__getitem__`` (/root/reference/src/data/dataset.py:332-516),
captured by IMPORTING the Python reference in the build container.  Run once, here:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dyn_batch_goldens.py

The dataset object is made with ``object.__new__`` from in-memory arrays (no episode files); ``np.random`` is wrapped so that every draw
of a sample is recorded -- they are the inputs of ``gsdyn.make_dynamics_batch``.  ``dgl.geometry.farthest_point_sampler`` is an absent
third-party function: the project's definition (first maximum on ties) stands in for it.  Two configurations at small sizes, a rope-like
one (connect_all off, topk 5) and a cloth-like one (connect_all on, topk 6), P = 60 particles, max_nobj = 20.

The reference evaluates its distances with other roundings than the project (numpy's norm, a BLAS product, float64 noise), so a sample is
only a fair golden when none of its decisions is near a tie.  Checked here in fp64 (tests/dyn_batch_ref.decision_margins), and the scene
is REDRAWN until all samples of a configuration pass -- no sample is skipped:
  no pair distance within 1e-5 relative of the threshold; the k-th and (k + 1)-th nearest object at least 1e-5 relative apart; the best
  and second-best candidate of every sampling pick and every thinning round at least 1e-5 relative apart; no thinning maximum within 1e-5
  relative of the radius.
Only inputs, draws and outputs are stored -- data, no reference source text.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src"
OUT = os.path.join(HERE, "dyn_batch_golden.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "gs-dynamics_amd"))
MARGIN = 1e-5

CONFIGS = dict(
    rope=dict(n_his=3, n_future=3, max_nobj=20, max_nR=200, topk=5, connect_all=False, fps_radius_range=[0.03, 0.05],
              adj_radius_range=[0.06, 0.1], state_noise=0.004),
    cloth=dict(n_his=3, n_future=3, max_nobj=20, max_nR=300, topk=6, connect_all=True, fps_radius_range=[0.02, 0.04],
               adj_radius_range=[0.05, 0.09], state_noise=0.004),
)
P, FRAMES, SAMPLES = 60, 10, 3


def import_reference():
    sys.dont_write_bytecode = True
    from gsdyn.dynamics import farthest_point_sampler
    for name in ("open3d", "cv2", "dgl", "dgl.geometry", "ipdb", "tqdm"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["dgl.geometry"].farthest_point_sampler = lambda pos, npoints, start_idx=0: farthest_point_sampler(pos, npoints, start_idx)
    sys.modules["dgl"].geometry = sys.modules["dgl.geometry"]
    sys.modules["tqdm"].tqdm = lambda x, **k: x
    sys.path.insert(0, REF)
    from data.dataset import DynDataset  # noqa
    return DynDataset


class Recorder:
    """np.random.randint / uniform / permutation, recording what they return."""

    def __init__(self, rng):
        self.rng, self.log = rng, []

    def randint(self, *a, **k):
        v = self.rng.randint(*a, **k)
        self.log.append(("randint", v))
        return v

    def uniform(self, *a, **k):
        v = self.rng.uniform(*a, **k)
        self.log.append(("uniform", v))
        return v

    def permutation(self, *a, **k):
        v = self.rng.permutation(*a, **k)
        self.log.append(("permutation", v))
        return v


def scene(rng, kind):
    """A strip (rope) or a sheet (cloth) of P particles that drifts and bends over FRAMES frames, and a tool path above it."""
    if kind == "rope":
        base = np.stack([rng.uniform(0, 0.4, P), rng.uniform(-0.015, 0.015, P), rng.uniform(0, 0.01, P)], 1)
    else:
        base = np.stack([rng.uniform(0, 0.25, P), rng.uniform(0, 0.2, P), rng.uniform(0, 0.01, P)], 1)
    t = np.arange(FRAMES)[:, None, None]
    bend = 0.004 * t * np.sin(9.0 * base[None, :, 0:1]) * np.array([0.0, 1.0, 0.3])
    xyz = (base[None] + bend + 0.002 * t * np.array([1.0, 0.5, 0.0])).astype(np.float32)
    eef = (np.array([0.1, 0.05, 0.03]) + 0.006 * np.arange(FRAMES)[:, None] * np.array([1.0, 0.4, 0.0]) + rng.uniform(-0.002, 0.002, (FRAMES, 3)))
    return xyz, eef.astype(np.float32)


def one_config(DynDataset, kind, cfg, rng):
    from dyn_batch_ref import decision_margins
    n_his, n_future = cfg["n_his"], cfg["n_future"]
    T = n_his + n_future
    xyz, eef = scene(rng, kind)
    ds = object.__new__(DynDataset)
    ds.phase = "train"
    ds.dataset_config = dict(n_his=n_his, n_future=n_future, datasets=[dict(
        max_n=1, max_tool=1, max_nobj=cfg["max_nobj"], max_nR=cfg["max_nR"], fps_radius_range=cfg["fps_radius_range"],
        adj_radius_range=cfg["adj_radius_range"], state_noise=dict(train=cfg["state_noise"], valid=0.0), topk=cfg["topk"],
        connect_all=cfg["connect_all"])])
    ds.obj_kypts, ds.tool_kypts = [{0: xyz}], [{0: eef[:, None, :]}]
    starts = rng.randint(0, FRAMES - T + 1, SAMPLES)
    pairs = starts[:, None] + np.arange(T)[None, :]
    ds.pair_lists = np.concatenate([np.zeros((SAMPLES, 1), int), pairs], 1)
    rec = Recorder(np.random.RandomState(int(rng.randint(0, 2 ** 31 - 1))))
    saved = np.random.randint, np.random.uniform, np.random.permutation
    np.random.randint, np.random.uniform, np.random.permutation = rec.randint, rec.uniform, rec.permutation
    samples = []
    try:
        for i in range(SAMPLES):
            rec.log = []
            out = ds[i]
            samples.append((out, list(rec.log)))
    finally:
        np.random.randint, np.random.uniform, np.random.permutation = saved
    draws = dict(start_idx=[], fps_radius=[], thin_start=[], noise=[], rot=[], adj_thresh=[])
    for out, log in samples:
        kinds = [k for k, _ in log]
        assert kinds == ["randint", "uniform", "randint", "permutation", "uniform", "uniform", "uniform"], kinds
        v = [x for _, x in log]
        ang = v[5]
        draws["start_idx"].append(v[0]); draws["fps_radius"].append(np.float32(v[1])); draws["thin_start"].append(v[2])
        draws["noise"].append(np.asarray(v[4]).astype(np.float32))
        draws["rot"].append(np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=np.float32))
        draws["adj_thresh"].append(np.float32(v[6]))
    d = {k: np.stack(v) for k, v in draws.items()}
    d["start_idx"], d["thin_start"] = d["start_idx"].astype(np.int64), d["thin_start"].astype(np.int64)
    res = {}
    for key in samples[0][0]:
        res[key] = np.stack([np.asarray(s[0][key]) for s in samples])
    # ---- every decision away from a tie, judged on the reference's own numbers (fp64)
    worst = {}
    for b in range(SAMPLES):
        m = decision_margins(xyz, eef, pairs, b, n_his=n_his, max_nobj=cfg["max_nobj"], topk=cfg["topk"], start_idx=d["start_idx"],
                             thin_start=d["thin_start"], fps_radius=d["fps_radius"].astype(np.float64), adj_thresh=d["adj_thresh"].astype(np.float64),
                             last=res["state"][b, n_his - 1])
        if m.pop("n_obj") != int(res["obj_mask"][b].sum()):
            return None, "object count differs from the fp64 restatement"
        for k, x in m.items():
            worst[k] = min(worst.get(k, np.inf), x)
    bad = {k: x for k, x in worst.items() if not x >= MARGIN}
    if bad:
        return None, f"near a tie: {bad}"
    return dict(particles=xyz, eef=eef, pairs=pairs.astype(np.int64), **d, **{"out_" + k: x for k, x in res.items()}), worst


def main():
    DynDataset = import_reference()
    out = {}
    rng = np.random.RandomState(0)
    for kind, cfg in CONFIGS.items():
        for attempt in range(200):
            got, info = one_config(DynDataset, kind, cfg, rng)
            if got is not None:
                break
            print(f"{kind}: scene {attempt} redrawn ({info})")
        else:
            raise SystemExit(f"{kind}: no scene away from every tie")
        print(f"{kind}: scene {attempt} kept, smallest relative gaps {info}; objects {got['out_obj_mask'].sum(1)}, "
              f"relations {(got['out_Rr'].sum(-1) > 0).sum(1)}")
        for k, v in got.items():
            out[f"{kind}_{k}"] = v
        out[f"{kind}_cfg_keys"] = np.array(["n_his", "n_future", "max_nobj", "max_nR", "topk", "connect_all"])
        out[f"{kind}_cfg_vals"] = np.array([cfg[k] for k in ("n_his", "n_future", "max_nobj", "max_nR", "topk", "connect_all")], np.int64)
        out[f"{kind}_state_noise"] = np.array([cfg["state_noise"]], np.float64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
