#!/usr/bin/env python
"""Do two builds of the library give the bones' rotation fit (gsr_fit_rotations, gsr_fit_bones) the same bits?

Used when the Jacobi sweep of ``fit_one_rotation`` moved into csrc/gsr_svd3.h (profiles/rigid_loss_fit_bits.txt): run ``dump`` once per
checkout (``--root`` names the checkout whose package and library are loaded; each in a process of its own), then ``compare``.

    python tools/fit_rotation_bits.py dump new.npz
    python tools/fit_rotation_bits.py dump parent.npz --root /path/to/the/parent/checkout
    python tools/fit_rotation_bits.py compare new.npz parent.npz

Inputs (seeded): 4096 moment matrices -- full rank of either handedness, every seventh of rank 2, every eleventh of rank 1, every
thirteenth scaled by 1e-6, every seventeenth without neighbours -- and two bone sets (100 and 150 bones, a 10 % relation matrix)."""
import argparse
import os
import sys


def dump(out, root):
    for p in (root, os.path.join(root, "gs-dynamics_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from diff_gaussian_rasterization import _hip
    if not torch.cuda.is_available():
        sys.exit("fit_rotation_bits.py dump runs on a HIP device; none found")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    nb = 4096
    F = rng.standard_normal((nb, 3, 3)).astype(np.float32)
    F[::7, :, 2] = 0
    k = len(F[3::11])
    F[3::11] = np.einsum("bi,bj->bij", rng.standard_normal((k, 3)), rng.standard_normal((k, 3))).astype(np.float32)
    F[5::13] *= 1e-6
    n = np.ones(nb, dtype=np.float32)
    n[::17] = 0
    R, code = _hip.fit_rotations(torch.from_numpy(F).to(dev), torch.from_numpy(n).to(dev))
    res = dict(R=R.cpu().numpy(), code=code.cpu().numpy())
    for i, m in enumerate((100, 150)):
        bones = rng.uniform(0, 0.4, (m, 3)).astype(np.float32)
        motions = (0.02 * rng.standard_normal((m, 3))).astype(np.float32)
        rel = (rng.uniform(size=(m, m)) < 0.1).astype(np.int64)
        r, q, c = _hip.fit_bones(torch.from_numpy(bones).to(dev), torch.from_numpy(motions).to(dev), torch.from_numpy(rel).to(dev))
        res.update({f"bones{i}_R": r.cpu().numpy(), f"bones{i}_quat": q.cpu().numpy(), f"bones{i}_code": c.cpu().numpy()})
    np.savez(out, **res)
    print(f"wrote {out}: library {_hip.LIB_PATH}, fit_rotations codes 0 / 1 / 2 / 3: {np.bincount(res['code'], minlength=4).tolist()}")


def compare(a, b):
    import numpy as np
    x, y = np.load(a), np.load(b)
    bad = [k for k in x.files if x[k].tobytes() != y[k].tobytes()]
    print(f"fit_rotations / fit_bones, {a} against {b}, bit for bit: " + ("IDENTICAL" if not bad else f"DIFFER in {bad}") + " -- "
          + ", ".join(f"{k} {tuple(x[k].shape)}" for k in x.files))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "dump":
        dump(args.out, os.path.abspath(args.root))
        return 0
    return compare(args.a, args.b)


if __name__ == "__main__":
    sys.exit(main())
