"""Generate ``clamp_edge_oracle.npz``: the clamp-edge scene (tests/util.py clamp_edge_scene), its inputs, and what oracle O2 computes
on it without ``decisions_of`` -- fp32 and fp64 builds: radii, the fp32 colour and depth, and the backward of a seeded dL/dcolour.

    python tests/golden/gen_clamp_edge_goldens.py

Generated with the oracle from before it recorded and took over frustum-clamp decisions: test_oracle_cpu.py pins that without
``decisions_of`` every output of both builds is still bit-identical.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from util import clamp_edge_camera, clamp_edge_scene  # noqa: E402
from oracle import TiledOracle  # noqa: E402

def loss_image(cam):
    return np.random.default_rng(5).uniform(-1, 1, (3, cam.image_height, cam.image_width)).astype(np.float32)


GRADS = ("means3D", "means2D", "colors_precomp", "opacities", "scales", "rotations")


def main():
    cam = clamp_edge_camera()
    g, edge = clamp_edge_scene(cam, seed=0)
    dL = loss_image(cam)
    out = {f"in_{k}": v for k, v in g.items()}
    out["edge"] = edge
    for tag, f64 in (("f32", False), ("f64", True)):
        o = TiledOracle(cam, g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"],
                        rotations=g["rotations"], nthreads=4, f64=f64)
        out[f"{tag}/radii"] = o.radii
        if not f64:
            out[f"{tag}/color"] = o.color
            out[f"{tag}/depth"] = o.depth
        gr = o.backward(dL)
        for k in GRADS:
            out[f"{tag}/grad_{k}"] = gr[k]
    np.savez_compressed(os.path.join(HERE, "clamp_edge_oracle.npz"), **out)


if __name__ == "__main__":
    main()
