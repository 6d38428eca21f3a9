"""Regenerates tests/golden/structures_vox.npz: the reference's two structure models (structures/tree.vox, 10x9x14 with
187 voxels, and structures/crystal.vox, 19x23x30 with 2 739), decoded like the models of blocks_vox.npz -- the SIZE
chunk's three numbers, the XYZI records in file order and the 256 palette words.  Data only; the tests write them back
out with cpu_octree.vox_write and load them through the product.

Run from the repo root:  python tests/golden/make_structure_fixtures.py <the reference's checkout>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("tree", "crystal")


def main(reference):
    models = {}
    for name in NAMES:
        size, xyzi, pal = O.vox_parse(open(os.path.join(reference, "structures", name + ".vox"), "rb").read())
        models[name + "_size"] = np.array(size, dtype=np.uint32)
        models[name + "_xyzi"] = xyzi
        models[name + "_palette"] = pal
    np.savez_compressed(os.path.join(HERE, "structures_vox.npz"), **models)
    print({name: (tuple(models[name + "_size"]), len(models[name + "_xyzi"])) for name in NAMES})


if __name__ == "__main__":
    main(sys.argv[1])
