"""Mesh voxelisation timings at depth 12 on two icospheres: 5.2 M triangles smaller than a cell (the cheap
path: a triangle whose bounding box lies in one cell takes a shift and a compare per level) and 320 triangles a few hundred
cells long (the full 13-axis test and many pairs per triangle).  Per case: the phases of the fill (HIP events,
svo_voxelize_timing) in ms and in entries per second, the wall time of mesh.voxelize (count query and fill), medians of
--reps warm calls; next to the build_nodes time of the result.  Checks that the tree built from the list lists
(list_voxels) as many voxels as the list has distinct cells.  Asserts no time.

    python tools/voxelize_probe.py [--out profiles/voxelize_probe.log] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

DEPTH = 12
EMPTY = (1 << 27) << 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_probe.log"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    render = pkg.Render(gpu, (64, 64), np.full(8, EMPTY, dtype=np.uint32), capacity=1 << 27)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    log(f"# meshes voxelised at depth {DEPTH}: the phases of the fill (HIP events) and the wall time of mesh.voxelize (count query and "
        f"fill, with their syncs), median of {args.reps} warm calls, ms; Mentries/s over the fill's device time")
    log(f"{'case':>28s} {'triangles':>10s} {'entries':>10s} {'setup':>8s} {'levels':>8s} {'last':>8s} {'emit':>8s} {'device':>8s} "
        f"{'Mentr/s':>8s} {'wall':>8s} {'build':>8s} {'cells':>10s}")
    for name, subdivisions, radius in (("sub-voxel triangles", 9, 0.15), ("large triangles", 2, 0.5)):
        vertices, triangles = pkg.mesh.icosphere(subdivisions, radius, (0.01, -0.02, 0.03))
        edge = float(np.linalg.norm(vertices[triangles[:, 0]] - vertices[triangles[:, 1]], axis=1).mean()) * (1 << (DEPTH - 1))
        vq = torch.from_numpy(pkg.mesh.quantize_vertices(vertices, DEPTH)).to(dev, torch.int32)
        tris = torch.from_numpy(triangles).to(dev)
        colours = torch.arange(1, len(triangles) + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        phases, wall = [], []
        for rep in range(args.reps + 1):  # (the first is the warm-up: it allocates the workspace)
            t0 = time.perf_counter()
            coords, cell_colours = pkg.mesh.voxelize(gpu, vq, tris, DEPTH, colours, quantized=True)
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                wall.append(w)
                phases.append(gpu.voxelize_timing()[:4])
        setup, levels, last, emit = (float(x) for x in np.median(np.array(phases), axis=0))
        device = setup + levels + last + emit
        n = coords.shape[0]
        n_words = render.build_nodes(coords, DEPTH, cell_colours)
        build = float(sum(gpu.build_timing()[:5]))
        c = coords.to(torch.int64)
        cells = int(torch.unique(c[:, 0] << 42 | c[:, 1] << 21 | c[:, 2]).numel())
        del c
        listed = render.list_voxels(DEPTH)[1].shape[0]
        ok &= listed == cells
        log(f"{name:>28s} {len(triangles):10d} {n:10d} {setup:8.3f} {levels:8.3f} {last:8.3f} {emit:8.3f} {device:8.3f} "
            f"{n / device / 1e3:8.1f} {float(np.median(wall)):8.3f} {build:8.3f} {cells:10d}")
        log(f"#   {name}: mean edge {edge:.2f} cells; the tree has {n_words} words and lists {listed} voxels, the list has {cells} "
            f"distinct cells")
        del coords, cell_colours, vq, tris, colours
    log(f"# the trees list as many voxels as the lists have distinct cells: {bool(ok)}")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("the counts differ")


if __name__ == "__main__":
    main()
