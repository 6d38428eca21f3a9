"""Shape edit timings: per phase (HIP events: plan with its per-level read-backs, status, fill, write) and
wall time of Render.edit_region for three edits on the height field of tools/build_probe.py, at depths 9 and 12: a carved
ball, a flooded box (EMPTY mode) and a stroke of 33 balls, every third a fill.  Next to each, the route without shapes:
the same cells enumerated with torch on the device (a flood samples the box first, to find its empty cells) and put with
Render.edit_nodes.  Same process, same build, medians of --reps warm calls; the base is rebuilt before every edit, outside
the timed region.  Sizes are given for depth 12 and scaled by 2^(depth - 12).

    python tools/region_probe.py [--out profiles/region_probe.log] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
import build_ref as B  # noqa: E402
from build_probe import height_field  # noqa: E402

PHASES = ("plan", "status", "fill", "write")
WATER, STONE = 0x2040FF, 0x808080


def edits(pkg, depth):
    """{name: shapes} on the depth grid; the terrain's surface runs through the grid's middle height"""
    G = pkg.region
    s = (1 << depth) / 4096
    mid = 1 << (depth - 1)
    n = lambda v: max(1, int(round(v * s)))  # noqa: E731
    stroke = [G.ball((mid - n(640) + n(40) * i + 0.5, mid + n(8) + 0.5, mid - n(320) + n(20) * i + 0.5), n(40), STONE if i % 3 == 0 else 0)
              for i in range(33)]
    return {
        "carved ball": [G.ball((mid, mid, mid), n(200), 0)],
        "flooded box": [G.box((mid - n(128), mid - n(48), mid - n(128)), (mid + n(128), mid + n(16), mid + n(128)), WATER, G.EMPTY)],
        "33-ball stroke": stroke,
    }


def shape_cells(torch, dev, render, shape, depth):
    """the cells a shape applies to, enumerated on the device: (coords int32 (N, 3), colours int32 (N,))"""
    side = 1 << depth
    if shape.kind == 0:
        lo, hi = shape.a, shape.b
    else:  # the ball's bounding box, clipped: centre and radius are in half cells
        lo = [max(0, (c - shape.b[0]) // 2) for c in shape.a]
        hi = [min(side, (c + shape.b[0]) // 2 + 1) for c in shape.a]
    axes = [torch.arange(a, b, device=dev, dtype=torch.int32) for a, b in zip(lo, hi)]
    cells = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    if shape.kind == 1:
        d = (2 * cells.to(torch.int64) + 1) - torch.tensor(shape.a, device=dev, dtype=torch.int64)
        cells = cells[(d * d).sum(1) <= shape.b[0] * shape.b[0]]
    if shape.mode != 3:  # the cells' state decides: ask the tree
        held = render.sample_voxels(cells, depth)
        cells = cells[(held == 0) if shape.mode == 1 else (held != 0)]
    return cells, torch.full((cells.shape[0],), shape.colour, device=dev, dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_probe.log"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    render = pkg.Render(gpu, (64, 64), np.full(8, B.EMPTY, dtype=np.uint32), capacity=1 << 27)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# shape edits of a height field: Render.edit_region (HIP events and wall) beside the cell-list route (torch enumeration, then "
        f"Render.edit_nodes); median of {args.reps} warm calls, ms")
    log(f"{'depth':>5s} {'edit':>15s} {'words':>9s} | {'new words':>9s} " + " ".join(f"{p:>7s}" for p in PHASES) +
        f" {'device':>8s} {'wall':>8s} | {'cells':>10s} {'new words':>9s} {'enumerate':>9s} {'edit_nodes':>10s} {'wall':>9s}")
    for depth in (9, 12):
        coords, colours = height_field(1, depth, (1 << depth) * 25 // 32)
        base_c = torch.from_numpy(coords).to(dev, torch.int32)
        base_col = torch.from_numpy(colours).to(dev, torch.int32)
        for name, shapes in edits(pkg, depth).items():
            times, walls, enum, put = [], [], [], []
            for rep in range(args.reps + 1):  # (the first is the warm-up: workspaces, code objects)
                n_base = render.build_nodes(base_c, depth, base_col)
                t0 = time.perf_counter()
                n_region = render.edit_region(shapes, depth)
                wall = (time.perf_counter() - t0) * 1e3  # includes the gpu.sync() behind the write
                if rep:
                    walls.append(wall)
                    times.append(gpu.region_timing())
            for rep in range(args.reps + 1):
                render.build_nodes(base_c, depth, base_col)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lists = [shape_cells(torch, dev, render, s, depth) for s in shapes]
                cells, cols = torch.cat([c for c, _ in lists]), torch.cat([c for _, c in lists])
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                n_cells = render.edit_nodes(cells, depth, cols)
                t2 = time.perf_counter()
                if rep:
                    enum.append((t1 - t0) * 1e3)
                    put.append((t2 - t1) * 1e3)
                n_list = cells.shape[0]
                del lists, cells, cols
            ms = np.median(np.array(times), axis=0)
            log(f"{depth:5d} {name:>15s} {n_base:9d} | {n_region - n_base:9d} " + " ".join(f"{t:7.3f}" for t in ms[:4]) +
                f" {float(ms[:4].sum()):8.3f} {float(np.median(walls)):8.3f} | {n_list:10d} {n_cells - n_base:9d} "
                f"{float(np.median(enum)):9.3f} {float(np.median(put)):10.3f} {float(np.median(enum) + np.median(put)):9.3f}")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
