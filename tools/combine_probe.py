"""Combine timings: per phase (HIP events: plan with its per-level read-backs, status, fill, write) and wall
time of Render.combine_nodes on the height field of tools/build_probe.py, at depths 9 and 12, with a merged solid ball as the
source: pasted (over), carved out of the terrain (carve), the terrain masked by it (keep), and a model one eighth of the
side placed in the cell (4, 4, 4) of level 3.  The ball has a radius of 205 cells around the grid's middle, at depth 9 the 36 M
cells of the merged solid ball of DESIGN.md 26; the model is the same ball at 0.4 of its own side.  Both are made on a second
context by Render.edit_region and merged by simplify_nodes.  Beside each paste, the route without the combine: the source's
Render.list_voxels(expand=True), the offset added with torch, Render.edit_nodes.  Same process, same build, medians of --reps
warm calls; the scene is rebuilt before every call, outside the timed region.

    python tools/combine_probe.py [--out profiles/combine_probe.log] [--reps 3]
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
STONE = 0x808080
RADIUS = 205


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_probe.log"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu, other = pkg.Gpu(0), pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    root = np.full(8, B.EMPTY, dtype=np.uint32)
    render = pkg.Render(gpu, (64, 64), root, capacity=1 << 27)
    model = pkg.Render(other, (64, 64), root, capacity=1 << 24)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def make_ball(depth, radius):
        """a solid ball around the middle of the depth grid in the model's buffer, merged; returns its words"""
        mid = 1 << (depth - 1)
        model.write_nodes(root)
        model.node_length = 8
        model.edit_region([pkg.region.ball((mid, mid, mid), radius, STONE)], depth)
        return model.simplify_nodes()

    log(f"# two trees combined on a height field: Render.combine_nodes (HIP events and wall) and, beside each paste, the cell-list route "
        f"(the source's list_voxels(expand=True), the offset, Render.edit_nodes); median of {args.reps} warm calls, ms")
    log(f"{'depth':>5s} {'combine':>26s} {'scene':>9s} {'source':>8s} | {'new words':>9s} " + " ".join(f"{p:>7s}" for p in PHASES) +
        f" {'device':>8s} {'wall':>8s} | {'cells':>10s} {'new words':>9s} {'list':>8s} {'edit_nodes':>10s} {'wall':>9s}")
    for depth in (9, 12):
        coords, colours = height_field(1, depth, (1 << depth) * 25 // 32)
        base_c = torch.from_numpy(coords).to(dev, torch.int32)
        base_col = torch.from_numpy(colours).to(dev, torch.int32)
        small = depth - 3
        rows = (("ball pasted (over)", "over", depth, RADIUS, 0, (0, 0, 0)), ("ball carved (carve)", "carve", depth, RADIUS, 0, (0, 0, 0)),
                ("model at level 3 (over)", "over", small, round(0.4 * (1 << small)), 3, (4, 4, 4)), ("masked by the ball (keep)", "keep", depth, RADIUS, 0, (0, 0, 0)))
        for name, op, src_depth, radius, at_level, at in rows:
            n_src = make_ball(src_depth, radius)
            times, walls = [], []
            for rep in range(args.reps + 1):  # (the first is the warm-up: workspaces, code objects)
                n_base = render.build_nodes(base_c, depth, base_col)
                t0 = time.perf_counter()
                n_new = render.combine_nodes(model, op, depth, at=at, at_level=at_level)
                wall = (time.perf_counter() - t0) * 1e3  # includes the gpu.sync() behind the write
                if rep:
                    walls.append(wall)
                    times.append(gpu.combine_timing())
            ms = np.median(np.array(times), axis=0)
            line = (f"{depth:5d} {name:>26s} {n_base:9d} {n_src:8d} | {n_new - n_base:9d} " + " ".join(f"{t:7.3f}" for t in ms[:4]) +
                    f" {float(ms[:4].sum()):8.3f} {float(np.median(walls)):8.3f} |")
            if op == "over":
                listing, put = [], []
                offset = torch.tensor([v << src_depth for v in at], device=dev, dtype=torch.int32)
                for rep in range(args.reps + 1):
                    render.build_nodes(base_c, depth, base_col)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    cells, cols = model.list_voxels(src_depth, expand=True)
                    cells = cells + offset
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    n_cells = render.edit_nodes(cells, depth, cols)
                    t2 = time.perf_counter()
                    if rep:
                        listing.append((t1 - t0) * 1e3)
                        put.append((t2 - t1) * 1e3)
                    n_list = cells.shape[0]
                    del cells, cols
                line += (f" {n_list:10d} {n_cells - n_base:9d} {float(np.median(listing)):8.3f} {float(np.median(put)):10.3f} "
                         f"{float(np.median(listing) + np.median(put)):9.3f}")
            log(line)
    other.close()
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
