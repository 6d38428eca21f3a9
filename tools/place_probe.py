"""Placement timings: per phase (HIP events: plan with its per-level read-backs, status, fill, write) and wall
time of Render.place_nodes on the scenes and with the source of tools/combine_probe.py: the height field of tools/build_probe.py
at depths 9 and 12, and a merged solid ball of radius 205 cells around the grid's middle, made on a second context by
Render.edit_region and merged by simplify_nodes.
  (a) place_nodes at offset (0, 0, 0) as it is, next to combine_nodes of the same paste and carve: the same words, so the
      difference is what eight items per group record instead of one cost;
  (b) over and carve at offset (1, 1, 1) with a quarter turn about +y, aligned on no level; next to the paste the only route
      without the placement: the source's Render.list_voxels(expand=True), the turn and the offset with torch, Render.edit_nodes.
      A cell list carries no "empty here", so the carve has no such route.
Same process, same build, median (and least .. most of the device total) of --reps warm calls; the scene is rebuilt before
every call, outside the timed region.

    python tools/place_probe.py [--out profiles/place_probe.log] [--reps 5]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_probe.log"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu, other = pkg.Gpu(0), pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    root = np.full(8, B.EMPTY, dtype=np.uint32)
    render = pkg.Render(gpu, (64, 64), root, capacity=1 << 27)
    model = pkg.Render(other, (64, 64), root, capacity=1 << 24)
    turn = pkg.orientation.quarter_turns_y(1)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# a tree placed on a height field: Render.place_nodes (HIP events and wall) next to Render.combine_nodes of the same aligned paste, "
        f"and, moved by (1, 1, 1) and turned a quarter, next to the cell-list route (the source's list_voxels(expand=True), the turn and the "
        f"offset, Render.edit_nodes); median of {args.reps} warm calls, ms; device = the four phases, with the least and the most of the calls")
    log(f"{'depth':>5s} {'call':>34s} {'scene':>9s} {'source':>8s} | {'new words':>9s} " + " ".join(f"{p:>7s}" for p in PHASES) +
        f" {'device':>8s} {'least':>8s} {'most':>8s} {'wall':>8s} | {'cells':>10s} {'new words':>9s} {'list':>8s} {'edit_nodes':>10s} {'wall':>9s}")
    for depth in (9, 12):
        coords, colours = height_field(1, depth, (1 << depth) * 25 // 32)
        base_c = torch.from_numpy(coords).to(dev, torch.int32)
        base_col = torch.from_numpy(colours).to(dev, torch.int32)
        mid = 1 << (depth - 1)
        model.write_nodes(root)
        model.node_length = 8
        model.edit_region([pkg.region.ball((mid, mid, mid), RADIUS, STONE)], depth)
        n_src = model.simplify_nodes()
        rows = []
        for op in ("over", "carve"):
            rows.append((f"combine_nodes, {op}", op, lambda op=op: render.combine_nodes(model, op, depth), gpu.combine_timing, False))
            rows.append((f"place_nodes, {op}, aligned", op, lambda op=op: render.place_nodes(model, op, depth), gpu.place_timing, False))
        for op in ("over", "carve"):
            rows.append((f"place_nodes, {op}, (1,1,1) turned", op, lambda op=op: render.place_nodes(model, op, depth, offset=(1, 1, 1), orient=turn),
                         gpu.place_timing, op == "over"))
        for name, op, call, timing, with_list in rows:
            times, walls = [], []
            for rep in range(args.reps + 1):  # (the first is the warm-up: workspaces, code objects)
                n_base = render.build_nodes(base_c, depth, base_col)
                t0 = time.perf_counter()
                n_new = call()
                wall = (time.perf_counter() - t0) * 1e3  # includes the gpu.sync() behind the write
                if rep:
                    walls.append(wall)
                    times.append(timing())
            device = np.array(times)[:, :4].sum(axis=1)
            ms = np.median(np.array(times), axis=0)
            line = (f"{depth:5d} {name:>34s} {n_base:9d} {n_src:8d} | {n_new - n_base:9d} " + " ".join(f"{t:7.3f}" for t in ms[:4]) +
                    f" {float(np.median(device)):8.3f} {float(device.min()):8.3f} {float(device.max()):8.3f} {float(np.median(walls)):8.3f} |")
            if with_list:
                listing, put = [], []
                side = 1 << depth
                for rep in range(args.reps + 1):
                    render.build_nodes(base_c, depth, base_col)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    cells, cols = model.list_voxels(depth, expand=True)
                    # the quarter turn about the cube, (x, y, z) -> (z, y, S - 1 - x), then the offset; the cells outside go
                    cells = torch.stack([cells[:, 2], cells[:, 1], side - 1 - cells[:, 0]], dim=1) + 1
                    inside = (cells < side).all(dim=1)
                    cells, cols = cells[inside].contiguous(), cols[inside].contiguous()
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
