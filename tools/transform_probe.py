"""Affine placement timings: per phase (HIP events: plan with its per-level read-backs, status, fill, write) and
wall time of Render.transform_nodes on the scenes and with the source of tools/place_probe.py: the height field of
tools/build_probe.py at depths 9 and 12, and a merged solid ball of radius 205 cells around the grid's middle, made on a second
context by Render.edit_region and merged by simplify_nodes.
  (a) over and carve of the ball turned by 30 degrees about y about the grid's middle;
  (b) the same two under a signed permutation, offset (1, 1, 1) with a quarter turn about +y, next to place_nodes of the same
      placement: the same words, so the ratio is what deciding by geometry costs over inherited items;
  (c) next to (a)'s paste the only route without the pass: the scene cells of the target's bounding box enumerated with torch,
      transform.source_cell, the source's Render.sample_voxels, Render.edit_nodes of the non-empty results.  It gives the same
      cells.  A cell list carries no "empty here", so the other ops have no such route.
Same process, same build, median (and least .. most of the device total) of --reps warm calls; the scene is rebuilt before
every call, outside the timed region.

    python tools/transform_probe.py [--out profiles/transform_probe.log] [--reps 7]
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
SLAB = 16  # x-layers of the bounding box per step of the cell route: bounds its memory


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_probe.log"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu, other = pkg.Gpu(0), pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    root = np.full(8, B.EMPTY, dtype=np.uint32)
    render = pkg.Render(gpu, (64, 64), root, capacity=1 << 27)
    model = pkg.Render(other, (64, 64), root, capacity=1 << 24)
    quarter = pkg.orientation.quarter_turns_y(1)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# a tree placed under an affine map on a height field: Render.transform_nodes (HIP events and wall) of a merged ball turned by 30 "
        f"degrees about y; under a signed permutation next to Render.place_nodes of the same placement; and next to the cell route "
        f"(the bounding box's cells, transform.source_cell, the source's sample_voxels, Render.edit_nodes); median of {args.reps} warm calls, "
        f"ms; device = the four phases, with the least and the most of the calls")
    log(f"{'depth':>5s} {'call':>38s} {'scene':>9s} {'source':>8s} | {'new words':>9s} " + " ".join(f"{p:>7s}" for p in PHASES) +
        f" {'device':>8s} {'least':>8s} {'most':>8s} {'wall':>8s} | {'cells':>10s} {'new words':>9s} {'sample':>8s} {'edit_nodes':>10s} {'wall':>9s}")
    for depth in (9, 12):
        coords, colours = height_field(1, depth, (1 << depth) * 25 // 32)
        base_c = torch.from_numpy(coords).to(dev, torch.int32)
        base_col = torch.from_numpy(colours).to(dev, torch.int32)
        mid = 1 << (depth - 1)
        model.write_nodes(root)
        model.node_length = 8
        model.edit_region([pkg.region.ball((mid, mid, mid), RADIUS, STONE)], depth)
        n_src = model.simplify_nodes()
        turn = pkg.transform.fixed(pkg.transform.rotation("y", 30), (mid,) * 3, (mid,) * 3)
        moved = pkg.transform.from_orientation(quarter, (1, 1, 1), depth)
        rows = []
        for op in ("over", "carve"):
            rows.append((f"transform_nodes, {op}, turn y 30", lambda op=op: render.transform_nodes(model, op, depth, *turn), gpu.transform_timing, op == "over"))
        for op in ("over", "carve"):
            rows.append((f"place_nodes, {op}, (1,1,1) turned", lambda op=op: render.place_nodes(model, op, depth, offset=(1, 1, 1), orient=quarter),
                         gpu.place_timing, False))
            rows.append((f"transform_nodes, {op}, the same", lambda op=op: render.transform_nodes(model, op, depth, *moved), gpu.transform_timing, False))
        medians = {}
        for name, call, timing, with_cells in rows:
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
            medians[name] = float(np.median(device))
            line = (f"{depth:5d} {name:>38s} {n_base:9d} {n_src:8d} | {n_new - n_base:9d} " + " ".join(f"{t:7.3f}" for t in ms[:4]) +
                    f" {float(np.median(device)):8.3f} {float(device.min()):8.3f} {float(device.max()):8.3f} {float(np.median(walls)):8.3f} |")
            if with_cells:
                sampling, put = [], []
                lo, hi = mid - RADIUS - 1, mid + RADIUS + 1  # the turned ball's bounding box, a cell to spare
                side = torch.arange(lo, hi, device=dev, dtype=torch.int32)
                for rep in range(args.reps + 1):
                    render.build_nodes(base_c, depth, base_col)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    found_c, found_v = [], []
                    for x0 in range(lo, hi, SLAB):
                        xs = torch.arange(x0, min(x0 + SLAB, hi), device=dev, dtype=torch.int32)
                        cells = torch.stack(torch.meshgrid(xs, side, side, indexing="ij"), -1).reshape(-1, 3)
                        q = pkg.transform.source_cell(*turn, cells)
                        values = model.sample_voxels(q.to(torch.int32), depth)
                        keep = (values > 0) & (values < pkg.SAMPLE_FINER)  # (a voxel: not empty, not the mark of a q outside the source's cube)
                        found_c.append(cells[keep])
                        found_v.append(values[keep])
                    cells, cols = torch.cat(found_c).contiguous(), torch.cat(found_v).contiguous()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    n_cells = render.edit_nodes(cells, depth, cols)
                    t2 = time.perf_counter()
                    if rep:
                        sampling.append((t1 - t0) * 1e3)
                        put.append((t2 - t1) * 1e3)
                    n_list = cells.shape[0]
                    del cells, cols, found_c, found_v
                line += (f" {n_list:10d} {n_cells - n_base:9d} {float(np.median(sampling)):8.3f} {float(np.median(put)):10.3f} "
                         f"{float(np.median(sampling) + np.median(put)):9.3f}")
            log(line)
        for op in ("over", "carve"):
            log(f"{depth:5d} {op}: transform_nodes / place_nodes of the same placement, device time: "
                f"{medians[f'transform_nodes, {op}, the same'] / medians[f'place_nodes, {op}, (1,1,1) turned']:.2f}")
    other.close()
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
