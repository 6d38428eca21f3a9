"""In-place tree edit timings: per phase (HIP events: keys, sort, plan, status read-back, fill + link) and
wall time of Render.edit_nodes on the depth-12 height field of tools/build_probe.py, for 1 000 and 1 000 000 edit voxels
(half of them on surface voxels that exist: recoloured or, with colour 0, removed; half one cell above the surface: new
paths), next to the wall time of Render.build_nodes over the merged voxel list -- same process, same build, medians of
--reps warm calls.  The base is rebuilt before every edit, outside the timed region.

    python tools/edit_probe.py [--out profiles/edit_probe.log] [--reps 5]
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

PHASES = ("keys", "sort", "plan", "readback", "fill+link")
DEPTH = 12


def edit_list(rng, coords, n):
    pick = coords[rng.choice(coords.shape[0], n, replace=False)].copy()
    pick[n // 2:, 1] += 1  # one cell above the surface
    colours = rng.integers(1, 1 << 24, n)
    colours[: n // 2: 2] = 0  # every other touched surface voxel is removed
    return pick, colours


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_probe.log"))
    ap.add_argument("--reps", type=int, default=5)
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

    coords, colours = height_field(1, DEPTH, 3200)
    base_c = torch.from_numpy(coords).to(dev, torch.int32)
    base_col = torch.from_numpy(colours).to(dev, torch.int32)
    rng = np.random.default_rng(16)
    log(f"# in-place edit of the depth-{DEPTH} height field ({coords.shape[0]} voxels): HIP events and wall, median of {args.reps} "
        "warm calls, ms; inputs already on the device (torch int32)")
    log(f"{'edit voxels':>11s} {'words':>10s} {'new words':>10s} " + " ".join(f"{p:>9s}" for p in PHASES) +
        f" {'device':>8s} {'wall':>8s} {'rebuild wall':>12s}")
    for n in (1_000, 1_000_000):
        ec, ecol = edit_list(rng, coords, n)
        c = torch.from_numpy(ec).to(dev, torch.int32)
        col = torch.from_numpy(ecol).to(dev, torch.int32)
        merged_c, merged_col = torch.cat([base_c, c]), torch.cat([base_col, col])
        torch.cuda.synchronize()
        times, walls, rebuild = [], [], []
        for rep in range(args.reps + 1):  # (the first is the warm-up: workspace, code objects)
            n_base = render.build_nodes(base_c, DEPTH, base_col)
            t0 = time.perf_counter()
            n_new = render.edit_nodes(c, DEPTH, col)
            wall = (time.perf_counter() - t0) * 1e3  # includes the gpu.sync() behind the link
            if rep:
                walls.append(wall)
                times.append(gpu.edit_timing())
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            render.build_nodes(merged_c, DEPTH, merged_col)
            if rep:
                rebuild.append((time.perf_counter() - t0) * 1e3)
        ms = np.median(np.array(times), axis=0)
        log(f"{n:11d} {n_base:10d} {n_new - n_base:10d} " + " ".join(f"{t:9.3f}" for t in ms[:5]) +
            f" {float(ms[:5].sum()):8.3f} {float(np.median(walls)):8.3f} {float(np.median(rebuild)):12.3f}")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
