"""Simplification timings: words before and after, and per phase (HIP events: discover, check, reduce, emit,
copy back) and wall time of Render.simplify_nodes -- MERGE in place, CUT at levels 6 and 9 out of place -- beside
Render.compact_nodes(prune=True) on the same tree in the same run, which shares the discovery and the emit's shape.  Three
trees of unit leaves: the solid icosphere of tools/solid_probe.py at depth 9; the height field of tools/build_probe.py at
depth 9 with every column filled down to the bottom; the same field at depth 12 with every column filled FILL_12 cells
deep (filled to the bottom it would be 2 * 10^10 unit leaves, which no node buffer holds: its words end at 2^27).  Stone
below one layer of grass.  Medians of --reps warm calls; the tree is written back from a host copy before every in-place
call, outside the timed region.  Checks a million random cells before and after the merge.

    python tools/simplify_probe.py [--out profiles/simplify_probe.log] [--reps 3]
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

PHASES = ("discover", "check", "reduce", "emit", "copy back")
GRASS, STONE = 0x30A040, 0x808080
FILL_12 = 4


def filled_field(torch, dev, depth, layers):
    """the height field's columns filled `layers` cells down from the surface (None: to the bottom), on the device"""
    coords, _ = height_field(1, depth, (1 << depth) * 25 // 32)
    top = torch.from_numpy(coords).to(dev, torch.int32)
    deepest = int(coords[:, 1].max()) + 1 if layers is None else layers
    parts, colours = [], []
    for k in range(deepest):
        keep = top[:, 1] >= k
        c = top[keep].clone()
        c[:, 1] -= k
        parts.append(c)
        colours.append(torch.full((c.shape[0],), GRASS if k == 0 else STONE, dtype=torch.int32, device=dev))
    return torch.cat(parts), torch.cat(colours)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_probe.log"))
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

    def ball():
        v, t = pkg.mesh.icosphere(6, 0.8, (0.01, -0.02, 0.03))
        return render.build_nodes_mesh(v, t, 9, colour=GRASS, solid=True, fill_colour=STONE)

    def field(depth, layers):
        coords, colours = filled_field(torch, dev, depth, layers)
        n = render.build_nodes(coords, depth, colours)
        del coords, colours
        return n

    scenes = (("solid icosphere(6), depth 9", 9, ball), ("height field filled to the bottom, depth 9", 9, lambda: field(9, None)),
              (f"height field filled {FILL_12} deep, depth 12", 12, lambda: field(12, FILL_12)))
    log(f"# Render.simplify_nodes beside Render.compact_nodes(prune=True) on the same trees: HIP events and wall, median of {args.reps} "
        f"warm calls, ms; words in -> words out")
    ok = True
    for name, depth, make in scenes:
        n_in = make()
        host = render.read_nodes()
        cells = torch.randint(0, 1 << depth, (1_000_000, 3), dtype=torch.int32, device=dev)
        before = render.sample_voxels(cells, depth)
        log(f"## {name}: {n_in} words ({n_in * 4 / 1e6:.1f} MB)")
        log(f"{'call':>28s} {'words out':>10s} " + " ".join(f"{p:>9s}" for p in PHASES) + f" {'device':>8s} {'wall':>8s}")
        calls = (("compact_nodes(prune=True)", lambda: render.compact_nodes(prune=True), gpu.compact_timing, True),
                 ("MERGE in place", lambda: render.simplify_nodes(), gpu.simplify_timing, True),
                 ("CUT at 6, out of place", lambda: render.simplify_nodes(merge=False, cut_level=6, out_of_place=True)[1], gpu.simplify_timing, False),
                 ("CUT at 9, out of place", lambda: render.simplify_nodes(merge=False, cut_level=9, out_of_place=True)[1], gpu.simplify_timing, False),
                 ("MERGE, out of place", lambda: render.simplify_nodes(out_of_place=True)[1], gpu.simplify_timing, False))
        for what, call, timing, writes in calls:
            times, walls = [], []
            for rep in range(args.reps + 1):  # (the first is the warm-up: workspace, code objects)
                if writes and rep:
                    render.write_nodes(host)
                    render.node_length = n_in
                t0 = time.perf_counter()
                n_out = call()
                wall = (time.perf_counter() - t0) * 1e3  # includes the gpu.sync() behind the call
                if rep:
                    walls.append(wall)
                    times.append(timing())
            ms = np.median(np.array(times), axis=0)
            log(f"{what:>28s} {n_out:10d} " + " ".join(f"{t:9.3f}" for t in ms[:5]) + f" {float(ms[:5].sum()):8.3f} {float(np.median(walls)):8.3f}")
            if what == "MERGE in place":
                same = bool((render.sample_voxels(cells, depth) == before).all().item())
                ok &= same
                log(f"# a million random cells sample alike before and after the merge: {same}")
            if writes:
                render.write_nodes(host)
                render.node_length = n_in
        del host, cells, before
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("cells changed under the merge")


if __name__ == "__main__":
    main()
