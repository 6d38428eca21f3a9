"""Compaction timings: per phase (HIP events: discover, check, prune, emit, copy back) and wall time of
Render.compact_nodes on the depth-12 height field of tools/build_probe.py after tools/edit_probe.py's 1 000 000-voxel edit
(every second edited surface voxel removed), with and without pruning, next to the two ways there were before: read_nodes
+ scenes.relayout(words, 32) + write_nodes, and build_nodes over the merged voxel list -- same process, same build,
medians of --reps warm calls.  The edited tree is made again before every compaction, outside the timed region.  Checks
that the pruned words equal that rebuild and the unpruned ones the host's relayout.

    python tools/compact_probe.py [--out profiles/compact_probe.log] [--reps 5]
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
from edit_probe import DEPTH, edit_list  # noqa: E402

PHASES = ("discover", "check", "prune", "emit", "copy back")


def surviving(coords, colours, ec, ecol):
    """the cells that hold a colour after the edit: the last voxel of a cell wins, colour 0 removes"""
    c = np.concatenate([coords, ec]).astype(np.int64)
    col = np.concatenate([colours, ecol]).astype(np.int64) & 0xFFFFFF
    key = (c[:, 0] << 2 * DEPTH | c[:, 1] << DEPTH | c[:, 2])[::-1]
    _, first = np.unique(key, return_index=True)
    last = c.shape[0] - 1 - first
    last = last[col[last] != 0]
    return c[last], col[last]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_probe.log"))
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
    ec, ecol = edit_list(np.random.default_rng(16), coords, 1_000_000)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.int32)  # noqa: E731
    base_c, base_col, c, col = to_dev(coords), to_dev(colours), to_dev(ec), to_dev(ecol)
    left_c, left_col = (to_dev(a) for a in surviving(coords, colours, ec, ecol))
    torch.cuda.synchronize()

    def edited():
        render.build_nodes(base_c, DEPTH, base_col)
        return render.edit_nodes(c, DEPTH, col)

    log(f"# compaction of the depth-{DEPTH} height field ({coords.shape[0]} voxels) after a {ec.shape[0]}-voxel edit "
        f"({int((ecol == 0).sum())} removed): HIP events and wall, median of {args.reps} warm calls, ms")
    log(f"{'prune':>5s} {'words':>10s} {'words out':>10s} " + " ".join(f"{p:>9s}" for p in PHASES) + f" {'device':>8s} {'wall':>8s}")
    result = {}
    for prune in (False, True):
        times, walls = [], []
        for rep in range(args.reps + 1):  # (the first is the warm-up: workspace, code objects)
            n_in = edited()
            t0 = time.perf_counter()
            n_out = render.compact_nodes(prune=prune)
            wall = (time.perf_counter() - t0) * 1e3  # includes the gpu.sync() behind the copy
            if rep:
                walls.append(wall)
                times.append(gpu.compact_timing())
        result[prune] = render.read_nodes()
        ms = np.median(np.array(times), axis=0)
        log(f"{str(prune):>5s} {n_in:10d} {n_out:10d} " + " ".join(f"{t:9.3f}" for t in ms[:5]) +
            f" {float(ms[:5].sum()):8.3f} {float(np.median(walls)):8.3f}")

    host, rebuild = [], []
    for rep in range(args.reps + 1):
        edited()
        parts = [time.perf_counter()]
        words = render.read_nodes()
        parts.append(time.perf_counter())
        relaid = pkg.scenes.relayout(words, 32)
        parts.append(time.perf_counter())
        render.write_nodes(relaid)
        parts.append(time.perf_counter())
        if rep:
            host.append(np.diff(parts) * 1e3)
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        n_built = render.build_nodes(left_c, DEPTH, left_col)
        if rep:
            rebuild.append((time.perf_counter() - t0) * 1e3)
    built = render.read_nodes()
    h = np.median(np.array(host), axis=0)
    log(f"# read_nodes + scenes.relayout(words, 32) + write_nodes (no pruning): {h[0]:.3f} + {h[1]:.3f} + {h[2]:.3f} = {h.sum():.3f} ms")
    log(f"# build_nodes over the {left_c.shape[0]} surviving voxels: {float(np.median(rebuild)):.3f} ms wall, {n_built} words "
        "(the list is already merged and on the device: finding the surviving voxels, which a caller would also pay, is not in that time)")
    log(f"# compacted without pruning == the host's relayout: {np.array_equal(result[False], relaid)}")
    log(f"# compacted with pruning == that rebuild: {np.array_equal(result[True], built)}")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not (np.array_equal(result[False], relaid) and np.array_equal(result[True], built)):
        sys.exit("the compacted words differ from the alternatives'")


if __name__ == "__main__":
    main()
