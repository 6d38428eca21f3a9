"""Chunk-tree and world builder timings: per phase (HIP events: sort -- keys included --, levels -- count
read-back included --, emit, mips; host wall: chunk read-back, writes; median of --reps warm builds) for three inputs at
world_depth 0 (CpuOctree.build) and 2 (World.build_world), next to the host path where one exists: phantom_mansion via
CpuOctree.from_voxels + generate_mip_tree.

    python tools/world_build_probe.py [--out profiles/world_build_probe.log] [--scratch DIR] [--reps 5]

The worlds are written to fresh directories under --scratch and removed afterwards."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
import build_ref as B  # noqa: E402
from build_probe import height_field  # noqa: E402

PHASES = ("sort", "levels", "emit", "mips", "readback", "writes")


def phases(ms):
    """svo_world_build_timing -> the probe's columns"""
    return [ms[0] + ms[1], ms[2] + ms[3], ms[4], ms[5], ms[6], ms[7]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_build_probe.log"))
    ap.add_argument("--scratch", default=tempfile.gettempdir())
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    (_, size, xyzi, pal), = B.fixture_models(os.path.join(ROOT, "tests", "golden"), "phantom_mansion")
    mansion, mansion_col, mansion_depth = B.vox_voxels(size, xyzi, pal)
    cases = [("phantom_mansion", mansion, mansion_col, mansion_depth),
             ("height field 10M", *height_field(1, 12, 3200), 12),
             ("height field 20M", *height_field(2, 16, 4480), 16)]
    log(f"# chunk builds: device phases from HIP events, read-back and writes host wall; median of {args.reps} warm runs, ms")
    log(f"# sort includes the keys, levels the count read-back; world_depth 0 = CpuOctree.build (writes: the CpuOctree), "
        f"2 = World.build_world (writes: chunk files and 0.bin)")
    log(f"{'input':18s} {'voxels':>9s} {'depth':>5s} {'wd':>2s} {'nodes':>10s} {'files':>5s} " +
        " ".join(f"{p:>8s}" for p in PHASES) + f" {'wall':>8s}")
    scratch = tempfile.mkdtemp(prefix="world_build_probe_", dir=args.scratch)
    try:
        for name, coords, colours, depth in cases:
            c = torch.from_numpy(coords).to(dev, torch.int32)
            col = torch.from_numpy(colours).to(dev, torch.int32)
            torch.cuda.synchronize()
            for wd in (0, 2):
                runs, walls, nodes, files = [], [], 0, 1
                for r in range(args.reps + 1):  # run 0: warm-up (workspace, code objects, pinned stage)
                    t0 = time.perf_counter()
                    if wd == 0:
                        t = pkg.CpuOctree.build(gpu, c, depth, col)
                        nodes = len(t)
                    else:
                        path = os.path.join(scratch, f"w{r}")
                        pkg.World.build_world(path, gpu, c, depth, col, world_depth=wd)
                        files = len(os.listdir(path))
                        nodes = sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path)) // 8
                    walls.append((time.perf_counter() - t0) * 1e3)
                    runs.append(phases(gpu.world_build_timing()))
                    if wd:
                        shutil.rmtree(path)
                ms = np.median(np.array(runs[1:]), axis=0)
                log(f"{name:18s} {coords.shape[0]:9d} {depth:5d} {wd:2d} {nodes:10d} {files:5d} " +
                    " ".join(f"{t:8.2f}" for t in ms) + f" {float(np.median(walls[1:])):8.1f}")
        log("")
        log("# host path: phantom_mansion via CpuOctree.from_voxels + generate_mip_tree, one run, ms")
        t0 = time.perf_counter()
        host = pkg.CpuOctree.from_voxels(size, xyzi, pal)
        t1 = time.perf_counter()
        host.generate_mip_tree()
        t2 = time.perf_counter()
        same = len(host) == len(pkg.CpuOctree.build(gpu, mansion, mansion_depth, mansion_col))
        log(f"from_voxels {(t1 - t0) * 1e3:.1f} + generate_mip_tree {(t2 - t1) * 1e3:.1f} = {(t2 - t0) * 1e3:.1f} "
            f"({len(host)} nodes; same node count as CpuOctree.build: {same})")
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    gpu.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
