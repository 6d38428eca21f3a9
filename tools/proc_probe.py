"""Procedural generator timings: kernel time per phase of the reference's 512^3 chunks (base_depth 1,
chunk_depth 9; HIP events around the classify, pyramid-and-ranks and emit launches), and the wall time of a full
World.generate_world(world_depth=1, chunk_depth=9) split into GPU, read-back, mips and chunk file writes.

    python tools/proc_probe.py [--out profiles/proc_probe.log] [--scratch DIR] [--reps 3]

The world (about a gigabyte of .bin files) is written to a fresh directory under --scratch and removed afterwards."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

BLOCKS = ("stone", "dirt", "grass", "wood", "leaf", "slate", "crystal", "glass")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proc_probe.log"))
    ap.add_argument("--scratch", default=tempfile.gettempdir())
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-depth", type=int, default=9)
    args = ap.parse_args()
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    proc = pkg.Procedural(gpu)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    cd = args.chunk_depth
    layout = pkg.procedural.chunk_layout(1)
    proc.generate_chunk(layout[0][2], 1, cd)  # warm-up: code objects, workspace, pinned staging
    log(f"# per chunk (base_depth 1, chunk_depth {cd}: {1 << cd}^3 cells), median of {args.reps} runs, ms")
    log("chunk pos             nodes      classify  pyr+ranks  emit    gpu_wall  copy    build")
    total = {}
    for _, cid, pos in layout:
        runs, n = [], 0
        for _ in range(args.reps):
            c = proc.generate_chunk(pos, 1, cd)
            n = len(c) if c is not None else 0
            runs.append(proc.timing())
            del c
        med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        for k, v in med.items():
            total[k] = total.get(k, 0.0) + v
        log(f"{str(tuple(pos)):20s} {n:10d}  {med['classify']:8.3f}  {med['pyramid_and_ranks']:8.3f}  {med['emit']:6.3f}  "
            f"{med['chunk_gpu_wall']:8.3f}  {med['chunk_copy']:6.2f}  {med['chunk_build']:6.2f}")
    log(f"{'sum of 8 chunks':31s}  {total['classify']:8.3f}  {total['pyramid_and_ranks']:8.3f}  {total['emit']:6.3f}  "
        f"{total['chunk_gpu_wall']:8.3f}  {total['chunk_copy']:6.2f}  {total['chunk_build']:6.2f}")

    scratch = tempfile.mkdtemp(prefix="proc_probe_", dir=args.scratch)
    try:
        z = np.load(os.path.join(ROOT, "tests", "golden", "blocks_vox.npz"))
        bdir = os.path.join(scratch, "blocks")
        os.makedirs(bdir)
        for name in BLOCKS:
            with open(os.path.join(bdir, name + ".vox"), "wb") as f:
                f.write(pkg.cpu_octree.vox_write(16, z[name + "_xyzi"], z[name + "_palette"]))
        path = os.path.join(scratch, "world")
        t0 = time.perf_counter()
        pkg.World.generate_world(path, proc, world_depth=1, chunk_depth=cd, blocks_dir=bdir)
        wall = (time.perf_counter() - t0) * 1e3
        t = proc.timing()
        size = sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))
        rest = wall - t["world_gpu"] - t["world_copy_and_build"] - t["world_mips"] - t["world_writes"]
        log(f"# generate_world(world_depth=1, chunk_depth={cd}): {len(os.listdir(path))} files, {size / 1e6:.1f} MB")
        log(f"wall {wall:.1f} ms = gpu {t['world_gpu']:.1f} + read-back {t['world_copy_and_build']:.1f} + "
            f"device mips {t['world_mips']:.1f} + file writes {t['world_writes']:.1f} + other {rest:.1f}")
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    gpu.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
