"""GPU tree builder timings: per phase (HIP events: keys, sort, levels, count read-back, emit; median of
--reps warm builds) and Mvoxels/s for three inputs, next to the host path for the same voxels -- CpuOctree.from_voxels
-> to_octree_words -> write_nodes where the model fits u8 coordinates, else the numpy restatement (tests/build_ref.py)
-> write_nodes.

    python tools/build_probe.py [--out profiles/build_probe.log] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import build_ref as B  # noqa: E402

PHASES = ("keys", "sort", "levels", "readback", "emit")


def height_field(seed, depth, side):
    """one surface voxel per column of a side x side patch (seeded smooth height), the patch centred in x and z"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.5, 3.0, 3)
    x, z = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    h = (np.sin(x * f[0] / side * 6) + np.cos(z * f[1] / side * 6) + 0.5 * np.sin((x + z) * f[2] / side * 9)) * side / 16
    off = ((1 << depth) - side) // 2
    coords = np.stack([x.ravel() + off, ((1 << depth) // 2 + h).astype(np.int64).ravel(), z.ravel() + off], 1)
    return coords, (coords[:, 1] * 2654435761) & 0xFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_probe.log"))
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

    (_, size, xyzi, pal), = B.fixture_models(os.path.join(ROOT, "tests", "golden"), "phantom_mansion")
    mansion, mansion_col, mansion_depth = B.vox_voxels(size, xyzi, pal)
    cases = [("phantom_mansion", mansion, mansion_col, mansion_depth, (size, xyzi, pal)),
             ("height field d12", *height_field(1, 12, 3200), 12, None),
             ("height field d16", *height_field(2, 16, 4480), 16, None)]
    log(f"# GPU build: HIP events, median of {args.reps} warm builds, ms; inputs already on the device (torch int32)")
    log(f"{'input':18s} {'voxels':>9s} {'depth':>5s} {'words':>10s} " + " ".join(f"{p:>8s}" for p in PHASES) +
        f" {'device':>8s} {'wall':>8s} {'Mvox/s':>8s}")
    host_rows = []
    for name, coords, colours, depth, vox in cases:
        c = torch.from_numpy(coords).to(dev, torch.int32)
        col = torch.from_numpy(colours).to(dev, torch.int32)
        torch.cuda.synchronize()
        n_words = render.build_nodes(c, depth, col)  # warm-up (workspace, code objects)
        times, walls = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            assert render.build_nodes(c, depth, col) == n_words
            walls.append((time.perf_counter() - t0) * 1e3)  # includes the gpu.sync() behind the emit
            times.append(gpu.build_timing())
        ms = np.median(np.array(times), axis=0)
        dev_ms = float(ms[:5].sum())
        wall = float(np.median(walls))
        log(f"{name:18s} {coords.shape[0]:9d} {depth:5d} {n_words:10d} " + " ".join(f"{t:8.3f}" for t in ms[:5]) +
            f" {dev_ms:8.3f} {wall:8.3f} {coords.shape[0] / dev_ms / 1e3:8.1f}")
        got = render.read_nodes(n_words)
        # the host path for the same voxels
        t0 = time.perf_counter()
        if vox is not None:
            words = pkg.CpuOctree.from_voxels(*vox).to_octree_words()
            path = "CpuOctree.from_voxels + to_octree_words"
        else:
            words = B.build(coords, depth, colours)
            path = "numpy restatement (tests/build_ref.py)"
        t1 = time.perf_counter()
        render.write_nodes(words)
        t2 = time.perf_counter()
        same = np.array_equal(got, B.build(coords, depth, colours) if vox is not None else words)
        host_rows.append(f"{name:18s} {path:42s} {(t1 - t0) * 1e3:10.1f} {(t2 - t1) * 1e3:10.1f} {(t2 - t0) * 1e3:10.1f}  "
                         f"GPU words equal numpy: {same}")
    log("")
    log("# host path for the same voxels, ms (one run)")
    log(f"{'input':18s} {'build':42s} {'build ms':>10s} {'write ms':>10s} {'total ms':>10s}")
    for r in host_rows:
        log(r)
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
