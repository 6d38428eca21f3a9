"""Sampling timings on tools/build_probe.py's depth-12 height field (10.24 M voxels): the kernel (HIP events,
svo_sample_timing) and the wall time of the call with its sync, medians of --reps warm calls, for 1 000 and 10 000 000
points near the surface in random and in Morton order, for a 256^3 box on the surface and for a 512^3 box that is mostly
empty; next to the ways there were before: read_nodes plus Octree.find_voxel on the host (10 000 cells, scaled to the
point counts and labelled as scaled) and list_voxels of the whole tree.  Checks that the voxels sample to their colours and
that the boxes hold the voxels that lie in them.  Asserts no time.

    python tools/sample_probe.py [--out profiles/sample_probe.log] [--reps 5]
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

DEPTH, SIDE = 12, 3200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_probe.log"))
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

    coords, colours = height_field(1, DEPTH, SIDE)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.int32)  # noqa: E731
    n_words = render.build_nodes(to_dev(coords), DEPTH, to_dev(colours))
    rng = np.random.default_rng(19)
    ok = True

    def timed(f):
        kernel, wall = [], []
        for rep in range(args.reps + 1):  # (the first is the warm-up)
            t0 = time.perf_counter()
            out = f()
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                wall.append(w)
                kernel.append(gpu.sample_timing()[0])
        return out, float(np.median(kernel)), float(np.median(wall))

    log(f"# the depth-{DEPTH} height field ({coords.shape[0]} voxels, {n_words} words) sampled: kernel (HIP events) and wall of the "
        f"call with its sync, median of {args.reps} warm calls, ms")
    log(f"{'case':>34s} {'cells':>11s} {'kernel':>9s} {'wall':>9s} {'Gcells/s':>9s}")
    # points: voxels of the surface, half of them moved up or down by up to 2 cells
    for n in (1000, 10_000_000):
        pick = rng.choice(coords.shape[0], n, replace=False)
        cells = coords[pick].copy()
        cells[n // 2:, 1] += rng.integers(-2, 3, n - n // 2)
        for order in ("random", "Morton"):
            if order == "Morton":
                by_key = np.argsort(B.morton(cells, DEPTH), kind="stable")
                cells, pick = cells[by_key], pick[by_key]
            c = to_dev(cells)
            torch.cuda.synchronize()
            values, kernel, wall = timed(lambda: render.sample_voxels(c, DEPTH))
            log(f"{f'points, {order} order':>34s} {n:11d} {kernel:9.3f} {wall:9.3f} {n / kernel / 1e6:9.2f}")
            same = cells[:, 1] == coords[pick, 1]
            ok &= np.array_equal(values.cpu().numpy()[same], colours[pick][same])
    # boxes: 256^3 with the surface of the patch's middle through it, 512^3 above it with little of the surface inside
    mid = coords[(SIDE // 2) * SIDE + SIDE // 2]
    for name, origin, side in (("dense, 256^3 on the surface", mid - 128, 256), ("dense, 512^3, mostly empty", mid - (256, 64, 256), 512)):
        origin = [int(v) for v in origin]
        grid, kernel, wall = timed(lambda: render.sample_dense(origin, (side,) * 3, DEPTH))
        inside = ((coords >= origin) & (coords < np.array(origin) + side)).all(axis=1)
        full = int(torch.count_nonzero(grid))
        log(f"{name:>34s} {side ** 3:11d} {kernel:9.3f} {wall:9.3f} {side ** 3 / kernel / 1e6:9.2f}   # {full} cells hold a voxel")
        ok &= full == int((inside & (colours != 0)).sum())
        at = coords[inside] - origin
        ok &= np.array_equal(grid.cpu().numpy()[at[:, 0], at[:, 1], at[:, 2]], colours[inside])
    log(f"# the voxels sample to their colours and the boxes hold the voxels that lie in them: {bool(ok)}")

    # the ways there were before
    t0 = time.perf_counter()
    words = render.read_nodes()
    t1 = time.perf_counter()
    octree = pkg.Octree.from_words(words)
    t2 = time.perf_counter()
    probe_at = rng.choice(coords.shape[0], 10_000, replace=False)
    probe = coords[probe_at]
    centres = ((probe + 0.5) * (2.0 / (1 << DEPTH)) - 1.0).tolist()
    t3 = time.perf_counter()
    found = [octree.find_voxel(p, max_depth=DEPTH)[0] for p in centres]
    t4 = time.perf_counter()
    per_cell = (t4 - t3) / len(centres) * 1e3
    log(f"# read_nodes {(t1 - t0) * 1e3:.1f} ms ({words.nbytes / 1e6:.0f} MB), Octree.from_words {(t2 - t1) * 1e3:.1f} ms, Octree.find_voxel "
        f"{per_cell * 1e3:.2f} us per cell over {len(centres)} cells: SCALED, not run, {per_cell * 1e3:.1f} ms for 1 000 points, "
        f"{per_cell * 1e7 / 1e3:.1f} s for 10 000 000 points, {per_cell * 256 ** 3 / 1e3:.1f} s for the 256^3 box")
    ok &= np.array_equal((words[np.array(found)] >> 4).astype(np.int64) - B.VOXEL_OFFSET, colours[probe_at])
    t0 = time.perf_counter()
    listed = render.list_voxels(DEPTH)
    wall = (time.perf_counter() - t0) * 1e3
    log(f"# list_voxels of the whole tree ({listed[1].shape[0]} entries): {float(sum(gpu.list_timing()[:4])):.3f} ms on the device for the fill, "
        f"{wall:.3f} ms wall for count query and fill; finding one cell in it is a search on top")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("the samples differ")


if __name__ == "__main__":
    main()
