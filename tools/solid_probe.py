"""Solid voxelisation timings at depth 9 on three closed meshes: an icosphere of 81 920 triangles about a
cell long, a torus, and 320 large triangles closed into a box (two faces of 156 triangles each, eight more on the sides):
few triangles, each over thousands of columns.  Per case: the phases of the fill (HIP events, svo_solid_timing) in ms, the
cells per second over the fill's device time, the wall time of mesh.voxelize_solid (count query and fill), medians of
--reps warm calls; the crossings (counted by the restatement's refinement, tests/solid_ref.py, on the host); and beside
the emit a device-to-device copy of the output's bytes timed in the same run, the yardstick for a pass that only writes.
Checks that spans and cells agree in their totals and that no column is open.  Asserts no time.

    python tools/solid_probe.py [--out profiles/solid_probe.log] [--reps 3]
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
import solid_ref  # noqa: E402

DEPTH = 9


def box_of_320(depth):
    """(vq, triangles): a box over 90 % of the grid; top and bottom are 6 x 13 quads each, the sides two triangles each"""
    top = 1 << (depth + 6)
    lo, hi = top // 20, top - top // 20
    xs, zs = np.linspace(lo, hi, 7).astype(np.int64), np.linspace(lo, hi, 14).astype(np.int64)
    vq, tris = [], []
    for y, flip in ((lo, True), (hi, False)):
        base = len(vq)
        vq += [[x, y, z] for x in xs for z in zs]
        for i in range(6):
            for k in range(13):
                a, b, c, d = base + i * 14 + k, base + (i + 1) * 14 + k, base + (i + 1) * 14 + k + 1, base + i * 14 + k + 1
                quad = [[a, d, c], [a, c, b]]  # normal +y
                tris += [q[::-1] for q in quad] if flip else quad
    corner = {(i, j, k): len(vq) + 4 * i + 2 * j + k for i in (0, 1) for j in (0, 1) for k in (0, 1)}
    vq += [[(lo, hi)[i], (lo, hi)[j], (lo, hi)[k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    for axis in (0, 2):
        for side in (0, 1):
            at = lambda u, y: corner[(side, y, u) if axis == 0 else (u, y, side)]  # noqa: E731
            tris += [[at(0, 0), at(1, 0), at(1, 1)], [at(0, 0), at(1, 1), at(0, 1)]]
    assert len(tris) == 320
    return np.array(vq, dtype=np.int64), np.array(tris, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solid_probe.log"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    meshes = []
    for name, (v, t) in (("icosphere(6)", pkg.mesh.icosphere(6, 0.8, (0.01, -0.02, 0.03))), ("torus(512, 256)", pkg.mesh.torus(512, 256, 0.6, 0.25))):
        meshes.append((name, pkg.mesh.quantize_vertices(v, DEPTH), t.astype(np.int64)))
    meshes.append(("320 large triangles", *box_of_320(DEPTH)))
    ok = True
    log(f"# closed meshes voxelised solid at depth {DEPTH} (even-odd rule, cells): the phases of the fill (HIP events) and the wall time of "
        f"mesh.voxelize_solid (count query and fill, with their syncs), median of {args.reps} warm calls, ms; Mcells/s over the fill's "
        f"device time; copy: a device-to-device copy of the output's bytes, same run")
    log(f"{'case':>20s} {'triangles':>9s} {'crossings':>10s} {'spans':>9s} {'cells':>10s} {'setup':>7s} {'levels':>7s} {'sort':>7s} {'spans':>7s} "
        f"{'emit':>7s} {'copy':>7s} {'device':>8s} {'Mcell/s':>8s} {'wall':>8s}")
    for name, vq_host, tris_host in meshes:
        levels = []
        solid_ref.refine(solid_ref.doubled(vq_host, tris_host), DEPTH, levels=levels)
        vq = torch.from_numpy(vq_host).to(dev, torch.int32)
        tris = torch.from_numpy(tris_host).to(dev, torch.int32)
        torch.cuda.synchronize()
        phases, wall = [], []
        for rep in range(args.reps + 1):  # (the first is the warm-up: it allocates the workspace)
            t0 = time.perf_counter()
            cells, n_open = pkg.mesh.voxelize_solid(gpu, vq, tris, DEPTH, with_open=True, quantized=True)
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                wall.append(w)
                phases.append(gpu.solid_timing()[:5])
        setup, lev, sort, spans_ms, emit = (float(x) for x in np.median(np.array(phases), axis=0))
        device = setup + lev + sort + spans_ms + emit
        copies = []
        for _ in range(args.reps + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            twin = cells.clone()
            stop.record()
            torch.cuda.synchronize()
            copies.append(start.elapsed_time(stop))
            del twin
        spans = pkg.mesh.voxelize_solid(gpu, vq, tris, DEPTH, spans=True, quantized=True)
        total = int((spans[:, 3] - spans[:, 2]).to(torch.int64).sum())
        ok &= total == len(cells) and n_open == 0
        log(f"{name:>20s} {len(tris_host):9d} {levels[-1]:10d} {len(spans):9d} {len(cells):10d} {setup:7.3f} {lev:7.3f} {sort:7.3f} {spans_ms:7.3f} "
            f"{emit:7.3f} {float(np.median(copies[1:])):7.3f} {device:8.3f} {len(cells) / device / 1e3:8.1f} {float(np.median(wall)):8.3f}")
        log(f"#   {name}: pairs per level {levels[:-1]}, then {levels[-1]} crossings; {n_open} open columns")
        del cells, spans, vq, tris
    log(f"# the spans' lengths add up to the cells and no column is open: {bool(ok)}")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("the counts differ")


if __name__ == "__main__":
    main()
