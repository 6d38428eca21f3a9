"""Surface extraction timings: per phase (HIP events: discover, count, offsets, mask, the compaction's count,
emit) of the fill of svo_nodes_list_surface, next to the composition of existing calls that it replaces -- list_voxels, six
offset lists, six sample_voxels, a torch mask and nonzero -- whose device time is the listing's and the samplers' own HIP
events plus torch events around the torch work.  Two scenes built on the device: an icosphere(4) voxelised at depth 10, a
thin shell where nearly every voxel shows a face, and a filled ball of radius 100 in a 256^3 dense grid at depth 8, which
is mostly hidden.  Both ways run alternated in one process; medians of --reps rounds after a warm-up round.  Checks that
both give the same voxels and masks.  Asserts no time.

    python tools/surface_probe.py [--out profiles/surface_probe.log] [--reps 7]
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

PHASES = ("discover", "count", "offsets", "mask", "scan", "emit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_probe.log"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    render = pkg.Render(gpu, (64, 64), np.full(8, B.EMPTY, dtype=np.uint32), capacity=1 << 26)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def shell():
        v, t = pkg.mesh.icosphere(4)
        coords, colours = pkg.mesh.voxelize(gpu, v, t, 10)
        render.build_nodes(coords, 10, colours)
        return 10

    def ball():
        r = torch.arange(256, device=dev, dtype=torch.float32) - 127.5
        inside = r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2 <= 100.0 ** 2
        render.build_nodes_dense(torch.where(inside, 0x80C0FF, 0).to(torch.int32))
        return 8

    steps = torch.tensor([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=torch.int32, device=dev)

    def new_way(depth):
        t0 = time.perf_counter()
        coords, colours, masks = render.list_surface(depth)
        wall = (time.perf_counter() - t0) * 1e3
        return (coords, masks), np.array(gpu.surface_timing()[:6]), wall

    def composition(depth):
        """(coords, masks) of the voxels with an exposed face; device ms of the library calls' fills and of the torch work"""
        t0 = time.perf_counter()
        coords, colours, levels = render.list_voxels(depth, with_levels=True)
        device = float(sum(gpu.list_timing()[:4]))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(14)]
        masks = torch.zeros(len(coords), dtype=torch.int32, device=dev)
        side = torch.bitwise_left_shift(torch.ones_like(levels), depth - levels)
        for f in range(6):
            ev[2 * f].record()
            cells = coords + steps[f][None, :] * side[:, None]
            ev[2 * f + 1].record()
            behind = render.sample_voxels(cells, depth)  # (a cell outside the grid: SAMPLE_OUTSIDE)
            device += gpu.sample_timing()[0]
            ev[2 * f].synchronize()
            device += ev[2 * f].elapsed_time(ev[2 * f + 1])
            ev[12].record()
            masks |= ((behind == 0) | (behind >= pkg.render.SAMPLE_FINER)).to(torch.int32) << f
            ev[13].record()
            ev[13].synchronize()
            device += ev[12].elapsed_time(ev[13])
        ev[12].record()
        keep = masks.nonzero().reshape(-1)
        out = coords[keep], masks[keep]
        ev[13].record()
        ev[13].synchronize()
        device += ev[12].elapsed_time(ev[13])
        return out, device, (time.perf_counter() - t0) * 1e3

    log(f"# the voxels with an exposed face and their masks: svo_nodes_list_surface (HIP events of the fill) against list_voxels + 6 offset "
        f"lists + 6 sample_voxels + a torch mask and nonzero (the fills' HIP events + torch events); alternated, median of {args.reps} rounds after a warm-up, ms")
    log(f"{'scene':>16s} {'words':>9s} {'voxels':>9s} {'surface':>9s} " + " ".join(f"{p:>8s}" for p in PHASES) +
        f" {'device':>8s} {'composed':>8s} {'ratio':>6s} {'wall':>8s} {'wall c.':>8s}")
    ok = True
    for name, scene in (("icosphere shell", shell), ("filled ball", ball)):
        depth = scene()
        new, old = [], []
        for rep in range(args.reps + 1):  # (the first round is the warm-up: workspaces, code objects, torch's allocator)
            a, phases, wall = new_way(depth)
            b, device, wall_c = composition(depth)
            if rep:
                new.append(np.concatenate([phases, [wall]]))
                old.append([device, wall_c])
        same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ok = ok and same
        n_voxels = int(render.list_voxels(depth)[1].shape[0])
        new, old = np.median(np.array(new), axis=0), np.median(np.array(old), axis=0)
        total = float(new[:6].sum())
        log(f"{name:>16s} {render.node_length:9d} {n_voxels:9d} {len(a[0]):9d} " + " ".join(f"{t:8.3f}" for t in new[:6]) +
            f" {total:8.3f} {old[0]:8.3f} {total / old[0]:6.3f} {new[6]:8.3f} {old[1]:8.3f}")
        log(f"# {name}: both ways give the same voxels and masks: {same}")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("the two ways differ")


if __name__ == "__main__":
    main()
