"""Morphology timings: per phase (HIP events: plan with its per-level read-backs, status, fill, write) and wall
time of one grow and one shrink step of Render.morph_nodes per conn, and the wall time of Render.shell_nodes of thickness 1 and
3, on the scenes of tools/combine_probe.py: the height field of tools/build_probe.py at depths 9 and 12 (one voxel per column,
every voxel a cell of the last level) and a merged solid ball of radius 205 cells around the grid's middle, made by
Render.edit_region and merged by simplify_nodes.  Beside each, the route that existed before the pass:
  grow, shrink   a snapshot (simplify_nodes(out_of_place=True)) and one place_nodes of it per offset d of conn at -d, in
                 priority order: "under" for a grow (inherited colours), "keep" for a shrink (closed boundary)
  shell          DESIGN.md 23's hollowing: list_surface, its leaves expanded to cells with torch, build_nodes.  It knows one
                 thickness, 1, and 6 neighbours
Same process, same build, median (and least .. most) of --reps warm calls; the scene is rebuilt before every call, outside the
timed region.  A call that the library refuses (a grown tree over the buffer's 2^27 words) is logged with its message.

    python tools/morph_probe.py [--out profiles/morph_probe.log] [--reps 7]
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
# conn's offsets in the pass's priority order: ascending (|d|_1, dx, dy, dz)
OFFSETS = sorted(((x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)),
                 key=lambda d: (sum(abs(v) for v in d), d))


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return f"{float(np.median(v)):9.3f} {float(v.min()):9.3f} {float(v.max()):9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_probe.log"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="field9,field12,ball9,ball12")
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    root = np.full(8, B.EMPTY, dtype=np.uint32)
    render = pkg.Render(gpu, (64, 64), root, capacity=1 << 27)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def log(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    def timed(rebuild, call):
        """-> (the scene's words, the words added, walls (ms) of the warm calls, what `call` returned in the last) or the refusal"""
        walls, n_base, n_new, last = [], 0, 0, None
        for rep in range(args.reps + 1):  # (the first is the warm-up: workspaces, code objects)
            n_base = rebuild()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                last = call()
            except pkg.SvoError as e:
                return n_base, None, str(e), None
            gpu.sync()
            wall = (time.perf_counter() - t0) * 1e3
            n_new = render.node_length
            if rep:
                walls.append((wall, last))
        return n_base, n_new - n_base, [w for w, _ in walls], [x for _, x in walls]

    log(f"# morphology on a device tree: one step of Render.morph_nodes (HIP events and wall) next to a snapshot and one place_nodes per "
        f"offset of conn, and Render.shell_nodes next to list_surface + build_nodes; median, least and most of {args.reps} warm calls, ms; "
        f"device = the four phases")
    log(f"{'scene':>8s} {'call':>22s} {'words':>9s} | {'new words':>10s} " + " ".join(f"{p:>7s}" for p in PHASES) +
        f" {'device':>9s} {'least':>9s} {'most':>9s} {'wall':>9s} {'least':>9s} {'most':>9s} | {'old route':>24s} {'new words':>10s} {'wall':>9s} {'least':>9s} {'most':>9s}")
    for scene in args.scenes.split(","):
        depth = int(scene.lstrip("fieldba"))
        if scene.startswith("field"):
            coords, colours = height_field(1, depth, (1 << depth) * 25 // 32)
            base_c = torch.from_numpy(coords).to(dev, torch.int32)
            base_col = torch.from_numpy(colours).to(dev, torch.int32)

            def rebuild():
                return render.build_nodes(base_c, depth, base_col)
        else:
            mid = 1 << (depth - 1)

            def rebuild():
                render.write_nodes(root)
                render.node_length = 8
                render.edit_region([pkg.region.ball((mid, mid, mid), RADIUS, STONE)], depth)
                return render.simplify_nodes()

        def places(place_op, conn):
            snapshot = render.simplify_nodes(out_of_place=True)
            for d in OFFSETS:
                if sum(abs(v) for v in d) <= {6: 1, 18: 2, 26: 3}[conn]:
                    render.place_nodes(snapshot, place_op, depth, offset=tuple(-v for v in d))

        def hollow():
            cells, cols, _, levels = render.list_surface(depth, with_levels=True)
            parts_c, parts_v = [], []
            for level in torch.unique(levels).tolist():  # a coarse leaf's cells (few: a surface's leaves are mostly of the last level)
                pick = levels == level
                s = 1 << (depth - level)
                k = torch.arange(s, device=dev, dtype=torch.int32)
                off = torch.stack(torch.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
                parts_c.append((cells[pick][:, None, :] + off[None, :, :]).reshape(-1, 3))
                parts_v.append(cols[pick].repeat_interleave(s ** 3))
            if not parts_c:
                return render.node_length
            return render.build_nodes(torch.cat(parts_c).contiguous(), depth, torch.cat(parts_v).contiguous())

        for op, place_op in (("grow", "under"), ("shrink", "keep")):
            for conn in (6, 18, 26):
                def step():
                    render.morph_nodes(op, 1, conn, depth=depth)
                    return gpu.morph_timing()
                n_base, added, walls, times = timed(rebuild, step)
                line = f"{scene:>8s} {op + ' ' + str(conn):>22s} {n_base:9d} | "
                if added is None:
                    line += f"refused: {walls}"
                else:
                    t = np.array(times)
                    device = t[:, :4].sum(axis=1)
                    line += f"{added:10d} " + " ".join(f"{v:7.3f}" for v in np.median(t, axis=0)[:4]) + f" {spread(device)} {spread(walls)}"
                _, added, walls, _ = timed(rebuild, lambda: places(place_op, conn))
                line += f" | {'snapshot + ' + str(conn) + ' ' + place_op:>24s} "
                line += f"refused: {walls}" if added is None else f"{added:10d} {spread(walls)}"
                log(line)
        for thickness in (1, 3):
            n_base, added, walls, _ = timed(rebuild, lambda: render.shell_nodes(thickness, 6, depth))
            line = f"{scene:>8s} {'shell ' + str(thickness) + ', conn 6':>22s} {n_base:9d} | "
            line += f"refused: {walls}" if added is None else f"{added:10d} " + " " * 68 + f"{spread(walls)}"
            if thickness == 1:
                _, added, walls, _ = timed(rebuild, hollow)
                line += f" | {'list_surface + build':>24s} " + (f"refused: {walls}" if added is None else f"{added:10d} {spread(walls)}")
            log(line)
    out.close()
    gpu.close()


if __name__ == "__main__":
    main()
