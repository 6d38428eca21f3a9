"""Height-map edit timings: per phase (HIP events: pyramid, plan with its per-level read-backs, status, fill,
write) and wall time of Render.edit_heightmap on the height field of tools/build_probe.py at depths 9 and 12 (a patch of 25/32
of the grid's side, centred; the map is that field's surface height per column):
  solid      the terrain made from the empty root group, solid down to y = 0, in three layers (1 grass, 3 dirt, stone)
  bump       a terraform of that terrain: a disc of 256 columns across, raised by a cosine dome of 24 cells, below SET and
             above SET carving, over the disc's 256 x 256 square of columns
  pyramid    the min/max pyramid alone (Render.height_minmax of its top level: every launch runs) beside a device-to-device
             copy of the map, the bandwidth yardstick: both by a host clock around calls that end in a synchronise, and the
             pyramid phase of `solid` by events
  old route  at depth 9, what a solid terrain took before the pass: every cell under the surface enumerated in torch with its
             layer's colour, build_nodes, simplify_nodes().  The ground stands where build_probe puts it, around y = 2^depth / 2:
             about 40 M cells at depth 9, whose tree stays under the buffer's 2^27 words.  Both routes' trees are simplified
             and compared byte for byte.  At depth 12 the same terrain is about 2 * 10^10 cells, a word each before the merge:
             the route cannot run, and the log says what it would need
Same process, same build, median (and least .. most) of --reps warm calls; the scene is rebuilt before every call, outside the
timed region.

    python tools/heightmap_probe.py [--out profiles/heightmap_probe.log] [--reps 7] [--depths 9,12]
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

PHASES = ("pyramid", "plan", "status", "fill", "write")
LAYERS = ((1, 0x3A9D23), (3, 0x8B5A2B), (0, 0x808080))
DISC, DOME = 256, 24


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return f"{float(np.median(v)):9.3f} {float(v.min()):9.3f} {float(v.max()):9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heightmap_probe.log"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--depths", default="9,12")
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

    def empty():
        render.write_nodes(root)
        render.node_length = 8
        return 8

    def timed(rebuild, call):
        """-> (the scene's words, the words added, walls (ms) of the warm calls, what `call` returned in them) or the refusal"""
        walls, n_base, n_new = [], 0, 0
        for rep in range(args.reps + 1):  # (the first is the warm-up: workspaces, code objects)
            n_base = rebuild()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                last = call()
            except pkg.SvoError as e:
                return n_base, None, str(e), None
            gpu.sync()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            n_new = render.node_length
            if rep:
                walls.append((wall, last))
        return n_base, n_new - n_base, [w for w, _ in walls], [x for _, x in walls]

    def edit_line(scene, name, n_base, added, walls, times):
        line = f"{scene:>8s} {name:>10s} {n_base:10d} | "
        if added is None:
            return line + f"refused: {walls}"
        t = np.array(times)
        return line + f"{added:10d} " + " ".join(f"{v:8.3f}" for v in np.median(t, axis=0)[:5]) + f" {spread(t[:, :5].sum(axis=1))} {spread(walls)}"

    log(f"# a device tree shaped by a height map: Render.edit_heightmap (HIP events and wall), its pyramid beside a copy of the map, and "
        f"the cell-list route at depth 9; median, least and most of {args.reps} warm calls, ms; device = the five phases")
    log(f"{'scene':>8s} {'call':>10s} {'words':>10s} | {'new words':>10s} " + " ".join(f"{p:>8s}" for p in PHASES) +
        f" {'device':>9s} {'least':>9s} {'most':>9s} {'wall':>9s} {'least':>9s} {'most':>9s}")
    for depth in (int(d) for d in args.depths.split(",")):
        scene, side = f"field{depth}", (1 << depth) * 25 // 32
        coords, _ = height_field(1, depth, side)
        off = ((1 << depth) - side) // 2
        heights = torch.from_numpy((coords[:, 1] + 1).reshape(side, side).astype(np.int32)).to(dev)
        cells = int(heights.to(torch.int64).sum())

        def solid():
            render.edit_heightmap(heights, LAYERS, (off, off), depth)
            return gpu.heightmap_timing()

        n_base, added, walls, times = timed(empty, solid)
        log(edit_line(scene, "solid", n_base, added, walls, times))
        pyramid_events = None if added is None else [t[0] for t in times]

        # the bump: a dome over a disc in the middle of the patch, on the terrain as `solid` left it
        c0 = (side - DISC) // 2
        i = torch.arange(DISC, device=dev, dtype=torch.float32) - (DISC - 1) / 2
        r = torch.sqrt(i[:, None] ** 2 + i[None, :] ** 2) / (DISC / 2)
        dome = torch.where(r < 1, DOME * 0.5 * (1 + torch.cos(r * np.pi)), torch.zeros_like(r)).to(torch.int32)
        bumped = (heights[c0:c0 + DISC, c0:c0 + DISC] + dome).contiguous()

        def terrain():
            empty()
            return render.edit_heightmap(heights, LAYERS, (off, off), depth)

        def bump():
            render.edit_heightmap(bumped, LAYERS, (off + c0, off + c0), depth, below="set", above="set")
            return gpu.heightmap_timing()

        if added is not None:
            n_base, added_b, walls, times = timed(terrain, bump)
            log(edit_line(scene, "bump", n_base, added_b, walls, times))

        # the pyramid alone beside a copy of the map
        def clocked(call):
            ms = []
            for rep in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                gpu.sync()
                torch.cuda.synchronize()
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
            return ms

        target = torch.empty_like(heights)
        pyr = clocked(lambda: render.height_minmax(heights, depth, (off, off), depth))
        copy = clocked(lambda: target.copy_(heights))
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        copy_events = []
        for rep in range(args.reps + 1):
            ev0.record()
            target.copy_(heights)
            ev1.record()
            torch.cuda.synchronize()
            if rep:
                copy_events.append(ev0.elapsed_time(ev1))
        mb = heights.numel() * 4 / 1e6
        log(f"{scene:>8s} {'pyramid':>10s} map {side} x {side} = {mb:.2f} MB, {cells} cells under the ground | height_minmax wall {spread(pyr)} | "
            f"copy wall {spread(copy)} | ratio of the medians {np.median(pyr) / np.median(copy):.2f}")
        if pyramid_events:
            log(f"{scene:>8s} {'pyramid':>10s} by events: the pyramid phase of `solid` {spread(pyramid_events)} | the copy {spread(copy_events)} | "
                f"ratio of the medians {np.median(pyramid_events) / np.median(copy_events):.2f}; the copy moves {2 * mb:.2f} MB, "
                f"{2 * mb / 1e3 / np.median(copy_events):.2f} TB/s; the pyramid reads {mb:.2f} MB and writes {mb * 2 / 3:.2f} MB")

        # the route before the pass: the cells under the surface as a list, build_nodes, simplify_nodes
        if cells >= 1 << 31:
            log(f"{scene:>8s} {'old route':>10s} cannot run: {cells} cells under the ground, a word each before the merge, against the node "
                f"buffer's 2^27 = {1 << 27} words and build_nodes' 2^31 voxels")
            continue

        def by_cells():
            h = heights.reshape(-1).to(torch.int64)
            col = torch.repeat_interleave(torch.arange(h.numel(), device=dev), h)
            y = torch.arange(col.numel(), device=dev) - (torch.cumsum(h, 0) - h)[col]
            d = h[col] - 1 - y
            colour = torch.where(d < LAYERS[0][0], LAYERS[0][1], torch.where(d < LAYERS[0][0] + LAYERS[1][0], LAYERS[1][1], LAYERS[2][1]))
            xyz = torch.stack([off + col // side, y, off + col % side], 1).to(torch.int32).contiguous()
            built = render.build_nodes(xyz, depth, colour.to(torch.int32))
            return built, render.simplify_nodes()

        n_base, added_o, walls_o, counts = timed(empty, by_cells)
        if added_o is None:
            log(f"{scene:>8s} {'old route':>10s} refused: {walls_o}")
            continue
        old_words = render.read_nodes()
        empty()
        new_len = render.edit_heightmap(heights, LAYERS, (off, off), depth)
        merged = render.simplify_nodes()
        same = merged == old_words.size and np.array_equal(render.read_nodes(), old_words)
        log(f"{scene:>8s} {'old route':>10s} {cells} cells in torch, build_nodes {counts[-1][0]} words, simplify_nodes {counts[-1][1]} words | wall "
            f"{spread(walls_o)} | edit_heightmap {new_len} words, simplified {merged}: {'the same bytes' if same else 'DIFFERENT BYTES'}")
    out.close()
    gpu.close()


if __name__ == "__main__":
    main()
