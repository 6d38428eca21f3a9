"""Component labelling timings: per phase (HIP events: plan, link, union, ids, fill) and the rounds of the fill
of svo_nodes_label_components, and the wall time of Render.label_components with its syncs, next to the only route there
was before: Render.read_nodes, a walk of the words on the host into a dense occupancy grid (numpy, level by level) and
scipy.ndimage.label on it.  Scenes built on the device: a filled ball of radius 100 at depth 8, in unit leaves and after
simplify_nodes(); a depth-9 height field with tree.vox scattered over it; a 256^3 grid filled at random with probability
0.31; and Render.drop_floating after a slab was carved through the ball.  Medians of --reps warm calls after a warm-up; the
host route runs once per scene.  Checks that both routes count the same components.  Asserts no time.

    python tools/components_probe.py [--out profiles/components_probe.log] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
from structure_probe import height_field  # noqa: E402

VOXEL_OFFSET = 1 << 27
PHASES = ("plan", "link", "union", "ids", "fill")


def demorton(keys, level):
    x, y, z = (np.zeros(keys.size, dtype=np.int64) for _ in range(3))
    for b in range(level):
        z |= ((keys >> (3 * b)) & 1) << b
        y |= ((keys >> (3 * b + 1)) & 1) << b
        x |= ((keys >> (3 * b + 2)) & 1) << b
    return x, y, z


def host_grid(words, depth):
    """the occupancy of the `depth` grid, [x, y, z], by a breadth-first walk of the words"""
    side = 1 << depth
    grid = np.zeros((side,) * 3, dtype=bool)
    groups, keys, lanes = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), np.arange(8)
    for level in range(1, depth + 1):
        if not groups.size:
            break
        p = (words[groups[:, None] + lanes] >> 4).astype(np.int64)
        k = keys[:, None] * 8 + lanes
        voxel, interior = p > VOXEL_OFFSET, p < VOXEL_OFFSET
        x, y, z = demorton(k[voxel], level)
        s = 1 << (depth - level)
        if s == 1:
            grid[x, y, z] = True
        else:
            o = np.arange(s)
            for lo in range(0, x.size, max(1, (1 << 22) // s ** 3)):  # (a few million cells at a time)
                part = slice(lo, lo + max(1, (1 << 22) // s ** 3))
                grid[(x[part] * s)[:, None, None, None] + o[None, :, None, None], (y[part] * s)[:, None, None, None] + o[None, None, :, None],
                     (z[part] * s)[:, None, None, None] + o[None, None, None, :]] = True
        groups, keys = p[interior], k[interior]
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_probe.log"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from scipy import ndimage
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    render = pkg.Render(gpu, (64, 64), np.full(8, VOXEL_OFFSET << 4, dtype=np.uint32), capacity=1 << 26)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def ball():
        r = torch.arange(256, device=dev, dtype=torch.float32) - 127.5
        inside = r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2 <= 100.0 ** 2
        render.build_nodes_dense(torch.where(inside, 0x80C0FF, 0).to(torch.int32))
        return 8

    def merged_ball():
        ball()
        render.simplify_nodes()
        return 8

    def field():
        coords, colours, _ = height_field(torch, dev, 9, 3)
        render.build_nodes(coords, 9, colours)
        z = np.load(os.path.join(ROOT, "tests", "golden", "structures_vox.npz"))
        tree = pkg.Structure.from_vox_bytes(pkg.cpu_octree.vox_write(tuple(int(v) for v in z["tree_size"]), z["tree_xyzi"], z["tree_palette"]))
        render.scatter_structures(tree, (0, 0), (512, 512), 100, depth=9)
        return 9

    def random_grid():
        g = torch.Generator(device=dev)
        g.manual_seed(31)
        fill = torch.rand((256, 256, 256), generator=g, device=dev) < 0.31
        render.build_nodes_dense(torch.where(fill, 0x808080, 0).to(torch.int32))
        return 8

    def host_route(depth):
        """(components, ms of the read-back, of the walk, of scipy's labelling, the labelled grid)"""
        t0 = time.perf_counter()
        words = render.read_nodes()
        t1 = time.perf_counter()
        grid = host_grid(words, depth)
        t2 = time.perf_counter()
        lab, n = ndimage.label(grid)
        t3 = time.perf_counter()
        return n, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, lab

    log(f"# svo_nodes_label_components: the fill's HIP events per phase and its rounds, the wall time of Render.label_components (the listing's "
        f"count query, the fill, syncs), median of {args.reps} warm calls, against read_nodes + a numpy walk into a dense grid + scipy.ndimage.label, "
        f"once; ms")
    log(f"{'scene':>18s} {'words':>9s} {'entries':>9s} {'comps':>8s} {'rounds':>6s} " + " ".join(f"{p:>7s}" for p in PHASES) +
        f" {'device':>8s} {'wall':>8s} | {'read':>8s} {'walk':>9s} {'scipy':>9s} {'host':>9s} {'host/wall':>9s}")
    ok = True
    for name, scene in (("ball, unit leaves", ball), ("ball, merged", merged_ball), ("height field+trees", field), ("random 0.31", random_grid)):
        depth = scene()
        rows = []
        for rep in range(args.reps + 1):  # (the first call is the warm-up: workspaces, code objects, torch's allocator)
            t0 = time.perf_counter()
            labels, ids, n = render.label_components(depth)
            wall = (time.perf_counter() - t0) * 1e3
            ms, rounds = gpu.components_timing()
            if rep:
                rows.append(ms[:5] + [wall])
        med = np.median(np.array(rows), axis=0)
        n_host, read, walk, scipy_ms, _ = host_route(depth)
        ok = ok and n_host == n
        host = read + walk + scipy_ms
        log(f"{name:>18s} {render.node_length:9d} {len(labels):9d} {n:8d} {rounds:6d} " + " ".join(f"{t:7.3f}" for t in med[:5]) +
            f" {float(med[:5].sum()):8.3f} {med[5]:8.3f} | {read:8.3f} {walk:9.3f} {scipy_ms:9.3f} {host:9.3f} {host / med[5]:9.1f}")
        log(f"# {name}: scipy counts {n_host} components, the device {n}")
        del labels, ids

    # drop_floating: a slab carved through the ball, the lower half held by an anchor box under the cut
    anchor = ((0, 0, 0), (256, 120, 256))
    walls = []
    for rep in range(args.reps + 1):
        ball()
        render.edit_region([pkg.region.box((0, 120, 0), (256, 136, 256), 0)], 8)
        if rep == 0:
            n_host, read, walk, scipy_ms, lab = host_route(8)
            t0 = time.perf_counter()
            held = np.zeros(n_host + 1, dtype=bool)
            held[np.unique(lab[:, :120, :])] = True
            cells = int((~held[lab] & (lab > 0)).sum())
            decide = (time.perf_counter() - t0) * 1e3
            del lab
        t0 = time.perf_counter()
        result = render.drop_floating(8, anchor)
        walls.append((time.perf_counter() - t0) * 1e3)
    host = read + walk + scipy_ms + decide
    wall = float(np.median(walls[1:]))
    log(f"# drop_floating after a carve of the slab y in [120, 136) through the ball, anchor y < 120: (components, dropped components, dropped "
        f"leaves) = {result}; wall {wall:.3f} ms (label_components, list_voxels, the torch selection, scatter_nodes_device; median of "
        f"{args.reps}); the host route finds {n_host} components and {cells} cells to drop in read {read:.3f} + walk {walk:.3f} + scipy "
        f"{scipy_ms:.3f} + decide {decide:.3f} = {host:.3f} ms, and has yet to write them back; host / wall = {host / wall:.1f}")
    ok = ok and n_host == result[0] and cells == result[2]
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("the two routes differ")


if __name__ == "__main__":
    main()
