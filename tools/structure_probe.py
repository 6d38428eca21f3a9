"""Structure scattering timings on height fields built with Render.from_voxels: wall time of each call with
its sync (and the device events of svo_structure_timing), median and spread of --reps warm calls after one warm-up.

  (a) the tops of a 512 x 512 rectangle at depth 9, against the only way there was before: sample_dense of the 512^3 box
      plus a torch reduction to the same two arrays.  The two must agree, and (a) must not be the slower one.
  (b) the tops of 4096 x 4096 at depth 12 (sample_dense refuses that box: 2^36 cells), the time alone.
  (c) tree.vox (tests/golden/structures_vox.npz) stamped at the sites of (a) with one_in = 100, against the same list made
      with torch broadcasting and a mask; the two must agree, and the stamp must not be the slower one.  Then the stamp
      followed by edit_nodes (place_structures) on the freshly built tree.

    python tools/structure_probe.py [--out profiles/structure_probe.log] [--reps 7]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def height_field(torch, dev, depth, thick):
    """h = side * (0.4 + 0.1 sin(u / 37) + 0.08 cos(w / 53)) with (u, w) = (x, z) * 512 / side, the same hills at every depth,
    `thick` cells under it in every column: (coords, colours, h) on dev"""
    side = 1 << depth
    x, z = torch.meshgrid(torch.arange(side, device=dev), torch.arange(side, device=dev), indexing="ij")
    h = (side * (0.4 + 0.1 * torch.sin(x * (512.0 / side) / 37.0) + 0.08 * torch.cos(z * (512.0 / side) / 53.0))).to(torch.int32)
    coords = torch.cat([torch.stack([x, h - k, z], dim=-1).reshape(-1, 3) for k in range(thick)]).to(torch.int32)
    colours = (0x204020 + (coords[:, 1] & 0xFF) * 0x100).to(torch.int32)
    return coords.contiguous(), colours.contiguous(), h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_probe.log"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def timed(f, before=None):
        wall, events = [], []
        for rep in range(args.reps + 1):  # (the first is the warm-up)
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                wall.append(w)
                events.append(gpu.structure_timing()[:2])
        return out, wall, np.median(np.array(events), axis=0)

    def row(name, wall, note=""):
        log(f"{name:>52s} {np.median(wall):10.3f} {min(wall):10.3f} {max(wall):10.3f}  {note}")
        return float(np.median(wall))

    ok = True
    log(f"# wall ms of each call with its sync: median, min, max of {args.reps} warm calls; library {os.path.basename(pkg._lib.LIB_PATH)}")
    log(f"{'case':>52s} {'median':>10s} {'min':>10s} {'max':>10s}")

    # (a) depth 9
    coords, colours, h = height_field(torch, dev, 9, 3)
    render = pkg.Render.from_voxels(gpu, (64, 64), coords, 9, colours, capacity=1 << 25)
    whole = ((0, 0), (512, 512))
    (tops, values), wall, ev = timed(lambda: render.column_tops(*whole, 9, with_values=True))
    a_new = row("(a) column_tops 512 x 512, depth 9", wall, f"kernel {ev[0]:.3f} ms (device events); {render.node_length} words")

    def dense_way():
        grid = render.sample_dense((0, 0, 0), (512, 512, 512), 9)
        full = grid != 0
        ys = torch.arange(1, 513, device=dev, dtype=torch.int32)
        top = (full * ys[None, :, None]).amax(dim=1) - 1  # -1: nothing in the column
        value = torch.gather(grid, 1, top.clamp(min=0)[:, None, :].long())[:, 0, :]
        return top, torch.where(top >= 0, value, 0)

    (old_tops, old_values), wall, _ = timed(dense_way)
    a_old = row("(a) sample_dense 512^3 + torch reduction", wall)
    same = bool(torch.equal(tops, old_tops.to(torch.int32)) and torch.equal(values, old_values.to(torch.int32)))
    same &= bool(torch.equal(tops, h))
    ok &= same and a_new <= a_old
    log(f"# (a) the two ways agree and give the field's heights: {same}; column_tops is {a_old / a_new:.1f} x the speed of the dense way")

    # (c) the sites of (a), tree.vox stamped on them
    z = np.load(os.path.join(ROOT, "tests", "golden", "structures_vox.npz"))
    tree = pkg.Structure.from_vox_bytes(pkg.cpu_octree.vox_write(tuple(int(v) for v in z["tree_size"]), z["tree_xyzi"], z["tree_palette"]))
    (origins, rots), wall, ev = timed(lambda: render.structure_sites(tops, values, (0, 0), 100))
    row(f"(c) structure_sites one_in = 100: {len(origins)} sites", wall, f"count {ev[0]:.3f} ms, fill {ev[1]:.3f} ms (device events)")
    (xyz, col), wall, ev = timed(lambda: render.stamp_structures(tree, origins, 9, rots))
    c_new = row(f"(c) stamp_structures {len(tree)} voxels x {len(origins)} sites", wall, f"count {ev[0]:.3f} ms, fill {ev[1]:.3f} ms; {len(col)} entries")
    offsets, tree_colours = tree.on(dev)
    turned = [offsets]
    for _ in range(3):
        o = turned[-1]
        turned.append(torch.stack([o[:, 2], o[:, 1], -o[:, 0]], dim=1))
    turned = torch.stack(turned)  # [4, m, 3]

    def torch_way():
        cells = origins[:, None, :] + turned[rots.long()]
        inside = ((cells >= 0) & (cells < 512)).all(dim=2)
        return cells[inside], tree_colours[None, :].expand(len(origins), -1)[inside]

    (old_xyz, old_col), wall, _ = timed(torch_way)
    c_old = row("(c) the same list by torch broadcasting and a mask", wall)
    same = bool(torch.equal(xyz, old_xyz.to(torch.int32)) and torch.equal(col, old_col.to(torch.int32)))
    ok &= same and c_new <= c_old
    log(f"# (c) the two lists agree: {same}; stamp_structures is {c_old / c_new:.1f} x the speed of the torch way")
    n0 = render.node_length
    _, wall, _ = timed(lambda: render.place_structures(tree, origins, 9, rots), before=lambda: render.build_nodes(coords, 9, colours))
    edit = gpu.edit_timing()
    row("(c) place_structures: stamp + edit_nodes, fresh tree", wall, f"edit {sum(edit[:5]):.3f} ms on the device; {n0} -> {render.node_length} words")
    del render, coords, colours

    # (b) depth 12: the parent commit has no way at all
    coords, colours, h = height_field(torch, dev, 12, 1)
    render = pkg.Render.from_voxels(gpu, (64, 64), coords, 12, colours, capacity=1 << 27)
    del coords, colours
    tops, wall, ev = timed(lambda: render.column_tops((0, 0), (4096, 4096), 12))
    row("(b) column_tops 4096 x 4096, depth 12", wall, f"kernel {ev[0]:.3f} ms (device events); {render.node_length} words")
    same = bool(torch.equal(tops, h))
    ok &= same
    log(f"# (b) the tops are the field's heights: {same}")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("a comparison failed or a new call was the slower one")


if __name__ == "__main__":
    main()
