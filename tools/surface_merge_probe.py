"""Merged-surface timings: per phase (HIP events: the quads, then keys, sort, flags and scan, emit of the U
and the V phase, the output's fill) of the fill of svo_nodes_merge_surface with one round, next to the same merge composed
in torch from Render.surface_quads -- two stable torch.sort calls per phase, the follow condition on neighbours, nonzero --
whose device time is the surface call's own HIP events plus torch events around the torch work.  Three scenes built on the
device: DESIGN.md 23's icosphere(4) shell at depth 10 and filled ball of radius 100 at depth 8, both of one colour, and a
solid height field at depth 9 coloured in bands of height.  Both ways run alternated in one process; medians of --reps
rounds after a warm-up round.  Checks that both give the same rectangles.  Then the triangles of
mesh.extract_surface(merge=True) against merge=False, and the rectangles of two rounds.  Asserts no time.

    python tools/surface_merge_probe.py [--out profiles/surface_merge_probe.log] [--reps 7]
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

PHASES = ("quads", "U keys", "U sort", "U flags", "U emit", "V keys", "V sort", "V flags", "V emit", "fill")


def torch_merge(coords, colours, faces, levels, depth):
    """one round of the contract's merge over surface_quads' tensors in plain torch: (rects (n, 6) int32, values)"""
    import torch
    dev = coords.device
    c, f = coords.to(torch.int64), faces.to(torch.int64)
    s = torch.bitwise_left_shift(torch.ones_like(f), depth - levels.to(torch.int64))
    a = f >> 1
    along = lambda axis: c.gather(1, axis[:, None]).squeeze(1)  # noqa: E731
    fp = f << 22 | (along(a) + (f & 1) * s)
    lo = torch.stack([along((a + 1) % 3), along((a + 2) % 3)], dim=1)
    hi = lo + s[:, None]
    val = colours
    for d in (0, 1):
        o = 1 - d
        order = torch.sort((hi[:, o] - lo[:, o]) << depth | lo[:, d], stable=True).indices
        order = order[torch.sort((fp << depth | lo[:, o])[order], stable=True).indices]
        fp, lo, hi, val = fp[order], lo[order], hi[order], val[order]
        follows = ((fp[1:] == fp[:-1]) & (lo[1:, o] == lo[:-1, o]) & (hi[1:, o] == hi[:-1, o]) & (hi[:-1, d] == lo[1:, d]) &
                   (val[1:] == val[:-1]))
        head = torch.cat([torch.ones(1, dtype=torch.bool, device=dev), ~follows]).nonzero().squeeze(1)
        last = torch.cat([head[1:] - 1, torch.tensor([len(fp) - 1], device=dev)])
        far = hi[last, d]
        fp, lo, hi, val = fp[head], lo[head], hi[head].clone(), val[head]
        hi[:, d] = far
    rects = torch.stack([fp >> 22, fp & 0x3FFFFF, lo[:, 0], lo[:, 1], hi[:, 0] - lo[:, 0], hi[:, 1] - lo[:, 1]], dim=1).to(torch.int32)
    return rects, val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_merge_probe.log"))
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

    def height_field():
        i = torch.arange(512, device=dev, dtype=torch.float32)
        height = (64.0 + 24.0 * torch.sin(i / 40.0)[:, None] * torch.cos(i / 55.0)[None, :] + 8.0 * torch.sin(i / 9.0)[:, None]).floor()
        height[128:256, 300:420] = 70.0  # a plateau
        y = torch.arange(512, device=dev, dtype=torch.float32)
        band = (0x203010 + 0x101808 * (y / 16.0).floor().to(torch.int32))[None, :, None]  # a colour per 16 cells of height
        solid = y[None, :, None] < height[:, None, :]
        render.build_nodes_dense(torch.where(solid, band, 0).to(torch.int32))
        return 9

    def new_way(depth):
        t0 = time.perf_counter()
        rects, values = render.surface_rects(depth)
        wall = (time.perf_counter() - t0) * 1e3
        ms = gpu.surface_merge_timing()
        return (rects, values), np.array(ms[:9] + ms[33:34]), wall

    def composition(depth):
        """(rects, values) of one round; device ms of surface_quads' fill and of the torch work"""
        t0 = time.perf_counter()
        coords, colours, faces, levels = render.surface_quads(depth)
        device = float(sum(gpu.surface_timing()[:6]))
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rects, val = torch_merge(coords, colours, faces, levels, depth)
        stop.record()
        stop.synchronize()
        device += start.elapsed_time(stop)
        return (rects, val), device, (time.perf_counter() - t0) * 1e3, len(faces)

    log(f"# the exposed faces merged into rectangles, one round: svo_nodes_merge_surface (HIP events of the fill) against Render.surface_quads + "
        f"two stable torch.sort per phase + the follow condition and nonzero in torch (the fill's HIP events + torch events); alternated, "
        f"median of {args.reps} rounds after a warm-up, ms")
    log(f"{'scene':>16s} {'words':>9s} {'quads':>9s} {'rects':>9s} " + " ".join(f"{p:>7s}" for p in PHASES) +
        f" {'device':>8s} {'composed':>8s} {'ratio':>6s} {'wall':>8s} {'wall c.':>8s}")
    ok = True
    counts = []
    for name, scene in (("icosphere shell", shell), ("filled ball", ball), ("height field", height_field)):
        depth = scene()
        new, old = [], []
        for rep in range(args.reps + 1):  # (the first round is the warm-up: workspaces, code objects, torch's allocator)
            a, phases, wall = new_way(depth)
            b, device, wall_c, n_quads = composition(depth)
            if rep:
                new.append(np.concatenate([phases, [wall]]))
                old.append([device, wall_c])
        same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ok = ok and same
        new, old = np.median(np.array(new), axis=0), np.median(np.array(old), axis=0)
        total = float(new[:10].sum())
        log(f"{name:>16s} {render.node_length:9d} {n_quads:9d} {len(a[0]):9d} " + " ".join(f"{t:7.3f}" for t in new[:10]) +
            f" {total:8.3f} {old[0]:8.3f} {total / old[0]:6.3f} {new[10]:8.3f} {old[1]:8.3f}")
        log(f"# {name}: both ways give the same rectangles: {same}")
        plain = pkg.mesh.extract_surface(render, depth)
        merged = pkg.mesh.extract_surface(render, depth, merge=True)
        two = render.surface_rects(depth, rounds=2)[0]
        anyv = render.surface_rects(depth, any_value=True)[0]
        counts.append(f"# {name}: extract_surface: {len(plain[1])} triangles and {len(plain[0])} vertices, with merge=True {len(merged[1])} and "
                      f"{len(merged[0])}; rectangles after two rounds {len(two)}, with any_value {len(anyv)}")
        del plain, merged, two, anyv, a, b
    for line in counts:
        log(line)
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("the two ways differ")


if __name__ == "__main__":
    main()
