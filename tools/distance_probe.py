"""Distance field timings: per phase (HIP events: the occupancy bits, the first slab's z and y pass, the first
slab's x pass, all slabs) and wall time of Render.distance_dense for a 256^3 and a 512^3 box, R = 4, 16 and 64, the three
modes, with and without sites (to the voxels), on three scenes built on the device: the height field of tools/build_probe.py
at depth 9 (one voxel per column), a merged solid ball of radius 205 cells around the middle of the depth-9 grid (36 M cells
in coarse leaves, tools/morph_probe.py's), and an icosphere(4) voxelised at depth 10 (a shell of 3.2 M voxels,
tools/surface_probe.py's).  Beside them:
  copy        a device-to-device copy of the outputs (torch events): the floor of anything that writes them
  old route   what there was before the pass, for the same box: sample_dense of the box grown by R and cut to the grid, the
              read-back, scipy.ndimage.distance_transform_edt on the host, squared, rounded and cut to R, the upload.  Once
              per case, after one warm-up on a small box: its seconds do not need a median.  --old picks the cases
  morph_ball  Render.morph_ball("grow", r) on the 256^3 box next to Render.morph_nodes("grow", steps=r, conn=26) on the same
              tree: the ball in one pass, the cube in r walks of the whole tree
Same process, same build, median (and least .. most) of --reps warm calls after a warm-up call.  Asserts no time.

    python tools/distance_probe.py [--out profiles/distance_probe.log] [--reps 5] [--scenes field9,ball9,shell10] [--old 256:4,256:16,256:64,512:16]
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

PHASES = ("bits", "zy 1st", "x 1st", "slabs")
SCENES = {"field9": ("field", 9), "ball9": ("ball", 9), "shell10": ("shell", 10)}  # name -> (what, depth)
STONE = 0x808080
RADIUS = 205


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return f"{float(np.median(v)):9.3f} {float(v.min()):9.3f} {float(v.max()):9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_probe.log"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="field9,ball9,shell10")
    ap.add_argument("--old", default="256:4,256:16,256:64,512:16")
    args = ap.parse_args()
    import torch
    from scipy.ndimage import distance_transform_edt
    pkg = entry.load_package()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    root = np.full(8, B.EMPTY, dtype=np.uint32)
    render = pkg.Render(gpu, (64, 64), root, capacity=1 << 26)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    old_cases = {tuple(int(v) for v in c.split(":")) for c in args.old.split(",") if c}

    def log(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    def build(scene):
        kind, depth = SCENES[scene]
        if kind == "field":
            coords, colours = height_field(1, depth, (1 << depth) * 25 // 32)
            render.build_nodes(torch.from_numpy(coords).to(dev, torch.int32), depth, torch.from_numpy(colours).to(dev, torch.int32))
        elif kind == "ball":
            mid = 1 << (depth - 1)
            render.write_nodes(root)
            render.node_length = 8
            render.edit_region([pkg.region.ball((mid, mid, mid), RADIUS, STONE)], depth)
            render.simplify_nodes()
        else:
            v, t = pkg.mesh.icosphere(4)
            coords, colours = pkg.mesh.voxelize(gpu, v, t, depth)
            render.build_nodes(coords, depth, colours)
        return depth

    def box_of(scene, depth, side):
        """a box that holds surface: the field's and the ball's around the grid's middle, the shell's at its +x pole"""
        full, mid = 1 << depth, 1 << (depth - 1)
        if side >= full:
            return (0, 0, 0), (full,) * 3
        if SCENES[scene][0] == "shell":
            return (full - side, mid - side // 2, mid - side // 2), (side,) * 3
        return (mid - side // 2,) * 3, (side,) * 3

    def old_route(depth, origin, size, R):
        lo = [max(0, o - R) for o in origin]
        hi = [min(1 << depth, o + s + R) for o, s in zip(origin, size)]
        t0 = time.perf_counter()
        grid = render.sample_dense(lo, [b - a for a, b in zip(lo, hi)], depth).cpu().numpy()
        t1 = time.perf_counter()
        d = distance_transform_edt(grid == 0) if grid.any() else np.full(grid.shape, np.inf)  # (scipy wants a zero to measure from)
        d2 = np.where(np.isfinite(d), np.rint(d * d), float(pkg.distance.FAR))
        d2 = np.where(d2 <= R * R, d2, pkg.distance.FAR).astype(np.int32)
        d2 = np.ascontiguousarray(d2[tuple(slice(o - a, o - a + s) for o, a, s in zip(origin, lo, size))])
        t2 = time.perf_counter()
        up = torch.from_numpy(d2).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return up, ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)

    def copy_ms(tensors):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = []
        for _ in range(args.reps + 1):
            ev[0].record()
            kept = [t.clone() for t in tensors]
            ev[1].record()
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]))
            del kept
        return float(np.median(times[1:]))

    log(f"# exact distance fields of a device tree: Render.distance_dense (HIP events and wall; median, least and most of {args.reps} warm "
        f"calls, ms) next to a device-to-device copy of its outputs and to the old route (sample_dense of the grown box, read-back, scipy "
        f"distance_transform_edt, upload; one call, ms); then morph_ball next to morph_nodes")
    log(f"{'scene':>8s} {'box':>5s} {'R':>3s} {'mode':>7s} {'sites':>5s} {'words':>9s} | " + " ".join(f"{p:>8s}" for p in PHASES) +
        f" {'device':>9s} {'least':>9s} {'most':>9s} {'wall':>9s} {'least':>9s} {'most':>9s} {'copy':>8s} | {'old: sample+read':>16s} {'edt':>10s} {'upload':>8s} {'sum':>10s}")
    old_route(build("field9"), (0, 0, 0), (32, 32, 32), 4)  # (the warm-up of the old route's calls)
    for scene in args.scenes.split(","):
        depth = build(scene)
        words = render.node_length
        for side in (256, 512):
            origin, size = box_of(scene, depth, side)
            for R in (4, 16, 64):
                for mode, sites in (("voxels", False), ("voxels", True), ("empty", False), ("signed", False)):
                    times, walls = [], []
                    for rep in range(args.reps + 1):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got = render.distance_dense(origin, size, R, depth, mode, with_sites=sites)
                        wall = (time.perf_counter() - t0) * 1e3
                        if rep:
                            times.append(gpu.distance_timing())
                            walls.append(wall)
                    t = np.array(times)
                    device = t[:, 0] + t[:, 3]
                    line = (f"{scene:>8s} {side:5d} {R:3d} {mode:>7s} {str(sites):>5s} {words:9d} | " + " ".join(f"{v:8.3f}" for v in np.median(t, axis=0)[:4]) +
                            f" {spread(device)} {spread(walls)} {copy_ms(got if sites else [got]):8.3f}")
                    if mode == "voxels" and not sites and (side, R) in old_cases:
                        up, (t_sample, t_edt, t_up) = old_route(depth, origin, size, R)
                        assert torch.equal(up, got), "the old route gives another field"
                        line += f" | {t_sample:16.1f} {t_edt:10.1f} {t_up:8.1f} {t_sample + t_edt + t_up:10.1f}"
                        del up
                    del got
                    log(line)
    log("")
    log(f"{'scene':>8s} {'r':>3s} {'words':>9s} | {'morph_ball grow: new words':>26s} {'wall':>9s} {'least':>9s} {'most':>9s} | "
        f"{'morph_nodes grow 26 x r: new words':>34s} {'wall':>9s} {'least':>9s} {'most':>9s}")
    for scene in [s for s in args.scenes.split(",") if SCENES[s][0] != "shell"]:
        for r in (4, 16):
            line = ""
            for call in ("ball", "nodes"):
                walls = []
                for rep in range(min(args.reps, 3) + 1):
                    depth = build(scene)
                    words = render.node_length
                    origin, size = box_of(scene, depth, 256)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    try:
                        if call == "ball":
                            render.morph_ball("grow", r, origin, size, STONE, depth)
                        else:
                            render.morph_nodes("grow", r, 26, STONE, depth)
                    except pkg.SvoError as e:
                        walls = str(e)
                        break
                    gpu.sync()
                    if rep:
                        walls.append((time.perf_counter() - t0) * 1e3)
                line += " | " + (f"refused: {walls}" if isinstance(walls, str) else f"{render.node_length - words:{26 if call == 'ball' else 34}d} {spread(walls)}")
            log(f"{scene:>8s} {r:3d} {words:9d}" + line)
    out.close()
    gpu.close()


if __name__ == "__main__":
    main()
