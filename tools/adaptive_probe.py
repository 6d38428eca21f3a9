"""The streaming loop's list processing on the host against the device step, frame by frame.

A world from World.generate_world (world_depth 1, --chunk-depth), every chunk resident, expanded with world.expand toward
the camera (--expand-depth, --lod), twice: one copy for the host path (incremental upload, sorted lists), one attached to
the device step.  Each frame traces and scans the host copy; its lists go through the host path and, as explicit device
lists, through svo_adaptive_step on the other copy.  (Two loops that scanned for themselves would part ways as soon as
the unsubdivide list is at its cap: which candidates the scan keeps then depends on its atomics.)  The counts must match
every frame and the two trees, positions and hole stacks after the last one.

  trace      the traced frame (svo_last_render_ms)
  scan       svo_scan_dispatch, wall time with a sync
  host path  read-back (svo_scan_read), svo_adaptive_subdivide + _unsubdivide, dirty words -> svo_nodes_scatter (wall)
  device     svo_adaptive_timing: sort, subdivide pass, unsubdivide pass (HIP events on the stream), step wall time

    python tools/adaptive_probe.py [--out profiles/adaptive_probe.log] [--chunk-depth 9] [--expand-depth 12] [--lod 4096]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
sys.path[:0] = [ROOT, TOOLS]
import __graft_entry__ as entry  # noqa: E402
from expand_probe import state_digest  # noqa: E402

BLOCKS = ("stone", "dirt", "grass", "wood", "leaf", "slate", "crystal", "glass")
CAM, LOOK = (0.0, 0.25, -1.2), (0.0, -0.3, 1.0)  # above the island, looking in and down


def write_blocks(pkg, d):
    z = np.load(os.path.join(ROOT, "tests", "golden", "blocks_vox.npz"))
    os.makedirs(d)
    for name in BLOCKS:
        with open(os.path.join(d, name + ".vox"), "wb") as f:
            f.write(pkg.cpu_octree.vox_write(16, z[name + "_xyzi"], z[name + "_palette"]))


def open_world(pkg, path, blocks):
    w = pkg.World.new(path, blocks)
    for name in sorted(os.listdir(path)):
        w.load_chunk(int(name.split(".")[0]))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_probe.log"))
    ap.add_argument("--chunk-depth", type=int, default=9)
    ap.add_argument("--expand-depth", type=int, default=12)
    ap.add_argument("--lod", type=float, default=4096.0)
    ap.add_argument("--max-words", type=int, default=40_000_000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    pkg = entry.build()
    W, H = (int(v) for v in args.size.split("x"))
    tmp = tempfile.mkdtemp(prefix="adaptive_probe_")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        blocks = os.path.join(tmp, "blocks")
        write_blocks(pkg, blocks)
        g0 = pkg.Gpu(0)
        path = os.path.join(tmp, "world")
        t = time.perf_counter()
        pkg.World.generate_world(path, pkg.Procedural(g0), world_depth=1, chunk_depth=args.chunk_depth, blocks_dir=blocks)
        g0.close()
        say(f"# generate_world(world_depth=1, chunk_depth={args.chunk_depth}): {time.perf_counter() - t:.1f} s")
        loops = []
        for on_device in (False, True):
            world = open_world(pkg, path, blocks)
            octree = world.root_octree()
            t = time.perf_counter()
            n = world.expand(octree, args.expand_depth, cam=CAM, lod_c=args.lod, max_words=args.max_words)
            if not on_device:
                say(f"# expand(max_depth={args.expand_depth}, lod_c={args.lod}) toward {CAM}: {n} subdivisions, "
                    f"{len(octree)} words ({4 * len(octree) / 1e6:.0f} MB), {time.perf_counter() - t:.1f} s on the host")
            g = pkg.Gpu(0)
            render = pkg.Render.new(g, (W, H), octree, capacity=len(octree) + 8 * 2_100_000)
            render.set_flags(pause_adaptive=False, shadows=True)
            g.set_option(pkg.gpu.OPT_TREE_DEPTH, max(16, args.expand_depth))
            g.set_option(pkg.gpu.OPT_TIMING, 1)
            compute = pkg.Compute.new(g, render)
            g.set_option(pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, 1)
            octree.take_dirty()
            loops.append((g, render, compute, octree, world, pkg.adaptive.DeviceAdaptive(g, render, octree, world) if on_device else None))
        settings = pkg.Settings(fov=90.0)
        say(f"# {W}x{H}; camera drifts +x by 0.01 per frame; ms per frame (host path: wall; device: HIP events + step wall)")
        say("frame  n_sub  n_unsub   trace   scan | host: readback  adaptive  scatter   total | device: sort  subdiv  unsub"
            "  step_wall | speed-up")
        rows = []
        for f in range(args.frames):
            cam = (CAM[0] + 0.01 * f, CAM[1], CAM[2])
            ch = pkg.Character(cam, LOOK)
            # host path, stage by stage (AdaptiveLoop.frame's body)
            g, render, compute, octree, world, _ = loops[0]
            render.update(settings, ch)
            render.render()
            g.sync()
            trace = g.last_render_ms()
            t0 = time.perf_counter()
            compute.update(len(octree))
            g.sync()
            t1 = time.perf_counter()
            sub, unsub = compute.read_lists()
            sub.sort()
            unsub.sort()
            t2 = time.perf_counter()
            ns = pkg.adaptive.process_subdivision(sub, octree, world)
            nu = pkg.adaptive.process_unsubdivision(unsub, octree, world)
            t3 = time.perf_counter()
            idx, val = octree.take_dirty()
            render.scatter_nodes(idx, val, node_length=len(octree))
            t4 = time.perf_counter()
            scan = 1e3 * (t1 - t0)
            host = [1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t4 - t3)]
            # device path, same lists (the null-list form of the step adds the read of the two counts)
            dev = loops[1][5]
            ds, du = torch.from_numpy(sub.view(np.int32)).cuda(), torch.from_numpy(unsub.view(np.int32)).cuda()
            torch.cuda.synchronize()
            dn = dev.step(ds, du)
            ms = dev.timing()
            assert dn == (ns, nu), f"frame {f}: device counts {dn} != host {(ns, nu)}"
            dev_total = ms[3]
            say(f"{f:5d} {ns:6d} {nu:8d} {trace:7.3f} {scan:6.3f} |       {host[0]:8.3f}  {host[1]:8.2f} {host[2]:8.3f} "
                f"{sum(host):7.2f} |   {ms[0]:7.3f} {ms[1]:7.3f} {ms[2]:6.3f}  {dev_total:8.3f} | {sum(host) / dev_total:7.1f}x")
            rows.append((ns, nu, host, ms))
        loops[1][5].download()
        a, b = loops[0][3], loops[1][3]
        same = (np.array_equal(a.raw_data(), b.raw_data()) and np.array_equal(a.positions().view(np.uint32), b.positions().view(np.uint32))
                and np.array_equal(a.hole_stack(), b.hole_stack()) and loops[0][4].chunk_ids() == loops[1][4].chunk_ids())
        say(f"# after {args.frames} frames: host and device words, positions, hole stacks and chunk sets equal: {same}; "
            f"length {len(a)}, holes {a.hole_count()}")
        say(f"# the device copy's downloaded state (list sizes above vary from run to run with the scan's atomics; two runs "
            f"with the same sizes must print the same digest): {state_digest(b)}")
        big = [r for r in rows if r[1] >= 1_000_000]
        if big:
            say(f"# frames at the 1 023 999-entry unsubdivide cap: {len(big)}; device step median "
                f"{np.median([r[3][3] for r in big]):.3f} ms (events: sort {np.median([r[3][0] for r in big]):.3f}, "
                f"subdivide {np.median([r[3][1] for r in big]):.3f}, unsubdivide {np.median([r[3][2] for r in big]):.3f}), "
                f"host path median {np.median([sum(r[2]) for r in big]):.1f} ms")
        for g, *_ in loops:
            g.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
