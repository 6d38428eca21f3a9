"""Opening a world at a view's level of detail: host World.expand + upload against Render.from_world.

The probe world of tools/adaptive_probe.py (World.generate_world, world_depth 1, --chunk-depth, every chunk resident) is
expanded toward the camera (--expand-depth, --lod, --max-words) both ways in one process, after a warm-up and the small case, monu9 to depth 6
(launches and read-backs are its floor):

  host path    World.expand (host, one node at a time), Render.new (the words go up), DeviceAdaptive (attach: the
               positions go up, the world is mirrored); wall times, the last one ending in a device synchronise
  device path  Render.from_world: 8 words go up, attach, svo_adaptive_expand; wall time ending in a device synchronise,
               and svo_adaptive_expand_timing: leaves, candidates, subdivide (HIP events), the call's wall time, levels

and the two trees (words, positions, hole stacks, lengths, counts, chunk sets) must be identical.

    python tools/expand_probe.py [--out profiles/expand_probe.log] [--chunk-depth 9] [--expand-depth 12] [--lod 4096]
"""
import argparse
import hashlib
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

BLOCKS = ("stone", "dirt", "grass", "wood", "leaf", "slate", "crystal", "glass")
CAM = (0.0, 0.25, -1.2)  # above the island (tools/adaptive_probe.py)


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


def monu9_world(pkg):
    z = np.load(os.path.join(ROOT, "tests", "golden", "monu9_vox.npz"))
    return pkg.adaptive.World(pkg.CpuOctree.from_voxels(int(z["size"][0]), z["xyzi"], z["palette"]))


def state_digest(octree):
    """What two builds of the library are compared by: the same inputs must give the same digest."""
    h = hashlib.sha256()
    for a in (octree.raw_data(), octree.positions(), octree.hole_stack()):
        h.update(np.ascontiguousarray(a).tobytes())
    return f"{len(octree)} words {h.hexdigest()[:32]}"


def both_ways(pkg, say, name, make_world, size, max_depth, cam, lod_c, capacity, runs):
    """One case: the host path once, the device path `runs` times (a fresh context each), the trees compared."""
    ms = lambda a, b: 1e3 * (b - a)  # noqa: E731
    world = make_world()
    octree = world.root_octree()
    t0 = time.perf_counter()
    n_host = world.expand(octree, max_depth, cam=cam, lod_c=lod_c, max_words=capacity)
    t1 = time.perf_counter()
    g = pkg.Gpu(0)
    render = pkg.Render.new(g, size, octree, capacity=capacity)
    g.sync()
    t2 = time.perf_counter()
    g.set_option(pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, 1)
    pkg.adaptive.DeviceAdaptive(g, render, octree, world)
    g.sync()
    t3 = time.perf_counter()
    g.close()
    host_total = ms(t0, t3)
    say(f"{name}: expand(max_depth={max_depth}, cam={cam}, lod_c={lod_c}, max_words={capacity}): {n_host} subdivisions, "
        f"{len(octree)} words ({4 * len(octree) / 1e6:.1f} MB)")
    say(f"  host path    total {host_total:9.2f} ms = World.expand {ms(t0, t1):9.2f} + Render.new {ms(t1, t2):8.2f} + attach {ms(t2, t3):8.2f}")
    totals, expands, host_expand = [], [], ms(t0, t1)
    for run in range(runs):
        world_d = make_world()
        g = pkg.Gpu(0)
        t0 = time.perf_counter()
        render, dev = pkg.Render.from_world(g, size, world_d, max_depth, cam=cam, lod_c=lod_c, capacity=capacity)
        g.sync()
        t1 = time.perf_counter()
        tm = dev.expand_timing()
        totals.append(ms(t0, t1))
        expands.append(tm[3])
        say(f"  device path  total {ms(t0, t1):9.2f} ms, of which svo_adaptive_expand {tm[3]:8.2f} (events: leaves {tm[0]:.3f}, "
            f"candidates {tm[1]:.3f}, subdivide {tm[2]:.3f}; {tm[4]} levels); the rest is node buffer, attach and mirror")
        same_words = np.array_equal(render.read_nodes(dev.length), octree.raw_data())
        got = dev.download()
        same = (same_words and dev.last["n_sub"] == n_host and len(got) == len(octree)
                and np.array_equal(got.raw_data(), octree.raw_data())
                and np.array_equal(got.positions().view(np.uint32), octree.positions().view(np.uint32))
                and np.array_equal(got.hole_stack(), octree.hole_stack()) and world.chunk_ids() == world_d.chunk_ids())
        say(f"               words, positions, hole stack, length, count and chunk set equal the host's: {same}")
        say(f"               sha256 of the downloaded words, positions and hole stack: {state_digest(got)}")
        g.close()
        if not same:
            raise SystemExit(f"{name}: the device-expanded tree differs from the host's")
    say(f"  host path / device path (median of {runs}): {host_total / float(np.median(totals)):.1f}x; "
        f"World.expand / svo_adaptive_expand (median): {host_expand / float(np.median(expands)):.1f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_probe.log"))
    ap.add_argument("--chunk-depth", type=int, default=9)
    ap.add_argument("--expand-depth", type=int, default=12)
    ap.add_argument("--lod", type=float, default=4096.0)
    ap.add_argument("--max-words", type=int, default=40_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    pkg = entry.build()
    size = tuple(int(v) for v in args.size.split("x"))
    tmp = tempfile.mkdtemp(prefix="expand_probe_")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        say("# wall times in ms around work that ends in a device synchronise; events: svo_adaptive_expand_timing")
        both_ways(pkg, lambda s: None, "warm-up", lambda: monu9_world(pkg), size, 6, None, 0.0, 200_000, 1)  # (first context, code objects)
        both_ways(pkg, say, "monu9 (the small case)", lambda: monu9_world(pkg), size, 6, None, 0.0, 200_000, args.runs)
        blocks = os.path.join(tmp, "blocks")
        write_blocks(pkg, blocks)
        g0 = pkg.Gpu(0)
        path = os.path.join(tmp, "world")
        t = time.perf_counter()
        pkg.World.generate_world(path, pkg.Procedural(g0), world_depth=1, chunk_depth=args.chunk_depth, blocks_dir=blocks)
        g0.close()
        say(f"# generate_world(world_depth=1, chunk_depth={args.chunk_depth}): {time.perf_counter() - t:.1f} s")
        both_ways(pkg, say, "generated world, every chunk resident", lambda: open_world(pkg, path, blocks), size, args.expand_depth, CAM,
                  args.lod, args.max_words, args.runs)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
