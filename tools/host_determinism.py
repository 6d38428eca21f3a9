"""Host results of two builds of the library, byte for byte (no GPU): the calls whose arithmetic lives in csrc/svo_rules.h.

    SVO_HIP_LIB=/path/to/other/libsvo_hip.so python tools/host_determinism.py --dump DIR_A
    python tools/host_determinism.py --dump DIR_B            # the library of this tree
    python tools/host_determinism.py --compare DIR_A DIR_B   # exit status 1 when a file differs

Inputs (tests/golden fixtures and fixed parameters):
  expand_K         svo_world_expand on monu9 for every (max_depth, cam, lod_c, max_words) of tests/test_expand_host.py's
                   CASES: words, positions, hole stack, count
  terrain_S, fractal_S   svo_gen_terrain (max_depth 12, min_depth 4) and svo_gen_fractal (max_depth 14, min_depth 3) at
                   seeds 3 and 11, cam (0.31, 0.12, -0.4), lod_c 600, at most 4 M words: the words
  find_monu9       svo_world_find_voxel on monu9 over the lattice k / 8, k = -8 .. 8 per axis (every centre plane of the
                   first three levels, so p == centre ties on one, two and three axes) plus the neighbouring floats of
                   each lattice value, for max_depth none, 1, 3 and 6: status, chunk, index, depth, node position
  find_blocks      the same lattice on a root whose leaves reference chunk 5 (resident, itself referencing the missing
                   chunk 9) and chunk 7 (missing): the walks that hop and the ones that fail
"""
import argparse
import ctypes as C
import filecmp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

CAM = (0.31, 0.12, -0.4)


def monu9_world(pkg):
    z = np.load(os.path.join(ROOT, "tests", "golden", "monu9_vox.npz"))
    return pkg.adaptive.World(pkg.CpuOctree.from_voxels(int(z["size"][0]), z["xyzi"], z["palette"]))


def blocks_world(pkg):
    root, inner = pkg.CpuOctree.new(0), pkg.CpuOctree.new(0)
    root.put_in_block((0.5, 0.5, 0.5), 5, 1)
    root.put_in_block((-0.25, -0.25, -0.25), 5, 2)
    root.put_in_block((-0.5, 0.5, 0.5), 7, 1)
    inner.put_in_voxel((0.25, 0.25, 0.25), pkg.cpu_octree.Voxel(10, 20, 30), 3)
    inner.put_in_block((-0.5, -0.5, -0.5), 9, 1)
    world = pkg.World()  # (no mips: chunk 7 and 9 are missing on purpose)
    world.insert(0, root)
    world.insert(5, inner)
    return world


def lattice():
    axis = []
    for k in range(-8, 9):
        v = np.float32(k / 8.0)
        axis += [np.nextafter(v, np.float32(-2)), v, np.nextafter(v, np.float32(2))]
    axis = np.array(axis, dtype=np.float32)
    return np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)


def find_all(pkg, world, points):
    lib = pkg._lib.lib()
    rows = np.zeros((4, len(points)), dtype=[("rc", "i4"), ("chunk", "u4"), ("index", "u8"), ("depth", "u4"), ("pos", "u4", 3)])
    ch, idx, d, out = C.c_uint32(), C.c_uint64(), C.c_uint32(), (C.c_float * 3)()
    for m, max_depth in enumerate((-1, 1, 3, 6)):
        for i, p in enumerate(points):
            rc = lib.svo_world_find_voxel(world._h, (C.c_float * 3)(*p), max_depth, C.byref(ch), C.byref(idx), C.byref(d), out)
            rows[m, i] = (rc, ch.value, idx.value, d.value, np.array(out, dtype=np.float32).view(np.uint32))
    return rows


def dump(out):
    from test_expand_host import CASES
    pkg = entry.load_package()
    os.makedirs(out, exist_ok=True)
    save = lambda name, a: np.ascontiguousarray(a).tofile(os.path.join(out, name + ".bin"))  # noqa: E731
    for k, (max_depth, cam, lod_c, max_words) in enumerate(CASES):
        world = monu9_world(pkg)
        octree = world.root_octree()
        n = world.expand(octree, max_depth, cam=cam, lod_c=lod_c, max_words=max_words)
        save(f"expand_{k}_words", octree.raw_data())
        save(f"expand_{k}_positions", octree.positions())
        save(f"expand_{k}_holes", np.concatenate([octree.hole_stack().astype(np.uint64), np.array([n], dtype=np.uint64)]))
    for seed in (3, 11):
        save(f"terrain_{seed}", pkg.scenes.terrain(seed=seed, max_depth=12, cam=CAM, lod_c=600.0, min_depth=4, max_words=4_000_000))
        save(f"fractal_{seed}", pkg.scenes.fractal(seed=seed, max_depth=14, cam=CAM, lod_c=600.0, min_depth=3, max_words=4_000_000))
    points = lattice()
    ties = int(np.sum(np.any((points * 8 == np.round(points * 8)), axis=1)))
    mo, bl = find_all(pkg, monu9_world(pkg), points), find_all(pkg, blocks_world(pkg), points)
    save("find_monu9", mo)
    save("find_blocks", bl)
    print(f"{pkg._lib.LIB_PATH}: {len(os.listdir(out))} files in {out}; {len(points)} lattice points, {ties} with a coordinate on a centre "
          f"plane; failing walks: monu9 {int((mo['rc'] != 0).sum())}, blocks {int((bl['rc'] != 0).sum())} of {bl.size}")


def compare(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        same = os.path.exists(pa) and os.path.exists(pb) and filecmp.cmp(pa, pb, shallow=False)
        bad += not same
        print(f"{n:28s} {os.path.getsize(pa) if os.path.exists(pa) else -1:10d} bytes  identical: {same}")
    print("RESULT: " + ("all files identical (names and bytes)" if not bad else f"{bad} files differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
    if args.compare:
        sys.exit(compare(*args.compare))
