"""Voxel listing timings: per phase (HIP events: discover, count, offsets, emit) of the fill, and wall time of
the count query and of the fill, of Render.list_voxels' two library calls on tools/compact_probe.py's scene -- the depth-12
height field of tools/build_probe.py after tools/edit_probe.py's 1 000 000-voxel edit -- in put order and compacted,
medians of --reps warm calls; next to the way there was before, read_nodes + the host walk (tests/list_ref.py:
list_voxels, sequential, run once; list_parallel, its numpy form), in the same process.  Checks that both layouts list
identical bytes, that the host walk gives the same list, and that build_nodes of the list equals compact_nodes(prune=True).
Asserts no time.

    python tools/list_probe.py [--out profiles/list_probe.log] [--reps 5]
"""
import argparse
import ctypes as C
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
import list_ref as L  # noqa: E402
from build_probe import height_field  # noqa: E402
from edit_probe import DEPTH, edit_list  # noqa: E402

PHASES = ("discover", "count", "offsets", "emit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_probe.log"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    lib = pkg._lib.lib()
    gpu = pkg.Gpu(0)
    dev = torch.device("cuda", 0)
    render = pkg.Render(gpu, (64, 64), np.full(8, B.EMPTY, dtype=np.uint32), capacity=1 << 27)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    coords, colours = height_field(1, DEPTH, 3200)
    ec, ecol = edit_list(np.random.default_rng(16), coords, 1_000_000)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.int32)  # noqa: E731
    base_c, base_col, c, col = to_dev(coords), to_dev(colours), to_dev(ec), to_dev(ecol)
    torch.cuda.synchronize()
    render.build_nodes(base_c, DEPTH, base_col)
    render.edit_nodes(c, DEPTH, col)

    def call(p, *outs):
        n = C.c_uint64()
        t0 = time.perf_counter()
        gpu.check(lib.svo_nodes_list_voxels(gpu._h, C.byref(p), *[o.data_ptr() if o is not None else None for o in outs], C.byref(n)))
        gpu.sync()
        return n.value, (time.perf_counter() - t0) * 1e3

    log(f"# voxels listed from the depth-{DEPTH} height field ({coords.shape[0]} voxels) after a {ec.shape[0]}-voxel edit "
        f"({int((ecol == 0).sum())} removed): HIP events of the fill, wall of the count query and of the fill, median of {args.reps} warm calls, ms")
    log(f"{'layout':>9s} {'words':>10s} {'entries':>10s} " + " ".join(f"{p:>9s}" for p in PHASES) + f" {'device':>8s} {'count q.':>8s} {'fill':>8s}")
    lists = {}
    for layout in ("put order", "compacted"):
        if layout == "compacted":
            render.compact_nodes(prune=False)
        p = pkg._lib.ListParams()
        p.flags, p.depth, p.n_words = 0, DEPTH, render.node_length
        n, _ = call(p, None, None, None)
        xyz = torch.empty((n, 3), dtype=torch.int32, device=dev)
        value, level = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        p.max_voxels = n
        times, query, fill = [], [], []
        for rep in range(args.reps + 1):  # (the first is the warm-up: workspace, code objects)
            _, q = call(p, None, None, None)
            _, f = call(p, xyz, value, level)
            if rep:
                query.append(q)
                fill.append(f)
                times.append(gpu.list_timing())
        lists[layout] = tuple(t.cpu().numpy().view(np.uint32) for t in (xyz, value, level))
        ms = np.median(np.array(times), axis=0)
        log(f"{layout:>9s} {render.node_length:10d} {n:10d} " + " ".join(f"{t:9.3f}" for t in ms[:4]) +
            f" {float(ms[:4].sum()):8.3f} {float(np.median(query)):8.3f} {float(np.median(fill)):8.3f}")
    same = all(a.tobytes() == b.tobytes() for a, b in zip(lists["put order"], lists["compacted"]))
    log(f"# both layouts list identical bytes: {same}")

    # the way there was before: the words over PCIe and a walk on the host
    t0 = time.perf_counter()
    words = render.read_nodes()
    t1 = time.perf_counter()
    numpy_form = L.list_parallel(words, words.size, DEPTH)
    t2 = time.perf_counter()
    log(f"# read_nodes + list_ref.list_parallel (numpy): {(t1 - t0) * 1e3:.1f} + {(t2 - t1) * 1e3:.1f} ms")
    walked = L.list_voxels(words, words.size, DEPTH)
    t3 = time.perf_counter()
    log(f"# read_nodes + list_ref.list_voxels (sequential walk, one run): {(t1 - t0) * 1e3:.1f} + {(t3 - t2) * 1e3:.1f} ms")
    host = all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(lists["compacted"], walked, numpy_form))
    log(f"# the host walks give the device's list: {host}")

    # the loop closed: the list rebuilds the pruned tree
    n_pruned = render.compact_nodes(prune=True)
    pruned = render.read_nodes()
    coords_dev, colours_dev = render.list_voxels(DEPTH)
    t0 = time.perf_counter()
    n_built = render.build_nodes(coords_dev, DEPTH, colours_dev)
    built_ms = (time.perf_counter() - t0) * 1e3
    rebuilt = n_built == n_pruned and np.array_equal(render.read_nodes(), pruned)
    log(f"# build_nodes of the list ({coords_dev.shape[0]} voxels, {built_ms:.3f} ms wall) == compact_nodes(prune=True) ({n_pruned} words): {rebuilt}")
    gpu.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not (same and host and rebuilt):
        sys.exit("the lists differ")


if __name__ == "__main__":
    main()
