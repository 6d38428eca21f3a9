"""What the GPU pass tests share (imported by the test files; no conftest): a context of the module's own, the library's
last error, sentinel-filled device outputs, the depth-7 tree that the compact, list and sample tests edit, and the small
helpers of the world tests.  A helper is here only when every copy it replaces computed the same thing."""
import functools
import os

import numpy as np
import pytest

import build_ref as B
import edit_ref as E
from conftest import GOLDEN, load_vox_fixture

SENTINEL = 0x5EA70000  # what an output holds where nothing was written
SLACK = 64             # entries behind an output's end that must keep the sentinel


@pytest.fixture(scope="module")
def own_gpu(pkg):
    """a context of the importing module's own: its deep trees raise its SVO_OPT_TREE_DEPTH, not the session context's"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg.Gpu(0)
    yield g
    g.close()


def last_error(pkg, gpu):
    return pkg._lib.lib().svo_last_error(gpu._h).decode()


class SentinelOut:
    """int32 device tensors of the given shapes (an entry count or a tuple; None: no tensor), every entry SENTINEL"""

    def __init__(self, gpu, shapes):
        import torch
        dev = torch.device("cuda", gpu.device)
        self.t = [None if s is None else torch.full(s if isinstance(s, tuple) else (s,), SENTINEL, dtype=torch.int32, device=dev)
                  for s in shapes]
        torch.cuda.current_stream(dev).synchronize()

    def host(self):
        return tuple(t.cpu().numpy().view(np.uint32) for t in self.t if t is not None)

    def untouched_from(self, n):
        return all((a[n:] == SENTINEL).all() for a in self.host())


@functools.lru_cache(maxsize=None)
def tree7_base():
    """10 000 random voxels at depth 7 (the two lowest levels have more than 4 096 groups, a scan tile, and group counts
    that fill no whole wave) edited with 4 097 voxels of which a fifth are removed: the lists a and b, the canonical base
    and the edited words in put order.  Computed once per session; the fixtures that add their references copy the dict
    and nobody writes to the arrays."""
    from test_edit_gpu import edit_voxels  # (that module imports this one)
    rng = np.random.default_rng(70)
    a = rng.integers(0, 128, (10000, 3)), rng.integers(1, 1 << 24, 10000)
    b = edit_voxels(rng, 7, 4097, a[0], 0)
    base = B.build(a[0], 7, a[1])
    return {"a": a, "b": b, "base": base, "words": E.edit(base, base.size, b[0], 7, b[1])}


def assert_words(got, want, what):
    assert got.size == want.size, f"{what}: {got.size} words, want {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"


def assert_octrees_equal(a, b, what=""):
    assert len(a) == len(b), f"{what}: lengths {len(a)} != {len(b)}"
    assert np.array_equal(a.raw_data(), b.raw_data()), f"{what}: words differ"
    assert np.array_equal(a.positions().view(np.uint32), b.positions().view(np.uint32)), f"{what}: positions differ"
    assert np.array_equal(a.hole_stack(), b.hole_stack()), f"{what}: hole stacks differ"


def monu9_world(pkg):
    size, xyzi, pal, _, _ = load_vox_fixture("monu9")
    return pkg.adaptive.World(pkg.CpuOctree.from_voxels(size, xyzi, pal))


def write_blocks(pkg, d):
    """blocks/<name>.vox of the 8 block fixtures, as World.new reads them, into the new directory d (str or Path);
    returns the directory as a str"""
    z = np.load(os.path.join(GOLDEN, "blocks_vox.npz"))
    os.makedirs(d)
    for name in B.BLOCKS:
        with open(os.path.join(d, name + ".vox"), "wb") as f:
            f.write(pkg.cpu_octree.vox_write(16, z[name + "_xyzi"], z[name + "_palette"]))
    return str(d)
