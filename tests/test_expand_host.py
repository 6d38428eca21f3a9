"""svo_adaptive_expand without a GPU: the ABI is there, and the two statements its kernels rest on hold on
the host -- the candidate rule restated in float32 picks exactly the leaves svo_world_expand refines, and the host's
frontier walk equals process_subdivision fed one sorted candidate list per level, cut by the word cap."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pass_frame import monu9_world

VOXEL_OFFSET = 1 << 27

# (max_depth, cam, lod_c, max_words)
CASES = [
    (6, None, 0.0, 1 << 27),
    (8, (0.3, 0.4, -1.6), 40.0, 1 << 27),
    (7, (0.1, 0.2, -1.5), 12.0, 1 << 27),
    (6, None, 0.0, 5000),   # the cap ends on a level boundary
    (6, None, 0.0, 4001),   # the cap cuts a level
    (7, (0.1, 0.2, -1.5), 12.0, 300),
]


def refines(pos, depth, cam, lod_c):
    """The rule of svo_world_expand for one leaf, every operation rounded to float32 on its own."""
    f = np.float32
    h = f(1.0) / f(1 << depth)
    d2 = f(0.0)
    for k in range(3):
        c, ck = f(pos[k]), f(cam[k])
        lo, hi = f(c - h), f(c + h)
        d = f(lo - ck) if ck < lo else (f(ck - hi) if ck > hi else f(0.0))
        d2 = f(d2 + f(d * d))
    return bool(f(f(1 << depth) * np.sqrt(d2, dtype=np.float32)) < f(lod_c))


def leaves_with_depth(octree):
    words = octree.raw_data()
    return [(int(i), octree.find_voxel(octree.position(int(i)))[1]) for i in np.nonzero((words >> 4) >= VOXEL_OFFSET)[0]]


def expand_by_levels(pkg, world, octree, max_depth, cam, lod_c, max_words, seen=None):
    """svo_adaptive_expand's decomposition with the host's own list processing: per level the sorted candidate list, of
    which only the entries before the (S_max + 1)-th success are applied."""
    frontier = leaves_with_depth(octree)
    done = 0
    while frontier:
        s_max = (max_words - len(octree)) // 8 if max_words > len(octree) else 0
        if s_max == 0:
            return done
        pos = octree.positions()
        cand = [(i, d) for i, d in frontier if d < max_depth and (cam is None or not lod_c > 0 or refines(pos[i], d, cam, lod_c))]
        if seen is not None:
            seen.append(cand)
        lst = np.array([i for i, _ in cand], dtype=np.uint32)
        assert np.all(np.diff(lst.astype(np.int64)) > 0), "a frontier is not ascending"
        before = len(octree)
        if lst.size <= s_max:
            n = pkg.adaptive.process_subdivision(lst, octree, world)
        else:  # the entries before the (s_max + 1)-th success, found by feeding them one at a time
            n = 0
            for i in lst:
                if n >= s_max:
                    break
                n += pkg.adaptive.process_subdivision(np.array([i], dtype=np.uint32), octree, world)
        done += n
        words = octree.raw_data()
        frontier = []
        for i, d in cand:
            p = int(words[i] >> 4)
            if before <= p < VOXEL_OFFSET:
                frontier += [(p + k, d + 1) for k in range(8)]
        assert [i for i, _ in frontier] == list(range(before, len(octree))), "fresh groups are not appended in list order"
    return done


def test_abi_exports_and_signatures(pkg):
    lib = pkg._lib.lib()
    for name in ("svo_adaptive_expand", "svo_adaptive_expand_timing"):
        assert name in pkg._lib.DEVICE_SYMBOLS
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.svo_adaptive_expand.argtypes) == 6
    header = open(os.path.join(ROOT, "include", "svo_hip.h")).read()
    assert re.search(r"int svo_adaptive_expand\(svo_ctx \*ctx, uint32_t max_depth, const float cam\[3\], float lod_c,\s*"
                     r"uint64_t max_words,\s*svo_adaptive_result \*out\);", header)
    assert "#define SVO_ADAPT_TIMES 4" in header and "#define SVO_ADAPT_EXPAND_TIMES 5" in header
    assert "adaptive_expand" in open(os.path.join(ROOT, "include", "svo_render.hpp")).read()
    assert "svo_adaptive_expand" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for cls, name in ((pkg.adaptive.DeviceAdaptive, "expand"), (pkg.Render, "from_world")):
        assert callable(getattr(cls, name))
    # a context without an attached state refuses with a message, it does not crash
    assert lib.svo_adaptive_expand(None, 4, None, 0.0, 0, None) == -1


def node_depths(words):
    """Depth of every node from the tree's own structure (the root group is depth 1)."""
    depth = np.zeros(words.size, dtype=np.int64)
    depth[:8] = 1
    for i in range(words.size):  # (groups lie behind their parents: svo_world_expand appends)
        p = int(words[i] >> 4)
        if p < VOXEL_OFFSET:
            assert p > i
            depth[p:p + 8] = depth[i] + 1
    return depth


@pytest.mark.parametrize("max_depth,cam,lod_c", [c[:3] for c in CASES[1:3]])
def test_candidate_rule_restated_in_float32(pkg, max_depth, cam, lod_c):
    """In the tree World.expand leaves, every node it refined passes the restated rule, every leaf above max_depth that
    the host could still refine fails it, and the leaves that pass it are the ones the world cannot refine."""
    world = monu9_world(pkg)
    octree = world.root_octree()
    assert world.expand(octree, max_depth, cam=cam, lod_c=lod_c) > 0
    words, pos = octree.raw_data(), octree.positions()
    depth = node_depths(words)
    assert all(d == depth[i] for i, d in leaves_with_depth(octree))
    interior = np.nonzero((words >> 4) < VOXEL_OFFSET)[0]
    assert all(depth[i] < max_depth and refines(pos[i], int(depth[i]), cam, lod_c) for i in interior)
    leaves = [i for i in np.nonzero((words >> 4) >= VOXEL_OFFSET)[0] if depth[i] < max_depth]
    passing = [i for i in leaves if refines(pos[i], int(depth[i]), cam, lod_c)]
    refused = [i for i in leaves if not refines(pos[i], int(depth[i]), cam, lod_c)]
    assert len(refused) > 10
    assert pkg.adaptive.process_subdivision(np.array(passing, dtype=np.uint32), octree, world) == 0
    # the refused ones are refused by the rule alone: without it the host refines among them
    assert pkg.adaptive.process_subdivision(np.array(refused, dtype=np.uint32), octree, world) > 0


@pytest.mark.parametrize("max_depth,cam,lod_c,max_words", CASES)
def test_levels_reproduce_world_expand(pkg, max_depth, cam, lod_c, max_words):
    wa, wb = monu9_world(pkg), monu9_world(pkg)
    oa, ob = wa.root_octree(), wb.root_octree()
    na = wa.expand(oa, max_depth, cam=cam, lod_c=lod_c, max_words=max_words)
    seen = []
    nb = expand_by_levels(pkg, wb, ob, max_depth, cam, lod_c, max_words, seen)
    assert na > 0 and na == nb
    assert len(oa) == len(ob) and len(oa) <= max(max_words, 8)
    assert np.array_equal(oa.raw_data(), ob.raw_data())
    assert np.array_equal(oa.positions().view(np.uint32), ob.positions().view(np.uint32))
    assert np.array_equal(oa.hole_stack(), ob.hole_stack()) and oa.hole_stack().size == 0
    assert wa.chunk_ids() == wb.chunk_ids()
    assert len(seen) >= 2  # (more than one level, so the next-frontier rule is exercised)


def test_issue_counts(pkg):
    """The sizes the GPU cases run at (so an empty case cannot pass unnoticed)."""
    got = []
    for max_depth, cam, lod_c, max_words in CASES[:5]:
        world = monu9_world(pkg)
        octree = world.root_octree()
        got.append((world.expand(octree, max_depth, cam=cam, lod_c=lod_c, max_words=max_words), len(octree)))
    assert got == [(1831, 14656), (461, 3696), (68, 552), (624, 5000), (499, 4000)]
