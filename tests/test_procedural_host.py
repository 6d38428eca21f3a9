"""Procedural world generator, CPU side: the numpy checker's building blocks at hand-derived points,
the canonical breadth-first tree on a hand-written grid, and the chunk order / root references of generate_world."""
import numpy as np
import pytest

import proc_ref as R

F = np.float32
CO = R.CHUNK_OFFSET


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_box_at_hand_derived_points():
    s = (F(0.7), F(0.1), F(0.7))
    # inside: the nearest face is the top one, at distance 0.1
    assert bits(R.box(F(0), F(0), F(0), *s)) == bits(-F(0.1))
    # outside one face: distance along x only
    assert bits(R.box(F(1), F(0), F(0), *s)) == bits(F(1) - F(0.7))
    # outside an edge: Euclidean distance to it
    d = R.box(F(1), F(1), F(0), *s)
    assert abs(float(d) - np.hypot(0.3, 0.9)) < 1e-6
    assert R.box(F(-1), F(-1), F(0), *s) == d  # |p|


def test_cone_at_hand_derived_points():
    c = (F(0.5), F(0.5), F(0.9))
    assert R.cone(F(0), F(0), F(0), *c) == 0  # the apex
    assert R.cone(F(0), F(-0.9), F(0), *c) == 0  # centre of the base disc
    # on the axis, 0.45 below the apex: inside, 0.45 / sqrt(2) from the 45-degree slant
    d = R.cone(F(0), F(-0.45), F(0), *c)
    assert d < 0 and abs(float(d) + 0.45 / np.sqrt(2)) < 1e-6
    # above the apex: outside, distance to the apex
    assert abs(float(R.cone(F(0), F(0.5), F(0), *c)) - 0.5) < 1e-6
    # the cone is round: rotating x into z changes nothing
    assert bits(R.cone(F(0.3), F(-0.6), F(0), *c)) == bits(R.cone(F(0), F(-0.6), F(0.3), *c))


def test_smin_and_smoothstep_at_hand_derived_points():
    k = F(0.2)
    assert bits(R.smin(F(1), F(1), k)) == bits(F(1) - (k * F(0.5)) * F(0.5))  # h = 1/2: 1 - k/4
    assert R.smin(F(0), F(1), k) == 0 and R.smin(F(1), F(0), k) == 0  # far apart: plain min
    assert R.smin(F(0.3), F(0.35), k) < F(0.3)  # close: below both
    assert R.smoothstep(F(0), F(-1.5), F(0)) == 0
    assert R.smoothstep(F(0), F(-1.5), F(-1.5)) == 1
    assert R.smoothstep(F(0), F(-1.5), F(-0.75)) == F(0.5)  # edge0 > edge1: falls towards -y
    assert R.smoothstep(F(0), F(-1.5), F(1)) == 0
    assert R.smoothstep(F(0), F(0.2), F(0.1)) == F(0.5)
    assert R.smoothstep(F(0), F(0.2), F(0.05)) == F(0.25) * F(0.25) * (F(3) - F(2) * F(0.25))
    assert R.sign(F(0)) == 0 and R.sign(F(-0.0)) == 0 and R.sign(F(-2)) == -1


def test_sdf_stays_float32_and_has_an_island():
    xs = np.linspace(-1, 1, 41, dtype=np.float32)
    X, Y, Z = np.meshgrid(xs, xs, xs, indexing="ij")
    v = R.sdf(X.ravel(), Y.ravel(), Z.ravel())
    assert v.dtype == np.float32
    solid = v < 0
    assert 0 < solid.mean() < 0.5
    assert R.sdf(F(0), F(0.9), F(0)) > 0 and R.sdf(F(0), F(0), F(0)) < 0  # air above the island, rock inside


def test_breadth_first_tree_of_a_hand_written_grid():
    """chunk_depth 2 (4^3 cells): stone at (0,0,0) and (1,0,0), grass at (3,3,3)."""
    cls = np.zeros(64, dtype=np.uint8)  # id order x + 4y + 16z
    cls[0 + 0 + 0], cls[1], cls[3 + 4 * 3 + 16 * 3] = 1, 1, 3
    words = R.build_tree(R.to_morton(cls, 2), 2)
    want = ([8, CO, CO, CO, CO, CO, CO, 16] +          # root group: children 0 and 7 are interior
            [CO + 1, CO, CO, CO, CO + 1, CO, CO, CO] +  # child 0's group: (0,0,0) at 0, (1,0,0) at x*4 = 4
            [CO, CO, CO, CO, CO, CO, CO, CO + 3])       # child 7's group: (3,3,3) at 7
    assert words.tolist() == want
    side = np.arange(64)
    x, y, z = side % 4, side // 4 % 4, side // 16
    assert np.array_equal(R.descend(words, 2, x, y, z), cls)
    assert R.build_tree(np.zeros(64, dtype=np.uint8), 2) is None


def test_tree_shape_is_what_sequential_insertion_builds(pkg):
    """The canonical tree has exactly the nodes put_in_voxel's sequential insertion creates (procedual.wgsl:91-107 ==
    CpuOctree.put_in_block), only in breadth-first order."""
    rng = np.random.default_rng(3)
    depth = 4
    side = 1 << depth
    cls = np.where(rng.random(side ** 3) < 0.03, rng.choice([1, 3], side ** 3), 0).astype(np.uint8)
    words = R.build_tree(R.to_morton(cls, depth), depth)
    tree = pkg.CpuOctree.new(0)
    ids = np.flatnonzero(cls)
    for i in ids.tolist():
        x, y, z = i % side, i // side % side, i // side // side
        tree.put_in_block([float(F(c) / F(side) * F(2) - F(1)) for c in (x, y, z)], int(cls[i]), depth)
    assert len(tree) == words.size
    ptr, _ = tree.raw()
    for i in ids.tolist():
        x, y, z = i % side, i // side % side, i // side // side
        idx, d, _ = tree.find_voxel([(c + 0.5) / side * 2 - 1 for c in (x, y, z)])
        assert d == depth and ptr[idx] == CO + int(cls[i])
    everything = np.arange(side ** 3)
    assert np.array_equal(R.descend(words, depth, everything % side, everything // side % side, everything // side // side), cls)


@pytest.mark.parametrize("world_depth", [1, 2])
def test_chunk_order_and_root_references(pkg, world_depth):
    layout = pkg.procedural.chunk_layout(world_depth)
    assert layout == [(i, cid, tuple(float(c) for c in pos)) for i, cid, pos in R.chunk_layout(world_depth)]
    n = 1 << world_depth
    assert [cid for _, cid, _ in layout] == [CO // 2 + i for i in range(n ** 3)]
    # x outermost, z innermost (world.rs:102-104)
    assert layout[1][2][2] > layout[0][2][2] and layout[n][2][1] > layout[0][2][1] and layout[n * n][2][0] > layout[0][2][0]
    root = pkg.CpuOctree.new(0)
    for _, cid, pos in layout:
        root.put_in_block(pos, cid, world_depth)
    assert len(root) == 8 * sum(8 ** k for k in range(world_depth))
    ptr, _ = root.raw()
    edge = 2.0 / n
    for _, cid, pos in layout:  # the lower corner puts the reference into the chunk's own cube
        centre = [c + edge / 2 for c in pos]
        idx, d, node_pos = root.find_voxel(centre)
        assert d == world_depth and ptr[idx] == CO + cid
        assert np.allclose(node_pos, centre)


def test_generate_world_refuses_an_existing_path(pkg, tmp_path):
    with pytest.raises(ValueError, match="already exists"):
        pkg.World.generate_world(str(tmp_path), None)
