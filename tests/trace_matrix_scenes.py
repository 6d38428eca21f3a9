"""Inputs for the trace-kernel matrix (tests/test_trace_matrix_host.py, tests/test_trace_matrix_gpu.py): small deep trees and
cameras whose every ray starts on a tie.

`>` and `>=` (SVO_F_MISC_BOOL, shader.wgsl:138-150) pick different children only when a position component equals a cell centre
exactly; a perspective camera of oracle_camera almost never stands there.  So the trees here are clusters of random voxels in a
16^3 box of depth-D cells next to the cube's centre, and the cameras are written by hand: the origin is a corner of depth-D cells
a few cells in front of the cluster -- a small integer times 2^-(D-1), exact in f32 -- which is the centre of the level D-1 cell
around it on every axis (the tie at level D), and the centre of coarser cells wherever the integer is even.  The camera is inside
the cube: no culling pass.  D = 16 is the last depth the default ancestor stack resolves, 17 the first of the deep one, 21 the
deepest tree build_ref.morton can key (3 * D bits in a uint64).
"""
import itertools

import numpy as np

import build_ref

DEPTHS = (16, 17, 20, 21)
SIZE = (96, 64)
BOX_OFFSET = (40, -24, 8)     # the box's low corner, in depth-D cells from the cube's centre
BOX_SIDE = 16
FILL = 0.08
ORIGIN_IN_BOX = (-6, 5, 7)    # the camera's corner, in cells from the box's low corner: 6 cells in front of the face x = 0
SUN = (-1.0, -0.6, 0.3, 0.0)
FORWARD, RIGHT, UP = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)
TWO_AXIS_TIES = (0b000101, 0b000110, 0b001001, 0b001010, 0b010001, 0b010010,
                 0b100001, 0b100010, 0b010100, 0b011000, 0b100100, 0b101000)  # normal_bits of a step that ties on two axes


def lattice_camera_inverse(origin, forward=FORWARD, right=RIGHT, up=UP):
    """kat_cases.one_ray_camera_inverse for a W x H frame: camera_inverse (column-major) with column 3 = (origin, 1),
    column 2 = (forward, 0), columns 0 and 1 = (right, 0) and (up, 0).  Every w is 1, so (shader.wgsl:54-59, 253-259) every
    ray starts at exactly `origin`, and the ray of the pixel whose centre is clip (cx, cy) has the direction
    normalize(right * cx + up * cy + forward): a 90 degree frustum for axes of length 1, the same for any frame size."""
    m = np.zeros(16, dtype=np.float32)
    m[0:3] = right
    m[4:7] = up
    m[8:11] = forward
    m[12:15] = origin
    m[15] = 1.0
    return m


class Scene:
    """one depth: the voxels, their tree, and the lattice camera in front of them"""

    def __init__(self, depth):
        assert depth in DEPTHS
        self.depth = depth
        half = 1 << (depth - 1)
        self.box = np.array([half + o for o in BOX_OFFSET], dtype=np.int64)
        rng = np.random.default_rng(depth)
        cells = np.argwhere(rng.random((BOX_SIDE,) * 3) < FILL)
        self.coords = self.box + cells
        self.colours = rng.integers(1, 1 << 24, cells.shape[0])
        self.words = build_ref.build(self.coords, depth, self.colours)
        self.words.setflags(write=False)
        # the corner: cell index c stands at -1 + c * 2^-(D-1), so (c - 2^(D-1)) * 2^-(D-1) from the centre
        corner = self.box + np.array(ORIGIN_IN_BOX) - half
        exact = corner.astype(np.float64) * 2.0 ** -(depth - 1)
        self.origin = exact.astype(np.float32)
        assert np.array_equal(self.origin.astype(np.float64), exact), "the origin must be exact in f32"
        assert np.array_equal(self.origin.astype(np.float64) * 2.0 ** (depth - 1), corner), "and a corner of depth-D cells"
        assert np.abs(self.origin).max() < 1.0
        self.camera_inverse = lattice_camera_inverse(self.origin)

    def uniforms(self, O, flags, size=SIZE):
        """the oracle's Uniforms of this camera; `camera` (used by nobody who traces) is the inverse's inverse"""
        u = O.Uniforms()
        inv = self.camera_inverse.reshape(4, 4).T.astype(np.float64)
        u.camera[:] = np.linalg.inv(inv).T.reshape(-1).astype(np.float32).tolist()
        u.camera_inverse[:] = self.camera_inverse.tolist()
        u.dimensions[:] = [float(size[0]), float(size[1]), 0.0, 0.0]
        u.sun_dir[:] = list(SUN)
        u.flags = flags
        u.misc_value = 0.0
        return u

    def lattice_rays(self, n=3000):
        """test_lattice_rays_ties_and_boundaries' rays at this depth: origins on the 2^-(D-1) lattice in and around the
        box (a third of them moved to cell centres, odd multiples of 2^-D; every fiftieth outside the cube), directions along
        axes, face and space diagonals with bit-equal components.  (n, 6) float32."""
        depth = self.depth
        dirs = []
        for d in itertools.product((-1.0, 0.0, 1.0), repeat=3):
            if any(d):
                v = np.array(d, dtype=np.float32)
                dirs.append(v / np.float32(np.sqrt(np.float32((v * v).sum()))))  # equal components stay bit-equal
        dirs = np.array(dirs, dtype=np.float32)
        rng = np.random.default_rng(1000 + depth)
        half = 1 << (depth - 1)
        k = (self.box - half + rng.integers(-4, BOX_SIDE + 5, (n, 3))).astype(np.float64)
        k[::3] += 0.5
        org = (k * 2.0 ** -(depth - 1)).astype(np.float32)
        assert np.array_equal(org.astype(np.float64) * 2.0 ** depth, k * 2), "lattice origins must be exact in f32"
        d = dirs[rng.integers(0, len(dirs), n)]
        org[::50] -= np.float32(1.5) * np.sign(d[::50])  # outside, looking back at the cluster (rounded to f32: any value will do)
        return np.concatenate([org, d], axis=1).astype(np.float32)


_scenes = {}


def scene(depth):
    """the scene of `depth`, built once"""
    if depth not in _scenes:
        _scenes[depth] = Scene(depth)
    return _scenes[depth]


def flags_of(O, ge, cnt, shd):
    """the uniforms' flags that select a cell: GE = misc_bool, CNT = counters live (pause_adaptive clear), SHD = shadows"""
    return (O.F_MISC_BOOL if ge else 0) | (0 if cnt else O.F_PAUSE_ADAPTIVE) | (O.F_SHADOWS if shd else 0)
