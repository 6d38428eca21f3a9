"""A sequential restatement of the surface pass's contract (include/svo_hip.h, csrc/svo_surface.hip) over
GPU-layout words.

face_masks()    the entries of list_ref.list_voxels (flags 0) and, per entry, the 6-bit mask of its exposed faces: for
                face f the cell behind it on the voxel's own level is looked up by a plain walk from group 0, as the
                sampler walks; a voxel word met on the way covers the face, the empty word and a word that is still
                interior on the voxel's level expose it; a cell outside the grid exposes it unless the boundary is closed.
select()        the three modes of svo_nodes_list_surface from those: (xyz, value, level, face).
list_surface()  the two in one call.

Both raise what list_ref.list_voxels raises.
"""
import numpy as np

import list_ref as L
from build_ref import VOXEL_OFFSET

CLOSED_BOUNDARY, KEEP_HIDDEN, QUADS = 1, 2, 4


def covered(w, cell, level):
    """the walk from group 0 towards `cell` of the level-`level` grid stops on a voxel word"""
    group = 0
    for l in range(1, level + 1):
        shift = level - l
        child = (cell[0] >> shift & 1) << 2 | (cell[1] >> shift & 1) << 1 | (cell[2] >> shift & 1)
        pointer = w[group + child] >> 4
        if pointer >= VOXEL_OFFSET:
            return pointer > VOXEL_OFFSET
        group = pointer
    return False  # interior at `level`: the neighbour is finer


def face_masks(words, n_words, depth, closed=False):
    xyz, value, level = L.list_voxels(words, n_words, depth)
    w = [int(x) for x in np.asarray(words, dtype=np.uint32)[:n_words]]
    masks = np.zeros(value.size, dtype=np.uint32)
    for i in range(value.size):
        l = int(level[i])
        cell = [int(v) >> (depth - l) for v in xyz[i]]
        for f in range(6):
            n = list(cell)
            n[f >> 1] += 1 if f & 1 else -1
            if not 0 <= n[f >> 1] < 1 << l:
                exposed = not closed
            else:
                exposed = not covered(w, n, l)
            masks[i] |= int(exposed) << f
    return xyz, value, level, masks


def select(entries, flags):
    """(xyz, value, level, face) of the mode `flags` names, from face_masks' result for the same boundary"""
    if flags & ~(CLOSED_BOUNDARY | KEEP_HIDDEN | QUADS) or (flags & QUADS and flags & KEEP_HIDDEN):
        raise ValueError(f"unknown or incompatible flag bits {flags}")
    xyz, value, level, masks = entries
    if flags & QUADS:
        bits = (masks[:, None] >> np.arange(6, dtype=np.uint32)) & 1
        voxel, face = np.nonzero(bits)  # row-major: the voxels in order, a voxel's faces ascending
        return xyz[voxel], value[voxel], level[voxel], face.astype(np.uint32)
    keep = np.ones(masks.size, dtype=bool) if flags & KEEP_HIDDEN else masks != 0
    return xyz[keep], value[keep], level[keep], masks[keep]


def list_surface(words, n_words, depth, flags=0):
    select((np.zeros((0, 3), dtype=np.uint32),) + (np.zeros(0, dtype=np.uint32),) * 3, flags)  # (the flags come first)
    return select(face_masks(words, n_words, depth, bool(flags & CLOSED_BOUNDARY)), flags)
