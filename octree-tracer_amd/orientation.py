"""The cube's 48 symmetries as Render.place_nodes and svo_nodes_place number them (include/svo_hip.h).

orient = 8 p + 4 fx + 2 fy + fz: p indexes the axis permutations in lexicographic order (PERMS), and the oriented source has at
cell r what the source has at cell q with r[i] = S - 1 - q[perm[i]] when f_i is set and q[perm[i]] otherwise, S the side of the
source's cube.  The source is turned about its own cube: the cube stays where it is, its content moves.  0 is the identity; 24
of the 48 are rotations, the other 24 mirror.
"""
import itertools

PERMS = tuple(itertools.permutations(range(3)))  # lexicographic: (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0)


def orientation(perm=(0, 1, 2), flips=(False, False, False)):
    """the number of the symmetry r[i] = flips[i] ? S - 1 - q[perm[i]] : q[perm[i]]"""
    perm = tuple(int(v) for v in perm)
    if perm not in PERMS:
        raise ValueError(f"perm must be a permutation of (0, 1, 2), got {perm!r}")
    if len(flips) != 3:
        raise ValueError(f"flips must be three flags, got {flips!r}")
    return 8 * PERMS.index(perm) + 4 * bool(flips[0]) + 2 * bool(flips[1]) + bool(flips[2])


def _matrix(orient):
    """the signed permutation matrix m of a number, r - c = m (q - c) about the cube's centre c: m[i][perm[i]] = -1 where f_i
    is set, else 1"""
    orient = int(orient)
    if not 0 <= orient < 48:
        raise ValueError(f"orient must be 0..47 (got {orient})")
    perm = PERMS[orient >> 3]
    return [[(-1 if orient >> (2 - i) & 1 else 1) if j == perm[i] else 0 for j in range(3)] for i in range(3)]


def from_matrix(m):
    """the number of a signed 3 x 3 permutation matrix m (every row one entry of 1 or -1, every column used once): the
    symmetry that takes a direction d of the source to m d"""
    rows = [[int(v) for v in row] for row in m]
    if len(rows) != 3 or any(len(row) != 3 for row in rows):
        raise ValueError("m must be 3 x 3")
    perm, flips = [], []
    for row in rows:
        set_at = [j for j in range(3) if row[j]]
        if len(set_at) != 1 or abs(row[set_at[0]]) != 1:
            raise ValueError(f"every row of m must hold one entry of 1 or -1, got {row!r}")
        perm.append(set_at[0])
        flips.append(row[set_at[0]] < 0)
    if sorted(perm) != [0, 1, 2]:
        raise ValueError("m must use every column once")
    return orientation(perm, flips)


def quarter_turns_y(k):
    """k quarter turns about +y as Render.stamp_structures' `rots` count them: one takes an offset (dx, dy, dz) to
    (dz, dy, -dx)"""
    m = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    for _ in range(int(k) % 4):
        m = [m[2], m[1], [-v for v in m[0]]]  # (the turn applied to what m gives)
    return from_matrix(m)


def is_rotation(orient):
    """whether the symmetry is a rotation (determinant 1: 24 of the 48) and not a mirror image"""
    m = _matrix(orient)
    det = sum(m[0][i] * (m[1][(i + 1) % 3] * m[2][(i + 2) % 3] - m[1][(i + 2) % 3] * m[2][(i + 1) % 3]) for i in range(3))
    return det == 1
