"""Independent numpy float32 restatement of the procedural world generator: the signed distance
function, the cell classification and the canonical breadth-first tree.  It is the checker of
octree-tracer_amd/csrc/svo_proc.hip; the product never imports it.

Every literal is an np.float32 and every operation stays in float32 (no float64 promotion): one IEEE f32
operation per step, in the order DESIGN.md 11 pins down."""
import numpy as np

F = np.float32
CHUNK_OFFSET = 2147483648

ZERO, HALF, ONE, TWO, THREE = F(0.0), F(0.5), F(1.0), F(2.0), F(3.0)
C6 = ONE / F(6.0)
C3 = ONE / THREE
C6X2 = TWO * C6
C6X3 = THREE * C6
N7 = ONE / F(7.0)
NSX = N7 * TWO - ZERO
NSY = N7 * HALF - ONE
NSZ = N7 * ONE - ZERO
TAYLOR_A = F(1.79284291400159)
TAYLOR_B = F(0.85373472095314)
M289 = F(289.0)


def _f(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def step(edge, x):
    return (x >= edge).astype(np.float32)


def clamp(x, lo, hi):
    return np.minimum(np.maximum(x, lo), hi)


def sign(x):
    return np.where(x > ZERO, ONE, np.where(x < ZERO, -ONE, ZERO)).astype(np.float32)


def smoothstep(e0, e1, x):
    t = clamp((x - e0) / (e1 - e0), ZERO, ONE)
    return (t * t) * (THREE - TWO * t)


def box(px, py, pz, sx, sy, sz):
    qx, qy, qz = np.abs(px) - sx, np.abs(py) - sy, np.abs(pz) - sz
    mx, my, mz = np.maximum(qx, ZERO), np.maximum(qy, ZERO), np.maximum(qz, ZERO)
    return np.sqrt((mx * mx + my * my) + mz * mz) + np.minimum(np.maximum(np.maximum(qx, qy), qz), ZERO)


def cone(px, py, pz, cx, cy, h):
    qx, qy = h * (cx / cy), h * (-ONE)
    wx, wy = np.sqrt(px * px + pz * pz), py
    t = clamp((wx * qx + wy * qy) / (qx * qx + qy * qy), ZERO, ONE)
    ax, ay = wx - qx * t, wy - qy * t
    t2 = clamp(wx / qx, ZERO, ONE)
    bx, by = wx - qx * t2, wy - qy * ONE
    k = sign(F(qy))
    d = np.minimum(ax * ax + ay * ay, bx * bx + by * by)
    s = np.maximum(k * (wx * qy - wy * qx), k * (wy - qy))
    return np.sqrt(d) * sign(s)


def smin(a, b, k):
    h = clamp(HALF + (HALF * (a - b)) / k, ZERO, ONE)
    return (a * (ONE - h) + b * h) - (k * h) * (ONE - h)


def _permute(x):
    return np.fmod((x * F(34.0) + ONE) * x, M289)


def simplex(vx, vy, vz):
    vx, vy, vz = _f(vx), _f(vy), _f(vz)
    s = (vx * C3 + vy * C3) + vz * C3
    ix, iy, iz = np.floor(vx + s), np.floor(vy + s), np.floor(vz + s)
    t = (ix * C6 + iy * C6) + iz * C6
    x0 = [(vx - ix) + t, (vy - iy) + t, (vz - iz) + t]
    g = [step(x0[1], x0[0]), step(x0[2], x0[1]), step(x0[0], x0[2])]
    lo = [ONE - g[0], ONE - g[1], ONE - g[2]]
    i1 = [np.minimum(g[0], lo[2]), np.minimum(g[1], lo[0]), np.minimum(g[2], lo[1])]
    i2 = [np.maximum(g[0], lo[2]), np.maximum(g[1], lo[0]), np.maximum(g[2], lo[1])]
    x1 = [(x0[a] - i1[a]) + C6 for a in range(3)]
    x2 = [(x0[a] - i2[a]) + C6X2 for a in range(3)]
    x3 = [(x0[a] - ONE) + C6X3 for a in range(3)]
    ix, iy, iz = np.fmod(ix, M289), np.fmod(iy, M289), np.fmod(iz, M289)
    zero = np.zeros_like(vx)
    one = np.ones_like(vx)

    def corners(a):  # vec4(0, i1.a, i2.a, 1)
        return np.stack([zero, i1[a], i2[a], one])

    p = _permute(iz[None] + corners(2))
    p = _permute((p + iy[None]) + corners(1))
    p = _permute((p + ix[None]) + corners(0))
    j = p - F(49.0) * np.floor((p * NSZ) * NSZ)
    xs = np.floor(j * NSZ)
    ys = np.floor(j - F(7.0) * xs)
    gx = xs * NSX + NSY
    gy = ys * NSX + NSY
    h = (ONE - np.abs(gx)) - np.abs(gy)
    sh = -step(h, ZERO)
    ax = gx + (np.floor(gx) * TWO + ONE) * sh
    ay = gy + (np.floor(gy) * TWO + ONE) * sh
    norm = TAYLOR_A - TAYLOR_B * ((ax * ax + ay * ay) + h * h)
    ax, ay, az = ax * norm, ay * norm, h * norm
    xs4 = [x0, x1, x2, x3]
    out = None
    for k in range(4):
        xk = xs4[k]
        m = F(0.6) - ((xk[0] * xk[0] + xk[1] * xk[1]) + xk[2] * xk[2])
        m = np.maximum(m, ZERO)
        m = m * m
        d = (ax[k] * xk[0] + ay[k] * xk[1]) + az[k] * xk[2]
        term = (m * m) * d
        out = term if out is None else out + term
    return F(42.0) * out


def sdf(px, py, pz):
    px, py, pz = _f(px), _f(py), _f(pz)
    v = (ZERO + box(px, py, pz, F(0.7), F(0.1), F(0.7))) - F(0.1)
    s = F(1.6)
    q1 = (px * s, py * s, pz * s)
    q2 = (q1[0] * TWO, q1[1] * TWO, q1[2] * TWO)
    base = simplex(*q1) + HALF * simplex(*q2)
    v = v + F(0.07) * base
    dist = np.sqrt(px * px + pz * pz)
    cn = cone(px * F(1.5) - ZERO, py * F(-1.5) - ONE, pz * F(1.5) - ZERO, HALF, HALF, F(0.9)) - F(0.1)
    v = smin(v, cn, F(0.2))
    q3 = (px * F(2.3), py * F(0.4), pz * F(2.3))
    q4 = (q3[0] * TWO, q3[1] * TWO, q3[2] * TWO)
    spike = simplex(*q3) + HALF * simplex(*q4)
    hb = smoothstep(ZERO, F(-1.5), py) + smoothstep(ZERO, F(0.2), py)
    spike = ((spike + F(1.6) * dist) + hb * TWO) - ONE
    return v + F(0.3) * spike


def world_of_cells(pos, base_depth, chunk_depth, x, y, z):
    """world = pos + (cell / 2^full) * 2"""
    full = F(2.0 ** (base_depth + chunk_depth))
    p = [F(c) for c in pos]
    return tuple(p[a] + (np.asarray(c).astype(np.float32) / full) * TWO for a, c in enumerate((x, y, z)))


def classify_cells(pos, base_depth, chunk_depth, x, y, z):
    """class byte of cells (x, y, z): 0 empty, 3 grass (solid, nothing solid one voxel above), 1 stone"""
    wx, wy, wz = world_of_cells(pos, base_depth, chunk_depth, x, y, z)
    vs = TWO / F(2.0 ** (base_depth + chunk_depth))
    solid = sdf(wx, wy, wz) < ZERO
    above = sdf(wx + ZERO, wy + vs, wz + ZERO) > ZERO
    return np.where(solid, np.where(above, 3, 1), 0).astype(np.uint8)


def classify(pos, base_depth, chunk_depth):
    """class bytes of the whole chunk in the reference's id order (id = x + side*y + side^2*z)"""
    side = 1 << chunk_depth
    ids = np.arange(side ** 3, dtype=np.int64)
    return classify_cells(pos, base_depth, chunk_depth, ids % side, ids // side % side, ids // side // side)


def morton(x, y, z, depth):
    """index of cell (x, y, z) among the 8^depth nodes of its level, children ordered x*4 + y*2 + z"""
    x, y, z = (np.asarray(a, dtype=np.int64) for a in (x, y, z))
    m = np.zeros_like(x)
    for b in range(depth):
        m |= (((x >> b) & 1) << (3 * b + 2)) | (((y >> b) & 1) << (3 * b + 1)) | (((z >> b) & 1) << (3 * b))
    return m


def to_morton(cls_id_order, chunk_depth):
    side = 1 << chunk_depth
    ids = np.arange(side ** 3, dtype=np.int64)
    out = np.zeros(side ** 3, dtype=np.uint8)
    out[morton(ids % side, ids // side % side, ids // side // side, chunk_depth)] = cls_id_order
    return out


def build_tree(cls_morton, chunk_depth):
    """Breadth-first pointer words of the union of root-to-cell paths of the solid cells (None if there is none).
    Level L's groups follow the order of their parents; interior pointer = index of the child group, leaf =
    CHUNK_OFFSET + class, empty slot = CHUNK_OFFSET."""
    occ = [None] * (chunk_depth + 1)
    occ[chunk_depth] = np.asarray(cls_morton) != 0
    for lvl in range(chunk_depth - 1, -1, -1):
        occ[lvl] = occ[lvl + 1].reshape(-1, 8).any(axis=1)
    if not occ[0][0]:
        return None
    rank = [np.cumsum(o, dtype=np.int64) - o for o in occ]
    count = [int(o.sum()) for o in occ]
    base = [0, 0]
    for lvl in range(1, chunk_depth):
        base.append(base[lvl] + 8 * count[lvl - 1])
    levels = []
    for lvl in range(1, chunk_depth + 1):
        parents = np.flatnonzero(occ[lvl - 1])
        kids = (parents[:, None] * 8 + np.arange(8)).reshape(-1)
        if lvl < chunk_depth:
            w = np.where(occ[lvl][kids], base[lvl + 1] + 8 * rank[lvl][kids], CHUNK_OFFSET)
        else:
            w = CHUNK_OFFSET + np.asarray(cls_morton, dtype=np.int64)[kids]
        levels.append(w.astype(np.uint32))
    return np.concatenate(levels)


def descend(words, chunk_depth, x, y, z):
    """class byte of cells (x, y, z) read back from a tree of build_tree's form (0 where the walk meets an empty slot)"""
    words = np.asarray(words, dtype=np.int64)
    x, y, z = (np.asarray(a, dtype=np.int64) for a in (x, y, z))
    node = np.zeros_like(x)
    alive = np.ones(x.shape, dtype=bool)
    out = np.zeros(x.shape, dtype=np.uint8)
    for lvl in range(1, chunk_depth + 1):
        b = chunk_depth - lvl
        c = (((x >> b) & 1) << 2) | (((y >> b) & 1) << 1) | ((z >> b) & 1)
        w = words[node + c]
        if lvl < chunk_depth:
            empty = w == CHUNK_OFFSET
            assert not np.any(alive & (w > CHUNK_OFFSET)), "leaf above the chunk's last level"
            alive &= ~empty
            node = np.where(alive, w, 0)
        else:
            out = np.where(alive, (w - CHUNK_OFFSET).astype(np.uint8), 0).astype(np.uint8)
    return out


def chunk_layout(world_depth):
    """generate_world's loop (world.rs:100-130): (i, chunk id, lower corner) for x, y, z in that nesting order"""
    n = 1 << world_depth
    vs = TWO / F(n)
    out = []
    i = 0
    for x in range(n):
        for y in range(n):
            for z in range(n):
                out.append((i, CHUNK_OFFSET // 2 + i, (F(x) * vs - ONE, F(y) * vs - ONE, F(z) * vs - ONE)))
                i += 1
    return out
