"""What Render.distance_dense and svo_nodes_distance write (include/svo_hip.h), taken apart: the two marks,
the packed sites as offsets and as absolute cells, and the mask of a radius.  Every function takes a numpy array or a
torch tensor and answers in kind; everything is integers.
"""
import numpy as np

FAR = 0x7FFFFFFF       # in d2: no site within max_distance (signed mode: -FAR in an occupied cell)
NO_SITE = 0xFFFFFFFF   # in the packed sites: the same; as the int32 that a device tensor holds it is -1
MODES = ("voxels", "empty", "signed")
MAX_RADIUS = 127


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def pack_sites(offsets):
    """(..., 3) offsets s - c, each in [-128, 127], as svo_nodes_distance packs them: ((dx + 128) << 16) | ((dy + 128) << 8) |
    (dz + 128), int64"""
    o = offsets.long() if _is_torch(offsets) else np.asarray(offsets, dtype=np.int64)
    return (o[..., 0] + 128) << 16 | (o[..., 1] + 128) << 8 | (o[..., 2] + 128)


def unpack_sites(packed):
    """packed sites -> (offsets, valid): offsets an int32 (..., 3) of (dx, dy, dz) = s - c, valid False where the entry is
    NO_SITE (its offsets are then 0)"""
    if _is_torch(packed):
        import torch
        p = packed.long() & 0xFFFFFFFF
        valid = p != NO_SITE
        offsets = torch.stack([(p >> 16 & 0xFF) - 128, (p >> 8 & 0xFF) - 128, (p & 0xFF) - 128], dim=-1)
        return (offsets * valid[..., None]).to(torch.int32), valid
    p = np.asarray(packed).astype(np.int64) & 0xFFFFFFFF
    valid = p != NO_SITE
    offsets = np.stack([(p >> 16 & 0xFF) - 128, (p >> 8 & 0xFF) - 128, (p & 0xFF) - 128], axis=-1)
    return (offsets * valid[..., None]).astype(np.int32), valid


def site_cells(packed, origin):
    """the absolute cells of the sites of a box's packed sites ([x, y, z], as distance_dense returns them) whose first cell
    is `origin`: (cells, valid), cells an int32 (x, y, z, 3); a site outside the grid keeps its coordinates, negative ones
    included"""
    offsets, valid = unpack_sites(packed)
    if len(packed.shape) != 3 or len(origin) != 3:
        raise ValueError(f"packed must be the [x, y, z] array of a box and origin three cells, got {tuple(packed.shape)} and {origin!r}")
    if _is_torch(packed):
        import torch
        axes = [torch.arange(int(o), int(o) + n, dtype=torch.int32, device=packed.device) for o, n in zip(origin, packed.shape)]
        cells = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
    else:
        axes = [np.arange(int(o), int(o) + n, dtype=np.int32) for o, n in zip(origin, packed.shape)]
        cells = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
    return (cells + offsets) * valid[..., None], valid


def within(d2, radius):
    """the mask |d2| <= radius^2 of a field of squared distances, signed ones included; FAR is never within"""
    radius = int(radius)
    if radius < 0:
        raise ValueError(f"radius must not be negative (got {radius})")
    return (d2 <= radius * radius) & (d2 >= -radius * radius)
