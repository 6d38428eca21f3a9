"""Where arrays become device inputs of the C ABI: one integer converter, one voxel-list front end and the
hand-off from torch's stream.  Nothing here needs the library, and everything but the hand-off works on the CPU device."""
import numpy as np
import torch


def device_u32(a, dev, clamp=False, mask=None, cells=False, what=None, signed=False):
    """An integer array (numpy or torch, any integer dtype) as a contiguous int32 tensor on `dev` holding u32 bit patterns.
    clamp: values outside [0, 2^31) become -1 or 2^31 - 1, out of range for any depth, so the device's range checks still
    see them; mask: keep those bits, whatever the dtype -- colours are masked to 24 bits here for every caller, which for
    an int32 colour tensor with bits above 23 handed to mesh.voxelize used to happen on the device only (the kernels mask
    again, the result is the same); cells: a wide value stays non-zero iff it was (its low 24 bits kept).  An int32 input
    is taken as it is unless `mask` is given.  signed: the values are int32 numbers (a structure's offsets, placements'
    origins), and one outside int32 becomes its nearest bound, out of range for the device's checks.  what: the
    argument's name, put in front of the TypeError's text."""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"{what + ': ' if what else ''}integer input expected, got {t.dtype}")
    t = t.to(dev)
    if t.dtype != torch.int32 or mask is not None:
        t = t.to(torch.int64)
        if mask is not None:
            t = t & mask
        elif clamp:
            t = t.clamp(-1, 2**31 - 1)
        elif signed:
            t = t.clamp(-2**31, 2**31 - 1)
        elif cells:
            t = torch.where(t != 0, (t & 0xFFFFFF) | (1 << 24), 0)
    return t.to(torch.int32).contiguous()


def voxel_list(gpu, coords, colours=None, noun="voxels", what=None, rows="N"):
    """A voxel list as the library takes it: coords -> a (N, 3) int32 tensor on gpu's device (clamped), colours -> N
    values masked to 24 bits, or None.  Returns (coords tensor, colours tensor or None, n, coords pointer, colours
    pointer); an empty list gives None for both pointers.  The caller keeps the tensors until its call has synced.
    noun, what, rows word the errors of a list of something else: mesh.voxelize's ("triangles", "triangles", "T")."""
    dev = gpu.torch_device
    xyz = device_u32(coords, dev, clamp=True, what=what)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what or 'coords'} must be ({rows}, 3), got {tuple(xyz.shape)}")
    n = xyz.shape[0]
    col = None
    if colours is not None:
        col = device_u32(colours, dev, mask=0xFFFFFF, what="colours" if what else None).reshape(-1)
        if col.numel() != n:
            raise ValueError(f"{col.numel()} colours for {n} {noun}")
    return xyz, col, n, xyz.data_ptr() if n else None, col.data_ptr() if col is not None and n else None


def wait_for_torch(gpu):
    """Tensors handed to the library were allocated, copied and filled on torch's current stream, and the context may
    launch on a stream of its own (Gpu.use_own_stream, set_stream) that is not ordered with it: the host waits here, once,
    before the call that reads or writes them."""
    torch.cuda.current_stream(gpu.torch_device).synchronize()
