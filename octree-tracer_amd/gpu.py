"""Device context: replaces reference src/gpu.rs (wgpu instance/adapter/device/queue) with a
HIP context handle from the C ABI."""
import ctypes as C

import torch

from ._lib import SvoError, lib

OPT_VARIANT, OPT_TIMING, OPT_GRID_BLOCKS, OPT_REFILL_MIN, OPT_STRIP_ITEMS, OPT_DYNAMIC_STRIPS, OPT_PRIO_STEPS, OPT_DEBUG_BUFFER, OPT_SCHEDULE, OPT_TREE_DEPTH, OPT_BLOCK_SHAPE, OPT_SCAN_CLEARS_COUNTERS, OPT_FUSED_SHADOWS, OPT_PAIR_TABLE, OPT_CULL, OPT_CAMERA_SHORTCUT, OPT_SCHEDULE_MOTION, OPT_STATIC_DEAL = range(18)
VARIANT_RESTART, VARIANT_STACK = 0, 1
# OPT_DEBUG_BUFFER (include/svo_hip.h: SVO_DEBUG_WAVES, SVO_DEBUG_ROW_WORDS, SVO_DEBUG_BUFFER_WORDS): two regions of DEBUG_WAVES rows
DEBUG_WAVES, DEBUG_ROW_WORDS = 16384, 16
DEBUG_BUFFER_WORDS = 2 * DEBUG_WAVES * DEBUG_ROW_WORDS


class Gpu:
    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        rc = lib().svo_ctx_create(device, C.byref(h))
        if rc != 0:
            # the reference unwraps (gpu.rs:24,39): fail loudly, there is no fallback device
            raise SvoError(f"svo_ctx_create(device={device}) failed with status {rc} (no usable HIP device?)")
        self._h = h
        self.device = device
        self.torch_device = torch.device("cuda", device)  # where tensors handed to this context live (made once: the wrappers ask per call)
        self.tree_depth = 16  # what SVO_OPT_TREE_DEPTH holds: the library's default until set_option is told another
        # torch allocates and copies on its current stream: launch there so tensors handed to the
        # C ABI are ordered with the kernels that read or write them
        self.set_stream(stream if stream is not None else torch.cuda.current_stream(device).cuda_stream)

    @classmethod
    def new(cls, device=0):
        return cls(device)

    def check(self, rc):
        if rc != 0:
            raise SvoError(f"status {rc}: {lib().svo_last_error(self._h).decode()}")

    def set_stream(self, hip_stream):
        """hip_stream: a hipStream_t handle as int (0 = HIP's default stream)"""
        self.check(lib().svo_ctx_set_stream(self._h, C.c_void_p(hip_stream), 0))

    def use_own_stream(self):
        self.check(lib().svo_ctx_set_stream(self._h, None, 1))

    def set_option(self, option, value):
        self.check(lib().svo_set_option(self._h, option, int(value)))
        if option == OPT_TREE_DEPTH:
            self.tree_depth = int(value)

    def declare_depth(self, depth, most=21):
        """The trace kernels must know how deep the tree goes (SVO_OPT_TREE_DEPTH): a depth in 1..most above the one this
        context holds raises it; nothing here ever lowers it, whoever set it -- the caller or any Render on this context.
        most: 21, the deepest tree a build or an edit makes."""
        if 1 <= depth <= most and depth > self.tree_depth:
            self.set_option(OPT_TREE_DEPTH, depth)

    def sync(self):
        """device.poll(Maintain::Wait)"""
        self.check(lib().svo_sync(self._h))

    def last_render_ms(self):
        ms = C.c_float()
        self.check(lib().svo_last_render_ms(self._h, C.byref(ms)))
        return ms.value

    def _timing(self, fn, n):
        ms = (C.c_float * n)()
        self.check(fn(self._h, ms))
        return list(ms)

    def build_timing(self):
        """ms of the last Render.build_nodes / build_nodes_dense: keys, sort, levels, count read-back, emit (device events),
        host wall time of the call (svo_build_timing)"""
        return self._timing(lib().svo_build_timing, 6)

    def edit_timing(self):
        """ms of the last Render.edit_nodes: keys, sort, plan, status read-back, fill and link (device events), host wall
        time of the call (svo_edit_timing)"""
        return self._timing(lib().svo_edit_timing, 6)

    def region_timing(self):
        """ms of the last Render.edit_region: plan (with its per-level read-backs), status, fill, write (device events),
        host wall time of the call (svo_region_timing)"""
        return self._timing(lib().svo_region_timing, 5)

    def combine_timing(self):
        """ms of the last Render.combine_nodes: plan (with its per-level read-backs), status, fill, write (device events),
        host wall time of the call (svo_combine_timing)"""
        return self._timing(lib().svo_combine_timing, 5)

    def place_timing(self):
        """ms of the last Render.place_nodes: plan (with its per-level read-backs), status, fill, write (device events),
        host wall time of the call (svo_place_timing)"""
        return self._timing(lib().svo_place_timing, 5)

    def transform_timing(self):
        """ms of the last Render.transform_nodes: plan (with its per-level read-backs), status, fill, write (device events),
        host wall time of the call (svo_transform_timing)"""
        return self._timing(lib().svo_transform_timing, 5)

    def morph_timing(self):
        """ms of the last step of Render.morph_nodes: plan (with its per-level read-backs), status, fill, write (device
        events), host wall time of the call (svo_morph_timing)"""
        return self._timing(lib().svo_morph_timing, 5)

    def heightmap_timing(self):
        """ms of the last Render.edit_heightmap: the min/max pyramid, plan (with its per-level read-backs), status, fill,
        write (device events), host wall time of the call (svo_heightmap_timing)"""
        return self._timing(lib().svo_heightmap_timing, 6)

    def compact_timing(self):
        """ms of the last Render.compact_nodes: discover, check, prune, emit, copy back (device events), host wall time
        of the call (svo_compact_timing)"""
        return self._timing(lib().svo_compact_timing, 6)

    def simplify_timing(self):
        """ms of the last Render.simplify_nodes: discover, check, reduce, emit, copy back (device events), host wall time
        of the call (svo_simplify_timing)"""
        return self._timing(lib().svo_simplify_timing, 6)

    def list_timing(self):
        """ms of the last Render.list_voxels call into the library (its fill, or its count query when the list was empty
        or refused): discover, count, offsets, emit (device events), host wall time of the call (svo_list_timing)"""
        return self._timing(lib().svo_list_timing, 5)

    def surface_timing(self):
        """ms of the last Render.list_surface / surface_quads call into the library (its fill, or its count query when the
        list was empty or refused): discover, count, offsets, mask, the compaction's count, emit (device events), host
        wall time of the call (svo_surface_timing)"""
        return self._timing(lib().svo_surface_timing, 7)

    def surface_merge_timing(self):
        """ms of the last Render.surface_rects call into the library (its fill, or its count query when there was nothing
        to fill or the call was refused): the quads, then keys, sort, flags and scan, emit for each of the 8 phases a
        call can have (U and V of round 1 first; 0 for a phase that did not run), the output's fill (device events),
        host wall time of the call (svo_surface_merge_timing)"""
        return self._timing(lib().svo_surface_merge_timing, 35)

    def components_timing(self):
        """(ms, rounds) of the last Render.label_components call into the library (its fill, or its count query when there
        was nothing to fill or the call was refused): ms = plan, link, union, ids, the fill (device events), host wall time
        of the call; rounds = the rounds of the union, the last, which hooks nothing, included (svo_components_timing)"""
        ms, rounds = (C.c_float * 6)(), C.c_uint32()
        self.check(lib().svo_components_timing(self._h, ms, C.byref(rounds)))
        return list(ms), rounds.value

    def sample_timing(self):
        """ms of the last Render.sample_voxels / sample_dense call that ran: the kernel (device events), host wall time of
        the call (svo_sample_timing)"""
        return self._timing(lib().svo_sample_timing, 2)

    def distance_timing(self):
        """ms of the last Render.distance_dense call that ran: the occupancy bits, the first slab's z and y pass, the first
        slab's x pass, all slabs (device events), host wall time of the call (svo_distance_timing)"""
        return self._timing(lib().svo_distance_timing, 5)

    def voxelize_timing(self):
        """ms of the last mesh.voxelize call into the library that ran (its fill, or its count query when the list was
        empty): setup, the levels above the last, the last level's test and scan, emit (device events), host wall time of
        the call (svo_voxelize_timing)"""
        return self._timing(lib().svo_voxelize_timing, 5)

    def solid_timing(self):
        """ms of the last mesh.voxelize_solid call into the library that ran (its fill, or its count query when the mesh
        has no interior): setup, the column levels, the sort, spans, emit (device events), host wall time of the call
        (svo_solid_timing)"""
        return self._timing(lib().svo_solid_timing, 6)

    def structure_timing(self):
        """ms of the last Render.column_tops / structure_sites / stamp_structures call into the library that ran: count
        (column tops: the kernel; sites and stamp: checks, sums and scan with the read-back), fill (device events), host
        wall time of the call (svo_structure_timing)"""
        return self._timing(lib().svo_structure_timing, 3)

    def world_build_timing(self):
        """ms of the last CpuOctree.build / World.build_world: keys, sort, levels, count read-back, emit, mips (device
        events), chunk read-back, chunk files and root (CpuOctree.build: the tree), host wall time of the call
        (svo_world_build_timing)"""
        return self._timing(lib().svo_world_build_timing, 9)

    def strip_classes(self, n_strips):
        """class byte per 64-pixel block of the last pixel frame that ran the culling pass (0xFF = culled); diagnostics"""
        import numpy as np
        out = np.zeros(n_strips, dtype=np.uint8)
        self.check(lib().svo_diag_strip_classes(self._h, out.ctypes.data_as(C.c_void_p), n_strips))
        return out

    DEAL_STATUS = ("replayed", "seeds", "device_seeds", "moves", "step", "verdict", "seeded", "claims", "rows", "row_cap",
                   "best_ticks", "best_sample_ticks", "claim_ticks", "last_ticks", "last_moves", "learn_left")

    def deal_status(self, table=False, stamps=False):
        """the static deal of the context's resting view (OPT_STATIC_DEAL), read-only: a dict of DEAL_STATUS (svo_diag_deal),
        with the device table (rows x row_cap strip numbers, 0xFFFFFFFF behind a row's last) and the per-wave stamps (began
        its last strip, ended: 10 ns ticks) when asked for; diagnostics"""
        import numpy as np
        st = np.zeros(16, dtype=np.uint32)
        self.check(lib().svo_diag_deal(self._h, st.ctypes.data_as(C.c_void_p), None, 0, None, 0))
        out = dict(zip(self.DEAL_STATUS, (int(v) for v in st)))
        rows, cap = out["rows"], out["row_cap"]
        tab = np.zeros((rows, cap), dtype=np.uint32) if table else None
        stp = np.zeros((rows, 2), dtype=np.uint32) if stamps else None
        if rows and (table or stamps):
            self.check(lib().svo_diag_deal(self._h, st.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p) if table else None,
                                           tab.size if table else 0, stp.ctypes.data_as(C.c_void_p) if stamps else None, stp.size if stamps else 0))
        if table:
            out["table"] = tab
        if stamps:
            out["stamps"] = stp
        return out

    SCHEDULE_INFO = ("n_strips", "cap", "bpr", "valid", "order_filtered", "age", "balance_frames", "floored")

    def schedule_status(self, slot=0):
        """what schedule slot `slot` (0: primary frames, 1: shadow and secondary rays) holds, read-only (svo_diag_schedule): a dict
        of SCHEDULE_INFO and the numpy arrays classes (the measured cost classes), classes_now (those of the last filtered or
        floored build; 0xFF: in no list), lengths (8), lists (8 x cap strip numbers; entries behind a list's length are stale)
        and balance (32 words: [0..8] cumulative shares, [18] updates, [20] best time, [21..29] best shares); diagnostics"""
        import numpy as np
        info, bal = np.zeros(16, dtype=np.uint32), np.zeros(32, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self.check(lib().svo_diag_schedule(self._h, slot, ptr(info), None, 0, None, None, 0, ptr(bal)))
        n, cap = int(info[0]), int(info[1])
        cls, now = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        words = np.zeros(8 + 8 * cap, dtype=np.uint32)
        self.check(lib().svo_diag_schedule(self._h, slot, ptr(info), ptr(cls), n, ptr(now), ptr(words), words.size, ptr(bal)))
        out = dict(zip(self.SCHEDULE_INFO, (int(v) for v in info)))
        out.update(classes=cls, classes_now=now, lengths=words[:8].copy(), lists=words[8:].reshape(8, cap), balance=bal)
        return out

    def timing_collect(self, cap=65536):
        """durations (ms) of the trace launches recorded since the last collect"""
        import numpy as np
        buf = np.empty(cap, dtype=np.float32)
        n = C.c_size_t()
        self.check(lib().svo_timing_collect(self._h, buf.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n)))
        return buf[:n.value].copy()

    # ---- multi-GPU frame end: RCCL behind the C ABI (svo_comm_*, svo_gather_frame) ----
    @staticmethod
    def comm_unique_id():
        """128 bytes rank 0 hands to the other ranks (ncclGetUniqueId)"""
        buf = (C.c_uint8 * 128)()
        rc = lib().svo_comm_unique_id(buf)
        if rc != 0:
            raise SvoError(f"svo_comm_unique_id failed with status {rc} (librccl missing?)")
        return bytes(buf)

    def comm_init_rank(self, unique_id, world, rank):
        """collective: every rank's context, with rank 0's id (one process per GPU)"""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self.check(lib().svo_comm_init_rank(self._h, buf, world, rank))

    @staticmethod
    def comm_init_all(gpus):
        """one process driving several devices: gpus[r] becomes rank r (ncclCommInitAll)"""
        arr = (C.c_void_p * len(gpus))(*[g._h for g in gpus])
        rc = lib().svo_comm_init_all(len(gpus), arr)
        if rc != 0:
            raise SvoError(f"status {rc}: {lib().svo_last_error(gpus[0]._h).decode()}")

    def comm_destroy(self):
        self.check(lib().svo_comm_destroy(self._h))

    def gather_frame(self, send, recv_on_root=None, root=0):
        """this rank's part of the frame-end gather, on the context's stream: tensor `send` -> recv_on_root[rank] on root"""
        self.check(lib().svo_gather_frame(self._h, send.data_ptr(), send.numel() * send.element_size(),
                                          recv_on_root.data_ptr() if recv_on_root is not None else None, root))

    def gather_wait(self):
        """the context's stream waits for the gathers issued so far"""
        self.check(lib().svo_gather_wait(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().svo_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        if lib is not None:  # (module globals are gone at interpreter exit)
            self.close()
