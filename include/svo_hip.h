/*
 * svo_hip.h -- the drop-in boundary: a C ABI over the MI355X (gfx950) HIP implementation of
 * ria8651/octree-tracer's GPU path.  Plain pointers and sizes only; no torch / C++ types.
 *
 * What each entry point replaces in the reference (file:line under /root/reference/src):
 *   svo_ctx_create / destroy      Gpu::new (gpu.rs:11-49): instance/adapter/device/queue
 *   svo_nodes_alloc               Render::new node buffer, `octree.expanded(10_000_000)`
 *                                 create_buffer_init STORAGE|COPY_DST (render.rs:53-61)
 *   svo_nodes_write               queue.write_buffer(&render.node_buffer, 0, nodes)
 *                                 (app.rs:113-118, :163-168, :194-199, :239-244)
 *   svo_nodes_scatter             the same upload restricted to the words that changed (no reference counterpart)
 *   svo_set_uniforms              Render::update -> queue.write_buffer(uniform_buffer)
 *                                 (render.rs:191-212); struct Uniforms (render.rs:287-322,
 *                                 shader.wgsl:2-13)
 *   svo_render / svo_render_tiles Render::render: one pass, draw(0..4, 0..1) running fs_main once
 *                                 per pixel (render.rs:217-284, shader.wgsl:250-305)
 *   svo_trace_rays                octree_ray on caller-supplied rays (shader.wgsl:191-248; the
 *                                 shadow ray of shader.wgsl:276 is such a ray)
 *   svo_render_secondary /        no reference entry point: benchmark config 5 (BASELINE.json configs[4]) --
 *   svo_render_tiles_secondary    primary rays plus up to 4 secondary rays per hit pixel; ray 0 is fs_main's
 *                                 shadow ray (shader.wgsl:275-280), the others reuse its origin
 *   svo_scan_dispatch             Compute::update: dispatch(ceil(n/16/256), 256, 1) of
 *                                 compute.wgsl main (compute.rs:99-127, compute.wgsl:26-47)
 *   svo_scan_read                 map_async + device.poll(Wait) + counter reset
 *                                 (adaptive.rs:12-23, :76-87)
 *   svo_sync                      device.poll(Maintain::Wait)
 *   svo_proc_generate_chunk       Procedural::generate_chunk (procedural.rs:101-199, procedual.wgsl:150-201), restated
 *                                 deterministically: canonical breadth-first tree instead of the racy insertion
 *   svo_world_generate            World::generate_world (world.rs:63-139)
 *   svo_nodes_build / _dense      no reference counterpart (the reference builds trees on the host, cpu_octree.rs): the
 *                                 tree of a device voxel list or dense colour grid, built on the GPU into the node
 *                                 buffer, canonical breadth-first
 *   svo_comm_* / svo_gather_frame no reference counterpart (the reference drives one device, main.rs:40-88): the
 *                                 frame-end exchange of the tile-sharded multi-GPU frame, RCCL behind the boundary
 *                                 (SURVEY.md 8b "Threading", 8e): communicator set-up for one process per GPU
 *                                 (svo_comm_init_rank) or one process driving all GPUs (svo_comm_init_all), and the
 *                                 ONE gather of hit records to rank 0 per frame
 * Errors: the reference unwraps/panics (gpu.rs:24,39; adaptive.rs:66,124); here every call
 * returns 0 on success or a negative svo_status, and svo_last_error() gives the text.
 * Threading: like the reference (all device calls from one thread, main.rs:40-88) a ctx is not
 * thread-safe; one ctx per GPU, each ctx launches on one HIP stream.
 */
#ifndef SVO_HIP_H
#define SVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_VOXEL_OFFSET 134217728u /* octree.rs:5, shader.wgsl:30 */

typedef enum svo_status {
    SVO_OK = 0,
    SVO_ERR_ARG = -1,     /* bad argument */
    SVO_ERR_HIP = -2,     /* a HIP runtime call failed; see svo_last_error */
    SVO_ERR_STATE = -3,   /* call order (e.g. render before nodes_alloc) */
    SVO_ERR_NO_DEVICE = -4,
    SVO_ERR_COMM = -5,    /* RCCL missing or a collective call failed; see svo_last_error */
    SVO_ERR_CAP = -6      /* the result would exceed a caller-given cap (svo_proc_params.max_nodes); nothing was written */
} svo_status;

/* Uniform flags: the reference's five 1-byte bools (render.rs:294-299) as explicit bits. */
#define SVO_F_PAUSE_ADAPTIVE 1u
#define SVO_F_SHOW_STEPS 2u
#define SVO_F_SHOW_HITS 4u
#define SVO_F_SHADOWS 8u
#define SVO_F_MISC_BOOL 16u

typedef struct svo_uniforms {
    float camera[16];         /* column-major */
    float camera_inverse[16]; /* column-major */
    float dimensions[4];      /* (W, H, 0, 0) */
    float sun_dir[4];
    uint32_t flags;
    float misc_value;
} svo_uniforms;

/* HitInfo (shader.wgsl:182-189) as a 16-byte record.
 * steps_depth_hit: bits 0..7 steps, 8..15 depth, bit 16 hit, bits 17..22 normal code;
 * packed_normal: 2 bits per axis (x: bits 0..1, y: 2..3, z: 4..5), 0 -> 0, 1 -> +1, 2 -> -1.
 * voxel_index is HitInfo.value: the node-array index of the leaf word, or the reference's
 * sentinels 0 (never entered the cube), 0x20202000 (left the cube), 0xFF000000 (>100 steps).
 * t = ray_box_dist entry distance + t_current of the last DDA step. */
typedef struct svo_hit {
    uint32_t voxel_index;
    float t;
    uint32_t steps_depth_hit;
    uint32_t packed_normal;
} svo_hit;

typedef struct svo_ctx svo_ctx;

/* kernel variants (svo_set_option SVO_OPT_VARIANT) */
#define SVO_VARIANT_RESTART 0 /* reference-shaped: float-compare descent from the root every step */
#define SVO_VARIANT_STACK 1   /* integer path codes + per-ray ancestor stack in LDS + LDS top table + refill (default) */
/* (Round 3's two experiments over a device-built child-mask table -- one ray per lane, and two rays per lane software-pipelined --
 * measured slower than SVO_VARIANT_STACK on every scene and left the library in round 4; the source is kept under
 * tools/experiments/ with its logs in profiles/r03_*, DESIGN.md Appendix A.  Values 2 and 3 are refused.) */

/* SVO_OPT_DEBUG_BUFFER: the buffer is two regions of SVO_DEBUG_WAVES rows of SVO_DEBUG_ROW_WORDS words, one row per wave of
 * the trace launch in each.  While the buffer is set, a trace launch has at most SVO_DEBUG_WAVES waves: a larger
 * SVO_OPT_GRID_BLOCKS is cut back to that (the automatic grid is far below it). */
#define SVO_DEBUG_WAVES 16384u
#define SVO_DEBUG_ROW_WORDS 16u
#define SVO_DEBUG_BUFFER_WORDS (2u * SVO_DEBUG_WAVES * SVO_DEBUG_ROW_WORDS)

typedef enum svo_option {
    SVO_OPT_VARIANT = 0,
    SVO_OPT_TIMING = 1,      /* n > 0: bracket trace launches with HIP events on the launch stream (ring of n) */
    SVO_OPT_GRID_BLOCKS = 2, /* persistent grid size override (0 = auto) */
    SVO_OPT_REFILL_MIN = 3,  /* idle lanes needed before a wave refills (default 32 since round 5) */
    SVO_OPT_STRIP_ITEMS = 4, /* pixel slots a wave claims at a time (multiple of 64) */
    SVO_OPT_DYNAMIC_STRIPS = 5, /* accepted and ignored: the STACK kernel always claims its strips from device counters (the static
                                round-robin deal of round 1 cost the hot loop scalar registers) */
    SVO_OPT_SCHEDULE = 8,    /* n > 0 (default 2): trace the strips whose rays took the most steps in an earlier frame of
                                the same layout first, rebuilding that schedule every n frames; 0: screen order.
                                Results do not depend on it. */
    SVO_OPT_TREE_DEPTH = 9,  /* upper bound of the octree depth (Settings.octree_depth, app.rs:24); default 16.
                                <= 16: default kernel; <= 22: deep-stack kernel (the STACK variant's 23-bit path codes resolve 22 levels; it was 23 up to
                                round 3); above: the general RESTART kernel.  A tree deeper than the bound given here is refused: the launch
                                completes, svo_sync returns SVO_ERR_STATE (svo_last_error says so) and the frame's records are not to be used
                                (tests/test_parity_gpu.py: test_tree_deeper_than_declared_is_refused) */
    SVO_OPT_BLOCK_SHAPE = 10, /* log2 of the width of the 64-pixel blocks a wave works on (3: 8x8, 4: 16x4, ...) */
    SVO_OPT_DEBUG_BUFFER = 7, /* device pointer to SVO_DEBUG_BUFFER_WORDS words (0: off).  First region, 16 words per wave: start, queue-dry, end (10 ns
                                 ticks), rounds, ..., shader cycles per phase (refill, descent, step), descent-loop shape; second region
                                 (round 5), 16 words per wave: loop entry, the first 14 ray generations (10 ns ticks), XCC / hardware id
                                 (tools/wave_timeline.py, tools/timeline_by_xcd.py) */
    SVO_OPT_SCAN_CLEARS_COUNTERS = 11, /* 1: svo_scan_dispatch also zeroes the hit counters it has scanned, so that the
                                          host need not re-upload the whole array to reset them (svo_nodes_scatter) */
    SVO_OPT_FUSED_SHADOWS = 12, /* shaded frames with shadows (svo_render* with rgba_out), STACK variant: 1 = the lane that finds a hit goes
                                   on with that pixel's shadow ray inside the primary launch; 0 = shadow rays are a second launch;
                                   2 (default) = automatic, which fuses whenever the sun direction is one the fast arithmetic covers
                                   (1080p: 0.65 -> 0.58 ms, 4K: 2.04 -> 1.78 ms on the benchmark tree).  The image is the same either way. */
    SVO_OPT_PAIR_TABLE = 13, /* accepted and ignored: the two-levels-per-load table of round 2 measured a net loss and left the library */
    SVO_OPT_CULL = 14,       /* pixel frames, STACK variant: 64-pixel blocks whose rays all miss the cube (decided conservatively from
                                the block's corner rays) get their all-zero records from a pre-pass and are never claimed by the
                                trace.  0 off, 1 whenever the camera is outside the cube, 2 (default) when in addition at least 40 % of a
                                coarse grid of rays tested on the host look past the cube.  Results do not depend on it. */
    SVO_OPT_CAMERA_SHORTCUT = 15, /* pixel frames, camera inside the cube, STACK variant: every primary ray starts in the camera's leaf, so a wave
                                walks from the root to it once and its lanes copy that walk when they pick up a ray.  1 (default) on, 0 off.
                                Results do not depend on it. */
    SVO_OPT_SCHEDULE_MOTION = 16, /* strip schedule while the camera moves (pixel frames of one rectangle): strips that had at least
                                `min_count` strips with a step-limit ray among their (2 radius + 1)^2 neighbours are scheduled as at least
                                class `floor`.  value = floor (1..12; 0 = off) | radius << 8 | min_count << 12; default 0x1204 (at least class 4
                                for strips with one such strip among their 24 neighbours: 3 - 5 % off a moving camera's frame).  When the
                                camera comes to rest the lists are rebuilt once more from the classes as measured.
                                Results do not depend on it. */
    SVO_OPT_STATIC_DEAL = 17, /* resting views (same camera, tree and layout, plain pixel frames of the STACK variant, lists settled):
                                which wave traces which strips is written down once and replayed without claims, then improved from
                                per-wave time stamps over 16 frames; a view whose replay never beat its claims goes back to claiming.
                                1 (default) on, 0 off.  Results do not depend on it. */
    SVO_OPT_PRIO_STEPS = 6   /* accepted and ignored: raising the issue priority of waves with old rays measured no effect and
                                left the kernel */
} svo_option;

/* Number of HIP devices visible to the process (0 without a GPU). */
int svo_device_count(void);
int svo_ctx_create(int hip_device, svo_ctx **out);
int svo_ctx_destroy(svo_ctx *ctx);
/* Launch on a caller-owned hipStream_t (e.g. torch's current stream; NULL is HIP's default
 * stream), or, with use_own != 0, on the private non-blocking stream the ctx was created with. */
int svo_ctx_set_stream(svo_ctx *ctx, void *hip_stream, int use_own);
int svo_set_option(svo_ctx *ctx, int option, int64_t value);
const char *svo_last_error(const svo_ctx *ctx);
int svo_sync(svo_ctx *ctx);

int svo_nodes_alloc(svo_ctx *ctx, size_t capacity_words);
/* Use caller-owned device memory as the node buffer instead (no copy).  The library cannot see writes the caller makes to
 * that memory: call svo_nodes_invalidate after each of them, or the STACK kernel descends from a stale top table. */
int svo_nodes_bind_device(svo_ctx *ctx, uint32_t *device_words, size_t capacity_words);
/* Trace from the SAME node buffer as `owner` (same device; frames in flight on several contexts / streams, one buffer).
 * The contexts share the words, a generation counter and the stream ordering of writes: after svo_nodes_write /
 * svo_nodes_scatter / svo_nodes_invalidate through ANY of them, every one rebuilds its top table and strip schedule
 * before its next trace, and that trace waits (on the device) for the write.  A write does not wait for traces other
 * contexts still have in flight: that ordering stays with the caller (svo_sync them first), as with any shared buffer.
 * The buffer lives until the last context bound to it lets go. */
int svo_nodes_share(svo_ctx *ctx, svo_ctx *owner);
/* The words of the node buffer were changed behind the library's back (a kernel or copy of the caller's, enqueued on
 * this context's stream before this call): bump the generation, like a write. */
int svo_nodes_invalidate(svo_ctx *ctx);
int svo_nodes_write(svo_ctx *ctx, size_t word_offset, const uint32_t *host_words, size_t n);
/* Incremental form of the reference's per-frame `queue.write_buffer(&node_buffer, 0, nodes)` (app.rs:113-118): write
 * host_words[i] to word indices[i] (host pointers, n pairs, indices unique), e.g. the words the streaming loop changed
 * (svo_octree_take_dirty).  Asynchronous on the ctx stream like svo_nodes_write: both arrays must stay valid until the
 * next blocking call. */
int svo_nodes_scatter(svo_ctx *ctx, const uint32_t *indices, const uint32_t *host_words, size_t n);
int svo_nodes_read(svo_ctx *ctx, size_t word_offset, uint32_t *host_words, size_t n);
/* Device pointer of the node buffer (for zero-copy consumers). */
int svo_nodes_device_ptr(svo_ctx *ctx, uint32_t **out, size_t *capacity_words);

/* Device memory for hit records, wire records and gathered frames, for hosts that carry no HIP binding of their own (the
 * `*_out` parameters below are device pointers; any device pointer of the ctx's device will do).  svo_buffer_read copies
 * to host memory behind everything enqueued on the ctx stream and blocks until done. */
int svo_buffer_alloc(svo_ctx *ctx, size_t bytes, void **device_out);
int svo_buffer_free(svo_ctx *ctx, void *device_ptr);
int svo_buffer_read(svo_ctx *ctx, const void *device_ptr, void *host_out, size_t bytes);
/* The partner of svo_buffer_read: host memory to a device buffer, behind everything enqueued on the ctx stream; blocking. */
int svo_buffer_write(svo_ctx *ctx, void *device_dst, const void *host_src, size_t bytes);

int svo_set_uniforms(svo_ctx *ctx, const svo_uniforms *u);

/* Trace the primary rays of the pixel rectangle [x0,x0+tile_w) x [y0,y0+tile_h) of a
 * width x height frame (must equal uniforms.dimensions).  hits_out (tile_w*tile_h records,
 * row-major within the rectangle) and rgba_out (tile_w*tile_h RGBA8, optional, the shaded colour
 * of fs_main) are DEVICE pointers; either may be NULL.  Asynchronous on the ctx stream. */
int svo_render(svo_ctx *ctx, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0,
               uint32_t tile_w, uint32_t tile_h, svo_hit *hits_out, uint32_t *rgba_out);
/* Same with HOST output pointers; blocking (staging buffer + D2H). */
int svo_render_host(svo_ctx *ctx, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0,
                    uint32_t tile_w, uint32_t tile_h, svo_hit *hits_out, uint32_t *rgba_out);
/* Multi-GPU sharding: the frame is cut into tile_w x tile_h tiles numbered row-major; this call
 * traces tiles first_tile, first_tile + tile_stride, ... and writes them contiguously in that
 * order (tile k of this rank at hits_out[k * tile_w * tile_h], row-major inside the tile).
 * width and height must be multiples of the tile size. */
int svo_render_tiles(svo_ctx *ctx, uint32_t width, uint32_t height, uint32_t tile_w,
                     uint32_t tile_h, uint32_t first_tile, uint32_t tile_stride,
                     svo_hit *hits_out, uint32_t *rgba_out);
/* Primary rays of the rectangle / tile set as above, then n_secondary (1..4) rays from every pixel whose
 * primary ray hit: origin hit.pos + normal * 2.5e-6 (shader.wgsl:276); ray 0 towards -normalize(sun_dir) (the
 * shadow ray), ray k >= 1 along normalize(e) with e_i = float((h >> 10 i) & 1023) - 511.5,
 * h = mix32((py * width + px) * 4 + k + 0x9E3779B9) (mix32: xorshift-multiply, see oracle/svo_oracle.c),
 * negated if dot(normal, e) < 0.  secondary_out holds n_secondary * n records, ray-major
 * (secondary_out[k * n + i] belongs to primary record i); pixels without a primary hit get the miss record
 * {0, 0, 0, 0}.  Like the shadow ray, secondary rays bump the hit counters unless pause_adaptive.
 * primary_out may be NULL.  Device pointers; asynchronous on the ctx stream. */
int svo_render_secondary(svo_ctx *ctx, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0,
                         uint32_t tile_w, uint32_t tile_h, uint32_t n_secondary, svo_hit *primary_out,
                         svo_hit *secondary_out);
int svo_render_tiles_secondary(svo_ctx *ctx, uint32_t width, uint32_t height, uint32_t tile_w,
                               uint32_t tile_h, uint32_t first_tile, uint32_t tile_stride,
                               uint32_t n_secondary, svo_hit *primary_out, svo_hit *secondary_out);
/* Rank 0 after the frame-end gather: `gathered` holds world x n_pad tiles (rank r's k-th tile = tile r + k * world, the
 * layout svo_render_tiles writes); frame_out receives the row-major width x height frame.  Device pointers. */
int svo_assemble_tiles(svo_ctx *ctx, const svo_hit *gathered, uint32_t world, uint32_t n_pad, uint32_t width,
                       uint32_t height, uint32_t tile_w, uint32_t tile_h, svo_hit *frame_out);
/* The same with 12-byte wire records, and the packing that produces them: the fourth word of svo_hit (packed_normal)
 * repeats bits 17..22 of the third, so a rank can send {voxel_index, t, steps_depth_hit} only -- a quarter fewer bytes
 * on the links -- and rank 0 rebuilds full records while it un-permutes.  Device pointers. */
int svo_pack_records(svo_ctx *ctx, const svo_hit *records, size_t n, uint32_t *wire_out);
int svo_assemble_tiles_packed(svo_ctx *ctx, const uint32_t *gathered_wire, uint32_t world, uint32_t n_pad, uint32_t width,
                              uint32_t height, uint32_t tile_w, uint32_t tile_h, svo_hit *frame_out);
/* ---- multi-GPU frame end: one gather of hit records to the root rank per frame, RCCL over xGMI.  librccl is
 * loaded on first use (dlopen); without it these return SVO_ERR_COMM and everything else keeps working. ----
 * One process per GPU: rank 0 makes an id (svo_comm_unique_id), hands its 128 bytes to the other ranks by any means (the
 * launcher's rendezvous, a file, MPI, torch.distributed), and every rank calls svo_comm_init_rank on its context:
 * collective, blocks until all `world` ranks have called it. */
#define SVO_COMM_ID_BYTES 128
int svo_comm_unique_id(uint8_t id_out[SVO_COMM_ID_BYTES]);
int svo_comm_init_rank(svo_ctx *ctx, const uint8_t id[SVO_COMM_ID_BYTES], int world, int rank);
/* One process (one thread) driving n contexts on n different devices, the reference's threading model (main.rs:40-88):
 * ncclCommInitAll; ctxs[r] becomes rank r. */
int svo_comm_init_all(int n, svo_ctx *const *ctxs);
int svo_comm_destroy(svo_ctx *ctx);
/* This rank's contribution to the frame-end gather: `bytes` bytes (a multiple of 4, the same on every rank) from `send` to
 * `recv_on_root` + rank * bytes on rank `root` (device pointers; recv_on_root is ignored elsewhere and may be NULL).  Every
 * rank of the communicator must call it once per frame, in the same order of frames.  Asynchronous: the exchange runs on a
 * communication stream of the context, ordered BEHIND everything enqueued on the ctx stream so far (the trace / pack that
 * produced `send`), so the ctx stream is free to start the next frame while records travel.  svo_gather_wait makes the ctx
 * stream wait for the gathers issued so far: call it before work on the ctx stream reads recv_on_root (svo_assemble_tiles on
 * the root) or overwrites `send`; svo_sync waits for both streams. */
int svo_gather_frame(svo_ctx *ctx, const void *send, size_t bytes, void *recv_on_root, int root);
int svo_gather_wait(svo_ctx *ctx);
/* The same for the single-process form, all ranks in one call: send[r] is rank r's buffer (on ctxs[r]'s device);
 * recv_on_root lives on ctxs[root]'s device. */
int svo_gather_frame_all(int n, svo_ctx *const *ctxs, const void *const *send, size_t bytes, void *recv_on_root, int root);

/* The same un-permute for a gathered COLOUR frame: when the consumer of the sharded frame is a display -- the reference's
 * output is the RGBA image of fs_main -- the ranks gather rgba_out of svo_render_tiles, 4 bytes per ray on the links instead
 * of 12 (the gather into one GPU is what bounds an 8-GPU frame).  Device pointers. */
int svo_assemble_tiles_rgba(svo_ctx *ctx, const uint32_t *gathered_rgba, uint32_t world, uint32_t n_pad, uint32_t width,
                            uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t *rgba_frame_out);

/* octree_ray over n explicit rays (6 floats each: pos.xyz, dir.xyz; device pointers). */
int svo_trace_rays(svo_ctx *ctx, const float *rays, size_t n_rays, svo_hit *hits_out);

/* Duration of the most recent trace launch in ms (needs SVO_OPT_TIMING > 0); blocks on it. */
int svo_last_render_ms(svo_ctx *ctx, float *ms);
/* Durations (ms, oldest first) of the trace launches recorded since the last collect, at most the
 * ring size; blocks until they have finished and resets the record. */
int svo_timing_collect(svo_ctx *ctx, float *ms_out, size_t cap, size_t *n_out);

/* Diagnostic for profiling: n_loads single-dword buffer loads over the node buffer, lane i at byte i * stride_bytes
 * (the trace kernels' access shape), to calibrate hardware byte counters on a known line count. */
int svo_diag_gather(svo_ctx *ctx, uint32_t stride_bytes, uint32_t n_loads);

/* Diagnostic for the tests of the culling pass (SVO_OPT_CULL): the class byte of each of the first n_strips 64-pixel blocks of
 * the last pixel frame that ran the pass (block b of a width x height rectangle, 8x8 blocks row-major; 0xFF = culled: the pass
 * wrote the block's all-zero records and the trace never claimed it).  Blocking; SVO_ERR_STATE when that frame ran without it. */
int svo_diag_strip_classes(svo_ctx *ctx, uint8_t *host_out, size_t n_strips);

/* Diagnostic for the static deal (SVO_OPT_STATIC_DEAL), read-only and blocking.  status_out: frames traced by the replay kernel,
 * seeds asked for by the host, seeds and strips moved on the device, learning frames stepped since the last seed (16: over),
 * verdict (0 learning, 1 replay, 2 claims), table seeded (0/1), host knows "claims" (0/1), rows, entries per row, best replayed
 * frame (10 ns ticks: all waves; the sampled workgroups), the claiming kernel's last frame, the last stepped frame and its
 * moves, frames that still get a step.  table_out / stamps_out (or NULL): the first table_words words of the table (rows x
 * entries per row, 0xFFFFFFFF behind a row's last strip) and the first stamps_words of the per-wave stamps (2 per row). */
int svo_diag_deal(svo_ctx *ctx, uint32_t status_out[16], uint32_t *table_out, size_t table_words, uint32_t *stamps_out,
                  size_t stamps_words);

/* Diagnostic for the strip schedule, read-only and blocking: what schedule slot `slot` (0: primary frames, 1:
 * shadow and secondary rays) holds after the frames traced so far.  info_out: strips of the slot's work layout, entries reserved
 * per list, blocks per row the builder ranks column-major by (0: strip order), then the slot's state -- valid, lists filtered,
 * age, frames fed back, floored -- and zeros.  The first three describe the work layout of the slot's last rebuild (0 strips before the
 * first one) and say something about the buffers only while `valid` is set.  classes_out / classes_now_out (or NULL): the first n_classes class bytes as the
 * post pass measured them, and as the last filtered or floored build used them (0xFF: not in a list).  lists_out (or NULL): the
 * first list_words words of the 8 list lengths followed by the 8 lists (entries-per-list words each).  balance_out: the first 32
 * balance words -- [0..8] the cumulative shares, [18] updates, [20] best time, [21..29] best shares.  SVO_ERR_STATE when the
 * slot has no buffers (no scheduled STACK frame yet). */
int svo_diag_schedule(svo_ctx *ctx, int slot, uint32_t info_out[16], uint8_t *classes_out, size_t n_classes, uint8_t *classes_now_out,
                      uint32_t *lists_out, size_t list_words, uint32_t balance_out[32]);

/* Counter scan (compute.wgsl).  Lists hold `capacity` words: slot 0 = count, slots 1.. = indices. */
int svo_scan_dispatch(svo_ctx *ctx, uint32_t node_length);
int svo_scan_read(svo_ctx *ctx, uint32_t *sub, uint32_t *n_sub, uint32_t *unsub, uint32_t *n_unsub,
                  size_t capacity);

/* ---- procedural world generator (the reference's third kernel, procedual.wgsl) ----
 * A chunk covers the world cube [pos, pos + 2 / 2^base_depth)^3 with 2^chunk_depth cells per axis; cell (x, y, z) samples
 * the island's signed distance at world = pos + (cell / 2^(base_depth + chunk_depth)) * 2.  Solid cells (sdf < 0) are
 * block 3 (grass) when the cell one voxel above is outside (sdf > 0), else block 1 (stone).  The tree is the union of the
 * root-to-cell paths of the solid cells, breadth-first (root group at 0, each level's groups in the order of their
 * parents, so every level is in Morton order): interior word = index of the child group, leaf = SVO_CHUNK_OFFSET + block,
 * empty slot = SVO_CHUNK_OFFSET, colours 0.  Bit-exact and the same on every run. */
struct svo_cpu_octree;
struct svo_world;
typedef struct svo_proc_params {
    float pos[3];          /* the chunk's lower corner, world coordinates */
    uint32_t base_depth;   /* levels above the chunk (0..21); the reference passes world_depth */
    uint32_t chunk_depth;  /* 2..9 (the reference: 9); depth 1 is refused (the reference drops every depth-1 chunk) */
    uint64_t max_nodes;    /* cap on the chunk's node count; 0 = 256 000 000 (procedural.rs:4) */
} svo_proc_params;
/* *out = the chunk as a CpuOctree (caller frees it, or hands it to svo_world_insert), or NULL for a chunk without a solid
 * cell.  SVO_ERR_CAP (with a message) when the exact node count exceeds max_nodes.  Blocking. */
int svo_proc_generate_chunk(svo_ctx *ctx, const svo_proc_params *params, struct svo_cpu_octree **out);
/* World::generate_world into w's path, which must not exist yet (it is created): chunks x, y, z (that nesting) at
 * (x, y, z) * 2 / 2^world_depth - 1 with base_depth = world_depth, id SVO_CHUNK_OFFSET / 2 + i (i counts empty chunks
 * too); every non-empty chunk is inserted, mipped, saved as <id>.bin and reduced to its top_mip; the root (chunk 0)
 * references them and is saved as 0.bin.  Blocks 1..8 must be in w.  world_depth 1..4, chunk_depth 2..9. */
int svo_world_generate(svo_ctx *ctx, struct svo_world *w, uint32_t world_depth, uint32_t chunk_depth);
/* Diagnostics: the signed distance at n points (xyz: 3 floats each; host pointers, blocking), and one chunk's class
 * bytes (0 empty, 1 stone, 3 grass) in the reference's id order, id = x + side*y + side^2*z (host pointer, 8^chunk_depth
 * bytes, blocking). */
int svo_proc_sdf(svo_ctx *ctx, const float *xyz, size_t n, float *out);
int svo_proc_classify(svo_ctx *ctx, const svo_proc_params *params, uint8_t *cells_out);
/* Times (ms) of the last svo_proc_generate_chunk: [0] classify kernel, [1] occupancy pyramid and ranks, [2] emit (device
 * events); [3] host wall time until the nodes are emitted, [4] read-back copy, [5] CpuOctree build.  Of the last
 * svo_world_generate, summed over its chunks: [6] GPU (wall), [7] read-back (no CpuOctree is built: the chunks are
 * mipped on the device and written from the pinned stage), [8] mips (device events, and the root's on the host),
 * [9] chunk file writes. */
#define SVO_PROC_TIMES 10
int svo_proc_timing(svo_ctx *ctx, float ms_out[SVO_PROC_TIMES]);

/* ---- trees built on the GPU ----
 * Voxel i has cell (x, y, z), each in [0, 2^depth), and colour 0x00RRGGBB (Rgb::cpu_value; the low 24 bits count).  The
 * tree is the union of the voxels' root-to-leaf paths, every voxel a leaf at `depth`: what sequential put(p, leaf, depth)
 * builds with p = cell / 2^depth * 2 - 1, the last of several voxels in one cell winning.  Child index at level L:
 * x bit << 2 | y bit << 1 | z bit, bit depth - L.  Words in the GPU layout: interior = child group << 4, leaf =
 * (SVO_VOXEL_OFFSET + colour) << 4, empty = SVO_VOXEL_OFFSET << 4 (a colour-0 voxel is an empty leaf on an existing
 * path), hit counters 0; canonical breadth-first (root group at 0, each level's groups in the order of their parents):
 * svo_nodes_relayout(words, n, 32, ...) of the host-built tree.  The same words on every run and for any order of
 * distinct voxels.  Written from word 0 of the node buffer; *n_words_out = 8 * (1 + interior nodes below the root), 8
 * empty words for n == 0.
 * Errors leave the node buffer untouched: SVO_ERR_ARG for a bad depth, n >= 2^31, NULL xyz with n > 0, or a coordinate
 * outside [0, 2^depth) (checked on the device); SVO_ERR_CAP when the word count exceeds max_words, the capacity or 2^27;
 * SVO_ERR_STATE without a node buffer.  Runs on the ctx stream and blocks only to read the level counts back; the emit
 * is enqueued (a following svo_render on the stream sees the tree), ordered and recorded like svo_nodes_write, so every
 * context sharing the buffer rebuilds its top table.  Inputs must stay valid until svo_sync.  SVO_OPT_TREE_DEPTH is the
 * caller's to raise when depth exceeds it. */
typedef struct svo_build_params {
    uint32_t depth;          /* 1..21 (dense: 1..10) */
    uint32_t default_colour; /* used when colours == NULL */
    uint64_t max_words;      /* 0 = the node buffer's capacity; never above SVO_VOXEL_OFFSET */
} svo_build_params;
/* xyz: n * 3 u32 (x, y, z interleaved), colours: n u32 or NULL -- DEVICE pointers on the ctx's device */
int svo_nodes_build(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, const svo_build_params *p,
                    uint64_t *n_words_out);
/* grid: side^3 u32 (DEVICE), side = 2^depth, cell (x, y, z) at grid[(x * side + y) * side + z]; a cell is a voxel iff
 * non-zero, with the low 24 bits as its colour.  The same words as svo_nodes_build of the non-zero cells. */
int svo_nodes_build_dense(svo_ctx *ctx, const uint32_t *grid, const svo_build_params *p, uint64_t *n_words_out);
/* Times (ms) of the last build: [0] keys, [1] sort (0 for a dense grid), [2] levels, [3] count read-back, [4] emit (device
 * events; waits for the emit), [5] host wall time of the call. */
#define SVO_BUILD_TIMES 6
int svo_build_timing(svo_ctx *ctx, float ms_out[SVO_BUILD_TIMES]);

/* ---- a tree in the node buffer edited in place ----
 * Inserts and removes voxels in the first n_words words of the node buffer without rebuilding the tree.  Inputs as
 * svo_nodes_build: xyz n * 3 u32 and colours n u32 (0x00RRGGBB, the low 24 bits count) or NULL, DEVICE pointers on the
 * ctx's device, every coordinate in [0, 2^depth).
 * Afterwards the words [0, *n_words_out) are, bit for bit, what the host model makes of the same words with
 * put(p, leaf, depth), p = cell / 2^depth * 2 - 1, applied once per distinct cell in ascending Morton-key order (the
 * builder's key: child index x bit << 2 | y bit << 1 | z bit, level 1 in the top bits); of several voxels in one cell the
 * last in input order wins.  leaf = (SVO_VOXEL_OFFSET + (colour & 0xFFFFFF)) << 4, so a colour-0 voxel writes the empty
 * word: that is how a voxel is removed.  A leaf above `depth` on the way down is split into 8 EMPTY children -- the
 * reference's put_in_voxel (cpu_octree.rs:100-111) does not carry the coarse leaf's colour down, and neither does this.
 * Each new group is appended at the current end in the order the host creates them (by voxel, then by level), so
 * *n_words_out = n_words + 8 * (groups created).  Written words have hit counter 0; every other word keeps all 32 bits,
 * and nothing at or behind *n_words_out is touched.  The same words on every run and for any order of distinct cells.
 * SVO_ERR_STATE, nothing written, when a cell is an interior node at `depth` (the tree is finer there than the edit; the
 * host's put never ends on that input): svo_last_error names the input index of the first such voxel in key order.
 * Replacing a subtree by a coarser leaf (svo_nodes_edit_region does that) and reusing free groups are not done; groups that
 * became all-empty or were cut off are pruned and dropped afterwards, by svo_nodes_compact.
 * The other errors leave the node buffer untouched too, all decided by a read-only plan pass before any write:
 * SVO_ERR_ARG for a bad depth, n >= 2^31, NULL xyz with n > 0, a coordinate outside [0, 2^depth) (checked on the device),
 * or n_words not a positive multiple of 8 or above the capacity; SVO_ERR_CAP when the exact new length exceeds max_words,
 * the capacity or 2^27; SVO_ERR_STATE without a node buffer (or for words whose pointers lead outside [0, n_words)).
 * n == 0 succeeds and returns n_words.
 * Runs on the ctx stream and blocks once, to read the counts and the status back; the writes are enqueued (a following
 * svo_render on the stream sees the edit), ordered and recorded like svo_nodes_write, so every context sharing the buffer
 * rebuilds its top table and schedule.  Inputs must stay valid until svo_sync.  SVO_OPT_TREE_DEPTH is the caller's to
 * raise when depth exceeds it. */
typedef struct svo_edit_params {
    uint32_t depth;          /* 1..21: the level of the edited voxels */
    uint32_t default_colour; /* used when colours == NULL */
    uint64_t n_words;        /* the tree's current length: a multiple of 8, at least 8 */
    uint64_t max_words;      /* 0 = the node buffer's capacity; never above SVO_VOXEL_OFFSET */
} svo_edit_params;
int svo_nodes_edit(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, const svo_edit_params *p,
                   uint64_t *n_words_out);
/* Times (ms) of the last edit: [0] keys, [1] sort, [2] plan (leaf pass, walk, scan), [3] status read-back, [4] fill and
 * link (device events; waits for the link), [5] host wall time of the call.  All 0 after an empty edit. */
#define SVO_EDIT_TIMES 6
int svo_edit_timing(svo_ctx *ctx, float ms_out[SVO_EDIT_TIMES]);

/* ---- a tree in the node buffer edited by shapes: boxes and balls filled, carved and painted ----
 * Edits the first n_words words of the node buffer in place, top-down, touching only the tree along the shapes' surfaces.
 * Per cell c of the `depth` grid the call means this:
 *     v = what svo_nodes_sample returns at c
 *     for each shape, in input order:
 *         if c is inside the shape and (v == 0 ? mode & SVO_REGION_EMPTY : mode & SVO_REGION_VOXELS):  v = colour & 0xFFFFFF
 * and afterwards the tree samples to the final v in every cell.  Inside a box: lo <= c < hi on every axis (half-open, lo <
 * hi <= 2^depth).  Inside a ball: the cell's centre lies within the radius; with the centre and the radius given in HALF
 * cells that is sum over the axes of (2 c + 1 - centre2)^2 <= radius2^2, in 64-bit integers (a term is below 2^46): no float
 * anywhere.  A ball of radius 0 on an odd centre is one cell, on an even centre none.
 * The words are deterministic, the same bytes on every run (no atomics: the order is the contract), by this rule.  A word of
 * level l with cell q covers the cells [q << s, (q + 1) << s), s = depth - l.  Against that cube a shape is FULL (every cell
 * inside), OUT (none) or PART; for a ball the class is exact: per axis the centres run over the odd integers a = 2 (q << s)
 * + 1 .. b = 2 ((q + 1) << s) - 1, the farthest is at max(|a - C|, |b - C|), the nearest at a - C (C < a), C - b (C > b), else
 * 0 (C odd) or 1 (C even); FULL iff sum far^2 <= r^2, OUT iff sum near^2 > r^2.  At l == depth nothing is PART.
 * The tree is processed level by level from the root group; the frontier of level l + 1 is the eight children, by child
 * index, of every word of level l that was opened or split, those taken in frontier order.  For one word:
 *     every shape OUT:  the word and everything below it keep all 32 bits
 *     otherwise j = the last shape that is FULL with mode SVO_REGION_SET, or none, and
 *     a leaf of value v0 (a voxel, the empty word, or a virtual child of a split):
 *         v = colour_j (v0 without a j); for each shape k behind j, in order: FULL: apply it to v as above; PART: when
 *         applying it would change v, the leaf is SPLIT.  Not split: v != v0 writes the leaf word of v, counter 0; v == v0
 *         leaves the word untouched.  Split: a new group of eight leaf words OF v0, counter 0, is made, the word becomes the
 *         pointer to it, and the eight virtual children join the next frontier.  THE COLOUR IS CARRIED DOWN -- unlike
 *         svo_nodes_edit, which splits a coarse leaf into empty children
 *     an interior word:  with a j and every later shape OUT it COLLAPSES to the leaf word of colour_j (its subtree is cut off,
 *         for svo_nodes_compact to drop); otherwise it is opened.  Opening at l == depth is refused: SVO_ERR_STATE, nothing
 *         written, svo_last_error names the last shape that touches the cell and the cell
 * New groups are appended by level and within a level in frontier order: the g-th split gets the group n_words + 8 g, and
 * *n_words_out = n_words + 8 * splits.  Nothing at or behind *n_words_out is touched.  A second identical call on the result
 * writes nothing and appends nothing.  Merging equal siblings, reusing free groups and other shapes are not done.
 * `shapes` is HOST memory, read before the call returns.  Every error is decided by the read-only plan before any write.
 * SVO_ERR_ARG: NULL p or n_words_out, NULL shapes with n_shapes > 0, n_shapes > SVO_REGION_MAX_SHAPES, depth outside 1..21, an
 * unknown kind, a mode outside 1..3, a box with lo >= hi or hi > 2^depth on an axis, a ball with a centre coordinate above
 * 2^(depth + 1) or a radius above 2^23 half cells, n_words not a positive multiple of 8 or above the capacity.  SVO_ERR_STATE: no
 * node buffer; a device adaptive state attached to the context (subtrees are cut off under its positions); the "malformed
 * tree: ..." causes with svo_nodes_compact's wording, on the words that the shapes make the call open (an interior pointer
 * that is not a multiple of 8 or with pointer + 8 > n_words, a group reached twice); the refusal above.  SVO_ERR_CAP when the exact new length exceeds
 * max_words, the capacity or 2^27.  n_shapes == 0 succeeds and returns n_words.
 * Runs on the ctx stream; blocks once per level, to read back the next frontier's size and the level's split count, and once
 * more for the status.  The fill and the writes are enqueued (a following svo_render on the stream sees the edit), ordered and
 * recorded like svo_nodes_write, so every context sharing the buffer rebuilds its top table and schedule. */
#define SVO_REGION_BOX  0u
#define SVO_REGION_BALL 1u
#define SVO_REGION_EMPTY  1u   /* the shape applies to cells that are empty */
#define SVO_REGION_VOXELS 2u   /* ... to cells that hold a voxel */
#define SVO_REGION_SET    3u   /* both: fill (colour != 0) or carve (colour 0) */
#define SVO_REGION_MAX_SHAPES 1024u
typedef struct svo_region_shape {   /* 32 bytes, HOST memory */
    uint16_t kind;    /* SVO_REGION_BOX or SVO_REGION_BALL */
    uint16_t mode;    /* 1, 2 or 3 */
    uint32_t colour;  /* 0x00RRGGBB, the low 24 bits count; 0 = empty */
    uint32_t a[3];    /* box: lo (cells);  ball: the centre in HALF cells, [0, 2^(depth+1)] */
    uint32_t b[3];    /* box: hi (cells);  ball: b[0] = the radius in half cells, <= 2^23, b[1] = b[2] = 0 */
} svo_region_shape;
typedef struct svo_region_params {
    uint32_t depth;      /* 1..21: the grid the shapes are given on */
    uint32_t reserved;
    uint64_t n_words;    /* the tree's current length: a multiple of 8, at least 8 */
    uint64_t max_words;  /* 0 = the node buffer's capacity; never above SVO_VOXEL_OFFSET */
} svo_region_params;
int svo_nodes_edit_region(svo_ctx *ctx, const svo_region_shape *shapes, size_t n_shapes, const svo_region_params *p,
                          uint64_t *n_words_out);
/* Times (ms) of the last shape edit: [0] plan (with its per-level read-backs), [1] status, [2] fill, [3] write (device
 * events; waits for the write), [4] host wall time of the call.  All 0 after a call without shapes; a refused call leaves
 * the times of the last one that ran. */
#define SVO_REGION_TIMES 5
int svo_region_timing(svo_ctx *ctx, float ms_out[SVO_REGION_TIMES]);

/* ---- two device trees combined: paste, fill, paint, carve and mask by a tree ----
 * Edits the scene A, the first n_words words of the node buffer, in place by the source B, the src_words words at src_dev (a
 * DEVICE buffer on the ctx's device, rooted at group 0, ONLY READ), top-down, touching only the words where both trees have
 * something to say.  A leaf's value is (word >> 4) - SVO_VOXEL_OFFSET, all bits; 0 means empty; the source's hit counters are
 * ignored.  The source's root cube is the scene's cell `at` of level at_level (0: the whole cube).  Per cell, with s = depth -
 * at_level: a cell c of the `depth` grid with c >> s == at samples (svo_nodes_sample) afterwards to f(a, b), a = what the scene
 * sampled at c before, b = what the source samples at c - (at << s) on a grid of depth s, and f by op:
 *     OVER   b ? b : a          UNDER  a ? a : b          PAINT    (a && b) ? b : a
 *     CARVE  b ? 0 : a          KEEP   b ? a : 0          REPLACE  b
 * Every cell outside the cube samples as before.
 * The words are deterministic, the same bytes on every run (no atomics: the order is the contract), by this rule.  The tree is
 * processed level by level from the root group; the frontier of level l + 1 is the eight children, by child index, of every
 * word of level l that was opened or split, those taken in frontier order.  A frontier entry pairs a scene word -- real, or a
 * virtual child of a split, which holds one leaf value -- with what the source has for the same cube: OUT (the cube lies outside
 * the source's), PATH (a level above at_level on the way to `at`: as an interior word whose child towards `at` is PATH again, or
 * at at_level the source's root, an interior word pointing at the source's group 0, and whose seven other children are OUT), a
 * source leaf b or the constant b carried down from one, or a source interior word.  With at_level == 0 the level-1 frontier is
 * the scene's root group against the source's root group.  For one entry:
 *     source OUT:  the scene word and everything below it keep all 32 bits
 *     source leaf or constant b, scene leaf a:  v = f(a, b); v != a writes the leaf word of v, counter 0; otherwise untouched
 *     source leaf or constant b, scene interior:  by f(., b).  The identity (OVER, UNDER, PAINT, CARVE with b == 0; KEEP with b
 *         != 0): untouched with its subtree.  A constant c (OVER with b != 0: b; CARVE with b != 0: 0; KEEP with b == 0: 0;
 *         REPLACE: b): the word COLLAPSES to the leaf word of c (its subtree is cut off, for svo_nodes_compact to drop).
 *         Otherwise (UNDER, PAINT with b != 0) it is OPENED: its eight children are each paired with the constant b
 *     source interior or PATH, scene interior:  both are opened, their children paired by child index
 *     source interior or PATH, scene leaf a (real or virtual):  when f(a, .) is a whatever the source holds (UNDER with a != 0;
 *         PAINT, CARVE, KEEP with a == 0) untouched, and the source below is not looked at.  Otherwise it is SPLIT: a new group
 *         of eight leaf words OF a, counter 0, is made, the word becomes the pointer to it, and the eight virtual children are
 *         paired with the source's children.  THE COLOUR IS CARRIED DOWN, as in svo_nodes_edit_region and unlike svo_nodes_edit
 * Opening or splitting at level `depth` is refused: SVO_ERR_STATE, nothing written, svo_last_error names the cell and which
 * tree is finer there.  No word below level `depth` is made or opened.
 * New groups are appended by level and within a level in frontier order: the g-th split gets the group n_words + 8 g, and
 * *n_words_out = n_words + 8 * splits.  Nothing at or behind *n_words_out is touched.  A second identical call on the result
 * writes nothing and appends nothing.  Merging equal siblings is svo_nodes_simplify's job afterwards; free groups are not
 * reused.  A source group reached through two pointers is allowed: the source is only read, the result holds copies, and
 * `depth` ends any cycle.
 * Every error is decided by a read-only plan before any write; of several causes the first in this order is reported.
 * SVO_ERR_ARG: NULL p, n_words_out or src_dev; op > 5; depth outside 1..21; at_level >= depth; an `at` coordinate >= 2^at_level.
 * SVO_ERR_STATE: no node buffer; a device adaptive state attached to the context.  SVO_ERR_ARG: n_words not a positive multiple
 * of 8 or above the capacity; src_words not a positive multiple of 8 or above 2^27; [src_dev, src_dev + src_words) overlapping
 * the node buffer's allocation.  SVO_ERR_STATE: the "malformed tree: ..." causes with svo_nodes_compact's wording, on the scene
 * words that the call opens (an interior pointer that is not a multiple of 8 or with pointer + 8 > n_words, a group reached
 * twice); "malformed source: ..." for a source pointer that the call follows and that is not a multiple of 8 or has pointer + 8
 * > src_words; the refusal above.  SVO_ERR_CAP when the exact new length exceeds max_words, the capacity or 2^27.
 * Runs on the ctx stream; the source's words must be complete when the call is made.  Blocks once per level, to read back the
 * next frontier's size and the level's split count, and once more for the status.  The fill and the writes are enqueued (a
 * following svo_render on the stream sees the result), ordered and recorded like svo_nodes_write, so every context sharing the
 * buffer rebuilds its top table and schedule. */
#define SVO_COMBINE_OVER    0u  /* f(a,b) = b ? b : a        paste: the source's voxels over the scene */
#define SVO_COMBINE_UNDER   1u  /* f(a,b) = a ? a : b        fill: the source's voxels into the scene's empty cells */
#define SVO_COMBINE_PAINT   2u  /* f(a,b) = (a && b) ? b : a recolour the scene's voxels where the source has one */
#define SVO_COMBINE_CARVE   3u  /* f(a,b) = b ? 0 : a        remove the scene where the source is solid */
#define SVO_COMBINE_KEEP    4u  /* f(a,b) = b ? a : 0        keep the scene only where the source is solid */
#define SVO_COMBINE_REPLACE 5u  /* f(a,b) = b                the source's cube as it is, empties included */
typedef struct svo_combine_params {
    uint32_t op;         /* 0..5 */
    uint32_t depth;      /* 1..21: the scene grid; no word below this level is made or opened */
    uint32_t at_level;   /* 0..depth-1: the source's root cube is the scene's cell `at` of this level (0: the whole cube) */
    uint32_t at[3];      /* < 2^at_level each */
    uint64_t n_words;    /* the scene: words [0, n_words) of the node buffer */
    uint64_t src_words;  /* the source: words [0, src_words) at src_dev, rooted at group 0 */
    uint64_t max_words;  /* 0 = the capacity; never above SVO_VOXEL_OFFSET */
} svo_combine_params;
int svo_nodes_combine(svo_ctx *ctx, const uint32_t *src_dev, const svo_combine_params *p, uint64_t *n_words_out);
/* Times (ms) of the last combine: [0] plan (with its per-level read-backs), [1] status, [2] fill, [3] write (device events;
 * waits for the write), [4] host wall time of the call.  A refused call leaves the times of the last one that ran. */
#define SVO_COMBINE_TIMES 5   /* plan (with its per-level read-backs), status, fill, write, host wall */
int svo_combine_timing(svo_ctx *ctx, float ms_out[SVO_COMBINE_TIMES]);

/* ---- a device tree placed into the scene at any cell offset and orientation ----
 * svo_nodes_combine without the condition that the source's cube is a cell of the scene's octree.  The scene A is the first
 * n_words words of the node buffer on a grid of depth `depth` (side N); the source B is the src_words words at src_dev (DEVICE,
 * rooted at group 0, ONLY READ, hit counters ignored) on a grid of depth src_depth (side S) WITH THE SAME CELLS: one cell of the
 * source is one cell of the scene.  `offset` is in cells.  orient = 8 p + 4 fx + 2 fy + fz is one of the cube's 48 symmetries:
 * p indexes the axis permutations in lexicographic order, (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0), and the ORIENTED
 * source has at cell r what the source has at q, with r[i] = f_i ? S - 1 - q[perm[i]] : q[perm[i]]; 0 is the identity.
 * Per cell c of the `depth` grid, with r = c - offset: when r lies in [0, S)^3 the cell samples (svo_nodes_sample) afterwards
 * to f(a, b), a = what the scene sampled at c before, b = the oriented source at r, f by op as svo_nodes_combine's
 * (SVO_COMBINE_OVER .. SVO_COMBINE_REPLACE).  Every other cell samples as before: a source partly outside the scene is clipped,
 * one wholly outside writes nothing and *n_words_out = n_words.
 * The words are deterministic, the same bytes on every run (no atomics: the order is the contract), by this rule.  The walk is
 * svo_nodes_combine's: level by level from the scene's root group, the frontier of level l + 1 the eight children, by child
 * index, of every word of level l that was opened or split, those taken in frontier order; the g-th split gets the group
 * n_words + 8 g, *n_words_out = n_words + 8 * splits, and nothing at or behind *n_words_out is touched.
 * ITEMS.  A scene word of level l has cells of z = 2^(depth - l) and faces the cells of size z of the oriented source's grid
 * that its cube overlaps: per axis one when (-offset) mod z == 0 and two otherwise, so 1, 2, 4 or 8, the same count for every
 * word of a level, and one at level `depth`.  Each such item is OUT (outside the source's cube), a constant b (a source leaf,
 * or carried down from one), a source interior word, or, when z >= S, the cell at the origin that holds the source's cube:
 * with z == S the root, as an interior word pointing at the source's group 0, and with z > S a virtual word whose child
 * (0,0,0) leads on towards the root and whose other seven are OUT.  A virtual word holds the source's cube in its corner and
 * nothing else, so only a scene word whose cube overlaps the source's cube faces it: for a word beside the cube (x z - offset
 * >= S on an axis) the item is OUT.  A group's record holds the eight items of its parent's
 * cell; a word's items are children of those: per axis, with h = ((-offset) mod 2 z) >= z, item j (0, or 1 where there are
 * two) of child c is the child (c + h + j) & 1 of the parent's item (c + h + j) >> 1.  The oriented child index r maps to the
 * source's child index by one fixed permutation of 0..7, the same at every level (bit perm[i] of the source's index is bit i
 * of r, flipped when f_i); it is not applied above the root.
 * NORMALISATION, THEN THE DECISION.  For OVER, UNDER, PAINT and CARVE, where f(a, 0) = a, OUT counts as the constant 0; for KEEP
 * and REPLACE it stays a kind of its own.  For CARVE and KEEP every b != 0 counts as one value.  Then:
 *     all items OUT:  the scene word and everything below it keep all 32 bits
 *     all items one constant b:  svo_nodes_combine's "source leaf or constant b" rule: overwrite, identity, collapse, or open
 *         with the children facing the children of the same items
 *     anything else:  svo_nodes_combine's "source interior" rule: a scene interior word is opened; a scene leaf a stays
 *         untouched when f(a, .) is a whatever the source holds; any other leaf is SPLIT, its colour carried into eight new leaf
 *         words, counter 0, and the children are paired with their own items.  A coarse leaf may so be split where all cells
 *         come out equal again (its items differed only in kind); svo_nodes_simplify merges those afterwards
 * Opening or splitting at level `depth` is refused as svo_nodes_combine refuses it: the scene is finer there than `depth`, or
 * the source finer than src_depth.  SVO_ERR_STATE, nothing written, svo_last_error names the cell and the finer tree.
 * With orient 0, src_depth = depth - at_level and offset = at << src_depth the words are byte for byte those of
 * svo_nodes_combine: above at_level the words that overlap the source's cube are the path to `at`.  A second identical call on
 * the result writes nothing and appends nothing.
 * Every error is decided by a read-only plan before any write; of several causes the first in this order is reported.
 * SVO_ERR_ARG: NULL p, n_words_out or src_dev; op > 5; depth outside 1..21; src_depth outside 1..depth; orient >= 48; an offset
 * outside [-2^21, 2^21].  Then svo_nodes_combine's, from "no node buffer" on, with "malformed source: ..." for a source pointer
 * that the call follows: an interior item of a word that is opened or split.
 * Stream ordering, blocking (once per level and once for the status) and the recording of the write for the contexts that share
 * the buffer are svo_nodes_combine's. */
#define SVO_PLACE_ORIENTS 48u
typedef struct svo_place_params {
    uint32_t op;         /* SVO_COMBINE_OVER .. SVO_COMBINE_REPLACE */
    uint32_t depth;      /* 1..21: the scene grid; no word below this level is made or opened */
    uint32_t src_depth;  /* 1..depth: the source's cube has 2^src_depth cells a side */
    uint32_t orient;     /* 0..47: 8 p + 4 fx + 2 fy + fz; 0 = as it is */
    int32_t offset[3];   /* the scene cell of the oriented source's cell (0,0,0): -2^21..2^21 each */
    uint32_t reserved;
    uint64_t n_words;    /* the scene: words [0, n_words) of the node buffer */
    uint64_t src_words;  /* the source: words [0, src_words) at src_dev, rooted at group 0 */
    uint64_t max_words;  /* 0 = the capacity; never above SVO_VOXEL_OFFSET */
} svo_place_params;
int svo_nodes_place(svo_ctx *ctx, const uint32_t *src_dev, const svo_place_params *p, uint64_t *n_words_out);
/* Times (ms) of the last placement: [0] plan (with its per-level read-backs), [1] status, [2] fill, [3] write (device events;
 * waits for the write), [4] host wall time of the call.  A refused call leaves the times of the last one that ran. */
#define SVO_PLACE_TIMES 5   /* plan (with its per-level read-backs), status, fill, write, host wall */
int svo_place_timing(svo_ctx *ctx, float ms_out[SVO_PLACE_TIMES]);

/* ---- a device tree placed into the scene under any affine map: free turns, scale, shear ----
 * svo_nodes_place with the signed permutation and the cell offset replaced by a fixed-point affine map FROM SCENE CELLS TO
 * SOURCE CELLS, sampled at cell centres, nearest cell.  The scene A is the first n_words words of the node buffer on a grid of
 * depth `depth`; the source B is the src_words words at src_dev (DEVICE, rooted at group 0, ONLY READ, hit counters ignored) on a
 * grid of depth src_depth (side S), which `depth` does not bound: the source's cells need not be the scene's, the matrix says
 * how they relate.  matrix is row-major Q16 (value / 65536), translate Q16 in source cells.  The map is the one the rule needs,
 * scene to source (the inverse of "turn the model, then put it there"); a singular matrix is allowed, it is still a sampling rule.
 * Per cell c of the `depth` grid, in int64:
 *     P_i = sum_j matrix[i][j] * (2 c_j + 1) + 2 translate[i]      2^17 times A (c + 1/2) + t
 *     q_i = P_i >> 17                                               an arithmetic shift: floor
 * When q lies in [0, S)^3 the cell samples (svo_nodes_sample) afterwards to f(a, b), a = what the scene sampled at c before,
 * b = what the source samples at q, the leaf that holds q, coarse leaves included, f by op as svo_nodes_combine's
 * (SVO_COMBINE_OVER .. SVO_COMBINE_REPLACE).  Every other cell samples as before.  With the bounds below |P| < 2^45: nothing
 * overflows.  Point sampling aliases where the map shrinks the source; svo_nodes_simplify with a cut level on the source first
 * is the remedy.
 * The words are deterministic, the same bytes on every run (integers only, scans, no atomics), by this rule.  The walk is
 * svo_nodes_combine's: level by level from the scene's root group, the frontier of level l + 1 the eight children, by child
 * index, of every word of level l that was opened or split, those taken in frontier order; the g-th split gets the group
 * n_words + 8 g, *n_words_out = n_words + 8 * splits, and nothing at or behind *n_words_out is touched.
 * A WORD'S SOURCE BOX.  A scene word of level l with cell (x, y, z) has zc = 2^(depth - l) cells a side.  All source cells that
 * its cells can sample lie in a box, per source axis i:
 *     mid_i = sum_j matrix[i][j] * (2 cell_j zc + zc) + 2 translate[i]        rad_i = (zc - 1) * sum_j |matrix[i][j]|
 *     qlo_i = (mid_i - rad_i) >> 17                                           qhi_i = (mid_i + rad_i) >> 17
 * exact interval arithmetic over the cube's cell centres; at level `depth` the box is the one cell q above.
 * ITEMS.  With e = max_i (qhi_i - qlo_i + 1), s = min(src_depth, ceil(log2 e)) and k = src_depth - s, the word faces the cells
 * of the source's level-k grid, continued beyond the cube, that the box meets: the indices qlo_i >> s .. qhi_i >> s per axis, at
 * most two per axis unless e > S.  Each such item is OUT (outside [0, 2^k)^3), a constant b (a source leaf on the way down from
 * the root, carried down, or a leaf at level k) or a source interior word; at k = 0 the root, as an interior word pointing at
 * the source's group 0.  Only the set of kinds and values matters: with e > S every met cell but index 0 is OUT, and OUT counts
 * once.
 * NORMALISATION, THEN THE DECISION are svo_nodes_place's, word for word: all items OUT, the word and everything below keep all
 * 32 bits; all items one constant, svo_nodes_combine's leaf rule; anything else its interior rule, which opens an interior
 * word, leaves a leaf that f(a, .) = a lets stay and splits any other leaf with its colour carried.  Opening or splitting at
 * level `depth` is refused as svo_nodes_place refuses it: SVO_ERR_STATE, nothing written, svo_last_error names the cell and the
 * finer tree.
 * With the matrix a signed permutation times 65536 and a whole-cell translation, matrix[perm[i]][i] = f_i ? -65536 : 65536 and
 * translate[perm[i]] = 65536 * (f_i ? S + offset_i : -offset_i) in svo_nodes_place's terms, the words are byte for byte those
 * of svo_nodes_place: then e == zc on every level, so the level-k cells are the cells of the word's own size and the items are
 * svo_nodes_place's.
 * Every error is decided by a read-only plan before any write; of several causes the first in this order is reported.
 * SVO_ERR_ARG: NULL p, n_words_out or src_dev; op > 5; depth outside 1..21; src_depth outside 1..21; a matrix entry outside
 * [-2^20, 2^20]; a translation outside [-2^40, 2^40].  Then svo_nodes_place's, from "no node buffer" on, with "malformed
 * source: ..." for a source pointer that the call follows, unaligned or leaving src_words: one on the way down to a word's
 * items, or an interior item of a word that is opened or split.  No source pointer is followed before it is checked.
 * Stream ordering, blocking (once per level and once for the status) and the recording of the write for the contexts that share
 * the buffer are svo_nodes_combine's. */
typedef struct svo_transform_params {
    uint32_t op;           /* SVO_COMBINE_OVER .. SVO_COMBINE_REPLACE */
    uint32_t depth;        /* 1..21: the scene grid; no word below this level is made or opened */
    uint32_t src_depth;    /* 1..21: the source's cube has 2^src_depth cells a side; not bound by depth */
    int32_t matrix[9];     /* scene cells -> source cells, row-major Q16: -2^20..2^20 each */
    int64_t translate[3];  /* Q16, in source cells: -2^40..2^40 each */
    uint64_t n_words;      /* the scene: words [0, n_words) of the node buffer */
    uint64_t src_words;    /* the source: words [0, src_words) at src_dev, rooted at group 0 */
    uint64_t max_words;    /* 0 = the capacity; never above SVO_VOXEL_OFFSET */
} svo_transform_params;
int svo_nodes_transform(svo_ctx *ctx, const uint32_t *src_dev, const svo_transform_params *p, uint64_t *n_words_out);
/* Times (ms) of the last transform: [0] plan (with its per-level read-backs), [1] status, [2] fill, [3] write (device events;
 * waits for the write), [4] host wall time of the call.  A refused call leaves the times of the last one that ran. */
#define SVO_TRANSFORM_TIMES 5   /* plan (with its per-level read-backs), status, fill, write, host wall */
int svo_transform_timing(svo_ctx *ctx, float ms_out[SVO_TRANSFORM_TIMES]);

/* ---- one step of morphology on the device tree: grow, shrink ----
 * Edits the first n_words words of the node buffer in place, on a grid of depth `depth`, by one step of dilation (GROW) or
 * erosion (SHRINK) under conn = 6, 18 or 26 neighbours: the offsets d in {-1,0,1}^3, d != 0, with |dx| + |dy| + |dz| <= 1, 2, 3.
 * Per cell c of the grid, with a = what svo_nodes_sample gives at c before the call, the tree samples afterwards to
 *     GROW    a != 0: a.  Otherwise take conn's offsets in PRIORITY ORDER, ascending (|d|_1, dx, dy, dz) with -1 < 0 < 1 (faces
 *             before edges before corners), and let b be the value before the call at the first c + d that lies inside the grid
 *             and is not empty: the cell becomes colour ? colour : b (colour 0 INHERITS the neighbour's value); without such
 *             a d it stays 0
 *     SHRINK  a == 0: 0.  Otherwise 0 when some d of conn has c + d empty before the call -- with SVO_MORPH_OPEN_BOUNDARY a
 *             c + d outside the grid counts as empty too -- and a when none has
 * Without the flag the outside is neutral for both ops: it never changes a cell.
 * The words are deterministic, the same bytes on every run (no atomics: the order is the contract), by this rule.  The tree is
 * processed level by level from the root group; the frontier of level l + 1 is the eight children, by child index, of every
 * word of level l that was opened or split, those taken in frontier order.  A frontier entry is a scene word -- real, or a
 * virtual child of a split, which holds one leaf value -- with 27 ITEMS: for each e in {-1,0,1}^3 the cell q + e of the word's
 * own level, q its cell, as it was BEFORE the call.  An item is OUT (outside the grid), a constant (a leaf's value, carried down
 * unchanged from a coarser leaf) or an interior word of the scene.  A group's record holds the 27 items of its parent's cell;
 * item d of child c is, per axis with t = c + d in -1..2, the child t & 1 of the parent's item floor(t / 2).  The root group's
 * parent is the whole grid, an interior word pointing at group 0 with OUT on all sides.
 * NORMALISATION, THEN THE DECISION.  For GROW, OUT is the constant 0; for SHRINK a constant that is set, or 0 with
 * SVO_MORPH_OPEN_BOUNDARY.  An item is QUIET when it is a constant that cannot change the word: 0 for GROW, any set value for
 * SHRINK.  Only the items with d in conn COUNT, on coarse levels too: every neighbour of a cell of the word lies in the word or in
 * one of those.  For one entry:
 *     an interior word:  opened.  At level `depth` that is the refusal below: the tree is finer than `depth` there
 *     a leaf that the op cannot change (GROW: a voxel; SHRINK: the empty word):  untouched; its items are not looked at
 *     any other leaf, every counting item quiet:  untouched
 *     any other leaf at level `depth`, some counting item not quiet:  a counting item that is interior is the REFUSAL:
 *         SVO_ERR_STATE, nothing written, svo_last_error says "finer than depth" and names the cell.  Otherwise the leaf word
 *         of the per-cell value is written, counter 0
 *     any other leaf above level `depth`, some counting item not quiet:  SPLIT: a new group of eight leaf words OF ITS VALUE,
 *         counter 0, is made, the word becomes the pointer to it as svo_nodes_edit_region writes it, and the eight virtual
 *         children join the next frontier.  A coarse leaf may so be split where its cells come out equal again
 * New groups are appended by level and within a level in frontier order: the g-th split gets the group n_words + 8 g, and
 * *n_words_out = n_words + 8 * splits.  Nothing at or behind *n_words_out is touched; untouched words keep all 32 bits.  Merging
 * the equal siblings that splits leave behind is svo_nodes_simplify's job afterwards; free groups are not reused.  THE WHOLE TREE
 * IS WALKED, every interior word being opened: a merged tree (svo_nodes_simplify) is the cheap input.
 * Every error is decided by a read-only plan before any write; of several causes the first in this order is reported.
 * SVO_ERR_ARG: NULL p or n_words_out; op > 1; conn not 6, 18 or 26; depth outside 1..21; unknown flag bits; colour != 0 with
 * SHRINK.  SVO_ERR_STATE: no node buffer; a device adaptive state attached to the context.  SVO_ERR_ARG: n_words not a positive
 * multiple of 8 or above the capacity.  SVO_ERR_STATE: the "malformed tree: ..." causes with svo_nodes_compact's wording (an
 * interior pointer that is not a multiple of 8 or with pointer + 8 > n_words, a group reached twice), on every word that the call
 * opens and on every interior item it reads behind, each checked before the level that follows it; the refusal above.
 * SVO_ERR_CAP when the exact new length exceeds max_words, the capacity or 2^27.
 * Stream ordering, blocking (once per level and once for the status) and the recording of the write for the contexts that share
 * the buffer are svo_nodes_edit_region's. */
#define SVO_MORPH_GROW   0u
#define SVO_MORPH_SHRINK 1u
#define SVO_MORPH_OPEN_BOUNDARY 1u   /* flags: outside the grid counts as empty (only SHRINK can tell) */
typedef struct svo_morph_params {
    uint32_t op;         /* SVO_MORPH_GROW, SVO_MORPH_SHRINK */
    uint32_t conn;       /* 6, 18 or 26 */
    uint32_t depth;      /* 1..21: the grid of the cells; no word below this level is made or opened */
    uint32_t flags;      /* SVO_MORPH_OPEN_BOUNDARY */
    uint32_t colour;     /* GROW: the value of new cells, low 24 bits; 0 = inherit.  SHRINK: must be 0 */
    uint32_t reserved;
    uint64_t n_words;    /* the tree's current length: a multiple of 8, at least 8 */
    uint64_t max_words;  /* 0 = the node buffer's capacity; never above SVO_VOXEL_OFFSET */
} svo_morph_params;
int svo_nodes_morph(svo_ctx *ctx, const svo_morph_params *p, uint64_t *n_words_out);
/* Times (ms) of the last morphology step: [0] plan (with its per-level read-backs), [1] status, [2] fill, [3] write (device
 * events; waits for the write), [4] host wall time of the call.  A refused call leaves the times of the last one that ran. */
#define SVO_MORPH_TIMES 5   /* plan (with its per-level read-backs), status, fill, write, host wall */
int svo_morph_timing(svo_ctx *ctx, float ms_out[SVO_MORPH_TIMES]);

/* ---- a tree in the node buffer shaped by a height map: terrain raised, lowered and layered ----
 * Edits the first n_words words of the node buffer in place, top-down, touching only the tree along the ground's surface.
 * heights_dev (DEVICE, size_xz[0] * size_xz[1] u32, ONLY READ): heights_dev[i * size_xz[1] + k] is the height of the column
 * (origin_xz[0] + i, origin_xz[1] + k) of the `depth` grid, z fastest as in svo_nodes_column_tops and y up.  h = min(height,
 * 2^depth) is the column's number of ground cells: the cells y < h are below the ground, h == 0 is a column with none; a height
 * above the grid, 0xFFFFFFFF included, is clamped and no error.  With T_k = thickness_0 + .. + thickness_k (64 bits) the call
 * means this per cell c = (x, y, z) of the grid, v being what svo_nodes_sample returns at c:
 *     the column (x, z) outside the rectangle:  v stays
 *     y <  h and (v == 0 ? mode_below & SVO_REGION_EMPTY : mode_below & SVO_REGION_VOXELS):  v = layers[k].colour & 0xFFFFFF, k the
 *               first layer with h - 1 - y < T_k, or n_layers - 1 without one: the last layer's thickness is ignored, it reaches
 *               down to y = 0; a thickness of 0 elsewhere is a band that holds no cell; a layer of colour 0 is empty
 *     y >= h and (v == 0 ? mode_above & SVO_REGION_EMPTY : mode_above & SVO_REGION_VOXELS):  v = colour_above & 0xFFFFFF
 * and afterwards the tree samples to that v in every cell.  A mode of 0 leaves its side of the ground alone.
 * The words are deterministic, the same bytes on every run (no atomics: the order is the contract), by this rule.  The frontier,
 * its order and the appends are svo_nodes_edit_region's.  A word of level l with cell q covers the cube of S = 2^s cells, s =
 * depth - l, at (x0, y0, z0) = q << s.  `meets`: the cube's xz footprint meets the rectangle; `inside`: it lies within it; hmin,
 * hmax: the extremes of h over the footprint's columns WITHIN THE RECTANGLE; band(d): the layer index above.  Then
 *     k_lo = band(max(hmin - y0 - S, 0)),  k_hi = band(max(hmax - 1 - y0, 0))
 *     has_above = meets && y0 + S > hmin,  has_below = meets && y0 < hmax
 *     all_above = meets && y0 >= hmax,     all_below = meets && y0 + S <= hmin && k_lo == k_hi
 * The word's candidates are (mode_above, colour_above) when has_above && mode_above, and (mode_below, layers[k].colour) for k_lo
 * <= k <= k_hi when has_below && mode_below.  For one word:
 *     no candidate:  the word and everything below it keep all 32 bits
 *     UNIFORM, `inside` and (all_above or all_below), the one candidate (mode, colour):
 *         a leaf takes the colour when the mode applies to its value, and is written only when that changes it, counter 0
 *         an interior word COLLAPSES to the leaf word of the colour when the mode is SVO_REGION_SET (its subtree is cut off, for
 *         svo_nodes_compact to drop); otherwise it is opened
 *     otherwise (mixed):
 *         an interior word is opened
 *         a leaf of value v0 is SPLIT iff some candidate's mode applies to v0 with a colour other than v0: a new group of eight
 *         leaf words OF v0, counter 0, is made, THE COLOUR CARRIED DOWN, the word becomes the pointer to it, and the eight virtual
 *         children join the next frontier; otherwise it is untouched
 * At l == depth a footprint is one column, so nothing is mixed; an interior word that would be opened there is the REFUSAL:
 * SVO_ERR_STATE, nothing written, svo_last_error names the cell.  It occurs only under the modes 1 and 2: SVO_REGION_SET
 * collapses the word.  The test by the extremes is conservative: a leaf may be split whose children all end unchanged.
 * New groups are appended by level and within a level in frontier order: the g-th split gets the group n_words + 8 g, and
 * *n_words_out = n_words + 8 * splits.  Nothing at or behind *n_words_out is touched.  A second identical call on the result
 * writes nothing and appends nothing.  Merging equal siblings (svo_nodes_simplify does) and reusing free groups are not done.
 * Every error is decided before any write; of several causes the first in this order is reported.  SVO_ERR_ARG: NULL p or
 * n_words_out, NULL heights_dev unless a size is 0 or both modes are 0; reserved != 0; depth outside 1..21; a mode above 3;
 * n_layers > SVO_HEIGHTMAP_MAX_LAYERS, or 0 with a mode_below; origin + size > 2^depth on an axis; 2^31 columns or more.
 * SVO_ERR_STATE: no node buffer; a device adaptive state attached to the context.  SVO_ERR_ARG: n_words not a positive multiple of
 * 8 or above the capacity.  SVO_ERR_STATE: the "malformed tree: ..." causes with svo_nodes_compact's wording, on the words that
 * the call opens; the refusal above.  SVO_ERR_CAP when the exact new length exceeds max_words, the capacity or 2^27.  A size of 0
 * or two modes of 0 succeed, return n_words and enqueue nothing.
 * Runs on the ctx stream: the min/max pyramid below, then the levels; blocks once per level and once more for the status, so
 * heights_dev may be freed on return.  The fill and the writes are enqueued, ordered and recorded like svo_nodes_write. */
#define SVO_HEIGHTMAP_MAX_LAYERS 8u
typedef struct svo_heightmap_layer {   /* HOST memory */
    uint32_t thickness;  /* cells, counted down from the ground's top cell; the last layer's is ignored */
    uint32_t colour;     /* 0x00RRGGBB, the low 24 bits count; 0 = empty */
} svo_heightmap_layer;
typedef struct svo_heightmap_params {
    uint32_t depth;            /* 1..21: the grid the columns stand on */
    uint32_t n_layers;         /* 0..8; at least 1 when mode_below != 0 */
    uint64_t n_words;          /* the tree's current length: a multiple of 8, at least 8 */
    uint64_t max_words;        /* 0 = the node buffer's capacity; never above SVO_VOXEL_OFFSET */
    uint32_t origin_xz[2];     /* the map's rectangle of columns: its first column ... */
    uint32_t size_xz[2];       /* ... and its size; origin + size <= 2^depth */
    uint32_t mode_below;       /* 0 (leave alone) or SVO_REGION_EMPTY / _VOXELS / _SET */
    uint32_t mode_above;       /* the same for the cells at and above the height */
    uint32_t colour_above;     /* low 24 bits; 0 = carve what stands above the ground */
    uint32_t reserved;         /* 0 */
    svo_heightmap_layer layers[SVO_HEIGHTMAP_MAX_LAYERS];
} svo_heightmap_params;
int svo_nodes_edit_heightmap(svo_ctx *ctx, const svo_heightmap_params *p, const uint32_t *heights_dev, uint64_t *n_words_out);
/* The min/max pyramid that the edit walks by, for callers that cull or pick a level of detail by it: level s (1..depth) has one
 * entry per octree-aligned tile (tx, tz) of 2^s x 2^s columns with origin >> s <= t <= (origin + size - 1) >> s on each axis --
 * aligned in the SCENE's coordinates, not the map's -- holding the minimum and the maximum of the clamped heights of the
 * rectangle's columns in the tile.  minmax_out_dev (DEVICE, two u32 per entry) receives level s as (min, max) pairs, tz fastest.
 * Of p only depth, origin_xz and size_xz matter, the rest is checked as above.  SVO_ERR_ARG as above, and for s outside 1..depth
 * and a NULL minmax_out_dev.  Enqueued on the ctx stream; does not block.  A size of 0 succeeds and enqueues nothing. */
int svo_heightmap_minmax(svo_ctx *ctx, const svo_heightmap_params *p, const uint32_t *heights_dev, uint32_t s, uint32_t *minmax_out_dev);
/* Times (ms) of the last height-map edit: [0] the pyramid, [1] plan (with its per-level read-backs), [2] status, [3] fill, [4]
 * write (device events; waits for the write), [5] host wall time of the call.  All 0 after a call with nothing to edit; a
 * refused call leaves the times of the last one that ran. */
#define SVO_HEIGHTMAP_TIMES 6   /* pyramid, plan, status, fill, write, host wall */
int svo_heightmap_timing(svo_ctx *ctx, float ms_out[SVO_HEIGHTMAP_TIMES]);

/* ---- the tree in the node buffer compacted in place ----
 * Reads the first n_words words of the node buffer as a tree rooted at group 0.  E = SVO_VOXEL_OFFSET << 4 is the empty
 * word; a word is interior when word >> 4 < SVO_VOXEL_OFFSET.
 * flags == 0: the words [0, *n_words_out) become, bit for bit, what the host's svo_nodes_relayout(words, n_words, 32, out,
 * perm) returns: the reachable groups in breadth-first order, each level in the order of its parents, pointers rewritten,
 * the low 4 bits (hit counters) of every word kept, unreachable groups dropped.  perm_out_dev (DEVICE, at least n_words
 * u32, or NULL): perm[new word] = old word for [0, *n_words_out); nothing behind *n_words_out is written in it.
 * SVO_COMPACT_PRUNE_EMPTY: a group is dead when each of its 8 words, counter ignored, is E or an interior word whose group
 * is dead; the root group is never dead.  An interior word pointing at a dead group becomes exactly E (counter 0), dead
 * groups are dropped, and the rest is as above, applied to the pruned tree.  Pruning a pruned, canonical tree returns it
 * unchanged.
 * Afterwards the words [*n_words_out, n_words) hold E, no word at or behind n_words is touched, *n_words_out <= n_words,
 * and the result is the same on every run (no atomics: the order is the contract).
 * Errors are decided before any write and leave the node buffer and perm_out_dev as they were.  SVO_ERR_ARG: NULL p or
 * n_words_out, unknown flag bits, n_words not a positive multiple of 8 or above the capacity.  SVO_ERR_STATE, the cause in
 * svo_last_error ("malformed tree: ..." for the last four): no node buffer; a device adaptive state attached to the
 * context (svo_adaptive_attach: its positions and hole stack index the old layout); an interior pointer that is not a
 * multiple of 8 or with pointer + 8 > n_words; a tree deeper than 31 levels; a group reached twice.  Of several causes
 * the first in this order is reported: NULL p or n_words_out, flag bits, no node buffer, an attached adaptive state (both
 * SVO_ERR_STATE, before n_words is looked at: without a buffer there is no capacity to hold it against), n_words, the tree.
 * Runs on the ctx stream and blocks once per level of the tree (a count is read back) and once before the emit; the
 * copy back is enqueued (a following svo_render on the stream sees the compacted tree), ordered and recorded like
 * svo_nodes_write, so every context sharing the buffer rebuilds its top table and schedule. */
#define SVO_COMPACT_PRUNE_EMPTY 1u
typedef struct svo_compact_params {
    uint32_t flags;    /* 0 or SVO_COMPACT_PRUNE_EMPTY */
    uint32_t reserved;
    uint64_t n_words;  /* the tree's current length: a multiple of 8, at least 8 */
} svo_compact_params;
int svo_nodes_compact(svo_ctx *ctx, const svo_compact_params *p, uint32_t *perm_out_dev /* may be null */, uint64_t *n_words_out);
/* Times (ms) of the last compaction: [0] discover (with its per-level read-backs), [1] check, [2] prune, [3] emit,
 * [4] copy back (device events; waits for the copy), [5] host wall time of the call.  A refused call leaves the times
 * of the last compaction that ran. */
#define SVO_COMPACT_TIMES 6
int svo_compact_timing(svo_ctx *ctx, float ms_out[SVO_COMPACT_TIMES]);

/* ---- the tree in the node buffer simplified: uniform subtrees merged, the tree cut to a level by mip ----
 * Reads the first n_words words of the node buffer as a tree rooted at group 0.  Levels are svo_nodes_list_voxels': the root
 * group's words are level 1, the words of the group an interior word of level l points at are level l + 1.  f = word >> 4
 * is a word's field: the word is interior when f < SVO_VOXEL_OFFSET, otherwise a leaf of value f - SVO_VOXEL_OFFSET.  The
 * low 4 bits (hit counters) never take part in a comparison.  Two rewrites apply, in this order, then the layout:
 * 1. SVO_SIMPLIFY_CUT (lossy).  S(W) of a leaf is its value.  S(W) of an interior word pointing at group G: with s_c =
 *    S(G[c]) and n the number of c with s_c != 0, S = 0 when n == 0, otherwise per byte b in {0, 8, 16} ch_b = max(1, (sum
 *    over the c with s_c != 0 of (s_c >> b) & 0xFF) / n) in integer division and S = ch_0 | ch_8 << 8 | ch_16 << 16: on 24-bit
 *    colours the mip colour of svo_world_generate_mip_tree, applied bottom-up to averaged children, except that a subtree
 *    without a voxel gives 0.  Every interior word at level cut_level becomes the leaf word (SVO_VOXEL_OFFSET + S(W)) << 4,
 *    counter 0: a cube becomes solid when it holds any voxel.  Leaves at or above cut_level are untouched, and a tree no
 *    deeper than cut_level is unchanged.
 * 2. SVO_SIMPLIFY_MERGE (lossless), on the tree step 1 leaves.  U(W) of a leaf is its field f, all 28 bits (values above
 *    24 bits merge only with themselves).  U(W) of an interior word at level l pointing at G is f when l >= min_level and
 *    all eight U(G[c]) are defined and equal f, and undefined otherwise.  Every interior word with U defined becomes f << 4,
 *    counter 0.  The root group has no parent word and always stays.  With f the empty field this is
 *    SVO_COMPACT_PRUNE_EMPTY's rule; every cell of the tree samples (svo_nodes_sample) to what it sampled before.
 * 3. The result is svo_nodes_compact with flags == 0 of the rewritten words: the groups still reachable breadth-first, each
 *    level in the order of its parents, pointers rewritten, every kept word keeping its 4 counter bits.  perm_out_dev
 *    (DEVICE, at least n_words u32, or NULL): perm[new word] = old word for [0, *n_words_out), also for a word that was
 *    rewritten into a leaf.
 * out_dev == NULL writes in place, as the compaction does: afterwards the words [*n_words_out, n_words) hold the empty word,
 * nothing at or behind n_words is touched, and the write is ordered and recorded like svo_nodes_write.  out_dev != NULL
 * (DEVICE, out_cap words) gets the words [0, *n_words_out): the node buffer is only read, no write is recorded, and an
 * attached adaptive state is no obstacle -- a level-of-detail copy that another context takes with svo_nodes_bind_device
 * or svo_nodes_write.  *n_words_out <= n_words always, and the result is the same bytes on every run and for every layout
 * of the same tree (no atomics: the order is the contract).
 * THE TRAP: svo_nodes_edit splits a coarse leaf into EMPTY children (the reference's put_in_voxel), so voxels put into a
 * merged solid by cell list lose the solid's colour around the edit.  svo_nodes_edit_region carries the colour down, and
 * min_level bounds how coarse the merge goes.
 * Errors are decided before any write and leave the node buffer, out_dev and perm_out_dev as they were; of several causes
 * the first in this order is reported: NULL p or n_words_out (SVO_ERR_ARG); flags 0 or with unknown bits, cut_level outside
 * 1..31 with CUT or not 0 without, min_level not 0 without MERGE, reserved not 0 (SVO_ERR_ARG); no node buffer
 * (SVO_ERR_STATE); a device adaptive state attached, for an in-place call (SVO_ERR_STATE); n_words not a positive multiple
 * of 8 or above the capacity (SVO_ERR_ARG); the "malformed tree: ..." causes with svo_nodes_compact's wording
 * (SVO_ERR_STATE); SVO_ERR_CAP, with the exact length in svo_last_error, when *n_words_out > out_cap for an out-of-place call.
 * Runs on the ctx stream; blocks once per level of the tree (the discovery) and once before the emit. */
#define SVO_SIMPLIFY_MERGE 1u   /* lossless: an interior word whose whole subtree holds one leaf value becomes that leaf */
#define SVO_SIMPLIFY_CUT   2u   /* lossy: every interior word at level cut_level becomes a leaf of its subtree's mip colour */
typedef struct svo_simplify_params {
    uint32_t flags;       /* 1, 2 or 3; 0 and unknown bits: SVO_ERR_ARG (flags 0 is svo_nodes_compact's job) */
    uint32_t cut_level;   /* with CUT: 1..31; without: must be 0 */
    uint32_t min_level;   /* MERGE makes no leaf at a level below this; 0 or 1 = no limit; without MERGE must be 0 */
    uint32_t reserved;    /* 0 */
    uint64_t n_words;     /* the tree: words [0, n_words) of the node buffer, rooted at group 0 */
    uint64_t out_cap;     /* room in out_dev, in words; ignored when out_dev is NULL */
} svo_simplify_params;
int svo_nodes_simplify(svo_ctx *ctx, const svo_simplify_params *p, uint32_t *out_dev /* may be null */,
                       uint32_t *perm_out_dev /* may be null */, uint64_t *n_words_out);
/* Times (ms) of the last simplification: [0] discover (with its per-level read-backs), [1] check, [2] reduce, [3] emit,
 * [4] copy back (device events; waits for it; next to nothing out of place), [5] host wall time of the call.  A refused
 * call leaves the times of the last simplification that ran. */
#define SVO_SIMPLIFY_TIMES 6   /* discover, check, reduce, emit, copy back, host wall */
int svo_simplify_timing(svo_ctx *ctx, float ms_out[SVO_SIMPLIFY_TIMES]);

/* ---- the voxels of the tree in the node buffer listed on the device ----
 * The inverse of svo_nodes_build.  Reads the first n_words words of the node buffer as a tree rooted at group 0.
 * E = SVO_VOXEL_OFFSET << 4; a word is interior when word >> 4 < SVO_VOXEL_OFFSET and a *voxel* when word >> 4 >
 * SVO_VOXEL_OFFSET; the low 4 bits (hit counters) never matter.  The root group's words are level 1, the words of the
 * group an interior word at level l points at are level l + 1, and the child index is x * 4 + y * 2 + z.  A voxel word
 * reached at level l is a cube whose minimum corner on the `depth` grid is cell << (depth - l).
 * flags == 0: one entry per voxel word reachable from group 0: xyz (3 u32) its minimum corner on the `depth` grid, value =
 * (word >> 4) - SVO_VOXEL_OFFSET (the 24-bit colour of built and edited trees), level = l (written when level_out_dev is
 * not NULL).  The entries come in ascending Morton key of xyz at `depth` (the builder's key); the cubes are disjoint, so
 * that is the depth-first order of the tree by child index and the order is total.  The output does not depend on where
 * the groups sit in the buffer: a tree in put order, its compacted form and its canonical rebuild list identically, byte
 * for byte, on every run (no atomics: the order is the contract).
 * SVO_LIST_EXPAND: a voxel at level l < depth is replaced by its 8^(depth - l) cells of the `depth` grid, all with its
 * value and level = depth, in Morton order: the result is a list that svo_nodes_build accepts at `depth`.
 * xyz_out_dev == NULL is a count query: *n_out gets the number of entries, nothing else is written and max_voxels is
 * ignored.  Otherwise xyz_out_dev (3 * max_voxels u32), value_out_dev (max_voxels u32) and level_out_dev (max_voxels u32,
 * or NULL) are DEVICE pointers of which only the entries [0, *n_out) are written.  The node buffer is never written.
 * Errors are decided before any write to the outputs and leave them and *n_out as they were.  SVO_ERR_ARG: NULL p or
 * n_out; unknown flag bits; depth outside 1..21; NULL value_out_dev with xyz_out_dev given; n_words not a positive
 * multiple of 8 or above the capacity; a voxel or an interior word at a level deeper than `depth` (svo_last_error names
 * the deepest such level).  SVO_ERR_STATE: no node buffer; and the "malformed tree: ..." causes of svo_nodes_compact with
 * its wording: an interior pointer that is not a multiple of 8 or with pointer + 8 > n_words, a tree deeper than 31
 * levels, a group reached twice.  SVO_ERR_CAP, with the exact count in svo_last_error: more entries than max_voxels
 * (not for a count query), or 2^31 or more (also for a count query).  Counts are 64 bits wide: the cubes of a tree are
 * disjoint, so an expanded count is at most 8^21 = 2^63 and does not wrap; one level-1 voxel expanded at depth 21 is 2^60
 * entries and SVO_ERR_CAP.  Of several causes the first in this order is reported: NULL p, NULL n_out, flag bits, depth,
 * value_out_dev, no node buffer, n_words, the malformed-tree causes in svo_nodes_compact's order, the level deeper than
 * `depth`, the count.  A device adaptive state attached to the context is no obstacle: the call only reads, and free
 * groups are unreachable.
 * Runs on the ctx stream behind the store's last write, whichever context issued it, and records no write of its own.
 * Blocks once per level of the tree and once for the counts; the fill is enqueued (svo_sync before the outputs are read
 * on another stream). */
#define SVO_LIST_EXPAND 1u
typedef struct svo_list_params {
    uint32_t flags;       /* 0 or SVO_LIST_EXPAND */
    uint32_t depth;       /* 1..21: the grid the coordinates are given on */
    uint64_t n_words;     /* the tree: words [0, n_words) of the node buffer, rooted at group 0 */
    uint64_t max_voxels;  /* room in the output arrays, in entries */
} svo_list_params;
int svo_nodes_list_voxels(svo_ctx *ctx, const svo_list_params *p, uint32_t *xyz_out_dev, uint32_t *value_out_dev,
                          uint32_t *level_out_dev /* may be null */, uint64_t *n_out);
/* Times (ms) of the last listing: [0] discover (with its per-level read-backs), [1] count (with its read-back), [2] offsets,
 * [3] emit (device events; waits for the emit; 0 for a count query), [4] host wall time of the call.  A refused call
 * leaves the times of the last listing that ran. */
#define SVO_LIST_TIMES 5
int svo_list_timing(svo_ctx *ctx, float ms_out[SVO_LIST_TIMES]);

/* ---- the visible surface of the tree in the node buffer, found on the device ----
 * Which faces of the voxels that svo_nodes_list_voxels lists are exposed.  The tree is the first n_words words of the node
 * buffer rooted at group 0; the word test, the levels, the child index x * 4 + y * 2 + z, the coordinates on the `depth`
 * grid and the Morton order are exactly the listing's, and the low 4 bits of a word never matter.
 * A voxel word at level l is a cube with cell c on the level-l grid.  Its faces are numbered f = 0 .. 5: -x, +x, -y, +y,
 * -z, +z, and the cell behind face f is n = c - 1 (even f) or c + 1 (odd f) on axis f >> 1.
 *     n leaves [0, 2^l) on that axis:   the face is exposed; with SVO_SURFACE_CLOSED_BOUNDARY it is covered
 *     otherwise walk from group 0 towards n for at most l levels, by the sampler's rule (svo_nodes_sample):
 *         the walk stops on a voxel word (value > 0) at a level <= l:   covered
 *         it stops on the empty word:                                   exposed
 *         the word at level l is interior (the neighbour is finer):     exposed
 * The rule is conservative: a face reported covered is covered in every cell of it; a face reported exposed touches an
 * empty cell or finer detail.  It is exact for a tree whose voxels all sit at `depth`.
 * flags without SVO_SURFACE_KEEP_HIDDEN and SVO_SURFACE_QUADS: one entry per voxel with at least one exposed face, in the
 * listing's order (ascending Morton key of the minimum corner at `depth`): xyz the minimum corner, value and level as
 * in the listing, face the 6-bit mask, bit f set when face f is exposed.
 * SVO_SURFACE_KEEP_HIDDEN: the voxels with mask 0 are kept too: xyz, value and level are byte-identical to
 * svo_nodes_list_voxels with flags 0, and face lines up with them.
 * SVO_SURFACE_QUADS: one entry per exposed face, the voxels in the listing's order and the faces of a voxel in ascending
 * f: xyz, value and level are the voxel's, face is f (0..5).  Not together with SVO_SURFACE_KEEP_HIDDEN.
 * xyz_out_dev == NULL is a count query: *n_out gets the number of entries, nothing else is written and max_entries is
 * ignored.  Otherwise xyz_out_dev (3 * max_entries u32), value_out_dev, level_out_dev (or NULL) and face_out_dev
 * (max_entries u32 each) are DEVICE pointers of which only the entries [0, *n_out) are written.  The node buffer is never
 * written.  No atomics: the same bytes on every run and for every layout of the same tree.
 * Errors are decided before any write to the outputs and leave them and *n_out as they were; they are the listing's, in
 * its order and with its wording: SVO_ERR_ARG: NULL p or n_out; unknown or incompatible flag bits; depth outside 1..21;
 * NULL face_out_dev or value_out_dev with xyz_out_dev given; SVO_ERR_STATE: no node buffer; SVO_ERR_ARG: n_words; SVO_ERR_STATE:
 * the "malformed tree: ..." causes; SVO_ERR_ARG: a voxel or an interior word at a level deeper than `depth`; SVO_ERR_CAP, with
 * the exact count in svo_last_error: 2^31 voxels or more, then more entries than max_entries (not for a count query) or
 * 2^31 entries or more.  A device adaptive state attached to the context is no obstacle.
 * Runs on the ctx stream behind the store's last write, whichever context issued it, and records no write of its own.
 * Blocks where the listing blocks, once per level of the tree and once for the counts, and once more for the number of
 * entries; the fill is enqueued (svo_sync before the outputs are read on another stream). */
#define SVO_SURFACE_CLOSED_BOUNDARY 1u  /* the grid's own boundary covers the faces on it */
#define SVO_SURFACE_KEEP_HIDDEN     2u  /* voxels without an exposed face are listed too */
#define SVO_SURFACE_QUADS           4u  /* one entry per exposed face */
typedef struct svo_surface_params {
    uint32_t flags;        /* SVO_SURFACE_* */
    uint32_t depth;        /* 1..21: the grid the coordinates are given on */
    uint64_t n_words;      /* the tree: words [0, n_words) of the node buffer, rooted at group 0 */
    uint64_t max_entries;  /* room in the output arrays, in entries */
} svo_surface_params;
int svo_nodes_list_surface(svo_ctx *ctx, const svo_surface_params *p, uint32_t *xyz_out_dev, uint32_t *value_out_dev,
                           uint32_t *level_out_dev /* may be null */, uint32_t *face_out_dev, uint64_t *n_out);
/* Times (ms) of the last surface call: [0] discover (with its per-level read-backs), [1] count (with its read-back), [2]
 * offsets, [3] mask, [4] the compaction's count (with its read-back), [5] emit (device events; waits for the emit; 0 for a
 * count query), [6] host wall time of the call.  A refused call leaves the times of the last call that ran. */
#define SVO_SURFACE_TIMES 7
int svo_surface_timing(svo_ctx *ctx, float ms_out[SVO_SURFACE_TIMES]);

/* ---- the visible surface merged into rectangles on the device ----
 * Input: the exposed faces of the tree [0, n_words), exactly as svo_nodes_list_surface with SVO_SURFACE_QUADS defines them;
 * the same rule, boundary flag and errors apply.  A face f of a leaf at level l with minimum corner m on the `depth` grid
 * has s = 2^(depth - l), a = f >> 1, ua = (a + 1) % 3 and va = (a + 2) % 3, and is the rectangle
 *     face = f, plane = m[a] + (f & 1) * s (0 .. 2^depth), u0 = m[ua], v0 = m[va], w = h = s, value.
 * The input rectangles of one (face, plane) are pairwise disjoint.
 * Merge: one round is a U phase followed by a V phase.
 *     U phase: among rectangles with equal (face, plane, v0, h), B follows A when B.u0 == A.u0 + A.w and B.value ==
 *     A.value.  Every maximal chain becomes one rectangle (u0 of the first, w = the sum of the widths).
 *     V phase: the same with u and v, w and h exchanged: the class is (face, plane, u0, w), and B follows A when
 *     B.v0 == A.v0 + A.h.
 * rounds is 1 to 4; 1 is the classic two-pass greedy mesher.  Later rounds matter only for mixed-level trees, where a
 * 2 x 2 made of unit faces can then join a coarse leaf's 2 x 2.  The phases are defined on sets, so the result does not
 * depend on the input order or on the tree's layout.  SVO_SURFACE_MERGE_ANY_VALUE drops the value condition and reports
 * value 0 for every rectangle (collision and occluder meshes).
 * Output: rect_out_dev has 6 u32 per entry: face, plane, u0, v0, w, h; value_out_dev has 1 u32 per entry.  The entries
 * ascend by (face, plane, u0, w, v0), the last V phase's order, which is unique because the rectangles are disjoint.
 * rect_out_dev == NULL is a count query: *n_out gets the number of entries, nothing else is written and max_entries is
 * ignored.  Otherwise both are DEVICE pointers with room for max_entries entries, of which only the entries [0, *n_out) are
 * written.  The node buffer is never written.  No atomics: the same bytes on every run and for every layout of the same
 * tree; the low 4 bits of a word never matter.
 * Errors are decided before any write to the outputs and leave them and *n_out as they were; they are
 * svo_nodes_list_surface's, in its order and with its wording: SVO_ERR_ARG: NULL p or n_out; unknown or incompatible flag
 * bits, which here covers rounds outside 1..4 too; depth outside 1..21; NULL value_out_dev with rect_out_dev given;
 * SVO_ERR_STATE: no node buffer; SVO_ERR_ARG: n_words; SVO_ERR_STATE: the "malformed tree: ..." causes; SVO_ERR_ARG: a voxel
 * or an interior word at a level deeper than `depth`; SVO_ERR_CAP, with the exact count in svo_last_error: 2^31 voxels or
 * more, 2^31 exposed faces or more, then more rectangles than max_entries (not for a count query).  A device adaptive
 * state attached to the context is no obstacle.
 * Runs on the ctx stream behind the store's last write, whichever context issued it, and records no write of its own.
 * Blocks where svo_nodes_list_surface blocks (once per level of the tree, once for the counts, once for the number of
 * faces) and once per phase for the number of rectangles it leaves, 2 * rounds times at most: a round that joins nothing
 * is the last.  The fill is enqueued (svo_sync before the outputs are read on another stream).  The pass has a surface
 * workspace of its own and sorts in the builder's (svo_nodes_build), whose times it leaves alone. */
#define SVO_SURFACE_MERGE_ANY_VALUE 8u  /* rectangles join whatever their values; every value comes out 0 */
typedef struct svo_surface_merge_params {
    uint32_t flags;        /* SVO_SURFACE_CLOSED_BOUNDARY, SVO_SURFACE_MERGE_ANY_VALUE */
    uint32_t depth;        /* 1..21: the grid the coordinates are given on */
    uint32_t rounds;       /* 1..4 */
    uint32_t reserved;     /* not looked at */
    uint64_t n_words;      /* the tree: words [0, n_words) of the node buffer, rooted at group 0 */
    uint64_t max_entries;  /* room in the output arrays, in entries */
} svo_surface_merge_params;
int svo_nodes_merge_surface(svo_ctx *ctx, const svo_surface_merge_params *p, uint32_t *rect_out_dev, uint32_t *value_out_dev,
                            uint64_t *n_out);
/* Times (ms) of the last merge: [0] the quads (svo_nodes_list_surface's passes, with their read-backs), then four per
 * phase, the U phase of round 1 first: [1 + 4 k] keys, [2 + 4 k] the two sorts and the gather, [3 + 4 k] flags and scan
 * (with its read-back), [4 + 4 k] emit (0 for a phase that did not run), [33] the output's fill (device events; waits for
 * it; next to 0 for a count query), [34] host wall time of the call.  A refused call leaves the times of the last call that ran. */
#define SVO_SURFACE_MERGE_TIMES 35
int svo_surface_merge_timing(svo_ctx *ctx, float ms_out[SVO_SURFACE_MERGE_TIMES]);

/* ---- the connected components of the tree in the node buffer, labelled on the device ----
 * Which voxels of the tree hang together.  The entries are exactly those of svo_nodes_list_voxels with flags 0: the word
 * test, the levels, the child index x * 4 + y * 2 + z, the `depth` grid, the Morton order and the disregard for the low 4
 * bits of a word are the listing's.  Entry i is a voxel word at level l with cell c on the level-l grid.
 * Links: for each face f = 0 .. 5 of entry i (-x, +x, -y, +y, -z, +z) let n be the cell behind it, as svo_nodes_list_surface
 * defines it: c - 1 (even f) or c + 1 (odd f) on axis f >> 1.
 *     n leaves [0, 2^l) on that axis:   no link (the grid's boundary links nothing)
 *     otherwise walk from group 0 towards n for at most l levels, by the sampler's rule (svo_nodes_sample):
 *         the walk stops on a voxel word (value > 0) at a level <= l:   that word is entry j of the listing; i and j are linked
 *         it stops on the empty word:                                   no link
 *         the word at level l is interior (the neighbour is finer):     no link from this side; the finer voxels link from theirs
 * With SVO_COMPONENTS_SAME_VALUE a link also needs equal values ((word >> 4) of both).  The cubes of a tree are disjoint, so
 * two entries are linked exactly when their cubes share a piece of a face: the components are those of 6-connectivity of
 * the cubes (per value, with the flag).  Cubes that touch along an edge or at a corner only are not linked.
 * Outputs, all DEVICE pointers of max_entries u32 each, of which only the entries [0, *n_out) are written:
 *     label_out_dev[i]   the rank of the first entry (smallest rank) of i's component: label[i] <= i, label[label[i]] == label[i]
 *     id_out_dev[i]      (may be NULL) the component's number 0 .. C - 1; the components are numbered by ascending first entry
 *     index_out_dev[i]   (may be NULL) the index of the entry's word in the node buffer, as svo_nodes_sample reports it: the
 *                        address svo_nodes_scatter_device takes.  It is the one output that names a place
 *     *n_out the number of entries, *n_components_out the number of components C
 * label_out_dev == NULL is a count query for both numbers: nothing else is written and max_entries is ignored.
 * The result is the same bytes on every run and for every layout of the same tree (put order, compacted, canonical
 * rebuild), index excepted.  The union uses atomicMin on the pass's own workspace; its fixed point, the smallest rank of
 * each component, does not depend on the order they land in.
 * Errors are decided before any write to the outputs and leave them, *n_out and *n_components_out as they were; they are
 * the listing's, in its order and with its wording: SVO_ERR_ARG: NULL p; NULL n_out or n_components_out; unknown flag bits;
 * depth outside 1..21; SVO_ERR_STATE: no node buffer; SVO_ERR_ARG: n_words; SVO_ERR_STATE: the "malformed tree: ..." causes;
 * SVO_ERR_ARG: a voxel or an interior word at a level deeper than `depth`; SVO_ERR_CAP, with the exact count in
 * svo_last_error: 2^31 entries or more, then more entries than max_entries (not for a count query).  A device adaptive
 * state attached to the context is no obstacle.  The node buffer is never written.
 * Runs on the ctx stream behind the store's last write, whichever context issued it, and records no write of its own.
 * Blocks where the listing blocks, once per round of the union (a round that needs a second compress pass, once more per
 * pass) and once for the number of components; the fill is enqueued (svo_sync before the outputs are read on another stream). */
#define SVO_COMPONENTS_SAME_VALUE 1u  /* a link needs equal values: components of one colour */
typedef struct svo_components_params {
    uint32_t flags;        /* 0 or SVO_COMPONENTS_SAME_VALUE */
    uint32_t depth;        /* 1..21: the grid of the listing */
    uint64_t n_words;      /* the tree: words [0, n_words) of the node buffer, rooted at group 0 */
    uint64_t max_entries;  /* room in the output arrays, in entries */
} svo_components_params;
int svo_nodes_label_components(svo_ctx *ctx, const svo_components_params *p, uint32_t *label_out_dev,
                               uint32_t *id_out_dev /* may be null */, uint32_t *index_out_dev /* may be null */, uint64_t *n_out,
                               uint64_t *n_components_out);
/* Times (ms) of the last labelling: [0] plan (discover, count and offsets, with their read-backs), [1] link, [2] union
 * (with a read-back per round), [3] ids (the count of the roots, with its read-back), [4] the fill (device events; waits
 * for it; next to 0 for a count query), [5] host wall time of the call; *rounds_out (may be NULL) the rounds of the
 * union, the last one, which hooks nothing, included (0 for a tree without a voxel).  A refused call leaves the times of
 * the last call that ran. */
#define SVO_COMPONENTS_TIMES 6
int svo_components_timing(svo_ctx *ctx, float ms_out[SVO_COMPONENTS_TIMES], uint32_t *rounds_out /* may be null */);

/* The device twin of svo_nodes_scatter: words_dev[i], or the one word `fill` when words_dev is NULL, goes to word
 * index_dev[i] of the node buffer, for n entries (DEVICE pointers).  An index >= n_words (the sampler's 0xFFFFFFFF
 * included) is skipped.  Of duplicate indices with different words, which one lands is unspecified.  Nothing is read
 * back and the call does not block: both arrays must stay valid until svo_sync.  It does to the store what
 * svo_nodes_scatter does: the write is ordered behind the store's last write and recorded, so a later frame, and other
 * contexts sharing the store, wait for it and rebuild what they derived, and a resting view's replay is not reused.
 * Errors are decided on the host, the first in this order: SVO_ERR_ARG: NULL index_dev with n > 0; n >= 2^31.
 * SVO_ERR_STATE: no node buffer.  SVO_ERR_ARG: n_words not a positive multiple of 8 or above the capacity. */
int svo_nodes_scatter_device(svo_ctx *ctx, const uint32_t *index_dev, const uint32_t *words_dev /* may be null */, uint32_t fill,
                             size_t n, uint64_t n_words);

/* ---- the tree in the node buffer sampled on the device ----
 * What is at a cell of the `depth` grid, read from the first n_words words of the node buffer as a tree rooted at group 0;
 * coordinates, child index and levels are those of svo_nodes_build, svo_nodes_edit and svo_nodes_list_voxels.  For the
 * cell (x, y, z):
 *     if x, y or z >= 2^depth:           value SVO_SAMPLE_OUTSIDE, level 0, index 0xFFFFFFFF
 *     group = 0
 *     for l = 1 .. depth:
 *         i = group + (x bit << 2 | y bit << 1 | z bit), the bit depth - l of each coordinate
 *         ptr = words[i] >> 4                          (the hit counter never matters)
 *         if ptr >= SVO_VOXEL_OFFSET:    value ptr - SVO_VOXEL_OFFSET, level l, index i     (0: empty)
 *         if l == depth:                 value SVO_SAMPLE_FINER, level l, index i           (the pointer is not looked at)
 *         if ptr % 8 != 0 or ptr + 8 > n_words:  value SVO_SAMPLE_BROKEN, level l, index i
 *         group = ptr
 * A value is below 2^27, so no mark collides with one, and bit 31 is never set.  index is the word the walk stopped on:
 * for a leaf the number in a hit record's `value`, and the address svo_nodes_scatter takes.  No pointer is followed
 * before it passed the check, and the depth bound ends the walk on a cyclic tree.
 * svo_nodes_sample: xyz_dev holds n * 3 u32, interleaved as the builder takes them, in any order, duplicates included;
 * entry k of value_out_dev, level_out_dev and index_out_dev (n u32 each; the last two may be NULL) gets cell k's result.
 * svo_nodes_sample_dense: the cells [origin, origin + size) of the grid; grid_out_dev[(i * size[1] + j) * size[2] + k]
 * gets the value of cell origin + (i, j, k), which is svo_nodes_build_dense's [x][y][z] layout: the whole grid of a
 * dense-built tree samples to grid & 0xFFFFFF.  A size with a 0 succeeds and writes nothing; so does n == 0.
 * All pointers but p, origin and size are DEVICE pointers.  Both calls only read the node buffer, run on the ctx stream
 * behind the store's last write, whichever context issued it, record no write and DO NOT BLOCK: nothing is read back,
 * everything the device finds out is in the marks, and inputs and outputs must stay valid until svo_sync.  Only the n or
 * size[0] * size[1] * size[2] entries are written.  No atomics: the same bytes on every run and for every layout of the
 * same tree, but for index, which names a place.  A device adaptive state attached to the context is no obstacle.
 * Errors are decided on the host from the arguments before anything is enqueued; the first in this order is reported:
 * SVO_ERR_ARG: NULL p; non-zero flags; depth outside 1..21; NULL xyz_dev or value_out_dev with n > 0, n >= 2^31, NULL
 * origin, size or grid_out_dev, a box with origin + size > 2^depth on an axis or with 2^31 cells or more.  SVO_ERR_STATE:
 * no node buffer.  SVO_ERR_ARG: n_words not a positive multiple of 8 or above the capacity. */
#define SVO_SAMPLE_FINER   (1u << 28)  /* the tree is interior at `depth` in this cell */
#define SVO_SAMPLE_OUTSIDE (1u << 29)  /* a coordinate >= 2^depth */
#define SVO_SAMPLE_BROKEN  (1u << 30)  /* the path met a pointer that is unaligned or leaves [0, n_words) */
typedef struct svo_sample_params {
    uint32_t flags;    /* 0 */
    uint32_t depth;    /* 1..21: the grid the cells are given on */
    uint64_t n_words;  /* the tree: words [0, n_words) of the node buffer, rooted at group 0 */
} svo_sample_params;
int svo_nodes_sample(svo_ctx *ctx, const svo_sample_params *p, const uint32_t *xyz_dev, size_t n,
                     uint32_t *value_out_dev, uint32_t *level_out_dev /* may be null */, uint32_t *index_out_dev /* may be null */);
int svo_nodes_sample_dense(svo_ctx *ctx, const svo_sample_params *p, const uint32_t origin[3], const uint32_t size[3],
                           uint32_t *grid_out_dev);
/* Times (ms) of the last sampling call that ran: [0] the kernel (device events; waits for it), [1] host wall time of the
 * call.  A refused call, and one with nothing to do, leaves them. */
#define SVO_SAMPLE_TIMES 2
int svo_sample_timing(svo_ctx *ctx, float ms_out[SVO_SAMPLE_TIMES]);

/* ---- exact distance fields of the tree in the node buffer ----
 * How far is a cell from the nearest voxel, and which voxel is it: the exact squared Euclidean distance transform of the
 * tree on the `depth` grid, in integers, for every cell of a box, with the nearest site.
 * A cell of the grid is OCCUPIED when svo_nodes_sample gives it a value other than 0 (svo_nodes_column_tops' rule): a
 * colour counts, a coarse leaf's too, and so do SVO_SAMPLE_FINER and SVO_SAMPLE_BROKEN.  Every cell outside
 * [0, 2^depth)^3 is empty.  The SITES of a call, by mode:
 *     SVO_DISTANCE_TO_VOXELS  the occupied cells
 *     SVO_DISTANCE_TO_EMPTY   the empty cells, those outside the grid included (the grid's boundary exposes, as in
 *                             svo_nodes_list_surface)
 *     SVO_DISTANCE_SIGNED     for an empty cell the occupied cells, for an occupied cell the empty cells
 * For every cell c of the box [origin, origin + size), with R = max_distance: among the sites s with |s - c|^2 <= R^2 take
 * the one that is smallest by (|s - c|^2, s.x, s.y, s.z), lexicographically.  The cell itself, sites outside the box and
 * sites outside the grid all take part: a voxel one cell behind the box's face gives that face distance 1.
 *     d2_out_dev[(i * size[1] + j) * size[2] + k]     (svo_nodes_sample_dense's layout) gets |s - c|^2, or
 *                                                     SVO_DISTANCE_FAR when there is no such site; in signed mode an
 *                                                     occupied cell gets the negated value (-SVO_DISTANCE_FAR for none),
 *                                                     so a signed field is never 0
 *     site_out_dev[the same index]   (may be NULL)    ((dx + 128) << 16) | ((dy + 128) << 8) | (dz + 128) with (dx, dy, dz)
 *                                                     = s - c, or SVO_DISTANCE_NO_SITE
 * The lexicographic minimum decomposes over the axes (the best site is the best over x' of the best over y' of the best
 * over z'), so three one-dimensional passes give exactly this rule, ties included.
 * The call only reads the node buffer, runs on the ctx stream behind the store's last write, whichever context issued it,
 * records no write and DOES NOT BLOCK: nothing is read back, and the outputs must stay valid until svo_sync.  Only the
 * size[0] * size[1] * size[2] entries of each output are written; a size with a 0 succeeds and writes nothing.  No
 * atomics: the same bytes on every run and for every layout of the same tree.  No pointer is followed before it passed
 * svo_nodes_sample's check, and the depth bound ends every walk on a cyclic tree.  A device adaptive state attached to
 * the context is no obstacle.
 * WORKSPACE, owned by the context, grown on demand and reused.  With g[a] = size[a] + 2 R and w = the number of aligned
 * runs of 64 cells along z that meet [origin[2] - R, origin[2] + size[2] + R) (at most (size[2] + 2 R) / 64 + 2):
 *     occupancy bits          g[0] * g[1] * w * 8 bytes, for the box grown by R on every side
 *     the y pass's output     m * g[0] * t * size[2] * 4 bytes, m = 2 in signed mode and 1 otherwise
 * The call works in SLABS of t rows of the box along y, one after the other through the same buffer:
 * t = max(1, min(size[1], SVO_DISTANCE_SLAB_CELLS / (g[0] * size[2]))).  A box whose two terms together exceed
 * SVO_DISTANCE_MAX_WORKSPACE bytes is refused.
 * Errors are decided on the host from the arguments before anything is enqueued; the first in this order is reported, and a
 * refused call writes nothing:
 * SVO_ERR_ARG: NULL p; non-zero flags; depth outside 1..21; mode above 2; max_distance outside 1..SVO_DISTANCE_MAX_RADIUS;
 * NULL origin, size or d2_out_dev; a box with origin + size > 2^depth on an axis; a box with 2^31 cells or more; a box
 * whose workspace exceeds SVO_DISTANCE_MAX_WORKSPACE.  SVO_ERR_STATE: no node buffer.  SVO_ERR_ARG: n_words not a positive
 * multiple of 8 or above the capacity. */
#define SVO_DISTANCE_TO_VOXELS 0u
#define SVO_DISTANCE_TO_EMPTY  1u
#define SVO_DISTANCE_SIGNED    2u
#define SVO_DISTANCE_MAX_RADIUS 127u
#define SVO_DISTANCE_FAR     0x7FFFFFFF   /* in d2: no site within max_distance */
#define SVO_DISTANCE_NO_SITE 0xFFFFFFFFu  /* in site: the same */
#define SVO_DISTANCE_SLAB_CELLS (1u << 21)        /* entries of the y pass's output that a slab holds, when a row fits */
#define SVO_DISTANCE_MAX_WORKSPACE (1ull << 30)   /* bytes */
typedef struct svo_distance_params {
    uint32_t flags;         /* 0 */
    uint32_t mode;          /* SVO_DISTANCE_TO_VOXELS, _TO_EMPTY or _SIGNED */
    uint32_t depth;         /* 1..21: the grid the box is given on */
    uint32_t max_distance;  /* R, 1..SVO_DISTANCE_MAX_RADIUS: sites further than R cells away are not looked for */
    uint64_t n_words;       /* the tree: words [0, n_words) of the node buffer, rooted at group 0 */
} svo_distance_params;
int svo_nodes_distance(svo_ctx *ctx, const svo_distance_params *p, const uint32_t origin[3], const uint32_t size[3],
                       int32_t *d2_out_dev, uint32_t *site_out_dev /* may be null */);
/* Times (ms) of the last distance call that ran (device events; waits for them): [0] the occupancy bits, [1] the first
 * slab's z and y pass, [2] the first slab's x pass, [3] all slabs, the first included, [4] host wall time of the call.  A
 * refused call, and one with nothing to do, leaves them.  SVO_ERR_STATE on a context that never ran the pass. */
#define SVO_DISTANCE_TIMES 5
int svo_distance_timing(svo_ctx *ctx, float ms_out[SVO_DISTANCE_TIMES]);

/* ---- triangle meshes voxelised on the GPU ----
 * Conservative voxelisation of a triangle mesh on the 2^depth grid into the voxel list that svo_nodes_build,
 * svo_nodes_edit, svo_cpu_octree_build and svo_world_build take.  The geometry is exact.  A quantised coordinate q lies
 * in [0, 2^(depth + SVO_VOX_SUBBITS)); the vertex stands at (q + 1/2) / 64 cells, so no vertex ever lies on a cell
 * boundary and a wall modelled exactly on a grid plane falls on one side of it and is one cell thick.  Cell c is the
 * closed cube [c, c + 1]^3.  There is one entry (t, c) iff the closed triangle t meets the closed cube c; a triangle
 * that is a segment or a point counts too.  The test is done in integers, in doubled units (vertex 2q + 1, a level-l
 * cell [c * S, (c + 1) * S] with S = 2^(depth - l + 7)), with the 13 separating axes of a triangle and a box (3 box
 * axes, the plane, 9 edge x axis products) and every comparison strict; no float takes part.
 * Entries come in ascending triangle index and, within a triangle, in ascending Morton key of the cell at `depth`
 * (csrc/svo_morton.h: the builder's key).  xyz is the cell, colour the triangle's colour & 0xFFFFFF (default_colour when
 * tri_colours_dev is NULL), tri the triangle's index.  A cell touched by several triangles appears once per triangle:
 * fed to svo_nodes_build or svo_nodes_edit, where the last in input order wins, THE HIGHEST TRIANGLE INDEX COLOURS A
 * SHARED CELL.  No atomics: the same bytes on every run.
 * xyz_out_dev == NULL is a count query: *n_out gets the number of entries, nothing else is written and max_voxels is
 * ignored.  Otherwise xyz_out_dev (3 * max_voxels u32), colour_out_dev (max_voxels u32) and tri_out_dev (max_voxels u32,
 * or NULL) get the entries [0, *n_out) and nothing behind them.  n_tris == 0 succeeds with *n_out = 0.
 * All pointers but p and n_out are DEVICE pointers on the ctx's device.  The call needs no node buffer and never touches
 * one.  Runs on the ctx stream; blocks once per level to read that level's pair count; the last level's fill is
 * enqueued: inputs and outputs must stay valid until svo_sync.
 * A refused call leaves the outputs and *n_out as they were.  Of several causes the first in this order is reported.
 * SVO_ERR_ARG: NULL p or n_out; non-zero flags; depth outside 1..21; n_tris >= 2^31; NULL vq_dev or tri_dev with
 * n_tris > 0; NULL colour_out_dev with xyz_out_dev given; checked on the device: a vertex index >= n_vertices or a
 * coordinate >= 2^(depth + 6) (svo_last_error names the first triangle this applies to).  SVO_ERR_CAP: the pair count
 * passes max_voxels, or reaches 2^31 (also in a count query).  The pairs (triangle, cell) are refined one level at a time
 * and their number never decreases from a level to the next (every overlapping cell has an overlapping child), so the
 * refusal comes at the first level that exceeds the cap, names that level and its pair count, and no wider level is
 * allocated. */
typedef struct svo_voxelize_params {
    uint32_t depth;          /* 1..21: the grid is 2^depth cells a side */
    uint32_t flags;          /* must be 0 */
    uint32_t default_colour; /* used when tri_colours == NULL */
    uint32_t n_vertices;
    uint64_t max_voxels;     /* capacity of the outputs, in entries; ignored by a count query */
} svo_voxelize_params;
#define SVO_VOX_SUBBITS 6
int svo_mesh_voxelize(svo_ctx *ctx, const svo_voxelize_params *p,
                      const uint32_t *vq_dev,          /* n_vertices * 3 quantised coordinates */
                      const uint32_t *tri_dev,         /* n_tris * 3 vertex indices */
                      const uint32_t *tri_colours_dev, /* n_tris x 0x00RRGGBB, or NULL */
                      size_t n_tris,
                      uint32_t *xyz_out_dev, uint32_t *colour_out_dev, uint32_t *tri_out_dev /* may be NULL */,
                      uint64_t *n_out);
/* Times (ms) of the last voxelisation that ran: [0] setup (the vertex check and the triangles' gather), [1] the levels
 * 1 .. depth - 1 (test, scan, scatter and one read-back each), [2] the last level's test and scan (with its read-back),
 * [3] emit (device events; waits for the emit; 0 for a count query), [4] host wall time of the call.  A refused call
 * leaves the times of the last voxelisation that ran. */
#define SVO_VOXELIZE_TIMES 5
int svo_voxelize_timing(svo_ctx *ctx, float ms_out[SVO_VOXELIZE_TIMES]);

/* ---- closed meshes voxelised solid on the GPU ----
 * The cells of the 2^depth grid that lie inside a triangle mesh, as a voxel list for svo_nodes_build and svo_nodes_edit
 * or as y-spans.  Units, vertices and their checks are svo_mesh_voxelize's: a vertex is V = 2q + 1 in doubled units, a
 * cell c spans [128c, 128(c + 1)] per axis and its centre is C = 128c + 64.  A cell is judged at its centre moved by a
 * symbolic (dx, dy, dz) with 1 >> dy >> dx >> dz > 0, a generic point: every tie has one answer, the same for every
 * triangle.  For a triangle with edges e_i = V_(i+1) - V_i and n = e0 x e1:
 *   edge-on     n.y == 0: it covers no column and contributes nothing.
 *   covers the column (cx, cz) iff s * sgn_i > 0 for i = 0, 1, 2, with s = sign(-n.y),
 *               F_i = e_i.x (Cz - V_i.z) - e_i.z (Cx - V_i.x) (int64, below 2^57) and sgn_i = sign(F_i), or for F_i == 0
 *               sign(-e_i.z), or for e_i.z == 0 too sign(e_i.x).
 *   crosses above the centre cy iff D = n . (C - V0) (below 2^87: 128 bits) is non-zero and sign(D) != sign(n.y); a
 *               centre on the plane is above it.  D is monotone in Cy, so these cy are {0 .. k - 1}: k in [0, 2^depth] is
 *               the triangle's height in the column.
 *   w           sign(n.y).
 * The cell (cx, cy, cz) is inside under SVO_SOLID_EVENODD iff the number of covering triangles with k > cy is odd, under
 * SVO_SOLID_NONZERO iff the sum of their w is non-zero.  A column is open when that holds below every height (at cy = -1:
 * an odd number of covering triangles, or a non-zero sum of w); a watertight mesh has none, and the cells of an open
 * column are still the rule's.  The order of the triangles does not matter to the result at all.
 * With SVO_SOLID_SPANS the output is the maximal runs [y0, y1) of inside cells of a column as (x, z, y0, y1), ascending in
 * (x, z, y0); without, their cells (x, y, z), ascending in (x, z, y).  No float and no atomic takes part: the same bytes on
 * every run.  out_dev == NULL is a count query: *n_out gets the number of entries (cells, or spans), *n_open_out (when
 * given) the number of open columns, nothing else is written and max_out is ignored.  Otherwise out_dev gets the entries
 * [0, *n_out) and nothing behind them.  n_tris == 0 succeeds with 0.
 * All pointers but p, n_out and n_open_out are DEVICE pointers on the ctx's device.  The call needs no node buffer and
 * never touches one.  Runs on the ctx stream; blocks once per level of the column refinement and once per count (spans,
 * cells); the fill is enqueued: inputs and outputs must stay valid until svo_sync.
 * A refused call leaves out_dev, *n_out and *n_open_out as they were.  Of several causes the first in this order is
 * reported.  SVO_ERR_ARG: NULL p or n_out; unknown flag bits or non-zero reserved; depth outside 1..21; n_tris >= 2^31;
 * NULL vq_dev or tri_dev with n_tris > 0; checked on the device, with svo_mesh_voxelize's messages: a vertex index >=
 * n_vertices or a coordinate >= 2^(depth + 6).  SVO_ERR_CAP: a level's count of (triangle, column square) pairs passes
 * max_pairs (the message names the level and the count; the counts of the levels below the last never fall, so this is
 * the first such level and no wider one is allocated; the last level counts the crossings); the entry count passes
 * max_out (not in a count query) or reaches 2^31 (always), with the exact count in the message. */
#define SVO_SOLID_EVENODD 0u
#define SVO_SOLID_NONZERO 1u
#define SVO_SOLID_SPANS   2u
typedef struct svo_solid_params {
    uint32_t depth;        /* 1..21 */
    uint32_t flags;
    uint32_t n_vertices;
    uint32_t reserved;     /* 0 */
    uint64_t max_out;      /* room in the output, in entries (cells, or spans); ignored by a count query */
    uint64_t max_pairs;    /* cap on (triangle, column-square) pairs of any level; 0 = 2^27 */
} svo_solid_params;
int svo_mesh_voxelize_solid(svo_ctx *ctx, const svo_solid_params *p, const uint32_t *vq_dev, const uint32_t *tri_dev, size_t n_tris,
                            uint32_t *out_dev /* cells: 3 u32 (x, y, z); spans: 4 u32 (x, z, y0, y1); NULL = count query */,
                            uint64_t *n_out, uint64_t *n_open_out /* may be NULL */);
/* Times (ms) of the last solid voxelisation that ran: [0] setup, [1] the column levels (with the crossings' emit), [2] the
 * sort, [3] spans (heads, intervals, runs and their read-back; in cell mode the cells' count too), [4] emit (0 for a
 * count query), [5] host wall time of the call.  A refused call leaves the times of the last one that ran. */
#define SVO_SOLID_TIMES 6  /* setup, column levels, sort, spans, emit, host wall */
int svo_solid_timing(svo_ctx *ctx, float ms_out[SVO_SOLID_TIMES]);

/* ---- voxel structures scattered over the tree in the node buffer ----
 * Three calls that together populate a terrain without the tree leaving the device: where the ground is in every
 * column of a rectangle (svo_nodes_column_tops), which columns get a structure (svo_structures_sites), and the voxel
 * list of a structure stamped at every site (svo_structures_stamp), which svo_nodes_edit takes as it is.
 *
 * svo_nodes_column_tops: the highest occupied cell of each column of the `depth` grid, by the rule of svo_nodes_sample.
 * For the column (x, z) = (origin_xz[0] + i, origin_xz[1] + k), i < size_xz[0], k < size_xz[1]:
 *     for y = y_hi - 1 down to y_lo:
 *         v = the value svo_nodes_sample gives the cell (x, y, z) at `depth`
 *         if v != 0:  top = y, value = v, done
 *     top = SVO_TOP_NONE, value = 0
 * so value is a colour, SVO_SAMPLE_FINER (the tree is interior at `depth` there: occupied, and said so) or
 * SVO_SAMPLE_BROKEN.  Hit counters never matter.  A leaf above `depth` covers a run of the column's cells: y_hi and y_lo
 * may cut through it, and top is then the highest of its cells below y_hi.  top_out_dev[i * size_xz[1] + k] and, unless
 * it is NULL, value_out_dev[i * size_xz[1] + k] get the column's result (z runs fastest, as in svo_nodes_sample_dense);
 * only these size_xz[0] * size_xz[1] entries are written.  A size with a 0 succeeds and writes nothing.
 * The outputs are DEVICE pointers.  The call only reads the node buffer, runs on the ctx stream behind the store's last
 * write, whichever context issued it, records no write and DOES NOT BLOCK: outputs must stay valid until svo_sync.  No
 * atomics: the same bytes on every run and for every layout of the same tree.  No pointer is followed before it passed
 * svo_nodes_sample's check, and the depth bound ends every walk on a cyclic tree.  A device adaptive state attached to the
 * context is no obstacle.
 * Errors are decided on the host from the arguments before anything is enqueued; the first in this order is reported:
 * SVO_ERR_ARG: NULL p; NULL origin_xz, size_xz or top_out_dev; non-zero flags; depth outside 1..21; y_lo >= y_hi or
 * y_hi > 2^depth; a rectangle with origin + size > 2^depth on an axis; 2^31 columns or more.  SVO_ERR_STATE: no node
 * buffer.  SVO_ERR_ARG: n_words not a positive multiple of 8 or above the capacity. */
#define SVO_TOP_NONE 0xFFFFFFFFu /* nothing in the column within [y_lo, y_hi) */
typedef struct svo_tops_params {
    uint32_t flags;    /* 0 */
    uint32_t depth;    /* 1..21: the grid the columns stand on */
    uint64_t n_words;  /* the tree: words [0, n_words) of the node buffer, rooted at group 0 */
    uint32_t y_lo;     /* the search covers y_lo <= y < y_hi <= 2^depth */
    uint32_t y_hi;
} svo_tops_params;
int svo_nodes_column_tops(svo_ctx *ctx, const svo_tops_params *p, const uint32_t origin_xz[2], const uint32_t size_xz[2],
                          uint32_t *top_out_dev, uint32_t *value_out_dev /* may be null */);

/* svo_structures_sites: the columns of a rectangle that get a structure, from the two arrays svo_nodes_column_tops wrote
 * for it (top_dev, value_dev: DEVICE, size_xz[0] * size_xz[1] u32 each, z fastest).  With lowbias32(v): v ^= v >> 16,
 * v *= 0x7feb352d, v ^= v >> 15, v *= 0x846ca68b, v ^= v >> 16 in wrapping u32 arithmetic, and
 * h = lowbias32(lowbias32(x + seed) ^ z) for the column (x, z) = origin_xz + (i, k), the column is a site iff
 *     top != SVO_TOP_NONE,  value < 2^27 (neither FINER nor BROKEN),  on_value == 0 or value == on_value,  h % one_in == 0.
 * value_dev may be NULL when on_value == 0; the two tests on value are then skipped.  A site's origin is the three int32
 * (x, top + lift, z), its rotation lowbias32(h + 0x9E3779B9) >> 30 with SVO_SITES_ROTATE and 0 without.  The sites come
 * in the order of the arrays (x, then z).
 * origins_out_dev == NULL is a count query: *n_out gets the number of sites, nothing else is written and max_sites is
 * ignored.  Otherwise origins_out_dev (3 * max_sites int32) and rots_out_dev (max_sites u32, or NULL) are DEVICE pointers
 * that get the entries [0, *n_out) and nothing behind them.  An empty rectangle succeeds with *n_out = 0.
 * The call needs no node buffer.  Runs on the ctx stream, blocks once to read the count; the fill is enqueued: inputs and
 * outputs must stay valid until svo_sync.  Scans and no atomics: the same bytes on every run.
 * A refused call leaves the outputs and *n_out as they were; the first cause in this order is reported.  SVO_ERR_ARG: NULL
 * p or n_out; flag bits other than SVO_SITES_ROTATE; one_in == 0; NULL origin_xz or size_xz; an origin or a size of 2^31
 * or more on an axis, or 2^31 columns or more; NULL top_dev with columns to read; NULL value_dev with on_value != 0.
 * SVO_ERR_CAP, with the exact count in svo_last_error: more sites than max_sites (not for a count query). */
#define SVO_SITES_ROTATE 1u
typedef struct svo_sites_params {
    uint32_t flags;      /* 0 or SVO_SITES_ROTATE */
    uint32_t seed;
    uint32_t one_in;     /* >= 1: one column in one_in is picked, by the hash */
    uint32_t on_value;   /* 0, or the only value of a column's top that takes a structure */
    int32_t lift;        /* added to top: 1 stands the structure's y = 0 layer on the ground */
    uint32_t reserved;   /* 0 */
    uint64_t max_sites;  /* room in the outputs, in sites; ignored by a count query */
} svo_sites_params;
int svo_structures_sites(svo_ctx *ctx, const svo_sites_params *p, const uint32_t *top_dev, const uint32_t *value_dev /* may be null */,
                         const uint32_t origin_xz[2], const uint32_t size_xz[2], int32_t *origins_out_dev,
                         uint32_t *rots_out_dev /* may be null */, uint64_t *n_out);

/* svo_structures_stamp: k placements of a structure of m voxels as one voxel list.  offsets_dev (m * 3 int32) and
 * colours_dev (m u32) are the structure (svo_structure_load), origins_dev (k * 3 int32) and rots_dev (k u32, or NULL: all
 * 0) the placements (svo_structures_sites); all DEVICE pointers.  The entry (p, v) has the cell
 *     origins[p] + R^rots[p](offsets[v]),   R (dx, dy, dz) = (dz, dy, -dx): a quarter turn about +y,
 * and exists iff that cell lies in [0, 2^depth)^3: everything else is clipped, and a placement wholly outside gives
 * nothing.  The entries come placement by placement and, within a placement, in the structure's order: fed to
 * svo_nodes_edit, where the last in input order wins, A LATER PLACEMENT WINS A SHARED CELL.  xyz is the cell, colour
 * colours[v] as it is (svo_nodes_edit masks it to 24 bits; 0 removes the cell), placement p.
 * xyz_out_dev == NULL is a count query: *n_out gets the number of entries, nothing else is written and max_voxels is
 * ignored.  Otherwise xyz_out_dev (3 * max_voxels u32), colour_out_dev (max_voxels u32) and placement_out_dev (max_voxels
 * u32, or NULL) get the entries [0, *n_out) and nothing behind them.  k == 0 or m == 0 succeeds with *n_out = 0.
 * The call needs no node buffer.  Runs on the ctx stream, blocks once to read the count and the device's checks; the fill
 * is enqueued: inputs and outputs must stay valid until svo_sync.  Scans and no atomics: the same bytes on every run.
 * A refused call leaves the outputs and *n_out as they were; the first cause in this order is reported.  SVO_ERR_ARG: NULL
 * p or n_out; non-zero flags; depth outside 1..21; k * m >= 2^31 (decided in 64 bits before any launch); NULL offsets_dev,
 * colours_dev or origins_dev with k * m > 0; NULL colour_out_dev with xyz_out_dev given; checked on the device, the lowest
 * index named in svo_last_error: a placement with an origin component outside [-2^22, 2^22), else a placement with a
 * rotation >= 4, else a voxel with an offset component outside (-2^22, 2^22).  SVO_ERR_CAP, with the exact count in
 * svo_last_error: more entries than max_voxels (not for a count query). */
typedef struct svo_stamp_params {
    uint32_t flags;       /* 0 */
    uint32_t depth;       /* 1..21: the grid the cells are clipped to */
    uint64_t max_voxels;  /* room in the outputs, in entries; ignored by a count query */
} svo_stamp_params;
int svo_structures_stamp(svo_ctx *ctx, const svo_stamp_params *p, const int32_t *offsets_dev, const uint32_t *colours_dev, size_t m,
                         const int32_t *origins_dev, const uint32_t *rots_dev /* may be null */, size_t k,
                         uint32_t *xyz_out_dev, uint32_t *colour_out_dev, uint32_t *placement_out_dev /* may be null */,
                         uint64_t *n_out);
/* Times (ms) of the last of the three calls that ran on the context: [0] count (column tops: the kernel; sites and
 * stamp: the checks, the flags' sums and their scan, with the read-back), [1] fill (device events; waits for it; 0 for
 * column tops and for a count query), [2] host wall time of the call.  A refused call, and one with nothing to do,
 * leaves them. */
#define SVO_STRUCTURE_TIMES 3
int svo_structure_timing(svo_ctx *ctx, float ms_out[SVO_STRUCTURE_TIMES]);

/* ---- mip-coloured chunk trees and streamable worlds built on the GPU ----
 * Inputs as svo_nodes_build: xyz n * 3 u32 and colours n u32 (0x00RRGGBB) or NULL, DEVICE pointers on the ctx's device;
 * the last voxel of a cell wins; a colour-0 voxel is an empty leaf on a path that exists.  A chunk tree is the host
 * CpuOctree of sequential put_in_voxel(cell / 2^d * 2 - 1, rgb, d) with d its depth, in canonical breadth-first order and
 * with the bytes of svo_cpu_octree_bin: interior pointer = index of its child group, leaf = SVO_CHUNK_OFFSET with the
 * voxel's r g b (r = colour >> 16), empty = SVO_CHUNK_OFFSET with rgb 0.  Interior rgb and top_mip are what
 * svo_world_generate_mip_tree computes.  The same bytes on every run and for any order of distinct voxels.
 * Errors create nothing (no directory, no file) and leave the context usable: SVO_ERR_ARG for bad depths, n >= 2^31, NULL
 * xyz with n > 0, a coordinate outside [0, 2^depth) (checked on the device) or an existing path ("File already exists");
 * SVO_ERR_CAP (with a message) when a chunk's node count exceeds max_nodes or 2^31.  Blocking. */
typedef struct svo_chunk_build_params {
    uint32_t depth;          /* 1..21: cells in [0, 2^depth) per axis */
    uint32_t world_depth;    /* svo_world_build: 1..4, chunk depth = depth - world_depth >= 1; svo_cpu_octree_build: 0 */
    uint32_t default_colour; /* used when colours == NULL */
    uint64_t max_nodes;      /* per chunk; 0 = 256 000 000 (procedural.rs:4) */
} svo_chunk_build_params;
/* One mip-coloured CpuOctree from a DEVICE voxel list (caller frees it); *out NULL for n == 0. */
int svo_cpu_octree_build(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, const svo_chunk_build_params *p,
                         struct svo_cpu_octree **out);
/* A chunked world in w's path (must not exist; created), as svo_world_generate lays one out: chunk (cx, cy, cz) = the top
 * world_depth bits of the cells, id SVO_CHUNK_OFFSET / 2 + (cx * s + cy) * s + cz with s = 2^world_depth, local cells
 * cell & (2^(depth - world_depth) - 1).  <id>.bin per non-empty chunk (each stays in w with its nodes dropped and its
 * top_mip kept); the root references them by put_in_block in id order, is mipped over their top_mips and saved as 0.bin,
 * last. */
int svo_world_build(svo_ctx *ctx, struct svo_world *w, const uint32_t *xyz, const uint32_t *colours, size_t n,
                    const svo_chunk_build_params *p);
/* Times (ms) of the last svo_cpu_octree_build / svo_world_build: [0] keys, [1] sort, [2] levels, [3] count read-back,
 * [4] emit, [5] mips (device events); [6] chunk read-back, [7] chunk files and root (svo_cpu_octree_build: the CpuOctree),
 * [8] host wall time of the call. */
#define SVO_WORLD_BUILD_TIMES 9
int svo_world_build_timing(svo_ctx *ctx, float ms_out[SVO_WORLD_BUILD_TIMES]);

/* ---- the adaptive step on the GPU ----
 * Device form of the streaming loop's list processing: after svo_adaptive_step the node buffer, the node positions, the
 * hole stack, the tree length, the world's chunk set and the counts equal what svo_adaptive_subdivide(sorted(sub)) then
 * svo_adaptive_unsubdivide(sorted(unsub)) make of the same state, bit for bit.  The state lives with the context:
 * svo_adaptive_attach uploads the host octree's positions, hole stack and length and mirrors every resident chunk of w
 * (the words must already be in the node buffer; SVO_OPT_SCAN_CLEARS_COUNTERS must be 1).  w stays the owner of chunk
 * data and must outlive the attachment: chunk loads go through svo_world_load_chunk, removals through svo_world_remove.
 * Attach again after any other change to the tree or the world. */
typedef struct svo_adaptive_result {
    uint32_t n_sub, n_unsub;    /* nodes subdivided / unsubdivided (the host calls' return values) */
    uint64_t chunks_loaded;     /* chunks the subdivide pass loaded */
    uint64_t length;            /* the tree's length afterwards (svo_octree_len) */
    uint32_t n_removed;         /* chunks the unsubdivide pass dropped ... */
    const uint32_t *removed;    /* ... their ids, ascending; valid until the next call on ctx */
} svo_adaptive_result;
struct svo_octree;
int svo_adaptive_attach(svo_ctx *ctx, struct svo_world *w, const struct svo_octree *o);
/* d_sub / d_unsub: DEVICE lists of node indices (any order; both or neither).  NULL: the context's own scan lists, clamped
 * like svo_scan_read (min(count, capacity - 1)) with their counters reset -- no list crosses PCIe.  Blocking.
 * SVO_ERR_STATE, with nothing written, for a subdivide list that the parallel form cannot take (an entry listed twice,
 * an entry >= length, an entry inside a hole group the pass reuses, an entry whose walk ends at another listed leaf):
 * it needs the sequential host path.  SVO_ERR_CAP, nothing written, when the new groups would pass the capacity.  Any
 * other error (where the host calls fail too) leaves the state unspecified until the next attach. */
int svo_adaptive_step(svo_ctx *ctx, const uint32_t *d_sub, uint32_t n_sub, const uint32_t *d_unsub, uint32_t n_unsub,
                      svo_adaptive_result *out);
/* o := the device state (words without counters, positions, hole stack, length); clears o's dirty set.  Blocking. */
int svo_adaptive_download(svo_ctx *ctx, struct svo_octree *o);
int svo_adaptive_length(svo_ctx *ctx, uint64_t *len_out);
/* Times (ms) of the last step: [0] sorting both lists, [1] subdivide pass, [2] unsubdivide pass (device events, read-backs
 * and chunk loads included), [3] host wall time of the call. */
#define SVO_ADAPT_TIMES 4
int svo_adaptive_timing(svo_ctx *ctx, float ms_out[SVO_ADAPT_TIMES]);
/* Device form of svo_world_expand: refines the attached tree to a view's level of detail without the words
 * or the positions leaving the device.  Afterwards the node buffer's words [0, length), the positions, the length and
 * out->n_sub (the subdivisions; n_unsub, n_removed stay 0) equal, bit for bit, what
 * svo_world_expand(w, o, max_depth, cam, lod_c, min(max_words, capacity)) makes of the attached octree and world on the
 * host.  cam may be NULL (then, or with lod_c <= 0, every leaf above max_depth is refined); max_words 0 means the node
 * buffer's capacity and a larger value is clamped to it: reaching the cap is where expansion stops, not an error.
 * The world's chunk set equals the host's too, except when the cap cuts a level short: leaves behind the cut may then
 * have loaded chunks the host never asked for (a superset of the host's set).
 * SVO_ERR_ARG for max_depth > 31; SVO_ERR_STATE, nothing written, when the attached tree's hole stack is not empty (the
 * host then reuses groups in an order the sorted pass does not reproduce: expand such a tree with svo_world_expand);
 * otherwise the errors of svo_adaptive_step's subdivide pass.  Blocking. */
int svo_adaptive_expand(svo_ctx *ctx, uint32_t max_depth, const float cam[3], float lod_c, uint64_t max_words,
                        svo_adaptive_result *out);
/* Times of the last svo_adaptive_expand: [0] listing the leaves, [1] choosing each level's candidates, [2] the subdivide
 * passes with the next frontier (ms, device events, read-backs and chunk loads included), [3] host wall time of the call
 * (ms), [4] the number of levels. */
#define SVO_ADAPT_EXPAND_TIMES 5
int svo_adaptive_expand_timing(svo_ctx *ctx, float ms_out[SVO_ADAPT_EXPAND_TIMES]);

#ifdef __cplusplus
}
#endif
#endif
