// svo_ctx.h -- the device context behind the opaque `svo_ctx` of include/svo_hip.h, and the host helpers of the files that
// use it: svo_abi.cpp (trace / scan dispatch), svo_comm.cpp (RCCL frame gather) and the GPU tree passes (svo_proc.hip,
// svo_build.hip, svo_edit.hip, svo_region.hip, svo_combine.hip, svo_place.hip, svo_transform.hip, svo_morph.hip, svo_heightmap.hip, svo_compact.hip, svo_simplify.hip, svo_list.hip, svo_sample.hip, svo_distance.hip, svo_voxelize.hip, svo_solid.hip,
// svo_structure.hip, svo_surface.hip, svo_surface_merge.hip, svo_components.hip, svo_adapt.hip).  One rule of ownership for the context, the node store and every
// pass's state: a member owns what it holds, as svo_dev / svo_pinned (an allocation and its size), svo_events (events) or
// svo_stream (a stream).  The passes
// share the rest as their host frame: svo_grow / svo_grow_pinned / svo_grow_keep (workspaces, by the buffers' own
// sizes), svo_mirrored (device words with a pinned mirror), svo_pass_timer (events and times), svo_workspace_ensure
// (creation) and the svo_check_* argument checks; then what several passes run: the builder's sort and list front end,
// svo_tree_walk (the discovery of a tree in the node buffer, with the workspace it owns), svo_tree_rewrite (a tree
// rewritten into the canonical layout: the compaction's and the simplification's workspace and host frame),
// svo_list_plan (a listing's counts and offsets) and svo_world_writer (a generated world's directory).
// svo_scan.h (the tiled count, scan and emit with their launches), svo_frontier.h (the frontier walk of the six
// top-down edits: its workspace, svo_frontier_walk, its kernels and its host frame), svo_group.h, svo_mip.h and svo_morton.h hold the device pieces, svo_rules.h the walks and rules that svo_host.cpp and svo_adapt.hip both run.
// What a frame launches is decided in plain C++ beside the context, not in it: svo_sched.h (the schedule's plans, the trace
// kernel and its grid) and svo_deal.h (the static deal).  The context keeps what those decisions go by between frames: the
// options, the schedule slots, and per STACK instantiation the resident workgroups per CU that the runtime answered.
// Internal: not part of the boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "svo_deal.h"
#include "svo_device.h"
#include "svo_hip.h"
#include "svo_host.h"

// ---- owning members: what the context, the node store and the passes' states hold their resources in ----

// One device (or pinned host) allocation and its size: freed with its owner, moved but not copied, a T* wherever one is
// wanted.  size() is the room in items (in bytes of a void buffer); alloc() is the one place that allocates.
template <typename T, bool kPinned>
struct svo_mem {
    T *p = nullptr;
    size_t n = 0;
    svo_mem() = default;
    svo_mem(svo_mem &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    svo_mem &operator=(svo_mem &&o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~svo_mem() { reset(); }
    void reset() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        n = 0;
    }
    // frees what there is, then room for `items`; size() says so only when the allocation succeeded
    hipError_t alloc(size_t items) {
        reset();
        const size_t bytes = items * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
        const hipError_t e = kPinned ? hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) : hipMalloc((void **)&p, bytes);
        if (e == hipSuccess) n = items;
        else p = nullptr;
        return e;
    }
    size_t size() const { return n; }
    T *get() const { return p; }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};
template <typename T>
using svo_dev = svo_mem<T, false>;
template <typename T>
using svo_pinned = svo_mem<T, true>;

// N events, destroyed with their owner (or by reset()), moved but not copied.  create() makes the ones that are not
// there yet, with `flags` (hipEventDisableTiming for events that only order streams: they are cheaper to record).
template <int N>
struct svo_events {
    hipEvent_t e[N] = {};
    svo_events() = default;
    svo_events(svo_events &&o) noexcept {
        for (int k = 0; k < N; k++) e[k] = o.e[k], o.e[k] = nullptr;
    }
    svo_events &operator=(const svo_events &) = delete;
    svo_events &operator=(svo_events &&o) noexcept {
        for (int k = 0; k < N; k++) std::swap(e[k], o.e[k]);
        return *this;
    }
    ~svo_events() { reset(); }
    void reset() {
        for (hipEvent_t &x : e) {
            if (x) (void)hipEventDestroy(x);
            x = nullptr;
        }
    }
    hipError_t create(unsigned flags = hipEventDefault) {
        for (hipEvent_t &x : e)
            if (!x)
                if (hipError_t err = flags ? hipEventCreateWithFlags(&x, flags) : hipEventCreate(&x)) return err;
        return hipSuccess;
    }
    hipEvent_t operator[](int k) const { return e[k]; }
};

// A non-blocking stream, destroyed with its owner (or by reset()).
struct svo_stream {
    hipStream_t s = nullptr;
    svo_stream() = default;
    svo_stream(const svo_stream &) = delete;
    svo_stream &operator=(const svo_stream &) = delete;
    ~svo_stream() { reset(); }
    void reset() {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

// The device node buffer (render.rs:53-61) and what is derived from it.  Several contexts can trace from one store
// (svo_nodes_share: frames in flight on several streams): they share the words, the generation counter that tells every
// one of them when its own top table and strip schedule are stale, and the event that orders their reads behind the
// last write, whichever context issued it.  Every context bound to it holds a reference; it goes with the last one.
struct svo_node_store {
    int device = 0;
    uint32_t *nodes = nullptr;
    size_t capacity = 0;
    bool owned = false;          // allocated by svo_nodes_alloc (freed with the store)
    uint64_t version = 1;        // bumped whenever the words may have changed
    svo_events<1> last_write;    // recorded on the writing context's stream after every write (made by the first)
    hipStream_t last_writer = nullptr; // that stream: other streams wait for the event before they read
    ~svo_node_store() {  // (then last_write, on the same device)
        (void)hipSetDevice(device);
        if (nodes && owned) (void)hipFree(nodes);
    }
};

// The workspace of a GPU pass, kept per context and freed with it, member by member.  Its type is
// complete only in the pass's own file, so the deleter is bound there, by svo_workspace_new.
struct svo_proc_state;
struct svo_build_state;
struct svo_adapt_state;
struct svo_edit_state;
struct svo_compact_state;
struct svo_simplify_state;
struct svo_region_state;
struct svo_combine_state;
struct svo_place_state;
struct svo_transform_state;
struct svo_morph_state;
struct svo_heightmap_state;
struct svo_frontier_walk;
struct svo_list_state;
struct svo_sample_state;
struct svo_distance_state;
struct svo_voxelize_state;
struct svo_solid_state;
struct svo_structure_state;
struct svo_surface_state;
struct svo_surface_merge_state;
struct svo_components_state;
template <typename T>
using svo_workspace = std::unique_ptr<T, void (*)(T *)>;
template <typename T>
svo_workspace<T> svo_workspace_new() {
    return svo_workspace<T>(new T(), [](T *p) { delete p; });
}

// Every resource is a member that owns it, and svo_ctx_destroy only deletes the context.  The order of the members
// matters: they go in reverse, so the two streams stand first and outlive everything that may still be ordered on them.
struct svo_ctx {
    svo_stream own_stream;
    svo_stream comm_stream;      // the gathers run here, ordered against `stream` by the two events of comm_ev
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;  // own_stream, or the caller's (svo_ctx_set_stream)
    // node buffer (render.rs:53-61): `nodes` / `capacity` mirror the store this context is bound to
    std::shared_ptr<svo_node_store> store;
    uint32_t *nodes = nullptr;
    size_t capacity = 0;
    uint64_t top_version = 0;    // store version this context's top table was built from (0: none)
    svo_dev<uint32_t> top_table;
    int cull_mode = 2;           // SVO_OPT_CULL
    bool cam_shortcut = true;    // SVO_OPT_CAMERA_SHORTCUT
    void *comm = nullptr;        // ncclComm_t (svo_comm.cpp); world size and rank of this context in it
    int comm_world = 0, comm_rank = 0;
    svo_events<2> comm_ev;       // ready and done (svo_comm.cpp), made with the stream, without timing
    bool gathers_issued = false;
    svo_dev<uint32_t> status;          // device error word
    svo_dev<uint32_t> defer_buf;       // {strip counter, deferred count, deferred item indices...}
    size_t defer_items = 0;            // rays per deferred list (the allocation: kCounterWords + 2 * (defer_items + 1) words)
    // scan lists (compute.rs:46-64): slot 0 = count.  One allocation, the subdivide list in its first half
    svo_dev<uint32_t> scan_lists;
    size_t scan_capacity = 0;  // words per list: where the second list starts
    uint32_t *scan_sub() const { return scan_lists; }
    uint32_t *scan_unsub() const { return scan_lists + scan_capacity; }
    // device staging for svo_render_host
    svo_dev<char> stage;
    svo_uniforms uniforms{};
    bool have_uniforms = false;
    // options
    int variant = SVO_VARIANT_STACK;
    int grid_blocks = 0;
    int occupancy[svo::kTraceSlots] = {};  // resident workgroups per CU of each STACK instantiation on this device, by svo::trace_slot (0: not asked yet)
    uint32_t refill_min = 32;  // (round 5: 16 until the schedule's locality work; profiles/r05_refill_sweep.log)
    bool scan_clears = false;
    int fused_shadows = 2;  // 0: off, 1: on, 2: automatic (see fuse_shadow_rays)
    svo_dev<uint32_t> scatter_buf;  // svo_nodes_scatter: indices, then values
    svo_dev<uint32_t> scan_tiles;   // svo_scan_u32 (svo_scan.h): the tile sums of an in-place scan, whichever pass asks
    uint32_t block_w_log2 = 3;  // 64-pixel blocks of 8x8
    uint32_t tree_depth = 16;  // caller's bound on the octree depth (the reference's Settings.octree_depth)
    // scheduling feedback (strip order from an earlier frame of the same work layout); slot 1: shadow rays.  What is decided per
    // frame is svo_sched.h's; svo_abi.cpp's trace_launch measures its facts and runs the launches.
    struct Sched {
        svo::SchedState state;
        svo_dev<uint8_t> cost, cls_now;  // for up to `cap` strips: svo::SchedBuffers says what they hold
        svo_dev<uint32_t> order, balance;
        size_t cap = 0;  // strips the buffers were sized for
        svo::SchedBuffers buf() const { return {cost, cls_now, order, balance}; }
        svo::WorkDesc key{};  // the work layout of the costs
        // what the schedule was measured on: while camera and tree stay the same it stays exact and is not rebuilt
        svo_uniforms built_uniforms{};
        uint64_t built_nodes_version = 0;
        // camera motion (SVO_OPT_SCHEDULE_MOTION): the uniforms of the previous frame
        svo_uniforms prev_uniforms{};
        bool have_prev = false;
        // a resting view's static deal (svo_deal.h; slot 0 only): the table the replay kernel reads, its rows' lengths, the steps' move log, the lists
        // it was seeded from, the waves' stamps and the state words, with a pinned copy of those that the host looks at when
        // it has arrived (seen_ev) and never waits for
        struct DealBuffers {
            svo::DealState state;
            svo_dev<uint32_t> table, len, log, lists, stamps, words;
            svo_pinned<uint32_t> seen;
            svo_events<1> seen_ev;
            bool seen_pending = false;
            bool last_replayed = false;  // the frame before this one was traced by the replay kernel
            svo::Deal view(uint32_t order_cap, uint32_t pairs_div) const {
                return {table, len, log, lists, stamps, words, state.row_cap, state.grid_blocks, order_cap, pairs_div};
            }
        };
        DealBuffers deal;
        hipError_t alloc(uint32_t n_strips);  // frees what there is and starts the slot over (svo_abi.cpp)
        void release() { *this = Sched{}; }  // (the buffers go with the temporary)
    };
    Sched sched[2];
    bool static_deal = true;   // SVO_OPT_STATIC_DEAL
    uint32_t deal_pairs_div = svo::kDealPairsDiv;  // (SVO_DEAL_PAIRS_DIV: the sweep of tools/deal_probe.py)
    bool list_balance = true;  // unless SVO_NO_LIST_BALANCE is set (A/B switch of the list-share feedback, svo_kernels.hip: balance_step)
    uint32_t motion_floor = 0x1204;  // SVO_OPT_SCHEDULE_MOTION: class floor | radius << 8 | min_count << 12; 0 = off
    bool schedule = true;
    uint32_t sched_period = 2;  // frames between schedule rebuilds (tools/perf_probe.py --motion: 2 keeps the gain under camera motion)
    int frame_parity = 0;
    // shading pass scratch (svo_render with rgba_out)
    svo_dev<svo_hit> shade_hits, shade_shadow;
    svo_dev<float> shade_aux, shade_rays;
    svo_dev<uint8_t> shade_skip;
    uint32_t *debug_buf = nullptr;  // caller-provided device buffer for the per-wave timeline (diagnostics)
    uint32_t strip_items = 64;
    // launch timing: a ring of (start, stop) event pairs recorded around trace launches
    std::vector<svo_events<2>> ev;  // one pair per slot; only ever added to
    size_t ev_slots = 0, ev_count = 0;
    svo_workspace<svo_proc_state> proc{nullptr, nullptr};    // procedural generator's workspace (svo_proc.hip)
    svo_workspace<svo_build_state> build{nullptr, nullptr};  // tree builder's workspace (svo_build.hip)
    svo_workspace<svo_adapt_state> adapt{nullptr, nullptr};  // device adaptive state (svo_adapt.hip)
    svo_workspace<svo_edit_state> edit{nullptr, nullptr};    // in-place edits' workspace (svo_edit.hip)
    svo_workspace<svo_compact_state> compact{nullptr, nullptr};  // compaction's workspace (svo_compact.hip)
    svo_workspace<svo_simplify_state> simplify{nullptr, nullptr};  // simplification's workspace (svo_simplify.hip)
    // the six top-down edits walk the tree in one workspace, made by the first of them that runs (svo_frontier.h); each keeps its own timer beside it
    svo_workspace<svo_frontier_walk> frontier{nullptr, nullptr};
    svo_workspace<svo_region_state> region{nullptr, nullptr};  // shape edits' shapes (svo_region.hip)
    svo_workspace<svo_combine_state> combine{nullptr, nullptr};  // the source records of two trees combined (svo_combine.hip)
    svo_workspace<svo_place_state> place{nullptr, nullptr};  // the items of a tree placed at an offset and orientation (svo_place.hip)
    svo_workspace<svo_transform_state> transform{nullptr, nullptr};  // the hints of a tree placed under an affine map (svo_transform.hip)
    svo_workspace<svo_morph_state> morph{nullptr, nullptr};  // the items of a morphology step (svo_morph.hip)
    svo_workspace<svo_heightmap_state> heightmap{nullptr, nullptr};  // a height-map edit's pyramid (svo_heightmap.hip)
    svo_workspace<svo_list_state> list{nullptr, nullptr};  // voxel listing's workspace (svo_list.hip)
    svo_workspace<svo_sample_state> sample{nullptr, nullptr};  // sampling's events and times (svo_sample.hip)
    svo_workspace<svo_distance_state> distance{nullptr, nullptr};  // the distance pass's bits, its y pass's output and its times (svo_distance.hip)
    svo_workspace<svo_voxelize_state> voxelize{nullptr, nullptr};  // mesh voxeliser's workspace (svo_voxelize.hip)
    svo_workspace<svo_solid_state> solid{nullptr, nullptr};  // solid voxeliser's workspace (svo_solid.hip)
    svo_workspace<svo_structure_state> structure{nullptr, nullptr};  // structure scattering's workspace (svo_structure.hip)
    svo_workspace<svo_surface_state> surface{nullptr, nullptr};  // surface extraction's workspace (svo_surface.hip)
    svo_workspace<svo_surface_merge_state> surface_merge{nullptr, nullptr};  // the merged surface's workspace (svo_surface_merge.hip)
    svo_workspace<svo_components_state> components{nullptr, nullptr};  // the component labelling's workspace (svo_components.hip)
    std::string err;
};


// svo_abi.cpp
int svo_fail(svo_ctx *ctx, int code, const char *what);
int svo_fail_hip(svo_ctx *ctx, hipError_t e, const char *what);
inline int svo_fail(svo_ctx *ctx, int code, const std::string &what) { return svo_fail(ctx, code, what.c_str()); }

#define HIP_TRY(ctx, expr)                                          \
    do {                                                            \
        hipError_t e_ = (expr);                                     \
        if (e_ != hipSuccess) return svo_fail_hip(ctx, e_, #expr); \
    } while (0)

inline double svo_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// blocks of `per` items that cover n
inline uint32_t svo_div_up(uint64_t n, uint64_t per) { return (uint32_t)((n + per - 1) / per); }

// ---- the host frame of a GPU pass: workspaces, status words, the timer, creation, shared checks ----

// Grows a group of buffers to `want` items of its own type each (a void buffer counts bytes): when one of them is
// smaller, waits for the context's stream, frees all of them and allocates them again.  A failure half way leaves the
// rest empty, so the next call starts over.  svo_grow takes device buffers, svo_grow_pinned pinned host buffers.
template <bool kPinned, typename... T>
int svo_grow_group(svo_ctx *ctx, size_t want, svo_mem<T, kPinned> *...bufs) {
    if (std::min({bufs->size()...}) >= want) return SVO_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    (bufs->reset(), ...);
    hipError_t group_alloc = hipSuccess;  // (the first failure ends the fold)
    (void)(... && ((group_alloc = bufs->alloc(want)) == hipSuccess));
    HIP_TRY(ctx, group_alloc);
    return SVO_OK;
}
template <typename... T>
int svo_grow(svo_ctx *ctx, size_t want, svo_dev<T> *...bufs) { return svo_grow_group(ctx, want, bufs...); }
template <typename... T>
int svo_grow_pinned(svo_ctx *ctx, size_t want, svo_pinned<T> *...bufs) { return svo_grow_group(ctx, want, bufs...); }

// svo_grow for one device buffer whose first `keep` items stay: they are copied on the context's stream, which is waited
// for before the old buffer is freed
template <typename T>
int svo_grow_keep(svo_ctx *ctx, size_t want, svo_dev<T> *buf, size_t keep) {
    if (buf->size() >= want) return SVO_OK;
    svo_dev<T> bigger;
    HIP_TRY(ctx, bigger.alloc(want));
    if (keep) HIP_TRY(ctx, hipMemcpyAsync(bigger, *buf, keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *buf = std::move(bigger);  // (a swap: the old buffer goes with `bigger`)
    return SVO_OK;
}

// n items on the device that kernels write, and their pinned mirror that the host reads after read().
template <typename T = uint32_t>
struct svo_mirrored {
    svo_dev<T> dev;
    svo_pinned<T> mirror;
    int alloc(svo_ctx *ctx, size_t items) {
        HIP_TRY(ctx, mirror.alloc(items));
        HIP_TRY(ctx, dev.alloc(items));
        return SVO_OK;
    }
    hipError_t zero(svo_ctx *ctx) { return hipMemsetAsync(dev, 0, dev.size() * sizeof(T), ctx->stream); }
    // the first `items` of them (all by default) into the mirror: enqueued by copy(), there after read()
    hipError_t copy(svo_ctx *ctx, size_t items = ~size_t(0)) {
        return hipMemcpyAsync(mirror, dev, std::min(items, dev.size()) * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
    }
    int read(svo_ctx *ctx, size_t items = ~size_t(0)) {
        HIP_TRY(ctx, copy(ctx, items));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return SVO_OK;
    }
    T *host() const { return mirror; }
};

// The events of a pass and the times read from them: ms[k] is the time from span[k][0] to span[k][1] (a null span: 0 ms),
// the last slot the host's wall time.  The spans are consecutive events unless the pass sets others; the last span ends
// at the pass's last event.  Between finish() and read() the times are pending: begin() takes them before a new run
// records the events again, so a refused call leaves the times of the last run that completed.
template <int kEvents, int kTimes>
struct svo_pass_timer {
    svo_events<kEvents> ev;
    hipEvent_t span[kTimes - 1][2] = {};
    bool timed = true;
    float ms[kTimes] = {};

    hipError_t create() {
        const hipError_t err = ev.create();
        for (int k = 0; k < kTimes - 1 && k + 1 < kEvents; k++) span[k][0] = ev[k], span[k][1] = ev[k + 1];
        return err;
    }
    int begin(svo_ctx *ctx) {
        float unused[kTimes];
        return timed ? SVO_OK : read(ctx, unused);
    }
    hipError_t mark(svo_ctx *ctx, int k) { return hipEventRecord(ev[k], ctx->stream); }
    void finish(double t0) {
        ms[kTimes - 1] = float(svo_now_ms() - t0);
        timed = false;  // (the pass is still in flight: read() waits for the events)
    }
    void none() {  // a run that had nothing to do
        memset(ms, 0, sizeof ms);
        timed = true;
    }
    int read(svo_ctx *ctx, float *ms_out) {
        if (!timed) {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipEventSynchronize(span[kTimes - 2][1]));
            for (int k = 0; k < kTimes - 1; k++) {
                ms[k] = 0.0f;
                if (span[k][0]) HIP_TRY(ctx, hipEventElapsedTime(&ms[k], span[k][0], span[k][1]));
            }
            timed = true;
        }
        memcpy(ms_out, ms, sizeof ms);
        return SVO_OK;
    }
};

// A pass's state comes to the context only when all of it exists: S::create(ctx) makes the events and the fixed
// allocations, and a failure half way frees what there is and leaves the slot null.
template <typename S>
int svo_workspace_ensure(svo_ctx *ctx, svo_workspace<S> &slot) {
    if (slot) return SVO_OK;
    svo_workspace<S> fresh = svo_workspace_new<S>();
    if (int rc = fresh->create(ctx)) return rc;
    slot = std::move(fresh);
    return SVO_OK;
}

// The argument checks that the passes over the node buffer share, with one message each.
inline int svo_check_store(svo_ctx *ctx) {
    if (!ctx->store) return svo_fail(ctx, SVO_ERR_STATE, "svo_nodes_alloc / svo_nodes_bind_device not called");
    return SVO_OK;
}
inline int svo_check_n_words(svo_ctx *ctx, uint64_t n_words) {
    if (n_words < 8 || n_words % 8 || n_words > ctx->capacity)
        return svo_fail(ctx, SVO_ERR_ARG, "n_words must be a positive multiple of 8 within the node buffer's capacity (got " +
                                              std::to_string(n_words) + ", capacity " + std::to_string(ctx->capacity) + ")");
    return SVO_OK;
}
inline int svo_check_depth(svo_ctx *ctx, uint32_t depth, uint32_t max) {
    if (depth < 1 || depth > max)
        return svo_fail(ctx, SVO_ERR_ARG, "depth must be 1.." + std::to_string(max) + " (got " + std::to_string(depth) + ")");
    return SVO_OK;
}
inline int svo_check_flags(svo_ctx *ctx, uint32_t flags, uint32_t known) {
    if (flags & ~known) return svo_fail(ctx, SVO_ERR_ARG, "unknown flag bits " + std::to_string(flags));
    return SVO_OK;
}

// a write to the bound node store: enqueue it behind the store's last write (any context's), then record it, which makes
// every context bound to the store rebuild its top table and schedule
int svo_store_order_after_write(svo_ctx *ctx);
int svo_store_note_write(svo_ctx *ctx);
// svo_comm.cpp
void svo_comm_release(svo_ctx *ctx);
// svo_build.hip
// the builder's stable radix sort of n u32 keys (in -> out, may alias), for other passes on the ctx stream; it uses the
// builder's workspace
int svo_build_sort_u32(svo_ctx *ctx, const uint32_t *in, uint32_t n, uint32_t *out);
// the same sort of n (u64 key, u32 value) pairs by the keys' low `bits` bits, in ceil(bits / 8) passes; the two pointers
// come back pointing at the sorted arrays: the caller's own, or (an odd number of passes) the builder's, which have room
// for n + 1 items and hold until the next call that uses the builder's workspace
int svo_build_sort_u64(svo_ctx *ctx, uint64_t **keys_dev, uint32_t **vals_dev, uint32_t n, uint32_t bits);
// the front end of the builder's list entry points, for other passes over a voxel list (svo_edit.hip): the checks of
// depth (null: no params), n and xyz with the builder's messages, then keys, the stable sort and the leaf pass on the ctx
// stream.  Everything in svo_build_leaves lives in the builder's workspace and holds until the next call that uses it.
struct svo_build_leaves {
    const uint64_t *keys;       // the distinct cells' Morton keys, ascending (svo_morton.h)
    const uint32_t *colours;    // their colours (24 bits): of several voxels in one cell the last in input order
    const uint32_t *index;      // that voxel's input index
    const uint32_t *count;      // device word: how many there are
    const uint32_t *range_err;  // device word: non-zero when a coordinate was outside [0, 2^depth)
    uint32_t *spare32;          // `items` u32 and twice `items` u64 that the front end no longer needs
    uint64_t *spare64[2];
    size_t items;               // >= n
    hipEvent_t ev_start, ev_keys, ev_sort;  // recorded before the keys kernel, after it, after the sort
};
int svo_build_check_list(svo_ctx *ctx, const uint32_t *depth, const uint32_t *xyz, size_t n);
int svo_build_list_leaves(svo_ctx *ctx, const uint32_t *xyz, const uint32_t *colours, size_t n, uint32_t depth,
                          uint32_t default_colour, svo_build_leaves *out);
// svo_compact.hip
// The discovery of the tree in the first n_words words of the node buffer, for the
// compaction, the simplification (svo_simplify.hip) and the voxel listing (svo_list.hip), on the ctx stream, into its
// workspace: svo_tree_walk owns the four arrays of a u32 per group (grown together by grow(); scan is the scratch of the
// discovery's scans and free afterwards) and the status words that create() allocates and the caller zeroes on the
// stream; the first SVO_WALK_STATUS of them are the discovery's, and all of them come back once per level.  Afterwards order[level_off[l], level_off[l + 1]) holds the old
// group starts of level l + 1 in the order of their parents, first_child[k] the index in order of group k's first
// interior child, level_off has one entry per level and the total, and n_words and cap say what was walked: the words
// clamped to 2^27 (no pointer reaches further) and the groups they hold.  `discovered` (or null) is recorded before the
// check; the check's verdict is status[SVO_WALK_DUP] at the caller's next read-back.  Malformed trees are refused here
// with the compaction's messages (SVO_ERR_STATE).
enum { SVO_WALK_ALIGN, SVO_WALK_RANGE, SVO_WALK_NEXT, SVO_WALK_DUP, SVO_WALK_STATUS };
struct svo_tree_walk {
    svo_dev<uint32_t> order, first_child, new_of, scan;
    svo_mirrored<> status;
    std::vector<uint32_t> level_off;
    uint32_t n_words = 0, cap = 0;  // of the last discovery
    int create(svo_ctx *ctx, size_t status_words) { return status.alloc(ctx, status_words); }
    int grow(svo_ctx *ctx, size_t groups) { return svo_grow(ctx, groups, &order, &first_child, &new_of, &scan); }
};
int svo_tree_discover(svo_ctx *ctx, uint64_t n_words, svo_tree_walk *w, hipEvent_t discovered);
// A tree rewritten into the canonical breadth-first layout, the workspace and the host
// frame of the compaction and the simplification, each with an instance of its own: the walk, whose scan array is
// `number`, a fate per group, the image of an in-place call, the six events and the status (the walk's words and the
// kept groups' total).  The caller checks its arguments, then
//   begin()   the workspace for n_words words (the image only in place), behind the store's last write: the start event,
//             the status reset, the discovery and the check, the check's event
//   middle    the caller's own launches give every group k of order[0, total) number[k] = 1 when it stays and 0 when it
//             goes, and fate[k] = SVO_FATE_KEEP or the 28-bit field that its parent's word becomes (a child of one of
//             them behind `total` has a fate too), then mark SVO_REWRITE_MIDDLE
//   finish()  the scan of number, the read-back and the refusals (a group reached twice; out of place, more words than
//             out_cap), all before the first write; the emit into the image or out_dev; in place the copy back, the fill
//             of the freed tail [n_out, n_words_in) with the empty word and the note of the write; *n_words_out, the times
enum { SVO_REWRITE_START, SVO_REWRITE_DISCOVER, SVO_REWRITE_CHECK, SVO_REWRITE_MIDDLE, SVO_REWRITE_EMIT, SVO_REWRITE_END, SVO_REWRITE_EVENTS };
constexpr uint32_t SVO_FATE_KEEP = 0xFFFFFFFFu;  // (a field has 28 bits)
struct svo_tree_rewrite {
    svo_tree_walk walk;
    svo_dev<uint32_t> image, fate;
    svo_pass_timer<SVO_REWRITE_EVENTS, SVO_COMPACT_TIMES> timer;  // discover, check, the middle, emit, copy back, host wall
    double t0 = 0.0;
    uint32_t *number() const { return walk.scan; }
    int create(svo_ctx *ctx);
    int begin(svo_ctx *ctx, uint64_t n_words, bool in_place);
    int finish(svo_ctx *ctx, uint32_t total, uint32_t *out_dev, uint64_t out_cap, uint32_t *perm_out_dev, uint64_t n_words_in,
               uint64_t *n_words_out);
};
static_assert(SVO_SIMPLIFY_TIMES == SVO_COMPACT_TIMES, "the two rewrites share their timer");
// svo_list.hip
// The plan of a listing, for svo_nodes_list_voxels, the surface pass (svo_surface.hip) and the component
// labelling (svo_components.hip), each with a plan of its own: the discovery's workspace (walk), then per group k of order its entry and record counts (cnt, rcnt), the
// place of its first entry and record in the list (start, rstart) and its Morton prefix (key: a leading 1, then 3 bits
// per level above the group's words).  create() makes the status words, grow() room for `groups` groups.  svo_list_plan_count, on
// the ctx stream: the discovery (`discovered`, or null, is recorded behind it), the counts bottom-up and their read-back;
// it refuses, with the listing's messages and in its order, a malformed tree, a voxel or an interior word deeper than
// `depth`, and 2^31 entries or more; then walk.level_off (level l: order[level_off[l - 1], level_off[l])), listed =
// min(levels, depth), count and n_rec hold.  svo_list_plan_offsets enqueues the top-down pass: start, rstart and key of the
// groups of the levels 1..listed.
struct svo_list_plan {
    svo_tree_walk walk;
    svo_dev<uint32_t> rcnt, start, rstart;
    svo_dev<uint64_t> cnt, key;
    uint32_t listed = 0, n_rec = 0;
    uint64_t count = 0;
    int create(svo_ctx *ctx);
    int grow(svo_ctx *ctx, size_t groups);
};
int svo_list_plan_count(svo_ctx *ctx, svo_list_plan *plan, uint64_t n_words, uint32_t depth, bool expand, hipEvent_t discovered);
int svo_list_plan_offsets(svo_ctx *ctx, svo_list_plan *plan, uint32_t depth, bool expand);
// svo_surface.hip
// The exposed faces of the tree as svo_nodes_list_surface with SVO_SURFACE_QUADS lists them, for the merge
// (svo_surface_merge.hip): the plan, the mask and the compaction run on the ctx stream in the surface workspace `slot`, the
// caller's own (made here when it is null), and the quads stay in it: n entries of xyz (3 u32 each), value, level and
// face, which hold until the next call with that slot.  The caller has checked depth, the store and n_words; the
// refusals are the surface call's, from the malformed tree on, and it blocks where that call blocks.
struct svo_surface_quads {
    const uint32_t *xyz, *value, *level, *face;
    uint32_t n;
};
int svo_surface_list_quads(svo_ctx *ctx, svo_workspace<svo_surface_state> &slot, uint32_t closed_boundary, uint32_t depth,
                           uint64_t n_words, svo_surface_quads *out);
// The one writer of a generated world's directory (svo_build.hip), for svo_world_build and
// svo_world_generate: create() makes the directory and the empty root; add_chunk() writes <id>.bin (id = SVO_CHUNK_OFFSET
// / 2 + i) from `bytes` in the <id>.bin layout, keeps the chunk in w as a node-less CpuOctree carrying its top_mip (the
// mip of its root group) and references it from the root at i -> (x, y, z) * 2 / 2^world_depth - 1; finish() hands the
// root to w as chunk 0, mips it on the host and saves 0.bin (*mip_ms, *save_ms: the host times of the two).  The root is
// the writer's until finish(), so any early return frees it.  Failures are the context's (svo_fail).
struct svo_world_writer {
    svo_world_writer(svo_ctx *ctx, svo_world *w, uint32_t world_depth);
    ~svo_world_writer();
    int refuse_existing();  // SVO_ERR_ARG: the world has no path, or the path exists ("File already exists")
    int create();           // refuse_existing(), then the directory
    int add_chunk(uint32_t i, const void *bytes, uint64_t n_nodes);
    int finish(float *mip_ms, float *save_ms);

   private:
    svo_ctx *ctx;
    svo_world *w;
    uint32_t world_depth;
    std::string path;
    svo_cpu_octree *root = nullptr;
};
// svo_host.cpp (what the writer and the two chunk producers need of the host model beyond include/svo_host.h)
std::string svo_world_path(const svo_world *w);
void svo_cpu_octree_set_top_mip(svo_cpu_octree *t, const uint8_t rgb[3]);
void svo_cpu_octree_top_mip(const svo_cpu_octree *t, uint8_t rgb[3]);
// <w's path>/<id>.bin from `len` bytes in the <id>.bin layout; the chunk stays in w without nodes, as its top_mip alone
// (world.rs:122).  0 or -1 (svo_world_last_error says why)
int svo_world_write_chunk(svo_world *w, uint32_t id, const void *bytes, size_t len, const uint8_t top_mip[3]);
// svo_host.cpp (internal helpers of the device adaptive state): the octree's words, positions (3 floats per node) and hole
// stack (bottom first) as they are; svo_octree_assign replaces all three and clears the dirty set
size_t svo_octree_state(const svo_octree *o, const uint32_t **nodes, const float **positions, std::vector<uint32_t> &holes);
void svo_octree_assign(svo_octree *o, const uint32_t *nodes, const float *positions, size_t n, const uint32_t *holes, size_t n_holes);
