// svo_surface_merge.hip -- the visible surface of the tree in the node buffer merged into rectangles on the device
// (DESIGN.md 28): the exposed faces of svo_surface.hip's quads, as rectangles on the `depth` grid, joined along u and then
// along v wherever two of them of one plane, one extent across and one value touch; include/svo_hip.h states the rule on
// sets.  A phase joins along one direction d (0: u, 1: v; o = 1 - d is the other):
//
//   quads     svo_surface_list_quads (svo_ctx.h): svo_surface.hip's plan, mask and compaction in a surface workspace of this
//             pass's own, the quads left there
//   keys      merge_keys_kernel, one lane per rectangle: the low sort key (extent across, lo[d]) and the rectangle's index;
//             in the first phase the lane reads a quad and writes the rectangle's record too
//   sort      the order (face, plane, lo[o], extent across, lo[d]) has 4 * depth + 5 bits, 89 at depth 21, so it takes two
//             calls of the builder's stable radix sort (svo_build_sort_u64) with the index as the value: by the low key,
//             then, behind merge_gather_kernel, which computes the high key (face, plane, lo[o]) of the rectangle that now
//             stands at each place, by the high key.  The value is no part of the key: the rectangles of a plane are
//             disjoint, so at most one of them ends where another begins
//   flag      merge_flag_kernel, one lane per place of the order: the rectangle moves to its place, and it is a head unless
//             it has the class (face, plane, lo[o], hi[o]) of the one before it, begins where that ends and has its value
//             (or any, with SVO_SURFACE_MERGE_ANY_VALUE)
//   scan      svo_scan.h's tile_count_kernel and tile_offsets_kernel over the head bytes; the total comes back, since
//             the next phase's sort wants it
//   emit      tile_emit_kernel: a head writes its record at its rank; the last rectangle of a run, the one before a head
//             or the end, writes its hi[d] at the same rank, which its own tile's scan gives it: a run may cross tiles
//
// A record keeps the edges (lo, hi) and not the extents, so the two writers of a run need nothing of each other.  The last
// phase leaves the rectangles in the output's order; merge_out_kernel writes them as face, plane, u0, v0, w, h.  No
// atomics, no float, no LDS beside the scan's: the same bytes on every run and for every layout of the tree.  Every
// refusal comes before merge_out_kernel, the only kernel that writes to the outputs.
#include <hip/hip_runtime.h>

#include <string>

#include "svo_ctx.h"
#include "svo_group.h"  // (kThreads)
#include "svo_scan.h"   // (the tile pass, FlagBytes)

namespace {

constexpr uint32_t kMaxRounds = 4, kMaxPhases = 2 * kMaxRounds;
enum Status { kStTotal, kStWords };
// the events: the start, the quads, four per phase, the end
enum Ev { kEvStart, kEvQuads, kEvPhases, kEvEnd = kEvPhases + 4 * kMaxPhases, kEvs };
enum PhaseEv { kPhKeys, kPhSort, kPhScan, kPhEmit };
static_assert(kEvs == SVO_SURFACE_MERGE_TIMES, "one time per event behind the first, and the host's");

// A rectangle of a plane: a = (face << 22 | plane, lo[0], lo[1], value), b = (hi[0], hi[1]); [0] is u, [1] is v.
struct Rects {
    uint4 *a;
    uint2 *b;
};

__device__ inline uint32_t pick(uint32_t d, uint32_t x0, uint32_t x1) { return d ? x1 : x0; }

// the keys of the order of phase d: low (extent across, lo[d]) in 2 * depth + 1 bits, high (face, plane, lo[o]) in
// 2 * depth + 4
__device__ inline uint64_t low_key(const uint4 &a, const uint2 &b, uint32_t d, uint32_t depth) {
    const uint32_t across = pick(d, b.y - a.z, b.x - a.y);
    return uint64_t(across) << depth | pick(d, a.y, a.z);
}
__device__ inline uint64_t high_key(const uint4 &a, uint32_t d, uint32_t depth) {
    const uint64_t face = a.x >> 22, plane = a.x & 0x3FFFFFu;
    return (face << (depth + 1u) | plane) << depth | pick(d, a.z, a.y);
}

// Rectangle i < n: key[i] and index[i] for phase d.  kQuads: the rectangle is quad i of the surface pass, and rects[i]
// gets its record (value 0 with any_value).
template <bool kQuads>
__global__ __launch_bounds__(kThreads) void merge_keys_kernel(const uint32_t *__restrict__ xyz, const uint32_t *__restrict__ value,
                                                              const uint32_t *__restrict__ level, const uint32_t *__restrict__ face,
                                                              Rects rects, uint32_t n, uint32_t d, uint32_t depth, uint32_t any_value,
                                                              uint64_t *__restrict__ key, uint32_t *__restrict__ index) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint4 a;
    uint2 b;
    if (kQuads) {
        const uint32_t x = xyz[3ull * i], y = xyz[3ull * i + 1], z = xyz[3ull * i + 2], f = face[i], s = 1u << (depth - level[i]);
        const uint32_t axis = f >> 1;  // u is the axis behind it, v the one behind that, as in mesh.py's quads_to_mesh
        const uint32_t plane = (axis == 0 ? x : axis == 1 ? y : z) + (f & 1u) * s;
        const uint32_t u0 = axis == 0 ? y : axis == 1 ? z : x, v0 = axis == 0 ? z : axis == 1 ? x : y;
        a = uint4{f << 22 | plane, u0, v0, any_value ? 0u : value[i]};
        b = uint2{u0 + s, v0 + s};
        rects.a[i] = a;
        rects.b[i] = b;
    } else {
        a = rects.a[i];
        b = rects.b[i];
    }
    key[i] = low_key(a, b, d, depth);
    index[i] = i;
}

// Behind the sort by the low key: place i holds rectangle index_in[i]; its high key and the index again.
__global__ __launch_bounds__(kThreads) void merge_gather_kernel(const uint4 *__restrict__ rect_a, const uint32_t *__restrict__ index_in,
                                                                uint32_t n, uint32_t d, uint32_t depth, uint64_t *__restrict__ key,
                                                                uint32_t *__restrict__ index) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = index_in[i];
    key[i] = high_key(rect_a[r], d, depth);
    index[i] = r;
}

// Place i of the phase's order: the rectangle order[i] moves there, and head[i] says whether a run begins with it.
__global__ __launch_bounds__(kThreads) void merge_flag_kernel(Rects in, const uint32_t *__restrict__ order, uint32_t n, uint32_t d,
                                                              uint32_t any_value, Rects sorted, uint8_t *__restrict__ head) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = order[i];
    const uint4 a = in.a[r];
    const uint2 b = in.b[r];
    sorted.a[i] = a;
    sorted.b[i] = b;
    bool follows = false;
    if (i) {
        const uint32_t q = order[i - 1];
        const uint4 pa = in.a[q];
        const uint2 pb = in.b[q];
        const bool same_class = pa.x == a.x && pick(d, pa.z, pa.y) == pick(d, a.z, a.y) && pick(d, pb.y, pb.x) == pick(d, b.y, b.x);
        follows = same_class && pick(d, pb.x, pb.y) == pick(d, a.y, a.z) && (any_value || pa.w == a.w);
    }
    head[i] = follows ? 0u : 1u;
}

// The tile pass's items: the head bytes, 16 per thread (FlagBytes); ends(i) says whether item i of the m is the last of its run.
struct Runs : FlagBytes {
    uint32_t m;
    __device__ bool ends(uint32_t i) const { return i + 1u >= m || mask[i + 1u] != 0u; }
};

// Its emit: the run of rank r is out[r]; its head writes the record, its last rectangle hi[d].
struct RunsOut {
    Rects in, out;
    uint32_t d, n;  // n: the runs
    __device__ void operator()(const Runs &items, uint32_t i0, const uint4 &s, uint32_t rank) const {
        const uint32_t v[4] = {s.x, s.y, s.z, s.w};
        uint32_t *far = reinterpret_cast<uint32_t *>(out.b);
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) {
            const uint32_t i = i0 + j;
            if (i >= items.m) break;
            const bool is_head = (v[j >> 2] >> 8u * (j & 3u)) & 1u;
            rank += is_head ? 1u : 0u;
            const uint32_t at = rank - 1u;  // (item 0 is a head: no run has rank - 1 before it)
            if (at >= n) continue;          // (never: n is the scan's total)
            if (is_head) {
                out.a[at] = in.a[i];
                far[2ull * at + (1u - d)] = pick(d, in.b[i].y, in.b[i].x);
            }
            if (items.ends(i)) far[2ull * at + d] = pick(d, in.b[i].x, in.b[i].y);
        }
    }
};

// Rectangle i < n into the outputs: face, plane, u0, v0, w, h and the value.
__global__ __launch_bounds__(kThreads) void merge_out_kernel(Rects rects, uint32_t n, uint32_t *__restrict__ rect_out,
                                                             uint32_t *__restrict__ value_out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint4 a = rects.a[i];
    const uint2 b = rects.b[i];
    uint32_t *o = rect_out + 6ull * i;
    o[0] = a.x >> 22;
    o[1] = a.x & 0x3FFFFFu;
    o[2] = a.y;
    o[3] = a.z;
    o[4] = b.x - a.y;
    o[5] = b.y - a.z;
    value_out[i] = a.w;
}

}  // namespace

// Per-context workspace of the merge (svo_ctx::surface_merge): a surface workspace of its own with the quads, then per
// quad two records of 24 bytes (the phase's input and output; the sorted copy), two keys, two indices and a head byte.
struct svo_surface_merge_state {
    svo_workspace<svo_surface_state> quads{nullptr, nullptr};
    svo_dev<uint4> rect_a[2];
    svo_dev<uint2> rect_b[2];
    svo_dev<uint64_t> key[2];
    svo_dev<uint32_t> index[2];
    svo_dev<uint8_t> head;
    svo_dev<uint32_t> tile_sum;
    svo_mirrored<> status;  // kStWords words
    svo_pass_timer<kEvs, SVO_SURFACE_MERGE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return status.alloc(ctx, kStWords);
    }
    Rects rects(int k) const { return Rects{rect_a[k], rect_b[k]}; }
};

extern "C" {

int svo_nodes_merge_surface(svo_ctx *ctx, const svo_surface_merge_params *p, uint32_t *rect_out_dev, uint32_t *value_out_dev,
                            uint64_t *n_out) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (!n_out) return svo_fail(ctx, SVO_ERR_ARG, "null n_out");
    if ((p->flags & ~(SVO_SURFACE_CLOSED_BOUNDARY | SVO_SURFACE_MERGE_ANY_VALUE)) || p->rounds < 1 || p->rounds > kMaxRounds)
        return svo_fail(ctx, SVO_ERR_ARG, "unknown or incompatible flag bits " + std::to_string(p->flags) + " or rounds outside 1..4 (got " +
                                              std::to_string(p->rounds) + ")");
    int rc = svo_check_depth(ctx, p->depth, 21);
    if (rc) return rc;
    if (rect_out_dev && !value_out_dev) return svo_fail(ctx, SVO_ERR_ARG, "null value_out_dev with rect_out_dev given");
    if ((rc = svo_check_store(ctx)) || (rc = svo_check_n_words(ctx, p->n_words))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double t0 = svo_now_ms();
    const uint32_t depth = p->depth, any_value = p->flags & SVO_SURFACE_MERGE_ANY_VALUE ? 1u : 0u;
    if ((rc = svo_workspace_ensure(ctx, ctx->surface_merge))) return rc;
    svo_surface_merge_state *s = ctx->surface_merge.get();
    if ((rc = s->timer.begin(ctx))) return rc;

    HIP_TRY(ctx, s->timer.mark(ctx, kEvStart));
    svo_surface_quads quads{};
    if ((rc = svo_surface_list_quads(ctx, s->quads, p->flags & SVO_SURFACE_CLOSED_BOUNDARY, depth, p->n_words, &quads))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, kEvQuads));

    uint32_t n = quads.n, phases = 0;  // the rectangles: rects(0)[0, n)
    if (n) {
        const uint32_t room = svo_div_up(n, kTile) * kTile;  // (below 2^31 + kTile: the surface pass refused 2^31 quads)
        if ((rc = svo_grow(ctx, (size_t)n, &s->rect_a[0], &s->rect_a[1])) || (rc = svo_grow(ctx, (size_t)n, &s->rect_b[0], &s->rect_b[1])) ||
            (rc = svo_grow(ctx, (size_t)n, &s->key[0], &s->key[1])) || (rc = svo_grow(ctx, (size_t)n, &s->index[0], &s->index[1])) ||
            (rc = svo_grow(ctx, (size_t)room, &s->head)) || (rc = svo_grow(ctx, (size_t)room / kTile, &s->tile_sum)))
            return rc;
    }
    const Rects rects = s->rects(0), sorted = s->rects(1);
    for (uint32_t round = 0; round < p->rounds && n; round++) {
        const uint32_t before = n;
        for (uint32_t d = 0; d < 2; d++, phases++) {
            const int ev = kEvPhases + 4 * phases;
            const uint32_t blocks = svo_div_up(n, kThreads), n_tiles = svo_div_up(n, kTile);
            if (phases == 0)
                merge_keys_kernel<true><<<blocks, kThreads, 0, ctx->stream>>>(quads.xyz, quads.value, quads.level, quads.face, rects, n, d, depth,
                                                                              any_value, s->key[0], s->index[0]);
            else
                merge_keys_kernel<false><<<blocks, kThreads, 0, ctx->stream>>>(nullptr, nullptr, nullptr, nullptr, rects, n, d, depth, any_value,
                                                                               s->key[0], s->index[0]);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, s->timer.mark(ctx, ev + kPhKeys));

            // by the low key, then by the high key: each result is in this workspace or in the builder's
            uint64_t *key = s->key[0];
            uint32_t *index = s->index[0];
            if ((rc = svo_build_sort_u64(ctx, &key, &index, n, 2 * depth + 1))) return rc;
            merge_gather_kernel<<<blocks, kThreads, 0, ctx->stream>>>(rects.a, index, n, d, depth, s->key[1], s->index[1]);
            HIP_TRY(ctx, hipGetLastError());
            key = s->key[1];
            index = s->index[1];
            if ((rc = svo_build_sort_u64(ctx, &key, &index, n, 2 * depth + 4))) return rc;
            HIP_TRY(ctx, s->timer.mark(ctx, ev + kPhSort));

            merge_flag_kernel<<<blocks, kThreads, 0, ctx->stream>>>(rects, index, n, d, any_value, sorted, s->head);
            HIP_TRY(ctx, hipGetLastError());
            const Runs runs{{s->head}, n};
            if ((rc = svo_tile_count(ctx, runs, n_tiles, nullptr, n, s->tile_sum, s->status.dev + kStTotal))) return rc;
            if ((rc = s->status.read(ctx))) return rc;
            const uint32_t total = s->status.host()[kStTotal];  // (at most n)
            HIP_TRY(ctx, s->timer.mark(ctx, ev + kPhScan));

            tile_emit_kernel<<<n_tiles, kThreads, 0, ctx->stream>>>(runs, RunsOut{sorted, rects, d, total}, nullptr, n, s->tile_sum);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, s->timer.mark(ctx, ev + kPhEmit));
            n = total;
        }
        if (n == before) break;  // (a round that joined nothing: none after it joins anything, and the order is the output's)
    }
    if (rect_out_dev && n > p->max_entries)
        return svo_fail(ctx, SVO_ERR_CAP, "the list has " + std::to_string(n) + " entries, more than max_entries = " +
                                              std::to_string(p->max_entries));
    if (rect_out_dev && n) {
        merge_out_kernel<<<svo_div_up(n, kThreads), kThreads, 0, ctx->stream>>>(rects, n, rect_out_dev, value_out_dev);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, s->timer.mark(ctx, kEvEnd));
    // the times of the phases that ran; the last one is the output's, from the last event before it
    for (uint32_t k = 0; k < 4 * kMaxPhases; k++) {
        const bool ran = k < 4 * phases;
        s->timer.span[1 + k][0] = ran ? s->timer.ev[kEvQuads + k] : nullptr;
        s->timer.span[1 + k][1] = ran ? s->timer.ev[kEvQuads + k + 1] : nullptr;
    }
    s->timer.span[1 + 4 * kMaxPhases][0] = s->timer.ev[kEvQuads + 4 * phases];
    s->timer.span[1 + 4 * kMaxPhases][1] = s->timer.ev[kEvEnd];
    *n_out = n;
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_surface_merge_timing(svo_ctx *ctx, float ms_out[SVO_SURFACE_MERGE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->surface_merge) return svo_fail(ctx, SVO_ERR_STATE, "no surface merged on this context yet");
    return ctx->surface_merge->timer.read(ctx, ms_out);
}

}  // extern "C"
