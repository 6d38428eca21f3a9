// svo_distance.hip -- the exact squared Euclidean distance transform of the tree in the node buffer: for
// every cell of a box of the `depth` grid the nearest site within R cells and its squared distance, by the rule of
// include/svo_hip.h.  The call only reads the words, enqueues its kernels and returns.  No atomics: every output entry
// is one lane's, so the bytes depend on the tree alone.
//
//   bits   the occupancy of the box grown by R on every side, one u64 per aligned run of 64 cells along z.  Such a run
//          is one node of level depth - 6: a wave walks the levels above it once, with wave-uniform addresses (scalar
//          loads), and a walk that ends on a leaf, an empty word or a broken pointer settles the 64 cells at once.
//          Otherwise lane = z finishes its own last six levels, and one ballot of value != 0 is the word.  The only time
//          the tree is touched.  To-empty mode stores the complement, which sets the cells outside the grid.
//   zy     the z and the y pass in one kernel, for a slab of rows of the box and every plane of the grown box: lane = z,
//          a wave per run.  For each row y + dy, |dy| ascending, the five words round the wave's run are wave-uniform
//          (scalar loads); a lane takes the nearest set bit below and above its own from them with shifts and count
//          leading / trailing zeros, ties to the lower z, and keeps the minimum of (dy^2 + dz^2, dy, dz) as one u32.  The
//          loop ends when (|dy| + 1)^2 exceeds every lane's best.  Signed mode runs the kernel twice, the second time over
//          the complemented words into a second array: fused into one loop the cheap side rode along for the dear side's
//          whole window.  The z pass has no array of its own: the bits are 1/32 of its size and
//          stay in the scalar cache, and a slab then needs no halo of rows, which bounds the workspace (svo_hip.h).
//   x      lane = z again, so every load of the zy output and both stores are coalesced without a transpose: the minimum
//          over the planes x + dx, |dx| ascending, of (g + dx^2, dx, dy, dz) as one u64, ending when dx^2 exceeds the best
//          so far; then the R^2 test, the mode's sign and the two outputs.
#include <hip/hip_runtime.h>

#include <string>

#include "svo_ctx.h"
#include "svo_group.h"        // (kThreads)
#include "svo_sample_walk.h"  // (sample_walk)

namespace {

constexpr uint64_t kMaxCells = 1ull << 31;
constexpr uint32_t kNone = 0xFFFFFFFFu;  // in the zy output: no site of this plane within R
constexpr uint32_t kWaves = kThreads / 64u;
static_assert(kThreads % 64 == 0, "whole waves per workgroup");
static_assert(2u * SVO_DISTANCE_MAX_RADIUS * SVO_DISTANCE_MAX_RADIUS < 1u << 16, "dy^2 + dz^2 fits the zy key's 16 bits");

// The geometry of a call, the same in every kernel.  Bit b of word q of the row (i, j) is the cell (x0 + i, y0 + j,
// z0 + 64 q + b); z0 is a multiple of 64 and may, like x0 and y0, be negative.
struct Frame {
    int32_t x0, y0, z0;   // the grown box's first cell; on z the first cell of the first word
    uint32_t o[3], s[3];  // the box
    uint32_t gx, gy, nw;  // planes and rows of the grown box, words per row
    uint32_t q0, nq;      // the words that hold a cell of the box: [q0, q0 + nq)
    uint32_t R, depth;
};

// the wave's number, the same in every lane and said so to the compiler
__device__ inline uint64_t wave_index() {
    return uint64_t(blockIdx.x) * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

__global__ __launch_bounds__(kThreads) void distance_bits_kernel(const uint32_t *__restrict__ words, uint64_t n_words, Frame f,
                                                                 uint64_t flip, uint64_t n_waves, uint64_t *__restrict__ bits) {
    const uint64_t w = wave_index();
    if (w >= n_waves) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = uint32_t(w % f.nw);
    const uint64_t ij = w / f.nw;
    const int32_t side = 1 << f.depth;
    const int32_t x = f.x0 + int32_t(ij / f.gy), y = f.y0 + int32_t(ij % f.gy), zb = f.z0 + int32_t(q * 64u), z = zb + int32_t(lane);
    const uint32_t top = f.depth > 6 ? f.depth - 6 : 0;  // the levels above the run
    bool occupied = false;
    // (with depth >= 6 the run lies inside the grid or outside it as a whole; below, the lanes differ)
    if (x >= 0 && x < side && y >= 0 && y < side && zb + 63 >= 0 && zb < side) {
        uint32_t group = 0;
        bool settled = false;
        for (uint32_t level = 1; level <= top; level++) {
            const uint32_t i = __builtin_amdgcn_readfirstlane(group + morton_child(uint32_t(x), uint32_t(y), uint32_t(zb), f.depth - level));
            const uint32_t pointer = words[i] >> 4;
            if (pointer >= SVO_VOXEL_OFFSET || (pointer & 7u) || uint64_t(pointer) + 8u > n_words) {
                occupied = pointer != SVO_VOXEL_OFFSET;  // a colour or SVO_SAMPLE_BROKEN; the empty word is value 0
                settled = true;
                break;
            }
            group = pointer;
        }
        if (!settled && z >= 0 && z < side)
            occupied = sample_walk(words, n_words, uint32_t(x), uint32_t(y), uint32_t(z), f.depth, top + 1, group).value != 0;
    }
    const uint64_t word = __ballot(occupied) ^ flip;
    if (lane == 0) bits[w] = word;
}

// The nearest set bit to bit r of word c in the row ... m2 m1 c p1 p2 ... (ascending z), ties to the lower z: its
// distance (255 or more: none in these five words) and whether it lies below.
struct Nearest {
    uint32_t dist;
    bool below;
};
__device__ inline Nearest nearest_bit(uint64_t m2, uint64_t m1, uint64_t c, uint64_t p1, uint64_t p2, uint32_t r) {
    const uint32_t t = 63u - r;
    // bits r, r + 1, ... from bit 0 up, and bits r, r - 1, ... from bit 63 down, 128 of them each
    const uint64_t up0 = r ? (c >> r) | (p1 << (64u - r)) : c, up1 = r ? (p1 >> r) | (p2 << (64u - r)) : p1;
    const uint64_t dn1 = t ? (c << t) | (m1 >> (64u - t)) : c, dn0 = t ? (m1 << t) | (m2 >> (64u - t)) : m1;
    const uint32_t up = up0 ? uint32_t(__builtin_ctzll(up0)) : up1 ? 64u + uint32_t(__builtin_ctzll(up1)) : 255u;
    const uint32_t dn = dn1 ? uint32_t(__builtin_clzll(dn1)) : dn0 ? 64u + uint32_t(__builtin_clzll(dn0)) : 255u;
    return {dn <= up ? dn : up, dn <= up};
}

// (dy^2 + dz^2) << 16 | (dy + 128) << 8 | (dz + 128) of the row's candidate, or kNone when it lies further than R
__device__ inline uint32_t zy_key(Nearest n, int32_t dy, uint32_t R) {
    if (n.dist > R) return kNone;
    const uint32_t g = uint32_t(dy * dy) + n.dist * n.dist;
    if (g > R * R) return kNone;
    return g << 16 | uint32_t(dy + 128) << 8 | (n.below ? 128u - n.dist : 128u + n.dist);
}

// One wave per (plane i of the grown box, row jj of the slab, word of the box); `rows` rows from row j0 of the box.
// out[(i * rows + jj) * s[2] + k] for the cell k of the row.  flip: 0, or all ones for the complement of the stored bits
// (a word outside the row then counts as set, which lies further than R from every cell of the box).
__global__ __launch_bounds__(kThreads) void distance_zy_kernel(const uint64_t *__restrict__ bits, Frame f, uint64_t flip, uint32_t j0,
                                                               uint32_t rows, uint64_t n_waves, uint32_t *__restrict__ out) {
    const uint64_t w = wave_index();
    if (w >= n_waves) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = f.q0 + uint32_t(w % f.nq);
    const uint64_t ij = w / f.nq;
    const uint32_t jj = uint32_t(ij % rows), i = uint32_t(ij / rows);
    const int32_t k = f.z0 + int32_t(q * 64u + lane) - int32_t(f.o[2]);
    const bool valid = k >= 0 && uint32_t(k) < f.s[2];
    const uint32_t jg = j0 + jj + f.R;  // the cell's row in the grown box
    const uint32_t R2 = f.R * f.R;
    uint32_t best = kNone;
    for (uint32_t a = 0; a <= f.R; a++) {
        for (uint32_t up = 0; up < (a ? 2u : 1u); up++) {
            const int32_t dy = up ? int32_t(a) : -int32_t(a);
            const uint64_t *row = bits + (uint64_t(i) * f.gy + uint32_t(int32_t(jg) + dy)) * f.nw;
            const uint64_t m2 = (q >= 2 ? row[q - 2] : 0) ^ flip, m1 = (q >= 1 ? row[q - 1] : 0) ^ flip, c = row[q] ^ flip;
            const uint64_t p1 = (q + 1 < f.nw ? row[q + 1] : 0) ^ flip, p2 = (q + 2 < f.nw ? row[q + 2] : 0) ^ flip;
            if (m2 | m1 | c | p1 | p2) best = min(best, zy_key(nearest_bit(m2, m1, c, p1, p2, lane), dy, f.R));
        }
        // a row further out holds nothing better once (a + 1)^2 exceeds the best so far; at equality a lower y still wins
        const uint32_t next = (a + 1u) * (a + 1u);
        if (!__ballot(valid && next <= min(best >> 16, R2))) break;
    }
    if (!valid) return;
    const size_t at = (size_t(i) * rows + jj) * f.s[2] + uint32_t(k);
    out[at] = best;
}

// One wave per (plane i of the box, row jj of the slab, word of the box).  kSigned: an occupied cell reads in_inv and
// gets the negated distance; its own bit says which.
template <bool kSigned>
__global__ __launch_bounds__(kThreads) void distance_x_kernel(const uint32_t *__restrict__ in, const uint32_t *__restrict__ in_inv,
                                                              const uint64_t *__restrict__ bits, Frame f, uint32_t j0, uint32_t rows,
                                                              uint64_t n_waves, int32_t *__restrict__ d2_out, uint32_t *__restrict__ site_out) {
    const uint64_t w = wave_index();
    if (w >= n_waves) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = f.q0 + uint32_t(w % f.nq);
    const uint64_t ij = w / f.nq;
    const uint32_t jj = uint32_t(ij % rows), i = uint32_t(ij / rows);
    const int32_t k = f.z0 + int32_t(q * 64u + lane) - int32_t(f.o[2]);
    if (k < 0 || uint32_t(k) >= f.s[2]) return;
    bool occupied = false;
    if (kSigned) {
        occupied = (bits[(uint64_t(i + f.R) * f.gy + (j0 + jj + f.R)) * f.nw + q] >> lane) & 1u;
        if (occupied) in = in_inv;
    }
    const size_t plane = size_t(rows) * f.s[2];
    const uint32_t *col = in + size_t(i + f.R) * plane + size_t(jj) * f.s[2] + uint32_t(k);
    const uint32_t R2 = f.R * f.R;
    uint64_t best = ~0ull;
    uint32_t bound = R2;  // min(the best squared distance so far, R^2): at equality a lower x still wins
    for (uint32_t a = 0; a <= f.R && a * a <= bound; a++) {
        for (uint32_t up = 0; up < (a ? 2u : 1u); up++) {
            const int32_t dx = up ? int32_t(a) : -int32_t(a);
            const uint32_t cand = col[ptrdiff_t(dx) * ptrdiff_t(plane)];
            if (cand == kNone) continue;
            const uint32_t d2 = (cand >> 16) + a * a;
            if (d2 > R2) continue;
            best = min(best, uint64_t(d2) << 24 | uint64_t(dx + 128) << 16 | (cand & 0xFFFFu));
            bound = min(bound, d2);
        }
    }
    const bool found = best != ~0ull;
    const int32_t d2 = found ? int32_t(best >> 24) : SVO_DISTANCE_FAR;
    const size_t at = (size_t(i) * f.s[1] + (j0 + jj)) * f.s[2] + uint32_t(k);
    d2_out[at] = occupied ? -d2 : d2;
    if (site_out) site_out[at] = found ? uint32_t(best) & 0xFFFFFFu : SVO_DISTANCE_NO_SITE;
}

enum { EV_START, EV_BITS, EV_ZY, EV_X, EV_END, EV_COUNT };

}  // namespace

// Per-context state of the distance pass (svo_ctx::distance): the workspace of svo_hip.h and the events and times.
struct svo_distance_state {
    svo_dev<uint64_t> bits;
    svo_dev<uint32_t> zy, zy_inv;
    svo_pass_timer<EV_COUNT, SVO_DISTANCE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        timer.span[3][0] = timer.ev[EV_BITS];  // all slabs, the first included
        timer.span[3][1] = timer.ev[EV_END];
        return SVO_OK;
    }
};

extern "C" {

int svo_nodes_distance(svo_ctx *ctx, const svo_distance_params *p, const uint32_t origin[3], const uint32_t size[3],
                       int32_t *d2_out_dev, uint32_t *site_out_dev) {
    if (!ctx) return SVO_ERR_ARG;
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    int rc = svo_check_flags(ctx, p->flags, 0);
    if (rc) return rc;
    if ((rc = svo_check_depth(ctx, p->depth, 21))) return rc;
    if (p->mode > SVO_DISTANCE_SIGNED) return svo_fail(ctx, SVO_ERR_ARG, "mode must be 0..2 (got " + std::to_string(p->mode) + ")");
    if (p->max_distance < 1 || p->max_distance > SVO_DISTANCE_MAX_RADIUS)
        return svo_fail(ctx, SVO_ERR_ARG, "max_distance must be 1.." + std::to_string(SVO_DISTANCE_MAX_RADIUS) + " (got " +
                                              std::to_string(p->max_distance) + ")");
    if (!origin) return svo_fail(ctx, SVO_ERR_ARG, "null origin");
    if (!size) return svo_fail(ctx, SVO_ERR_ARG, "null size");
    if (!d2_out_dev) return svo_fail(ctx, SVO_ERR_ARG, "null d2_out_dev");
    const uint64_t side = 1ull << p->depth;
    uint64_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (uint64_t(origin[a]) + size[a] > side)
            return svo_fail(ctx, SVO_ERR_ARG, "the box leaves the grid on axis " + std::to_string(a) + ": origin " + std::to_string(origin[a]) +
                                                  " + size " + std::to_string(size[a]) + " > 2^depth = " + std::to_string(side));
        cells *= size[a];  // (each at most 2^21: no wrap)
    }
    if (cells >= kMaxCells) return svo_fail(ctx, SVO_ERR_ARG, "the box has " + std::to_string(cells) + " cells, 2^31 or more");

    // the geometry and the workspace it takes (svo_hip.h)
    const uint32_t R = p->max_distance;
    const bool both = p->mode == SVO_DISTANCE_SIGNED;
    Frame f;
    for (int a = 0; a < 3; a++) f.o[a] = origin[a], f.s[a] = size[a];
    f.R = R, f.depth = p->depth;
    f.x0 = int32_t(origin[0]) - int32_t(R), f.y0 = int32_t(origin[1]) - int32_t(R);
    f.z0 = (int32_t(origin[2]) - int32_t(R)) & ~63;  // (the multiple of 64 below, also of a negative number)
    f.gx = size[0] + 2u * R, f.gy = size[1] + 2u * R;
    f.nw = uint32_t((int32_t(origin[2] + size[2] + R) - 1 - f.z0) >> 6) + 1u;
    f.q0 = uint32_t(int32_t(origin[2]) - f.z0) >> 6;
    f.nq = cells ? (uint32_t(int32_t(origin[2] + size[2]) - 1 - f.z0) >> 6) - f.q0 + 1u : 0u;
    const uint64_t row_cells = uint64_t(f.gx) * f.s[2];  // one row of the box in every plane of the grown box
    const uint32_t slab = cells ? uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(f.s[1], SVO_DISTANCE_SLAB_CELLS / row_cells))) : 0u;
    const uint64_t n_bits = uint64_t(f.gx) * f.gy * f.nw, n_zy = row_cells * slab;
    const uint64_t bytes = n_bits * 8u + (both ? 2u : 1u) * n_zy * 4u;
    if (cells && bytes > SVO_DISTANCE_MAX_WORKSPACE)
        return svo_fail(ctx, SVO_ERR_ARG, "the box's workspace of " + std::to_string(bytes) + " bytes exceeds SVO_DISTANCE_MAX_WORKSPACE = " +
                                              std::to_string(SVO_DISTANCE_MAX_WORKSPACE));
    if ((rc = svo_check_store(ctx))) return rc;
    if ((rc = svo_check_n_words(ctx, p->n_words))) return rc;
    if (!cells) return SVO_OK;

    const double t0 = svo_now_ms();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = svo_workspace_ensure(ctx, ctx->distance))) return rc;
    svo_distance_state *s = ctx->distance.get();
    if ((rc = svo_grow(ctx, n_bits, &s->bits))) return rc;
    if ((rc = svo_grow(ctx, n_zy, &s->zy))) return rc;
    if (both && (rc = svo_grow(ctx, n_zy, &s->zy_inv))) return rc;
    if ((rc = svo_store_order_after_write(ctx))) return rc;

    HIP_TRY(ctx, s->timer.mark(ctx, EV_START));
    distance_bits_kernel<<<svo_div_up(n_bits, kWaves), kThreads, 0, ctx->stream>>>(
        ctx->nodes, p->n_words, f, p->mode == SVO_DISTANCE_TO_EMPTY ? ~0ull : 0ull, n_bits, s->bits);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, EV_BITS));
    for (uint32_t j0 = 0; j0 < f.s[1]; j0 += slab) {
        const uint32_t rows = std::min(slab, f.s[1] - j0);
        const uint64_t zy_waves = uint64_t(f.gx) * rows * f.nq, x_waves = uint64_t(f.s[0]) * rows * f.nq;
        distance_zy_kernel<<<svo_div_up(zy_waves, kWaves), kThreads, 0, ctx->stream>>>(s->bits, f, 0ull, j0, rows, zy_waves, s->zy);
        if (both) distance_zy_kernel<<<svo_div_up(zy_waves, kWaves), kThreads, 0, ctx->stream>>>(s->bits, f, ~0ull, j0, rows, zy_waves, s->zy_inv);
        HIP_TRY(ctx, hipGetLastError());
        if (!j0) HIP_TRY(ctx, s->timer.mark(ctx, EV_ZY));
        if (both)
            distance_x_kernel<true><<<svo_div_up(x_waves, kWaves), kThreads, 0, ctx->stream>>>(s->zy, s->zy_inv, s->bits, f, j0, rows, x_waves,
                                                                                             d2_out_dev, site_out_dev);
        else
            distance_x_kernel<false><<<svo_div_up(x_waves, kWaves), kThreads, 0, ctx->stream>>>(s->zy, nullptr, s->bits, f, j0, rows, x_waves,
                                                                                              d2_out_dev, site_out_dev);
        HIP_TRY(ctx, hipGetLastError());
        if (!j0) HIP_TRY(ctx, s->timer.mark(ctx, EV_X));
    }
    HIP_TRY(ctx, s->timer.mark(ctx, EV_END));
    s->timer.finish(t0);
    return SVO_OK;
}

int svo_distance_timing(svo_ctx *ctx, float ms_out[SVO_DISTANCE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->distance) return svo_fail(ctx, SVO_ERR_STATE, "no distance field computed on this context yet");
    return ctx->distance->timer.read(ctx, ms_out);
}

}  // extern "C"
