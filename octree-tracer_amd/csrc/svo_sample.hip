// svo_sample.hip -- the tree in the node buffer sampled on the device: what is at a cell of the `depth`
// grid, for a list of cells (svo_nodes_sample) and for every cell of a box as a dense [x][y][z] array
// (svo_nodes_sample_dense).  Both calls only read the words, enqueue one kernel and return: nothing comes back to the
// host, and what the device finds out is in the marks (SVO_SAMPLE_FINER, _OUTSIDE, _BROKEN).  No atomics: the outputs
// depend on the tree alone, the index output also on where its groups sit.
//
//   points   one lane per cell: the walk from group 0 by the cell's child indices, at most `depth` dependent loads
//   dense    the unit is an aligned 4x4x4 brick of the `depth` grid, which is one node of level depth - 2.  A wave takes
//            kRun bricks that follow each other along z.  For each of them it walks the levels 1 .. depth - 2 once, with
//            wave-uniform addresses (scalar loads); a walk that ends on a leaf, an empty word or a broken pointer settles
//            the whole brick.  Then the lanes take the wave's 4 x 4 x 16 cells in four steps, one x each: z = lane & 15
//            runs fastest, as in the output, so a store instruction writes four pieces of 64 contiguous bytes, and the
//            four lanes of a brick's z row read words of two 32-byte groups per level.  A lane of a brick that was not
//            settled finishes its own last two levels from the brick's group.
//
// The walk is the sampler's own (svo_sample_walk.h, which svo_distance.hip includes too): svo_edit.hip's plan walks the same
// path but answers another question (the first leaf, an address check without the alignment rule, a refusal at an interior
// word), and one function for both would have to branch on its caller.
#include <hip/hip_runtime.h>

#include <string>

#include "svo_ctx.h"
#include "svo_group.h"   // (kThreads, kEmptyWord; not svo_scan.h: this file needs none of its kernels)
#include "svo_morton.h"  // (morton_child)
#include "svo_sample_walk.h"  // (Sample, sample_walk: the rule for one cell, which svo_distance.hip walks too)

namespace {

constexpr uint64_t kMaxCells = 1ull << 31;
constexpr uint32_t kRun = 4;             // bricks along z per wave
constexpr uint32_t kSettled = 0xFFFFFFFFu;  // in Brick::group: every cell of the brick has Brick::value
static_assert(kThreads % 64 == 0, "whole waves per workgroup");
static_assert(kEmptyWord >> 4 == SVO_VOXEL_OFFSET, "an empty word is a leaf of value 0");

__global__ __launch_bounds__(kThreads) void sample_cells_kernel(const uint32_t *__restrict__ words, uint64_t n_words,
                                                                const uint32_t *__restrict__ xyz, uint32_t n, uint32_t depth,
                                                                uint32_t *__restrict__ value, uint32_t *__restrict__ level,
                                                                uint32_t *__restrict__ index) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const uint32_t x = xyz[3ull * k], y = xyz[3ull * k + 1], z = xyz[3ull * k + 2];
    Sample s{SVO_SAMPLE_OUTSIDE, 0u, 0xFFFFFFFFu};
    if (((x | y | z) >> depth) == 0) s = sample_walk(words, n_words, x, y, z, depth, 1, 0);
    value[k] = s.value;
    if (level) level[k] = s.level;
    if (index) index[k] = s.index;
}

struct Brick {
    uint32_t group, value;
};

// The common path of the brick (bx, by, bz) of the level-`top` grid, top = depth - 2: the same in every lane, and said
// so to the compiler, which then loads through the scalar unit.
__device__ inline Brick brick_walk(const uint32_t *__restrict__ words, uint64_t n_words, uint32_t bx, uint32_t by, uint32_t bz,
                                   uint32_t top) {
    uint32_t group = 0;
    for (uint32_t level = 1; level <= top; level++) {
        const uint32_t i = __builtin_amdgcn_readfirstlane(group + morton_child(bx, by, bz, top - level));
        const uint32_t pointer = words[i] >> 4;
        if (pointer >= SVO_VOXEL_OFFSET) return {kSettled, pointer - SVO_VOXEL_OFFSET};
        if ((pointer & 7u) || uint64_t(pointer) + 8u > n_words) return {kSettled, SVO_SAMPLE_BROKEN};
        group = pointer;
    }
    return {group, 0u};
}

struct Box {
    uint32_t o[3], s[3];  // origin and size on the `depth` grid
    uint32_t b0[3];       // the first brick on each axis
    uint32_t ny, nz;      // bricks along y, runs of kRun bricks along z
};

// One wave per run of kRun bricks along z; the runs in z, y, x order, so that waves next to each other write next to
// each other and share their paths.
__global__ __launch_bounds__(kThreads) void sample_dense_kernel(const uint32_t *__restrict__ words, uint64_t n_words, uint32_t depth,
                                                                Box box, uint32_t n_runs, uint32_t *__restrict__ grid) {
    const uint32_t run = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64u) + (threadIdx.x >> 6));
    if (run >= n_runs) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rz = run % box.nz, rxy = run / box.nz;
    const uint32_t bx = box.b0[0] + rxy / box.ny, by = box.b0[1] + rxy % box.ny, bz = box.b0[2] + rz * kRun;
    const uint32_t top = depth > 2 ? depth - 2 : 0;  // the levels of the common path
    const uint32_t z_end = box.o[2] + box.s[2];

    // this lane's brick of the run, its cell but for x, and its brick's walk
    const uint32_t mine = (lane >> 2) & (kRun - 1u);
    const uint32_t y = by * 4u + (lane >> 4), z = bz * 4u + (lane & 15u);
    Brick b{kSettled, 0u};
    for (uint32_t r = 0; r < kRun; r++) {
        if ((bz + r) * 4u >= z_end) break;  // (behind the box, perhaps behind the grid; the same in every lane)
        const Brick w = brick_walk(words, n_words, bx, by, bz + r, top);
        if (r == mine) b = w;
    }
    const bool inside = y >= box.o[1] && y - box.o[1] < box.s[1] && z >= box.o[2] && z < z_end;
    if (!inside) return;
    const size_t row = size_t(y - box.o[1]) * box.s[2] + (z - box.o[2]), plane = size_t(box.s[1]) * box.s[2];
    for (uint32_t step = 0; step < 4; step++) {
        const uint32_t x = bx * 4u + step;
        if (x < box.o[0] || x - box.o[0] >= box.s[0]) continue;
        const uint32_t v = b.group == kSettled ? b.value : sample_walk(words, n_words, x, y, z, depth, top + 1, b.group).value;
        grid[size_t(x - box.o[0]) * plane + row] = v;
    }
}

}  // namespace

// Per-context state of the sampling (svo_ctx::sample): the events around the last kernel and its times.
struct svo_sample_state {
    svo_pass_timer<2, SVO_SAMPLE_TIMES> timer;

    int create(svo_ctx *ctx) {
        HIP_TRY(ctx, timer.create());
        return SVO_OK;
    }
};

namespace {

// The checks both calls share behind their own arguments' (the contract's causes 1 to 3 come before, 5 and 6 after).
int check_params(svo_ctx *ctx, const svo_sample_params *p) {
    if (!p) return svo_fail(ctx, SVO_ERR_ARG, "null params");
    if (int rc = svo_check_flags(ctx, p->flags, 0)) return rc;
    return svo_check_depth(ctx, p->depth, 21);
}

int check_tree(svo_ctx *ctx, const svo_sample_params *p) {
    if (int rc = svo_check_store(ctx)) return rc;
    return svo_check_n_words(ctx, p->n_words);
}

// The kernel behind every earlier write to the store, whichever context issued it, between the two events.
template <typename Launch>
int run_timed(svo_ctx *ctx, double t0, Launch launch) {
    int rc = svo_workspace_ensure(ctx, ctx->sample);
    if (rc) return rc;
    svo_sample_state *s = ctx->sample.get();
    if ((rc = svo_store_order_after_write(ctx))) return rc;
    HIP_TRY(ctx, s->timer.mark(ctx, 0));
    launch();
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, s->timer.mark(ctx, 1));
    s->timer.finish(t0);
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_nodes_sample(svo_ctx *ctx, const svo_sample_params *p, const uint32_t *xyz_dev, size_t n, uint32_t *value_out_dev,
                     uint32_t *level_out_dev, uint32_t *index_out_dev) {
    if (!ctx) return SVO_ERR_ARG;
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (n && !xyz_dev) return svo_fail(ctx, SVO_ERR_ARG, "null xyz_dev");
    if (n && !value_out_dev) return svo_fail(ctx, SVO_ERR_ARG, "null value_out_dev");
    if (n >= kMaxCells) return svo_fail(ctx, SVO_ERR_ARG, "n must be below 2^31 (got " + std::to_string(n) + ")");
    if ((rc = check_tree(ctx, p))) return rc;
    if (!n) return SVO_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return run_timed(ctx, svo_now_ms(), [&] {
        sample_cells_kernel<<<svo_div_up(n, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, p->n_words, xyz_dev, (uint32_t)n, p->depth,
                                                                                   value_out_dev, level_out_dev, index_out_dev);
    });
}

int svo_nodes_sample_dense(svo_ctx *ctx, const svo_sample_params *p, const uint32_t origin[3], const uint32_t size[3],
                           uint32_t *grid_out_dev) {
    if (!ctx) return SVO_ERR_ARG;
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (!origin) return svo_fail(ctx, SVO_ERR_ARG, "null origin");
    if (!size) return svo_fail(ctx, SVO_ERR_ARG, "null size");
    if (!grid_out_dev) return svo_fail(ctx, SVO_ERR_ARG, "null grid_out_dev");
    const uint64_t side = 1ull << p->depth;
    uint64_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (uint64_t(origin[a]) + size[a] > side)
            return svo_fail(ctx, SVO_ERR_ARG, "the box leaves the grid on axis " + std::to_string(a) + ": origin " + std::to_string(origin[a]) +
                                                  " + size " + std::to_string(size[a]) + " > 2^depth = " + std::to_string(side));
        cells *= size[a];  // (each at most 2^21: no wrap)
    }
    if (cells >= kMaxCells) return svo_fail(ctx, SVO_ERR_ARG, "the box has " + std::to_string(cells) + " cells, 2^31 or more");
    if ((rc = check_tree(ctx, p))) return rc;
    if (!cells) return SVO_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Box box;
    uint32_t bricks[3];
    for (int a = 0; a < 3; a++) {
        box.o[a] = origin[a];
        box.s[a] = size[a];
        box.b0[a] = origin[a] >> 2;
        bricks[a] = ((origin[a] + size[a] - 1u) >> 2) - box.b0[a] + 1u;
    }
    box.ny = bricks[1];
    box.nz = svo_div_up(bricks[2], kRun);
    const uint64_t n_runs = uint64_t(bricks[0]) * box.ny * box.nz;  // (every run holds a cell of the box: below 2^31)
    return run_timed(ctx, svo_now_ms(), [&] {
        sample_dense_kernel<<<svo_div_up(n_runs * 64u, kThreads), kThreads, 0, ctx->stream>>>(ctx->nodes, p->n_words, p->depth, box,
                                                                                            (uint32_t)n_runs, grid_out_dev);
    });
}

int svo_sample_timing(svo_ctx *ctx, float ms_out[SVO_SAMPLE_TIMES]) {
    if (!ctx || !ms_out) return SVO_ERR_ARG;
    if (!ctx->sample) return svo_fail(ctx, SVO_ERR_STATE, "no tree sampled on this context yet");
    return ctx->sample->timer.read(ctx, ms_out);
}

}  // extern "C"
