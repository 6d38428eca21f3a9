// svo_render.hpp -- C++ host-side mirror of the reference's dispatch API over the C ABI (include/svo_hip.h,
// include/svo_host.h): the same type and method names, argument meaning and error behaviour as
//   src/gpu.rs      Gpu::new
//   src/render.rs   Render::{new, update, render, resize}, Uniforms
//   src/compute.rs  Compute::{new, update}
//   src/octree.rs   Octree        src/cpu_octree.rs  CpuOctree      src/main.rs  Settings, Character
// Where the reference unwraps/panics (gpu.rs:24,39; adaptive.rs:66,124; octree.rs:73-75) these classes throw
// svo::Error.  Header-only; link against libsvo_hip.so.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "svo_hip.h"
#include "svo_host.h"

namespace svo {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &what) : std::runtime_error(what), status(s) {}
};

struct Voxel {  // octree.rs:7-35
    uint8_t r = 0, g = 0, b = 0;
    uint32_t to_cpu_value() const { return (uint32_t(r) << 16) | (uint32_t(g) << 8) | b; }
    uint32_t to_value() const { return (SVO_VOXEL_OFFSET + to_cpu_value()) << 4; }
};

struct Settings {  // main.rs:116-120, defaults app.rs:23-27
    uint32_t octree_depth = 12;
    float fov = 90.0f;
    float sensitivity = 0.00005f;
};

struct Character {  // main.rs:122-137
    float pos[3] = {0.1f, 0.2f, -1.5f};
    float look[3] = {0.0f, 0.0f, 1.5f};
};

class Gpu {  // gpu.rs:3-50 (wgpu instance/adapter/device/queue -> one HIP context + stream)
  public:
    explicit Gpu(int device = 0) {
        int rc = svo_ctx_create(device, &ctx_);
        if (rc != SVO_OK) throw Error(rc, "svo_ctx_create failed (no usable HIP device?)");
    }
    ~Gpu() { svo_ctx_destroy(ctx_); }
    Gpu(const Gpu &) = delete;
    Gpu &operator=(const Gpu &) = delete;
    svo_ctx *ctx() const { return ctx_; }
    void check(int rc) const {
        if (rc != SVO_OK) throw Error(rc, svo_last_error(ctx_));
    }
    void poll_wait() const { check(svo_sync(ctx_)); }  // device.poll(Maintain::Wait)
    void set_option(int option, int64_t value) const { check(svo_set_option(ctx_, option, value)); }

  private:
    svo_ctx *ctx_ = nullptr;
};

// `words` u32 of device memory for the length of a call (svo_buffer_alloc), freed with the object
class Scratch {
  public:
    Scratch(const Gpu &gpu, uint64_t words) : gpu_(gpu) { gpu.check(svo_buffer_alloc(gpu.ctx(), size_t(words) * 4, &p_)); }
    ~Scratch() { (void)svo_buffer_free(gpu_.ctx(), p_); }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    uint32_t *u32() const { return static_cast<uint32_t *>(p_); }
    int32_t *i32() const { return static_cast<int32_t *>(p_); }

  private:
    const Gpu &gpu_;
    void *p_ = nullptr;
};

class CpuOctree {  // cpu_octree.rs:17-273
  public:
    explicit CpuOctree(uint8_t mask = 0) : t_(svo_cpu_octree_new(mask)) {}
    static CpuOctree load_file(const std::string &file, uint32_t octree_depth) {  // :113-125, Err(String) -> throw
        char err[256] = {0};
        svo_cpu_octree *t = svo_cpu_octree_load_file(file.c_str(), octree_depth, err, sizeof err);
        if (!t) throw Error(SVO_ERR_ARG, err);
        return CpuOctree(t);
    }
    ~CpuOctree() { svo_cpu_octree_free(t_); }
    CpuOctree(CpuOctree &&o) noexcept : t_(std::exchange(o.t_, nullptr)) {}
    CpuOctree(const CpuOctree &) = delete;
    size_t len() const { return svo_cpu_octree_len(t_); }
    void put_in_voxel(const float pos[3], Voxel v, uint32_t depth) {
        const uint8_t rgb[3] = {v.r, v.g, v.b};
        svo_cpu_octree_put_in_voxel(t_, pos, rgb, depth);
    }
    std::vector<uint32_t> to_octree_words() const {  // to_octree(), :233-252
        std::vector<uint32_t> w(len());
        svo_cpu_octree_to_octree(t_, w.data());
        return w;
    }
    Voxel generate_mip_tree() {  // world.rs:234-336
        uint8_t top[3];
        svo_cpu_octree_generate_mips(t_, top);
        return Voxel{top[0], top[1], top[2]};
    }
    void put_in_block(const float pos[3], uint32_t block_id, uint32_t depth) { svo_cpu_octree_put_in_block(t_, pos, block_id, depth); }
    std::vector<uint8_t> bin() const {  // CpuOctree::bin, :262-264
        std::vector<uint8_t> b(svo_cpu_octree_bin(t_, nullptr, 0));
        svo_cpu_octree_bin(t_, b.data(), b.size());
        return b;
    }
    static CpuOctree from_bin(const std::vector<uint8_t> &bin) {  // :266-272
        char err[256] = {0};
        svo_cpu_octree *t = svo_cpu_octree_from_bin(bin.data(), bin.size(), err, sizeof err);
        if (!t) throw Error(SVO_ERR_ARG, err);
        return CpuOctree(t);
    }
    // the mip-coloured tree of n voxels built on the GPU (svo_cpu_octree_build): xyz (n * 3) and colours (n,
    // or null for `colour`) are DEVICE pointers; nothing for n == 0
    static std::optional<CpuOctree> build(const Gpu &gpu, const uint32_t *xyz_dev, const uint32_t *colours_dev, size_t n, uint32_t depth,
                                          uint32_t colour = 0xFFFFFF, uint64_t max_nodes = 0) {
        const svo_chunk_build_params p{depth, 0, colour, max_nodes};
        svo_cpu_octree *t = nullptr;
        gpu.check(svo_cpu_octree_build(gpu.ctx(), xyz_dev, colours_dev, n, &p, &t));
        if (!t) return std::nullopt;
        return CpuOctree(t);
    }
    svo_cpu_octree *raw() const { return t_; }
    svo_cpu_octree *release() { return std::exchange(t_, nullptr); }  // hand the tree to a World

  private:
    explicit CpuOctree(svo_cpu_octree *t) : t_(t) {}
    svo_cpu_octree *t_;
};

class Octree {  // octree.rs:43-162
  public:
    explicit Octree(const std::vector<uint32_t> &words) : o_(svo_octree_from_words(words.data(), words.size())) {}
    explicit Octree(const Voxel (&mask)[8]) {
        uint8_t rgb[24];
        for (int i = 0; i < 8; i++) { rgb[3 * i] = mask[i].r; rgb[3 * i + 1] = mask[i].g; rgb[3 * i + 2] = mask[i].b; }
        o_ = svo_octree_new(rgb);
    }
    ~Octree() { svo_octree_free(o_); }
    Octree(const Octree &) = delete;
    size_t len() const { return svo_octree_len(o_); }
    const uint32_t *raw_data() const { return svo_octree_raw_data(o_); }
    uint32_t get_node(size_t i) const { return svo_octree_get_node(o_, i); }
    void subdivide(size_t node, const Voxel (&mask)[8], uint32_t depth) {
        uint8_t rgb[24];
        for (int i = 0; i < 8; i++) { rgb[3 * i] = mask[i].r; rgb[3 * i + 1] = mask[i].g; rgb[3 * i + 2] = mask[i].b; }
        if (svo_octree_subdivide(o_, node, rgb, depth) != 0) throw Error(SVO_ERR_STATE, "Node already subdivided!");
    }
    bool unsubdivide(size_t node) {
        int rc = svo_octree_unsubdivide(o_, node);
        if (rc < 0) throw Error(SVO_ERR_STATE, "Tried to unsubdivide a node without position!");
        return rc == 0;
    }
    // words written since the previous call (index, value), each index once: the input of Render::scatter_nodes
    std::pair<std::vector<uint32_t>, std::vector<uint32_t>> take_dirty() {
        const size_t n = svo_octree_take_dirty(o_, nullptr, nullptr, 0);
        std::vector<uint32_t> idx(n), val(n);
        if (n) svo_octree_take_dirty(o_, idx.data(), val.data(), n);
        return {std::move(idx), std::move(val)};
    }
    svo_octree *raw() const { return o_; }

  private:
    svo_octree *o_;
};

class World {  // world.rs:5-336: chunk table with block instancing
  public:
    struct Found { uint32_t chunk; size_t index; uint32_t depth; float pos[3]; };
    explicit World(const std::string &path = "") : w_(svo_world_new(path.c_str())) {}
    static World load_world(const std::string &path) {  // :159-174
        char err[256] = {0};
        svo_world *w = svo_world_load(path.c_str(), err, sizeof err);
        if (!w) throw Error(SVO_ERR_ARG, err);
        return World(w);
    }
    // a new streamable world in directory `path` (must not exist) from n voxels, built on the GPU (svo_world_build,
    // DESIGN.md 14); returns load_world(path)
    static World build_world(const std::string &path, const Gpu &gpu, const uint32_t *xyz_dev, const uint32_t *colours_dev, size_t n,
                             uint32_t depth, uint32_t world_depth = 1, uint32_t colour = 0xFFFFFF, uint64_t max_nodes = 0) {
        World w(path);
        const svo_chunk_build_params p{depth, world_depth, colour, max_nodes};
        gpu.check(svo_world_build(gpu.ctx(), w.raw(), xyz_dev, colours_dev, n, &p));
        return load_world(path);
    }
    ~World() { svo_world_free(w_); }
    World(World &&o) noexcept : w_(std::exchange(o.w_, nullptr)) {}
    World(const World &) = delete;
    void insert(uint32_t id, CpuOctree &&chunk) { check(svo_world_insert(w_, id, chunk.release())); }  // chunks.insert
    bool remove(uint32_t id) { return svo_world_remove(w_, id) == 0; }
    bool contains(uint32_t id) const { return svo_world_chunk(w_, id) != nullptr; }
    Found find_voxel(const float pos[3], int64_t max_depth = -1) const {  // :201-232; the reference panics on a missing chunk
        Found f{};
        uint64_t index = 0;
        check(svo_world_find_voxel(w_, pos, max_depth, &f.chunk, &index, &f.depth, f.pos));
        f.index = size_t(index);
        return f;
    }
    Voxel generate_mip_tree(uint32_t id) {  // :234-336
        uint8_t top[3];
        check(svo_world_generate_mip_tree(w_, id, top));
        return Voxel{top[0], top[1], top[2]};
    }
    void save_chunk(uint32_t id) { check(svo_world_save_chunk(w_, id)); }  // :176-184
    void load_chunk(uint32_t id) { check(svo_world_load_chunk(w_, id)); }  // :186-198, synchronous
    Octree root_octree() const {  // App::new, app.rs:47-48
        uint8_t rgb[24];
        const svo_cpu_octree *root = svo_world_chunk(w_, 0);
        if (!root) throw Error(SVO_ERR_STATE, "world has no root chunk");
        svo_cpu_octree_get_node_mask(root, 0, rgb);
        Voxel mask[8];
        for (int i = 0; i < 8; i++) mask[i] = Voxel{rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
        return Octree(mask);
    }
    // process_subdivision / process_unsubdivision over the lists Compute::read_lists returns (adaptive.rs:29-61, 93-121)
    size_t process_subdivision(const std::vector<uint32_t> &list, Octree &octree) {
        const int64_t n = svo_adaptive_subdivide(w_, octree.raw(), list.data(), list.size(), nullptr);
        check(n < 0 ? -1 : 0);
        return size_t(n);
    }
    size_t process_unsubdivision(const std::vector<uint32_t> &list, Octree &octree) {
        const int64_t n = svo_adaptive_unsubdivide(w_, octree.raw(), list.data(), list.size());
        check(n < 0 ? -1 : 0);
        return size_t(n);
    }
    uint64_t expand(Octree &octree, uint32_t max_depth, const float *cam = nullptr, float lod_c = 0.0f,
                    uint64_t max_words = 1ull << 27) {
        return svo_world_expand(w_, octree.raw(), max_depth, cam, cam ? lod_c : 0.0f, max_words);
    }
    svo_world *raw() const { return w_; }

  private:
    explicit World(svo_world *w) : w_(w) {}
    void check(int rc) const {
        if (rc < 0) throw Error(SVO_ERR_STATE, svo_world_last_error(w_));
    }
    svo_world *w_;
};

class Render {  // render.rs:3-285
  public:
    static constexpr size_t kDefaultCapacity = 10000000;  // render.rs:53
    svo_uniforms uniforms{};                              // render.rs:287-322 (bools as flag bits)
    uint32_t width, height;

    // Render::new: node buffer = octree.expanded(capacity), uniform defaults (render.rs:42-61, 306-321)
    Render(const Gpu &gpu, uint32_t w, uint32_t h, const uint32_t *words, size_t n_words, size_t capacity = kDefaultCapacity)
        : width(w), height(h), gpu_(gpu) {
        gpu_.check(svo_nodes_alloc(gpu_.ctx(), capacity > n_words ? capacity : n_words));
        write_nodes(words, n_words);
        const float sun[4] = {-1.7f, -1.0f, 0.8f, 0.0f};
        for (int i = 0; i < 4; i++) uniforms.sun_dir[i] = sun[i];
        uniforms.flags = SVO_F_SHADOWS;
    }
    Render(const Gpu &gpu, uint32_t w, uint32_t h, const Octree &octree, size_t capacity = kDefaultCapacity)
        : Render(gpu, w, h, octree.raw_data(), octree.len(), capacity) {}
    // queue.write_buffer(&node_buffer, 0, nodes) (app.rs:113-118)
    void write_nodes(const uint32_t *words, size_t n) { gpu_.check(svo_nodes_write(gpu_.ctx(), 0, words, n)); }
    // the tree of n voxels built on the GPU into the node buffer (svo_nodes_build): xyz (n * 3) and colours
    // (n, or null for `colour`) are DEVICE pointers; returns the word count.  Raises SVO_OPT_TREE_DEPTH to depth, never
    // lowers it.
    uint64_t build_nodes(const uint32_t *xyz_dev, const uint32_t *colours_dev, size_t n, uint32_t depth, uint32_t colour = 0xFFFFFF,
                         uint64_t max_words = 0) {
        if (depth > declared_depth_) {
            gpu_.set_option(SVO_OPT_TREE_DEPTH, depth);
            declared_depth_ = depth;
        }
        const svo_build_params p{depth, colour, max_words};
        uint64_t n_words = 0;
        gpu_.check(svo_nodes_build(gpu_.ctx(), xyz_dev, colours_dev, n, &p, &n_words));
        gpu_.poll_wait();  // the inputs may go away
        return n_words;
    }
    // n voxels put into the first n_words words of the node buffer, in place (svo_nodes_edit): inputs as
    // build_nodes, colour 0 removes a voxel; returns the new length.  Throws, with nothing written, for a cell the tree
    // refines below depth.
    uint64_t edit_nodes(uint64_t n_words, const uint32_t *xyz_dev, const uint32_t *colours_dev, size_t n, uint32_t depth,
                        uint32_t colour = 0xFFFFFF, uint64_t max_words = 0) {
        if (depth > declared_depth_) {
            gpu_.set_option(SVO_OPT_TREE_DEPTH, depth);
            declared_depth_ = depth;
        }
        const svo_edit_params p{depth, colour, n_words, max_words};
        uint64_t new_words = 0;
        gpu_.check(svo_nodes_edit(gpu_.ctx(), xyz_dev, colours_dev, n, &p, &new_words));
        gpu_.poll_wait();  // the inputs may go away
        return new_words;
    }
    // the first n_words words of the node buffer edited by n_shapes boxes and balls (host memory), in place and in input
    // order (svo_nodes_edit_region): a cell inside a shape whose mode names its state takes the shape's
    // colour, 0 empties it; returns the new length.  Throws, with nothing written, where the tree is finer than depth
    // under a shape that does not replace it.
    uint64_t edit_region(uint64_t n_words, const svo_region_shape *shapes, size_t n_shapes, uint32_t depth, uint64_t max_words = 0) {
        if (depth > declared_depth_) {
            gpu_.set_option(SVO_OPT_TREE_DEPTH, depth);
            declared_depth_ = depth;
        }
        const svo_region_params p{depth, 0u, n_words, max_words};
        uint64_t new_words = 0;
        gpu_.check(svo_nodes_edit_region(gpu_.ctx(), shapes, n_shapes, &p, &new_words));
        gpu_.poll_wait();
        return new_words;
    }
    // the first n_words words of the node buffer, the scene, combined in place with the source tree in the src_words words at
    // src_dev (device, only read) (svo_nodes_combine): per cell op (SVO_COMBINE_OVER .. SVO_COMBINE_REPLACE)
    // decides between the scene's value and the source's; the source's cube is the scene's cell `at` of level at_level (null
    // and 0: the whole scene).  Coarse leaves stay coarse, a split leaf keeps its colour; returns the new length.  Throws,
    // with nothing written, where either tree is finer than depth and the op has to look below.
    uint64_t combine_nodes(uint64_t n_words, const uint32_t *src_dev, uint64_t src_words, uint32_t op, uint32_t depth,
                           const uint32_t *at = nullptr, uint32_t at_level = 0, uint64_t max_words = 0) {
        if (depth > declared_depth_) {
            gpu_.set_option(SVO_OPT_TREE_DEPTH, depth);
            declared_depth_ = depth;
        }
        const svo_combine_params p{op, depth, at_level, {at ? at[0] : 0u, at ? at[1] : 0u, at ? at[2] : 0u}, n_words, src_words, max_words};
        uint64_t new_words = 0;
        gpu_.check(svo_nodes_combine(gpu_.ctx(), src_dev, &p, &new_words));
        gpu_.poll_wait();  // the source may go away
        return new_words;
    }
    // the source tree, a cube of 2^src_depth cells a side with the scene's cells, placed into the scene at any cell offset
    // (null: 0, 0, 0) and in any of the cube's 48 orientations (svo_nodes_place): combine_nodes without the
    // condition that the source's cube is a cell of the scene's octree.  The part outside the scene is clipped; returns the new
    // length.  Throws, with nothing written, where either tree is finer than its depth and the op has to look below.
    uint64_t place_nodes(uint64_t n_words, const uint32_t *src_dev, uint64_t src_words, uint32_t op, uint32_t depth, uint32_t src_depth,
                         const int32_t *offset = nullptr, uint32_t orient = 0, uint64_t max_words = 0) {
        if (depth > declared_depth_) {
            gpu_.set_option(SVO_OPT_TREE_DEPTH, depth);
            declared_depth_ = depth;
        }
        const svo_place_params p{op, depth, src_depth, orient, {offset ? offset[0] : 0, offset ? offset[1] : 0, offset ? offset[2] : 0}, 0u,
                                 n_words, src_words, max_words};
        uint64_t new_words = 0;
        gpu_.check(svo_nodes_place(gpu_.ctx(), src_dev, &p, &new_words));
        gpu_.poll_wait();  // the source may go away
        return new_words;
    }
    // the source tree, a cube of 2^src_depth cells a side, placed into the scene under an affine map from scene cells to source
    // cells (svo_nodes_transform): matrix, 9 row-major entries, and translate are Q16; the scene cell c samples
    // the source's cell floor(A (c + 1/2) + t) and stays as it is where that lies outside the source's cube.  Free turns, scale
    // and shear; returns the new length.  Throws, with nothing written, where either tree is finer than its depth and the op
    // has to look below.
    uint64_t transform_nodes(uint64_t n_words, const uint32_t *src_dev, uint64_t src_words, uint32_t op, uint32_t depth, uint32_t src_depth,
                             const int32_t matrix[9], const int64_t translate[3], uint64_t max_words = 0) {
        if (depth > declared_depth_) {
            gpu_.set_option(SVO_OPT_TREE_DEPTH, depth);
            declared_depth_ = depth;
        }
        svo_transform_params p{};
        p.op = op, p.depth = depth, p.src_depth = src_depth;
        for (int i = 0; i < 9; i++) p.matrix[i] = matrix[i];
        for (int i = 0; i < 3; i++) p.translate[i] = translate[i];
        p.n_words = n_words, p.src_words = src_words, p.max_words = max_words;
        uint64_t new_words = 0;
        gpu_.check(svo_nodes_transform(gpu_.ctx(), src_dev, &p, &new_words));
        gpu_.poll_wait();  // the source may go away
        return new_words;
    }
    // `steps` steps of morphology on the first n_words words of the node buffer, in place (svo_nodes_morph): op
    // SVO_MORPH_GROW adds every empty cell with a voxel among its conn (6, 18 or 26) neighbours, in `colour` or with 0 in its
    // first neighbour's value, SVO_MORPH_SHRINK empties every voxel with an empty cell among them (open_boundary: or the grid's
    // outside).  Closing is grows, then as many shrinks; opening the reverse.  Returns the new length.  Throws where the tree is
    // finer than `depth`; the steps before that one stay.  A merged tree (simplify_nodes) is the cheap input.
    uint64_t morph_nodes(uint64_t n_words, uint32_t op, uint32_t depth, uint32_t steps = 1, uint32_t conn = 26, uint32_t colour = 0,
                         bool open_boundary = false, uint64_t max_words = 0) {
        if (depth > declared_depth_) {
            gpu_.set_option(SVO_OPT_TREE_DEPTH, depth);
            declared_depth_ = depth;
        }
        for (uint32_t step = 0; step < steps; step++) {
            const svo_morph_params p{op, conn, depth, open_boundary ? SVO_MORPH_OPEN_BOUNDARY : 0u, op == SVO_MORPH_GROW ? colour & 0xFFFFFFu : 0u, 0u,
                                     n_words, max_words};
            gpu_.check(svo_nodes_morph(gpu_.ctx(), &p, &n_words));
        }
        return n_words;
    }
    // the first n_words words of the node buffer shaped by the height map heights_dev (device, size_xz[0] * size_xz[1] u32, z
    // fastest, only read) over the columns from origin_xz on, in place (svo_nodes_edit_heightmap): the cells
    // below a column's height that mode_below names take their layer's colour, the cells at and above it that mode_above
    // names take colour_above (modes: 0 leaves the side alone, SVO_REGION_EMPTY, _VOXELS, _SET).  Coarse leaves stay coarse
    // away from the ground's surface, a split leaf keeps its colour; returns the new length.  Throws, with nothing written,
    // where the tree is finer than depth under a mode that does not replace it.
    uint64_t edit_heightmap(uint64_t n_words, const uint32_t *heights_dev, const uint32_t origin_xz[2], const uint32_t size_xz[2], uint32_t depth,
                            const svo_heightmap_layer *layers, uint32_t n_layers, uint32_t mode_below = SVO_REGION_SET, uint32_t mode_above = 0,
                            uint32_t colour_above = 0, uint64_t max_words = 0) {
        if (depth > declared_depth_) {
            gpu_.set_option(SVO_OPT_TREE_DEPTH, depth);
            declared_depth_ = depth;
        }
        svo_heightmap_params p{depth, n_layers, n_words, max_words, {origin_xz[0], origin_xz[1]}, {size_xz[0], size_xz[1]}, mode_below, mode_above,
                               colour_above, 0u, {}};
        for (uint32_t k = 0; k < n_layers && k < SVO_HEIGHTMAP_MAX_LAYERS; k++) p.layers[k] = layers[k];
        uint64_t new_words = 0;
        gpu_.check(svo_nodes_edit_heightmap(gpu_.ctx(), &p, heights_dev, &new_words));
        gpu_.poll_wait();
        return new_words;
    }
    // the first n_words words of the node buffer compacted in place (svo_nodes_compact): unreachable groups
    // dropped, with `prune` also the groups that hold nothing, the rest in the builder's breadth-first order; returns the
    // new length.  perm_dev (device, n_words u32, or null): perm[new word] = old word.  Throws, with nothing written, for
    // a malformed tree or with a device adaptive state attached.
    uint64_t compact_nodes(uint64_t n_words, bool prune = true, uint32_t *perm_dev = nullptr) {
        const svo_compact_params p{prune ? SVO_COMPACT_PRUNE_EMPTY : 0u, 0u, n_words};
        uint64_t new_words = 0;
        gpu_.check(svo_nodes_compact(gpu_.ctx(), &p, perm_dev, &new_words));
        gpu_.poll_wait();
        return new_words;
    }
    // the first n_words words of the node buffer simplified (svo_nodes_simplify): with `merge` an interior
    // word whose whole subtree holds one leaf value becomes that leaf (lossless; no merged leaf above min_level), with
    // cut_level != 0 every interior word of that level becomes a leaf of its subtree's mip colour; the rest in the
    // compaction's breadth-first order; returns the new length.  out_dev null: in place, as compact_nodes; otherwise the
    // new tree goes to out_dev (device, out_cap words) and the node buffer is only read.  perm_dev (device, n_words u32,
    // or null): perm[new word] = old word.  Throws, with nothing written, for a malformed tree, for an in-place call with
    // a device adaptive state attached, or for more words than out_cap.  Mind that edit_nodes splits a coarse leaf into
    // EMPTY children: voxels put into a merged solid by cell list lose its colour around them; edit_region carries it down.
    uint64_t simplify_nodes(uint64_t n_words, bool merge = true, uint32_t cut_level = 0, uint32_t min_level = 0,
                            uint32_t *out_dev = nullptr, uint64_t out_cap = 0, uint32_t *perm_dev = nullptr) {
        const svo_simplify_params p{(merge ? SVO_SIMPLIFY_MERGE : 0u) | (cut_level ? SVO_SIMPLIFY_CUT : 0u), cut_level, min_level, 0u,
                                    n_words, out_cap};
        uint64_t new_words = 0;
        gpu_.check(svo_nodes_simplify(gpu_.ctx(), &p, out_dev, perm_dev, &new_words));
        gpu_.poll_wait();
        return new_words;
    }
    // the voxels of the tree in the first n_words words of the node buffer listed on the GPU (svo_nodes_list_voxels,
    // DESIGN.md 18), the inverse of build_nodes: xyz_dev (3 * max_voxels u32), values_dev (max_voxels) and levels_dev
    // (max_voxels, or null) are DEVICE pointers; entries in ascending Morton order on the `depth` grid, with `expand` a
    // leaf above depth as its cells; returns the entry count.  xyz_dev null: the count alone.  Throws, with nothing
    // written, for a tree deeper than depth, a malformed tree or more entries than max_voxels.
    uint64_t list_voxels(uint64_t n_words, uint32_t depth, uint32_t *xyz_dev, uint32_t *values_dev, uint64_t max_voxels,
                         bool expand = false, uint32_t *levels_dev = nullptr) {
        const svo_list_params p{expand ? SVO_LIST_EXPAND : 0u, depth, n_words, max_voxels};
        uint64_t n = 0;
        gpu_.check(svo_nodes_list_voxels(gpu_.ctx(), &p, xyz_dev, values_dev, levels_dev, &n));
        gpu_.poll_wait();
        return n;
    }
    // the visible surface of that tree, found on the GPU (svo_nodes_list_surface): list_voxels' entries that
    // show a face, in its order, with faces_dev (max_entries) the 6-bit mask of the exposed faces (bit f: -x, +x, -y, +y,
    // -z, +z); flags: SVO_SURFACE_CLOSED_BOUNDARY (the grid's boundary covers), SVO_SURFACE_KEEP_HIDDEN (masks of 0 stay)
    // or SVO_SURFACE_QUADS (one entry per exposed face, faces_dev its number 0..5).  A face is covered when a leaf of the
    // same or a coarser level stands behind it.  All outputs are DEVICE pointers; returns the entry count; xyz_dev null:
    // the count alone.  Throws, with nothing written, for what list_voxels throws and for more entries than max_entries.
    uint64_t list_surface(uint64_t n_words, uint32_t depth, uint32_t *xyz_dev, uint32_t *values_dev, uint32_t *faces_dev,
                          uint64_t max_entries, uint32_t flags = 0, uint32_t *levels_dev = nullptr) {
        const svo_surface_params p{flags, depth, n_words, max_entries};
        uint64_t n = 0;
        gpu_.check(svo_nodes_list_surface(gpu_.ctx(), &p, xyz_dev, values_dev, levels_dev, faces_dev, &n));
        gpu_.poll_wait();
        return n;
    }
    // that surface merged into rectangles on the GPU (svo_nodes_merge_surface): the exposed faces of
    // SVO_SURFACE_QUADS, joined along u and then along v, `rounds` (1..4) times, where faces of one plane and one value
    // touch; rects_dev (6 * max_entries u32: face, plane, u0, v0, w, h) and values_dev (max_entries) are DEVICE pointers;
    // flags: SVO_SURFACE_CLOSED_BOUNDARY, SVO_SURFACE_MERGE_ANY_VALUE (faces join whatever their values; every value 0).
    // Returns the entry count; rects_dev null: the count alone.  Throws, with nothing written, for what list_surface
    // throws and for more rectangles than max_entries.
    uint64_t surface_rects(uint64_t n_words, uint32_t depth, uint32_t *rects_dev, uint32_t *values_dev, uint64_t max_entries,
                           uint32_t flags = 0, uint32_t rounds = 1) {
        const svo_surface_merge_params p{flags, depth, rounds, 0u, n_words, max_entries};
        uint64_t n = 0;
        gpu_.check(svo_nodes_merge_surface(gpu_.ctx(), &p, rects_dev, values_dev, &n));
        gpu_.poll_wait();
        return n;
    }
    // the connected components of that tree's voxels, labelled on the GPU (svo_nodes_label_components):
    // list_voxels' entries (without expand), in its order; two leaves are linked when their cubes share a piece of a face,
    // with same_value only when their values are equal.  labels_dev (max_entries u32: the rank of the first entry of the
    // entry's component), ids_dev (the component's number, by ascending first entry; or null) and indices_dev (the index
    // of the entry's word in the node buffer, what scatter_nodes_device takes; or null) are DEVICE pointers.  Returns the
    // entry count, *n_components (when given) the number of components; labels_dev null: the counts alone.  Throws, with
    // nothing written, for what list_voxels throws and for more entries than max_entries.
    uint64_t label_components(uint64_t n_words, uint32_t depth, uint32_t *labels_dev, uint32_t *ids_dev, uint32_t *indices_dev,
                              uint64_t max_entries, bool same_value = false, uint64_t *n_components = nullptr) {
        const svo_components_params p{same_value ? SVO_COMPONENTS_SAME_VALUE : 0u, depth, n_words, max_entries};
        uint64_t n = 0, c = 0;
        gpu_.check(svo_nodes_label_components(gpu_.ctx(), &p, labels_dev, ids_dev, indices_dev, &n, &c));
        gpu_.poll_wait();
        if (n_components) *n_components = c;
        return n;
    }
    // words_dev[i], or the one word `fill` when words_dev is null, to the node buffer at indices_dev[i], n DEVICE entries
    // (svo_nodes_scatter_device); an index >= n_words is skipped.  Does not block: the arrays stay valid until gpu.poll_wait().
    void scatter_nodes_device(const uint32_t *indices_dev, const uint32_t *words_dev, uint32_t fill, size_t n, uint64_t n_words) {
        gpu_.check(svo_nodes_scatter_device(gpu_.ctx(), indices_dev, words_dev, fill, n, n_words));
    }
    // What a drop_floating call did.
    struct Dropped {
        uint64_t components, dropped_components, dropped_leaves;
    };
    // the leaves of every component that does not meet the anchor box [lo, hi) of the `depth` grid get the empty word
    // (label_components, then scatter_nodes_device); lo and hi null: the floor layer y == 0, y being up.  The labels and the
    // listing stay on the device but for the ids, corners and levels, which the host reads to decide which components
    // hold.  The groups this leaves empty are compact_nodes' (prune) to drop.
    Dropped drop_floating(uint64_t n_words, uint32_t depth, const uint32_t *lo = nullptr, const uint32_t *hi = nullptr,
                          bool same_value = false) {
        uint64_t c = 0;
        const uint64_t n = label_components(n_words, depth, nullptr, nullptr, nullptr, 0, same_value, &c);
        if (!n) return {0, 0, 0};
        const uint64_t side = 1ull << depth;
        const uint64_t box_lo[3] = {lo ? lo[0] : 0, lo ? lo[1] : 0, lo ? lo[2] : 0};
        const uint64_t box_hi[3] = {hi ? hi[0] : side, hi ? hi[1] : 1, hi ? hi[2] : side};
        Scratch labels(gpu_, n), ids(gpu_, n), indices(gpu_, n), xyz(gpu_, 3 * n), values(gpu_, n), levels(gpu_, n);
        label_components(n_words, depth, labels.u32(), ids.u32(), indices.u32(), n, same_value);
        list_voxels(n_words, depth, xyz.u32(), values.u32(), n, false, levels.u32());
        std::vector<uint32_t> id(n), at(n), corner(3 * n), level(n);
        gpu_.check(svo_buffer_read(gpu_.ctx(), ids.u32(), id.data(), n * 4));
        gpu_.check(svo_buffer_read(gpu_.ctx(), indices.u32(), at.data(), n * 4));
        gpu_.check(svo_buffer_read(gpu_.ctx(), xyz.u32(), corner.data(), 3 * n * 4));
        gpu_.check(svo_buffer_read(gpu_.ctx(), levels.u32(), level.data(), n * 4));
        std::vector<char> held(c, 0);
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t size = 1ull << (depth - level[i]);
            bool meets = true;
            for (int a = 0; a < 3; a++) meets = meets && corner[3 * i + a] < box_hi[a] && corner[3 * i + a] + size > box_lo[a];
            if (meets) held[id[i]] = 1;
        }
        std::vector<uint32_t> gone;
        for (uint64_t i = 0; i < n; i++)
            if (!held[id[i]]) gone.push_back(at[i]);
        Dropped d{c, 0, gone.size()};
        for (char h : held) d.dropped_components += !h;
        if (!gone.empty()) {
            gpu_.check(svo_buffer_write(gpu_.ctx(), indices.u32(), gone.data(), gone.size() * 4));
            scatter_nodes_device(indices.u32(), nullptr, SVO_VOXEL_OFFSET << 4, gone.size(), n_words);
            gpu_.poll_wait();  // (the indices go with this call)
        }
        return d;
    }
    // a triangle mesh voxelised on the GPU, conservatively and exactly (svo_mesh_voxelize): vq_dev
    // (3 * n_vertices quantised coordinates, 64 per cell of the 2^depth grid), tri_dev (3 * n_tris vertex indices),
    // tri_colours_dev (n_tris x 0x00RRGGBB, or null: `colour`) and the outputs xyz_dev (3 * max_voxels u32), colours_dev
    // (max_voxels) and tris_dev (max_voxels, or null) are DEVICE pointers; one entry per triangle and cell that meet,
    // triangles in order, cells in Morton order: a list that build_nodes and edit_nodes take, in which the highest triangle
    // index colours a shared cell.  Returns the entry count; xyz_dev null: the count alone.  Needs no node buffer.  Throws,
    // with nothing written, for a bad vertex index or coordinate or more entries than max_voxels.
    uint64_t voxelize_mesh(const uint32_t *vq_dev, uint32_t n_vertices, const uint32_t *tri_dev, size_t n_tris, uint32_t depth,
                           uint32_t *xyz_dev, uint32_t *colours_dev, uint64_t max_voxels, const uint32_t *tri_colours_dev = nullptr,
                           uint32_t colour = 0xFFFFFF, uint32_t *tris_dev = nullptr) {
        const svo_voxelize_params p{depth, 0u, colour, n_vertices, max_voxels};
        uint64_t n = 0;
        gpu_.check(svo_mesh_voxelize(gpu_.ctx(), &p, vq_dev, tri_dev, tri_colours_dev, n_tris, xyz_dev, colours_dev, tris_dev, &n));
        gpu_.poll_wait();  // the inputs may go away
        return n;
    }
    // the cells inside a closed triangle mesh, on the GPU and exactly (svo_mesh_voxelize_solid): vq_dev and
    // tri_dev as voxelize_mesh takes them; flags: SVO_SOLID_EVENODD or SVO_SOLID_NONZERO, with SVO_SOLID_SPANS the y-spans
    // (x, z, y0, y1) instead of the cells (x, y, z); out_dev (3, or 4, u32 per entry, max_out entries) is a DEVICE pointer.
    // Returns the entry count; out_dev null: the count alone.  *n_open (when given) gets the number of open columns: 0 for
    // a watertight mesh.  Needs no node buffer.  Throws, with nothing written, for a bad vertex index or coordinate, a
    // level of more than max_pairs (triangle, column square) pairs (0: 2^27) or more entries than max_out.
    uint64_t voxelize_mesh_solid(const uint32_t *vq_dev, uint32_t n_vertices, const uint32_t *tri_dev, size_t n_tris, uint32_t depth,
                                 uint32_t *out_dev, uint64_t max_out, uint32_t flags = SVO_SOLID_EVENODD, uint64_t *n_open = nullptr,
                                 uint64_t max_pairs = 0) {
        const svo_solid_params p{depth, flags, n_vertices, 0u, max_out, max_pairs};
        uint64_t n = 0;
        gpu_.check(svo_mesh_voxelize_solid(gpu_.ctx(), &p, vq_dev, tri_dev, n_tris, out_dev, &n, n_open));
        gpu_.poll_wait();  // the inputs may go away
        return n;
    }
    // what the tree in the first n_words words of the node buffer holds at n cells of the `depth` grid, looked up on the
    // GPU (svo_nodes_sample): xyz_dev (3 * n u32, as build_nodes takes them), values_dev (n u32) and
    // levels_dev, indices_dev (n u32 each, or null) are DEVICE pointers; a value is the leaf's, 0 for empty, or one of
    // SVO_SAMPLE_FINER, SVO_SAMPLE_OUTSIDE, SVO_SAMPLE_BROKEN.  The node buffer is only read.
    void sample_voxels(uint64_t n_words, uint32_t depth, const uint32_t *xyz_dev, size_t n, uint32_t *values_dev,
                       uint32_t *levels_dev = nullptr, uint32_t *indices_dev = nullptr) {
        const svo_sample_params p{0u, depth, n_words};
        gpu_.check(svo_nodes_sample(gpu_.ctx(), &p, xyz_dev, n, values_dev, levels_dev, indices_dev));
        gpu_.poll_wait();  // the inputs may go away
    }
    // the cells [origin, origin + size) of the `depth` grid as a dense array indexed [x][y][z], z fastest, like
    // build_nodes_dense's grid (svo_nodes_sample_dense): grid_dev holds size[0] * size[1] * size[2] u32
    // of DEVICE memory.  Throws for a box that leaves the grid or has 2^31 cells or more.
    void sample_dense(uint64_t n_words, uint32_t depth, const uint32_t origin[3], const uint32_t size[3], uint32_t *grid_dev) {
        const svo_sample_params p{0u, depth, n_words};
        gpu_.check(svo_nodes_sample_dense(gpu_.ctx(), &p, origin, size, grid_dev));
        gpu_.poll_wait();
    }
    // the exact squared distance of every cell of the box [origin, origin + size) of the `depth` grid to its nearest site
    // within max_distance (1..SVO_DISTANCE_MAX_RADIUS) cells (svo_nodes_distance): d2_dev holds size[0] *
    // size[1] * size[2] i32 of DEVICE memory, z fastest like sample_dense's grid, sites_dev (or null) as many u32 for the
    // packed offset to that site.  mode: SVO_DISTANCE_TO_VOXELS, _TO_EMPTY or _SIGNED.  SVO_DISTANCE_FAR and
    // SVO_DISTANCE_NO_SITE where no site is that near.  Throws for a box that leaves the grid, has 2^31 cells or more or
    // needs more workspace than SVO_DISTANCE_MAX_WORKSPACE.  The node buffer is only read.
    void distance_dense(uint64_t n_words, uint32_t depth, const uint32_t origin[3], const uint32_t size[3], uint32_t max_distance,
                        int32_t *d2_dev, uint32_t *sites_dev = nullptr, uint32_t mode = SVO_DISTANCE_TO_VOXELS) {
        const svo_distance_params p{0u, mode, depth, max_distance, n_words};
        gpu_.check(svo_nodes_distance(gpu_.ctx(), &p, origin, size, d2_dev, sites_dev));
        gpu_.poll_wait();
    }
    // the highest occupied cell of each column of a rectangle of the `depth` grid (svo_nodes_column_tops):
    // tops_dev and values_dev (or null) hold size_xz[0] * size_xz[1] u32 of DEVICE memory, z fastest; a top is the y of
    // the first cell from y_hi - 1 down to y_lo that sample_voxels gives a value other than 0, or SVO_TOP_NONE.  y_hi 0:
    // the whole height.  The node buffer is only read.
    void column_tops(uint64_t n_words, uint32_t depth, const uint32_t origin_xz[2], const uint32_t size_xz[2], uint32_t *tops_dev,
                     uint32_t *values_dev = nullptr, uint32_t y_lo = 0, uint32_t y_hi = 0) {
        const svo_tops_params p{0u, depth, n_words, y_lo, y_hi ? y_hi : depth < 32 ? 1u << depth : 0u};
        gpu_.check(svo_nodes_column_tops(gpu_.ctx(), &p, origin_xz, size_xz, tops_dev, values_dev));
        gpu_.poll_wait();
    }
    // the columns of that rectangle that get a structure (svo_structures_sites), from the two arrays
    // column_tops wrote: origins_dev (3 * max_sites int32: x, top + lift, z) and rots_dev (max_sites u32, or null) are
    // DEVICE pointers; returns the site count.  origins_dev null: the count alone.
    uint64_t structure_sites(const uint32_t *tops_dev, const uint32_t *values_dev, const uint32_t origin_xz[2], const uint32_t size_xz[2],
                             uint32_t one_in, int32_t *origins_dev, uint32_t *rots_dev, uint64_t max_sites, uint32_t seed = 0,
                             uint32_t on_value = 0, int32_t lift = 1, bool rotate = true) {
        const svo_sites_params p{rotate ? SVO_SITES_ROTATE : 0u, seed, one_in, on_value, lift, 0u, max_sites};
        uint64_t n = 0;
        gpu_.check(svo_structures_sites(gpu_.ctx(), &p, tops_dev, values_dev, origin_xz, size_xz, origins_dev, rots_dev, &n));
        gpu_.poll_wait();
        return n;
    }
    // k placements of a structure of m voxels as one voxel list (svo_structures_stamp): offsets_dev (3 * m
    // int32), colours_dev (m), origins_dev (3 * k int32), rots_dev (k quarter turns about +y, or null) and the outputs
    // xyz_dev (3 * max_voxels u32), out_colours_dev (max_voxels) and placements_dev (max_voxels, or null) are DEVICE
    // pointers; cells outside the `depth` grid are clipped; a list that edit_nodes takes, in which a later placement wins
    // a shared cell.  Returns the entry count; xyz_dev null: the count alone.
    uint64_t stamp_structures(const int32_t *offsets_dev, const uint32_t *colours_dev, size_t m, const int32_t *origins_dev,
                              const uint32_t *rots_dev, size_t k, uint32_t depth, uint32_t *xyz_dev, uint32_t *out_colours_dev,
                              uint64_t max_voxels, uint32_t *placements_dev = nullptr) {
        const svo_stamp_params p{0u, depth, max_voxels};
        uint64_t n = 0;
        gpu_.check(svo_structures_stamp(gpu_.ctx(), &p, offsets_dev, colours_dev, m, origins_dev, rots_dev, k, xyz_dev, out_colours_dev,
                                        placements_dev, &n));
        gpu_.poll_wait();  // the inputs may go away
        return n;
    }
    // stamp_structures, then edit_nodes with the list (held in device memory of this call's own): the structure put into
    // the first n_words words of the tree at every origin.  Returns the new length.
    uint64_t place_structures(uint64_t n_words, const int32_t *offsets_dev, const uint32_t *colours_dev, size_t m, const int32_t *origins_dev,
                              const uint32_t *rots_dev, size_t k, uint32_t depth, uint64_t max_words = 0) {
        const uint64_t n = stamp_structures(offsets_dev, colours_dev, m, origins_dev, rots_dev, k, depth, nullptr, nullptr, 0);
        if (!n) return n_words;
        Scratch xyz(gpu_, 3 * n), colours(gpu_, n);
        stamp_structures(offsets_dev, colours_dev, m, origins_dev, rots_dev, k, depth, xyz.u32(), colours.u32(), n);
        return edit_nodes(n_words, xyz.u32(), colours.u32(), n, depth, 0xFFFFFF, max_words);
    }
    // a structure scattered over the ground of a rectangle without the tree leaving the device: column_tops, then
    // structure_sites, then place_structures.  Returns the new length; *n_sites (or null) gets the number of sites.
    uint64_t scatter_structures(uint64_t n_words, const int32_t *offsets_dev, const uint32_t *colours_dev, size_t m,
                                const uint32_t origin_xz[2], const uint32_t size_xz[2], uint32_t depth, uint32_t one_in, uint32_t seed = 0,
                                uint32_t on_value = 0, int32_t lift = 1, bool rotate = true, uint64_t *n_sites = nullptr) {
        const uint64_t columns = uint64_t(size_xz[0]) * size_xz[1];
        if (n_sites) *n_sites = 0;
        if (!columns) return n_words;
        Scratch tops(gpu_, columns), values(gpu_, columns);
        column_tops(n_words, depth, origin_xz, size_xz, tops.u32(), values.u32());
        const uint64_t k = structure_sites(tops.u32(), values.u32(), origin_xz, size_xz, one_in, nullptr, nullptr, 0, seed, on_value, lift, rotate);
        if (n_sites) *n_sites = k;
        if (!k) return n_words;
        Scratch origins(gpu_, 3 * k), rots(gpu_, k);
        structure_sites(tops.u32(), values.u32(), origin_xz, size_xz, one_in, origins.i32(), rots.u32(), k, seed, on_value, lift, rotate);
        return place_structures(n_words, offsets_dev, colours_dev, m, origins.i32(), rots.u32(), k, depth);
    }
    // the adaptive step on the GPU (svo_adaptive_*): attach once (SVO_OPT_SCAN_CLEARS_COUNTERS = 1, the
    // octree's words in the node buffer, `world` kept alive), then after each scan step() over the scan's own lists (or
    // explicit DEVICE lists); download() brings the host octree up to date
    void adaptive_attach(World &world, const Octree &octree) { gpu_.check(svo_adaptive_attach(gpu_.ctx(), world.raw(), octree.raw())); }
    svo_adaptive_result adaptive_step(const uint32_t *sub_dev = nullptr, uint32_t n_sub = 0, const uint32_t *unsub_dev = nullptr,
                                      uint32_t n_unsub = 0) {
        svo_adaptive_result r{};
        gpu_.check(svo_adaptive_step(gpu_.ctx(), sub_dev, n_sub, unsub_dev, n_unsub, &r));
        return r;
    }
    // the device form of World::expand on the attached state (svo_adaptive_expand): r.n_sub subdivisions,
    // r.length words; max_words 0 = the node buffer's capacity.  Throws for a tree with free groups in its hole stack.
    svo_adaptive_result adaptive_expand(uint32_t max_depth, const float *cam = nullptr, float lod_c = 0.0f, uint64_t max_words = 0) {
        svo_adaptive_result r{};
        gpu_.check(svo_adaptive_expand(gpu_.ctx(), max_depth, cam, cam ? lod_c : 0.0f, max_words, &r));
        return r;
    }
    void adaptive_download(Octree &octree) { gpu_.check(svo_adaptive_download(gpu_.ctx(), octree.raw())); }
    // incremental form of the same upload: only the words that changed (svo_nodes_scatter; pair it with
    // gpu.set_option(SVO_OPT_SCAN_CLEARS_COUNTERS, 1), which takes over the counter reset of the full upload)
    void scatter_nodes(const std::vector<uint32_t> &indices, const std::vector<uint32_t> &words) {
        gpu_.check(svo_nodes_scatter(gpu_.ctx(), indices.data(), words.data(), indices.size()));
        gpu_.poll_wait();  // the vectors may go away
    }
    // Render::resize ignores zero sizes (render.rs:182-189)
    void resize(uint32_t w, uint32_t h) {
        if (w > 0 && h > 0) { width = w; height = h; }
    }
    // Render::update: camera = proj * look_at_rh, inverse, dimensions; upload (render.rs:191-212)
    void update(const Settings &settings, const Character &character) {
        svo_camera_matrices(character.pos, character.look, settings.fov, float(width), float(height), uniforms.camera,
                            uniforms.camera_inverse);
        uniforms.dimensions[0] = float(width);
        uniforms.dimensions[1] = float(height);
        uniforms.dimensions[2] = uniforms.dimensions[3] = 0.0f;
        gpu_.check(svo_set_uniforms(gpu_.ctx(), &uniforms));
    }
    // Render::render: one pass over every pixel (render.rs:217-284).  Device pointers; asynchronous.
    void render(svo_hit *hits_dev, uint32_t *rgba_dev = nullptr) {
        gpu_.check(svo_render(gpu_.ctx(), width, height, 0, 0, width, height, hits_dev, rgba_dev));
    }
    // primary rays + n_secondary rays per hit pixel (ray 0: the shadow ray of shader.wgsl:275-280); device pointers
    void render_secondary(uint32_t n_secondary, svo_hit *primary_dev, svo_hit *secondary_dev) {
        gpu_.check(svo_render_secondary(gpu_.ctx(), width, height, 0, 0, width, height, n_secondary, primary_dev, secondary_dev));
    }
    // same, results copied to host memory (blocking)
    void render_host(svo_hit *hits, uint32_t *rgba = nullptr) {
        gpu_.check(svo_render_host(gpu_.ctx(), width, height, 0, 0, width, height, hits, rgba));
    }
    // A second Render on another context of the same device over the SAME node buffer (svo_nodes_share): frames in
    // flight on several streams.  Writes through either one are seen by both (shared generation counter).
    struct Shared {};
    Render(const Gpu &gpu, const Render &owner, Shared) : uniforms(owner.uniforms), width(owner.width), height(owner.height), gpu_(gpu) {
        gpu_.check(svo_nodes_share(gpu_.ctx(), owner.gpu_.ctx()));
        gpu_.check(svo_set_uniforms(gpu_.ctx(), &uniforms));
    }
    // this rank's tiles of a frame sharded over `world` GPUs (tile t belongs to rank t % world), contiguous in hits_dev
    void render_tiles(uint32_t tile_w, uint32_t tile_h, uint32_t rank, uint32_t world, svo_hit *hits_dev, uint32_t *rgba_dev = nullptr) {
        gpu_.check(svo_render_tiles(gpu_.ctx(), width, height, tile_w, tile_h, rank, world, hits_dev, rgba_dev));
    }
    const Gpu &gpu() const { return gpu_; }

  private:
    const Gpu &gpu_;
    uint32_t declared_depth_ = 16;  // SVO_OPT_TREE_DEPTH as this Render last set it (the library's default: 16)
};

// One process, one thread, N GPUs -- the reference's threading model (main.rs:40-88) extended to a tile-sharded frame
// (SURVEY.md 8e): every device holds a replica of the node array and traces the tiles t = rank, rank + N, ...; the frame
// ends with ONE gather of 12-byte wire records to device 0 over RCCL (svo_gather_frame_all) and the un-permute there.
// Buffers live as long as the object; frame() returns a device pointer on device 0 that stays valid until the next frame().
class MultiGpuFrame {
  public:
    MultiGpuFrame(const std::vector<int> &devices, uint32_t w, uint32_t h, const uint32_t *words, size_t n_words, size_t capacity,
                  uint32_t tile_w = 64, uint32_t tile_h = 8)
        : w_(w), h_(h), tw_(tile_w), th_(tile_h), world_(uint32_t(devices.size())) {
        if (devices.empty() || w % tile_w || h % tile_h) throw Error(SVO_ERR_ARG, "frame must be a whole number of tiles");
        const uint32_t tiles = (w / tile_w) * (h / tile_h);
        n_pad_ = (tiles + world_ - 1) / world_;
        for (int d : devices) {
            gpus_.emplace_back(new Gpu(d));
            renders_.emplace_back(new Render(*gpus_.back(), w, h, words, n_words, capacity));
            ctxs_.push_back(gpus_.back()->ctx());
        }
        check(svo_comm_init_all(int(world_), ctxs_.data()));
        const size_t rec = size_t(n_pad_) * tw_ * th_;
        for (uint32_t r = 0; r < world_; r++) {
            hits_.push_back(static_cast<svo_hit *>(dev_alloc(r, rec * sizeof(svo_hit))));
            wire_.push_back(static_cast<uint32_t *>(dev_alloc(r, rec * 12)));
        }
        gathered_ = static_cast<uint32_t *>(dev_alloc(0, rec * 12 * world_));
        frame_ = static_cast<svo_hit *>(dev_alloc(0, size_t(w) * h * sizeof(svo_hit)));
    }
    ~MultiGpuFrame() {
        for (uint32_t r = 0; r < world_ && r < hits_.size(); r++) {
            (void)svo_buffer_free(ctxs_[r], hits_[r]);
            if (r < wire_.size()) (void)svo_buffer_free(ctxs_[r], wire_[r]);
        }
        if (!ctxs_.empty()) {
            (void)svo_buffer_free(ctxs_[0], gathered_);
            (void)svo_buffer_free(ctxs_[0], frame_);
        }
    }
    MultiGpuFrame(const MultiGpuFrame &) = delete;
    MultiGpuFrame &operator=(const MultiGpuFrame &) = delete;
    // the assembled frame of the last frame() call, copied to host memory (blocking)
    void read_frame(svo_hit *host) { check(svo_buffer_read(ctxs_[0], frame_, host, size_t(w_) * h_ * sizeof(svo_hit))); }
    Render &render(uint32_t rank) { return *renders_[rank]; }
    // trace every rank's tiles, gather, assemble: all asynchronous; sync() (or the next blocking call) completes it
    svo_hit *frame() {
        const size_t rec = size_t(n_pad_) * tw_ * th_;
        std::vector<const void *> send(world_);
        for (uint32_t r = 0; r < world_; r++) {
            // the previous frame's gather may still be reading wire_[r] on this rank's communication stream: this frame's
            // trace and pack, which overwrite hits_[r] / wire_[r], are ordered behind it (svo_hip.h: svo_gather_wait before
            // `send` is overwritten)
            check(svo_gather_wait(ctxs_[r]));
            renders_[r]->render_tiles(tw_, th_, r, world_, hits_[r]);
            check(svo_pack_records(ctxs_[r], hits_[r], rec, wire_[r]));
            send[r] = wire_[r];
        }
        check(svo_gather_frame_all(int(world_), ctxs_.data(), send.data(), rec * 12, gathered_, 0));
        check(svo_gather_wait(ctxs_[0]));
        check(svo_assemble_tiles_packed(ctxs_[0], gathered_, world_, n_pad_, w_, h_, tw_, th_, frame_));
        return frame_;
    }
    void sync() {
        for (auto &g : gpus_) g->poll_wait();
    }

  private:
    void check(int rc) const {
        if (rc != SVO_OK) throw Error(rc, svo_last_error(ctxs_.empty() ? nullptr : ctxs_[0]));
    }
    void *dev_alloc(uint32_t rank, size_t bytes) {
        void *p = nullptr;
        check(svo_buffer_alloc(ctxs_[rank], bytes, &p));
        return p;
    }
    uint32_t w_, h_, tw_, th_, world_, n_pad_ = 0;
    std::vector<std::unique_ptr<Gpu>> gpus_;
    std::vector<std::unique_ptr<Render>> renders_;
    std::vector<svo_ctx *> ctxs_;
    std::vector<svo_hit *> hits_;
    std::vector<uint32_t *> wire_;
    uint32_t *gathered_ = nullptr;
    svo_hit *frame_ = nullptr;
};

class Compute {  // compute.rs:6-127 + the read-back of adaptive.rs:12-23, 76-87
  public:
    static constexpr size_t kMaxPerFrame = 1024000;  // adaptive.rs:3-4
    Compute(const Gpu &gpu, const Render &) : gpu_(gpu) {}
    void update(size_t node_length) { gpu_.check(svo_scan_dispatch(gpu_.ctx(), uint32_t(node_length))); }
    void update(const Octree &octree) { update(octree.len()); }
    // (subdivide list, unsubdivide list); counts clamped and the device counters reset like adaptive.rs:22-23
    std::pair<std::vector<uint32_t>, std::vector<uint32_t>> read_lists() {
        std::vector<uint32_t> sub(kMaxPerFrame), unsub(kMaxPerFrame);
        uint32_t ns = 0, nu = 0;
        gpu_.check(svo_scan_read(gpu_.ctx(), sub.data(), &ns, unsub.data(), &nu, kMaxPerFrame));
        return {std::vector<uint32_t>(sub.begin() + 1, sub.begin() + 1 + ns),
                std::vector<uint32_t>(unsub.begin() + 1, unsub.begin() + 1 + nu)};
    }

  private:
    const Gpu &gpu_;
};

}  // namespace svo
