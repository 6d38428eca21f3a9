"""The host frame the GPU tree passes share (csrc/svo_ctx.h): one context runs every pass that keeps a
workspace, hands out each pass's times and is closed, which is where all of its owning members are released together;
a second context then builds the same tree.  Likewise the context's own members: its scratch grows, is reused and goes
with it, and a shared node store goes with the last context that holds it, whichever that is.  And the frame above the C
ABI (octree-tracer_amd/_device.py): the declared depth is the context's and no Render lowers it; a voxel
list builds the same tree whichever way it comes in."""
import numpy as np
import pytest

import build_ref as B
import compact_ref as C
import edit_ref as E
import list_ref as L
import sample_ref as S
import voxelize_ref as V
from conftest import assert_hits_equal, set_uniforms_from_oracle
from pass_frame import assert_words

pytestmark = pytest.mark.gpu

ROOT = np.full(8, B.EMPTY, dtype=np.uint32)


def test_every_pass_on_one_context_then_close(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(5)
    coords = rng.integers(0, 32, (300, 3))
    colours = rng.integers(1, 1 << 24, 300)
    want = B.build(coords, 5, colours)
    v, t = pkg.mesh.icosphere(0, 0.5)

    def timed(ms, n):
        assert len(ms) == n and all(x >= 0 for x in ms) and ms[-1] > 0, ms

    first = pkg.Gpu(0)
    try:
        render = pkg.Render(first, (64, 64), ROOT, capacity=1 << 16)
        assert render.build_nodes(coords, 5, colours) == want.size
        built = render.read_nodes()
        assert np.array_equal(built, want)
        timed(first.build_timing(), 6)
        assert render.edit_nodes(coords[:50] ^ 1, 5, colours[:50]) >= want.size
        timed(first.edit_timing(), 6)
        render.compact_nodes()
        timed(first.compact_timing(), 6)
        listed, _ = render.list_voxels(5)
        assert 300 - 50 <= listed.shape[0] <= 300 + 50
        timed(first.list_timing(), 5)
        assert (render.sample_voxels(listed, 5) > 0).all()
        timed(first.sample_timing(), 2)
        assert int((render.sample_dense((0, 0, 0), (32, 32, 32), 5) > 0).sum()) == listed.shape[0]
        timed(first.sample_timing(), 2)
        assert pkg.mesh.voxelize(first, v, t, 5)[0].shape[0] > 20
        timed(first.voxelize_timing(), 5)
    finally:
        first.close()

    second = pkg.Gpu(0)
    try:
        render = pkg.Render(second, (64, 64), ROOT, capacity=1 << 16)
        assert render.build_nodes(coords, 5, colours) == want.size
        assert np.array_equal(render.read_nodes(), built)
    finally:
        second.close()


def _pass_case(pkg, seed, n, depth, subdivisions):
    """n random voxels at `depth` (distinct when seed is odd), an edit that removes an eighth of them and puts as many,
    cells to sample and an icosphere, with every pass's reference result"""
    rng = np.random.default_rng(seed)
    side = 1 << depth
    cells = rng.choice(side ** 3, n, replace=False) if seed & 1 else rng.integers(0, side ** 3, n)
    coords = np.stack(np.unravel_index(cells, (side,) * 3), axis=1)
    colours = rng.integers(1, 1 << 24, n)
    ec = np.concatenate([coords[:n // 8], rng.integers(0, side, (n // 8, 3))])  # an eighth goes, as many come
    ecol = np.concatenate([np.zeros(n // 8, dtype=np.int64), rng.integers(1, 1 << 24, n // 8)])
    built = B.build(coords, depth, colours)
    edited = E.edit(built, built.size, ec, depth, ecol)
    compacted = C.compact(edited, edited.size, True)[0]
    listed = L.list_voxels(compacted, compacted.size, depth)
    probes = np.concatenate([listed[0].astype(np.int64), rng.integers(0, side + 2, (64, 3))])
    v, t = pkg.mesh.icosphere(subdivisions, 0.5)
    return {"depth": depth, "coords": coords, "colours": colours, "edit": (ec, ecol), "built": built, "edited": edited,
            "compacted": compacted, "listed": listed, "probes": probes, "sampled": S.sample(compacted, compacted.size, probes, depth)[0],
            "mesh": (v, t), "voxelized": V.voxelize(pkg.mesh.quantize_vertices(v, depth), t, depth)}


def test_pass_workspaces_grow_and_shrink_back_on_one_context(pkg):
    """One context builds, edits, compacts, lists, samples and voxelises a small input (40 voxels at depth 4, an
    icosahedron), then one that passes a scan tile of 4096 items in voxels, groups and triangle-cell pairs (5000 distinct
    voxels and icosphere(3) at depth 6), so the grouped buffers and the tile sums reallocate, then the small one again
    in the larger buffers.  Every result is its reference's."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    small, large = _pass_case(pkg, 40, 40, 4, 0), _pass_case(pkg, 41, 5000, 6, 3)
    assert large["built"].size // 8 > 4096 and large["voxelized"][1].size > 4096 > small["voxelized"][1].size

    def u32(tensor):
        return tensor.cpu().numpy().view(np.uint32)

    gpu = pkg.Gpu(0)
    try:
        render = pkg.Render(gpu, (8, 8), ROOT, capacity=1 << 18)
        for step, case in enumerate((small, large, small)):
            what, depth = f"input {step}", case["depth"]
            render.write_nodes(ROOT)
            assert render.build_nodes(case["coords"], depth, case["colours"]) == case["built"].size, what
            assert_words(render.read_nodes(), case["built"], f"{what}: built")
            assert render.edit_nodes(case["edit"][0], depth, case["edit"][1]) == case["edited"].size, what
            assert_words(render.read_nodes(), case["edited"], f"{what}: edited")
            assert render.compact_nodes() == case["compacted"].size, what
            assert_words(render.read_nodes(), case["compacted"], f"{what}: compacted")
            coords, colours, levels = render.list_voxels(depth, with_levels=True)
            for got, want in zip((coords, colours, levels), case["listed"]):
                assert np.array_equal(u32(got), want), f"{what}: listed"
            assert np.array_equal(u32(render.sample_voxels(case["probes"], depth)), case["sampled"]), f"{what}: sampled"
            got = pkg.mesh.voxelize(gpu, *case["mesh"], depth, with_triangles=True)
            for g, want in zip(got, case["voxelized"]):
                assert np.array_equal(u32(g), want), f"{what}: voxelised"
    finally:
        gpu.close()


def _frames(pkg, gpu, render, n=2):
    """The records of the n-th frame in a row (from the second on the trace claims from stored lists)."""
    for _ in range(n):
        hits = render.render()
        gpu.sync()  # (a lane runs on a stream of its own: torch's copy below would not wait for it)
    return pkg.render.hits_to_numpy(hits)


def test_context_buffers_grow_are_reused_and_go_with_the_context(pkg, O, monu9_words):
    """One context renders 320x192, 512x520 and 320x192 again.  512x520 is 4160 strips and 266 240 items, above the
    schedule slot's floor of 4096 strips and the deferred-ray buffer's floor of 65 536 items: both regrow once, and so
    does every shading scratch buffer; the third size runs in what the second left.  Then the timing ring, the scatter
    buffer and the scan lists, and a second context after the first is closed."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    words = monu9_words
    cap = words.size + 1024
    refs = {}

    def ref(size):  # (computed once per size)
        if size not in refs:
            u = O.make_uniforms(width=size[0], height=size[1], flags=O.F_PAUSE_ADAPTIVE | O.F_SHADOWS)
            want8 = np.floor(np.clip(O.shade_frame(words, u, threads=8), 0, 1) * 255.0 + 0.5).astype(np.int32)
            refs[size] = (u, O.trace_frame(words, u, threads=8), want8, O.secondary_frame(words, u, 2, threads=8))
        return refs[size]

    def shaded_ok(img, want8, what):  # test_shaded_frame's bar
        diff = np.abs(img.astype(np.int32) - want8)
        assert diff[..., 3].max() == 0 and (img[..., 3] == 128).all(), what
        assert diff.max() <= 1, f"{what}: colour off by {diff.max()}"
        assert (diff == 0).mean() > 0.98, what
        assert img[..., :3].any(), what

    first = pkg.Gpu(0)
    try:
        first.set_option(pkg.gpu.OPT_VARIANT, pkg.gpu.VARIANT_STACK)
        render = pkg.Render(first, (320, 192), words, capacity=cap)
        first_frame = None
        for step, size in enumerate(((320, 192), (512, 520), (320, 192))):
            W, H = size
            what = f"size {step}: {W}x{H}"
            u, want, want8, (oprim, osec) = ref(size)
            set_uniforms_from_oracle(render, u)
            got = _frames(pkg, first, render)
            assert_hits_equal(got, want, what)
            if first_frame is None:
                first_frame = got.copy()
            for fused in (0, 1):  # 0: aux, ray, skip and shadow scratch, schedule slot 1; 1: the shadow records alone
                first.set_option(pkg.gpu.OPT_FUSED_SHADOWS, fused)
                for _ in range(2):
                    hits, img = render.render_host(rgba=True)
                assert_hits_equal(hits, want, f"{what}: records under shading, fused {fused}")
                shaded_ok(img, want8, f"{what}: shaded frame, fused {fused}")
                # the image alone: the records stay in the context's scratch
                rgba = render.alloc_rgba(W * H)
                first.check(pkg._lib.lib().svo_render(first._h, W, H, 0, 0, W, H, None, rgba.data_ptr()))
                first.sync()
                assert np.array_equal(rgba.cpu().numpy().view(np.uint8).reshape(H, W, 4), img), f"{what}: image without records, fused {fused}"
                for _ in range(2):
                    prim, sec = render.render_secondary(2)
                    first.sync()
                assert_hits_equal(pkg.render.hits_to_numpy(prim), oprim, f"{what}: primary records of the secondary call, fused {fused}")
                assert_hits_equal(pkg.render.hits_to_numpy(sec).reshape(2, H, W), osec, f"{what}: secondary rays, fused {fused}")
            first.set_option(pkg.gpu.OPT_FUSED_SHADOWS, 2)
            assert_hits_equal(render.render_host(), _frames(pkg, first, render, 1), f"{what}: render_host")

        # the timing ring: only ever longer, restarted by every change
        for slots, frames in ((2, 5), (4, 3)):
            first.set_option(pkg.gpu.OPT_TIMING, slots)
            _frames(pkg, first, render, frames)
            ms = first.timing_collect()
            assert ms.size == min(slots, frames) and (ms > 0).all(), (slots, frames, ms)
        first.set_option(pkg.gpu.OPT_TIMING, 0)
        with pytest.raises(pkg.SvoError):
            first.timing_collect()

        # the scatter buffer, grown once: into the spare words behind the tree
        rng = np.random.default_rng(7)
        tail = np.zeros(1024, dtype=np.uint32)
        for n in (8, 64):
            idx = rng.choice(1024, n, replace=False).astype(np.uint32)
            vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            render.scatter_nodes(idx + words.size, vals)
            tail[idx] = vals
            assert np.array_equal(render.read_nodes(1024, words.size), tail), f"scatter of {n} words"

        # the scan lists, as test_scan_kernel compares them
        now = render.read_nodes(cap)
        assert np.array_equal(now[:words.size], words)
        compute = pkg.Compute(first, render)
        compute.update(cap)
        sub, unsub = compute.read_lists()
        osub, ounsub = O.scan(now, node_length=cap)
        assert osub[0] > 0 and ounsub[0] > 0
        assert sorted(sub.tolist()) == osub[1:1 + osub[0]].tolist()
        assert sorted(unsub.tolist()) == ounsub[1:1 + ounsub[0]].tolist()
    finally:
        first.close()

    second = pkg.Gpu(0)
    try:
        second.set_option(pkg.gpu.OPT_VARIANT, pkg.gpu.VARIANT_STACK)
        render = pkg.Render(second, (320, 192), words, capacity=cap)
        set_uniforms_from_oracle(render, ref((320, 192))[0])
        assert_hits_equal(_frames(pkg, second, render, 1), first_frame, "second context")
    finally:
        second.close()


def test_shared_node_store_outlives_its_contexts_in_either_order(pkg, O, small_words, monu9_words):
    """The store goes with the last context bound to it: lanes go on tracing after the owner's context is closed, and
    the owner after its lane's."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cap = max(monu9_words.size, small_words.size)
    u = O.make_uniforms(width=320, height=192, flags=O.F_PAUSE_ADAPTIVE)
    want = O.trace_frame(monu9_words, u, threads=8)
    opened = []

    def context(stream=None):
        g = pkg.Gpu(0, stream=stream.cuda_stream if stream is not None else None)
        opened.append(g)
        g.set_option(pkg.gpu.OPT_VARIANT, pkg.gpu.VARIANT_STACK)
        return g

    def lane_of(owner):
        g = context(torch.cuda.Stream())
        lane = pkg.Render.share_nodes(g, owner)
        set_uniforms_from_oracle(lane, u)
        return g, lane

    try:
        # the owner goes first, then one lane, then the other
        g0 = context()
        owner = pkg.Render(g0, (320, 192), monu9_words, capacity=cap)
        set_uniforms_from_oracle(owner, u)
        ga, lane_a = lane_of(owner)
        gb, lane_b = lane_of(owner)
        for g, r, what in ((g0, owner, "owner"), (ga, lane_a, "lane A"), (gb, lane_b, "lane B")):
            assert_hits_equal(_frames(pkg, g, r), want, what)
        g0.close()
        assert_hits_equal(_frames(pkg, ga, lane_a), want, "lane A after the owner's context is closed")
        assert_hits_equal(_frames(pkg, gb, lane_b), want, "lane B after the owner's context is closed")
        ga.close()
        assert_hits_equal(_frames(pkg, gb, lane_b), want, "lane B after lane A's context is closed")
        gb.close()

        # the lane goes first
        g0 = context()
        owner = pkg.Render(g0, (320, 192), monu9_words, capacity=cap)
        set_uniforms_from_oracle(owner, u)
        ga, lane_a = lane_of(owner)
        assert_hits_equal(_frames(pkg, ga, lane_a), want, "lane")
        ga.close()
        assert_hits_equal(_frames(pkg, g0, owner), want, "owner after the lane's context is closed")
        padded = np.zeros(cap, dtype=np.uint32)
        padded[:small_words.size] = small_words
        owner.write_nodes(padded)
        assert_hits_equal(_frames(pkg, g0, owner), O.trace_frame(padded, u, threads=8), "owner after its upload")
    finally:
        for g in opened:
            g.close()


DEEP = B.build([[0, 0, 0]], 20)  # one voxel at depth 20: 160 words


def _deep_frame(pkg, gpu, render, octree_depth):
    """update() with Settings.octree_depth, then one 8x8 frame from 1e-5 inside the cube's low corner, looking at the
    voxel there (the oracle finds it with two of these rays): they go down all 20 levels, which svo_sync refuses under a
    lower SVO_OPT_TREE_DEPTH.  Returns the records."""
    render.set_flags(pause_adaptive=True, shadows=False)
    render.update(pkg.Settings(octree_depth=octree_depth), pkg.Character(pos=(-0.99999,) * 3, look=(-1.0, -1.0, -1.0)))
    hits = render.render()
    gpu.sync()
    got = pkg.render.hits_to_numpy(hits)
    assert (got["info"] >> 16 & 1).any(), "no ray of the frame hit the depth-20 voxel: the frame does not test the depth"
    return got


def test_a_render_does_not_lower_the_depth_its_gpu_holds(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    gpu = pkg.Gpu(0)
    try:
        assert gpu.tree_depth == 16
        gpu.set_option(pkg.gpu.OPT_TREE_DEPTH, 20)
        render = pkg.Render(gpu, (8, 8), DEEP, capacity=1024)
        assert DEEP.size == 160 and gpu.tree_depth == 20
        _deep_frame(pkg, gpu, render, 18)
        assert gpu.tree_depth == 20
        _deep_frame(pkg, gpu, render, 21)  # (raising is still the wrapper's to do)
        assert gpu.tree_depth == 21
    finally:
        gpu.close()


def test_a_second_render_on_the_gpu_does_not_lower_it_either(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    gpu = pkg.Gpu(0)
    try:
        first = pkg.Render(gpu, (8, 8), ROOT, capacity=1024)
        assert first.build_nodes([[0, 0, 0]], 20) == DEEP.size and gpu.tree_depth == 20
        second = pkg.Render(gpu, (8, 8), DEEP, capacity=1024)
        _deep_frame(pkg, gpu, second, 17)
        assert gpu.tree_depth == 20
    finally:
        gpu.close()


def test_a_voxel_list_builds_the_same_tree_however_it_comes_in(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(21)
    coords, colours = rng.integers(0, 32, (64, 3)), rng.integers(1, 1 << 24, 64)
    want = B.build(coords, 5, colours)
    gpu = pkg.Gpu(0)
    try:
        render = pkg.Render(gpu, (8, 8), ROOT, capacity=4096)
        forms = {"numpy int64": (coords.astype(np.int64), colours.astype(np.int64)),
                 "torch int32 on the device": (torch.as_tensor(coords, dtype=torch.int32, device=gpu.torch_device),
                                               torch.as_tensor(colours, dtype=torch.int32, device=gpu.torch_device)),
                 "torch int64 on the CPU": (torch.as_tensor(coords, dtype=torch.int64), torch.as_tensor(colours, dtype=torch.int64))}
        for what, (xyz, col) in forms.items():
            render.write_nodes(ROOT)
            assert render.build_nodes(xyz, 5, col) == want.size, what
            assert render.read_nodes(want.size).tobytes() == want.tobytes(), what
    finally:
        gpu.close()
