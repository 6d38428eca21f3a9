"""Every instantiation of the STACK trace kernel against the oracle (csrc/svo_kernels.hip, stack_kernels): the sixteen cells
GE x NS x CNT x SHD of trace_stack_kernel and the two of trace_stack_replay_kernel, each its own code object with its own LDS
layout and its own copy of the walk.

  GE   the >= tie-break               SVO_F_MISC_BOOL
  NS   12, or 18 (deep ancestor stack) SVO_OPT_TREE_DEPTH above 16
  CNT  live hit counters               SVO_F_PAUSE_ADAPTIVE clear
  SHD  fused shadow rays               SVO_F_SHADOWS with SVO_OPT_FUSED_SHADOWS = 1, in a call that shades

The frames are the lattice cameras of tests/trace_matrix_scenes.py: every ray starts on a tie, so > and >= part ways in records
and in counter words (tests/test_trace_matrix_host.py holds the scenes to that).  Which kernel a cell launches is held on the
host: tests/test_trace_choice_host.py drives the one statement of those rules (csrc/svo_sched.h: launch_choice, trace_slot)
over every combination of what they depend on; that the deep instantiation was needed is shown by the same frame being refused
under a declared depth of 16.  The RESTART kernel runs every cell's flags too: a mismatch it does not share is the stack kernel's.

The eight timeline instantiations (DBG, with SVO_OPT_DEBUG_BUFFER set: GE x NS x CNT, there is none with fused shadows)
run the same frames: the same records and counter words, and a timeline that is consistent with the frame."""
import types

import numpy as np
import pytest

import trace_matrix_scenes as S
from conftest import assert_hits_equal, set_uniforms_from_oracle

pytestmark = pytest.mark.gpu

LIST_LEARN, DEAL_LEARN = 16, 16  # kBalanceLearnFrames, kDealLearnFrames (tests/test_deal_gpu.py)
SETTLE = 1 + LIST_LEARN
REPLAY_SIZE = (512, 256)


@pytest.fixture(scope="module")
def mgpu(pkg):
    """the module's context: STACK kernel, strips claimed (no static deal)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg.Gpu(0)
    g.set_option(pkg.gpu.OPT_VARIANT, pkg.gpu.VARIANT_STACK)
    g.set_option(pkg.gpu.OPT_STATIC_DEAL, 0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def wanted(O):
    """the oracle's side of a (depth, flags) frame, computed once and never written to: records, the node words after one
    and two frames (counters live), the shadow ray's records and the shaded image (shadows)"""
    cache = {}

    def want(depth, flags):
        key = (depth, flags)
        if key not in cache:
            sc = S.scene(depth)
            w = types.SimpleNamespace(scene=sc, words=sc.words, u=sc.uniforms(O, flags), flags=flags)
            w.rec = O.trace_frame(sc.words, w.u, threads=8)
            w.nodes = [sc.words, sc.words]
            if not flags & O.F_PAUSE_ADAPTIVE:
                once = O.count_frame(sc.words, w.u)
                w.nodes = [once, O.count_frame(once, w.u)]
                assert (w.nodes[1] & 15).max() == 15
            if flags & O.F_SHADOWS:
                prim, w.sec = O.secondary_frame(sc.words, w.u, 1, threads=8)
                assert np.array_equal(prim.view(np.uint32), w.rec.view(np.uint32))
                w.rgba8 = np.floor(np.clip(O.shade_frame(sc.words, w.u, threads=8), 0, 1) * 255.0 + 0.5).astype(np.int32)
                w.sec.setflags(write=False)
            w.rec.setflags(write=False)
            for n in w.nodes:
                n.setflags(write=False)
            cache[key] = w
        return cache[key]
    return want


def two_frames(pkg, gpu, w, shade, before_frame=None, after_frame=None):
    """Two frames of w's view into poisoned buffers, the second from the first one's schedule and on its counters.
    Returns per frame (records, image or None, node words)."""
    W, H = S.SIZE
    render = pkg.Render(gpu, S.SIZE, w.words, capacity=max(w.words.size, 1024))
    set_uniforms_from_oracle(render, w.u)
    out = []
    for frame in range(2):
        buf = render.alloc_hits(W * H)
        buf.fill_(-1)  # 0xFF bytes: a ray nobody traced keeps them
        rgba = render.alloc_rgba(W * H).fill_(-1) if shade else None
        if before_frame:
            before_frame()
        render.render(hits=buf, rgba=rgba)
        gpu.sync()
        if after_frame:
            after_frame(frame)
        img = rgba.cpu().numpy().view(np.uint8).reshape(H, W, 4) if shade else None
        out.append((pkg.render.hits_to_numpy(buf), img, render.read_nodes(w.words.size)))
    return out


def check_against_oracle(frames, w, what):
    for k, (rec, img, nodes) in enumerate(frames):
        assert_hits_equal(rec, w.rec, f"{what}, frame {k}")
        assert np.array_equal(nodes >> 4, w.words >> 4), f"{what}, frame {k}: pointer bits changed"
        bad = np.flatnonzero(nodes != w.nodes[k])
        assert bad.size == 0, (f"{what}, frame {k}: {bad.size} node words differ; first {bad[:5]}: "
                               f"got {nodes[bad[:5]] & 15} want {w.nodes[k][bad[:5]] & 15}")
        if img is not None:  # test_shaded_frame's bar: pow() differs between libm and the GPU by at most one code value
            diff = np.abs(img.astype(np.int32) - w.rgba8)
            assert diff[..., 3].max() == 0 and (img[..., 3] == 128).all(), f"{what}, frame {k}: alpha"
            assert diff.max() <= 1, f"{what}, frame {k}: colour off by {diff.max()}"
            assert (diff == 0).mean() > 0.98, f"{what}, frame {k}: {(diff == 0).mean():.4f} of the values equal"


def check_same(got, ref, what):
    for k, ((r1, i1, n1), (r0, i0, n0)) in enumerate(zip(got, ref)):
        assert_hits_equal(r1, r0, f"{what}, frame {k}: records")
        assert np.array_equal(n1, n0), f"{what}, frame {k}: {np.count_nonzero(n1 != n0)} node words differ"
        if i1 is not None and i0 is not None:
            assert np.array_equal(i1, i0), f"{what}, frame {k}: images differ"


@pytest.mark.parametrize("shd", [0, 1], ids=["plain", "shd"])
@pytest.mark.parametrize("cnt", [0, 1], ids=["static", "cnt"])
@pytest.mark.parametrize("depth", [16, 17, 21], ids=["ns12_d16", "ns18_d17", "ns18_d21"])
@pytest.mark.parametrize("ge", [0, 1], ids=["gt", "ge"])
def test_cell(pkg, mgpu, O, wanted, ge, depth, cnt, shd):
    G = pkg.gpu
    flags = S.flags_of(O, ge, cnt, shd)
    w = wanted(depth, flags)
    what = f"GE {ge} depth {depth} CNT {cnt} SHD {shd}"
    W, H = S.SIZE
    try:
        mgpu.set_option(G.OPT_TREE_DEPTH, depth)
        mgpu.set_option(G.OPT_FUSED_SHADOWS, 1)
        frames = two_frames(pkg, mgpu, w, shade=bool(shd))
        check_against_oracle(frames, w, what)
        if shd:
            # the shadow ray's own records, from the lane that found the hit
            render = pkg.Render(mgpu, S.SIZE, w.words, capacity=max(w.words.size, 1024))
            set_uniforms_from_oracle(render, w.u)
            prim, sec = render.alloc_hits(W * H).fill_(-1), render.alloc_hits(W * H).fill_(-1)
            render.render_secondary(1, hits=prim, secondary=sec)
            mgpu.sync()
            assert_hits_equal(pkg.render.hits_to_numpy(prim), w.rec, what + ": primary records of the secondary call")
            assert_hits_equal(pkg.render.hits_to_numpy(sec), w.sec[0], what + ": fused shadow records")
            assert np.array_equal(render.read_nodes(w.words.size), w.nodes[0]), what + ": node words after the secondary call"
            # the two-pass form of the same context: generator + explicit rays
            mgpu.set_option(G.OPT_FUSED_SHADOWS, 0)
            two_pass = two_frames(pkg, mgpu, w, shade=True)
            check_same(frames, two_pass, what + ", fused vs two-pass")
        # the general kernel under the same flags
        mgpu.set_option(G.OPT_VARIANT, G.VARIANT_RESTART)
        check_same(two_frames(pkg, mgpu, w, shade=bool(shd)), [(r, None, n) for r, _, n in frames], what + ", RESTART vs STACK")
    finally:
        mgpu.set_option(G.OPT_VARIANT, G.VARIANT_STACK)
        mgpu.set_option(G.OPT_FUSED_SHADOWS, 2)  # the default (automatic)
        mgpu.set_option(G.OPT_TREE_DEPTH, 16)


POISON = 0xAAAAAAAA


def check_timeline(dbg, G, what):
    """the debug buffer after one frame of S.SIZE: rows of waves that did not run keep the poison, every other wave's stamps are
    in order (10 ns ticks, compared as wrapped 32-bit differences), and the waves generated the frame's strips between them"""
    d = dbg.reshape(2, G.DEBUG_WAVES, G.DEBUG_ROW_WORDS)
    ran = (d[0] != POISON).any(axis=1)
    n = int(ran.sum())
    assert n >= 4 and n % 4 == 0 and ran[:n].all(), f"{what}: the rows written are not those of a grid's waves: {np.flatnonzero(ran)[:8]} ... ({n})"
    assert (d[:, n:] == POISON).all(), f"{what}: a row beyond the grid's {n} waves was written"
    row, ev = d[0, :n], d[1, :n]
    assert (row != POISON).all(), f"{what}: a wave left a slot of its row unwritten"
    start, dry, end, enter = row[:, 0], row[:, 1], row[:, 2], ev[:, 0]

    def ordered(a, b):  # a <= b on the wrapping clock
        return (b - a).astype(np.uint32) < 0x80000000
    assert ordered(start, enter).all() and ordered(enter, end).all(), f"{what}: start <= loop entry <= end"
    # (a wave that learned it was dry stored that stamp with bit 0 set: one tick late at most)
    assert ordered(start, dry).all() and ordered(dry & ~np.uint32(1), end).all(), f"{what}: start <= dry <= end"
    gens = row[:, 7]
    print(f"{what}: {n} waves, {int(gens.sum())} generations, rounds {int(row[:, 3].sum())}, slots 12..15 summed {[int(row[:, k].astype(np.uint64).sum()) for k in (12, 13, 14, 15)]}")
    W, H = S.SIZE
    assert W * H % 64 == 0
    assert int(gens.sum()) == W * H // 64, f"{what}: {int(gens.sum())} generations of 64 items for {W * H // 64} strips"
    # the first fourteen generations of a wave left their stamps, the others of the fourteen slots keep the poison
    for k in range(1, 15):
        assert ((ev[:, k] != POISON) == (gens >= k)).all(), f"{what}: generation stamp {k}"


@pytest.mark.parametrize("cnt", [0, 1], ids=["static", "cnt"])
@pytest.mark.parametrize("depth", [16, 17], ids=["ns12_d16", "ns18_d17"])
@pytest.mark.parametrize("ge", [0, 1], ids=["gt", "ge"])
def test_timeline_cell(pkg, mgpu, O, wanted, ge, depth, cnt):
    """trace_stack_kernel<.., DBG = true, CNT, SHD = false>: the plain cell's records and counter words, and its timeline"""
    import torch
    G = pkg.gpu
    w = wanted(depth, S.flags_of(O, ge, cnt, 0))
    what = f"timeline GE {ge} depth {depth} CNT {cnt}"
    dbg = torch.empty(G.DEBUG_BUFFER_WORDS, dtype=torch.int32, device="cuda")
    seen = []
    try:
        mgpu.set_option(G.OPT_TREE_DEPTH, depth)
        mgpu.set_option(G.OPT_DEBUG_BUFFER, dbg.data_ptr())
        frames = two_frames(pkg, mgpu, w, shade=False, before_frame=lambda: dbg.fill_(POISON - (1 << 32)),
                            after_frame=lambda k: seen.append(dbg.cpu().numpy().view(np.uint32).copy()))
        check_against_oracle(frames, w, what)
        for k, d in enumerate(seen):
            check_timeline(d, G, f"{what}, frame {k}")
    finally:
        mgpu.set_option(G.OPT_DEBUG_BUFFER, 0)
        mgpu.sync()
        mgpu.set_option(G.OPT_TREE_DEPTH, 16)


def test_timeline_grid_override_is_cut_back_to_the_buffers_rows(pkg, mgpu, O):
    """SVO_OPT_GRID_BLOCKS beyond DEBUG_WAVES / 4 workgroups while the debug buffer is set: the launch has DEBUG_WAVES waves, every
    row of both regions is theirs, and the words behind the buffer (room for the waves the override asked for) keep the poison"""
    import torch
    G = pkg.gpu
    size = (1024, 1024)  # 16384 strips of 64 pixels: work for 4096 workgroups of four waves, and more would be launched
    asked = G.DEBUG_WAVES // 4 + 1000
    sc = S.scene(16)
    u = sc.uniforms(O, O.F_PAUSE_ADAPTIVE, size=size)
    tail = 2 * 4 * 1000 * G.DEBUG_ROW_WORDS
    dbg = torch.empty(G.DEBUG_BUFFER_WORDS + tail, dtype=torch.int32, device="cuda").fill_(POISON - (1 << 32))
    try:
        mgpu.set_option(G.OPT_GRID_BLOCKS, asked)
        mgpu.set_option(G.OPT_DEBUG_BUFFER, dbg.data_ptr())
        render = pkg.Render(mgpu, size, sc.words, capacity=max(sc.words.size, 1024))
        set_uniforms_from_oracle(render, u)
        render.render()
        mgpu.sync()
    finally:
        mgpu.set_option(G.OPT_DEBUG_BUFFER, 0)
        mgpu.set_option(G.OPT_GRID_BLOCKS, 0)
        mgpu.sync()
    d = dbg.cpu().numpy().view(np.uint32)
    assert (d[G.DEBUG_BUFFER_WORDS:] == POISON).all(), "words behind the buffer were written"
    rows = d[:G.DEBUG_BUFFER_WORDS].reshape(2, G.DEBUG_WAVES, G.DEBUG_ROW_WORDS)
    assert (rows[0] != POISON).all(), "a wave of the cut-back grid left no row"
    assert (rows[1, :, 0] != POISON).all() and (rows[1, :, 15] != POISON).all()
    assert int(rows[0, :, 7].sum()) == size[0] * size[1] // 64


@pytest.mark.parametrize("depth", [17, 21])
@pytest.mark.parametrize("ge", [0, 1], ids=["gt", "ge"])
def test_deep_frame_needs_the_deep_stack(pkg, mgpu, O, wanted, ge, depth):
    """the NS = 18 cells' frame under a declared depth of 16 is refused by sync(), and the honest frame after it is right"""
    G = pkg.gpu
    w = wanted(depth, S.flags_of(O, ge, 0, 0))
    try:
        mgpu.set_option(G.OPT_TREE_DEPTH, 16)
        render = pkg.Render(mgpu, S.SIZE, w.words, capacity=max(w.words.size, 1024))
        set_uniforms_from_oracle(render, w.u)
        render.render()
        with pytest.raises(pkg.SvoError):
            mgpu.sync()
        del render
        mgpu.set_option(G.OPT_TREE_DEPTH, depth)
        check_against_oracle(two_frames(pkg, mgpu, w, shade=False), w, f"depth {depth} GE {ge}, after the refused frame")
    finally:
        mgpu.set_option(G.OPT_TREE_DEPTH, 16)


@pytest.mark.parametrize("variant", [0, 1], ids=["restart", "stack"])
@pytest.mark.parametrize("depth", [17, 21])
def test_deep_lattice_rays(pkg, mgpu, O, depth, variant):
    """test_lattice_rays_ties_and_boundaries below level 16: origins on the depth-D lattice, directions that tie, both
    tie-breaks, through the explicit-ray path of both kernels"""
    import torch
    G = pkg.gpu
    sc = S.scene(depth)
    rays = sc.lattice_rays()
    try:
        mgpu.set_option(G.OPT_TREE_DEPTH, depth)
        mgpu.set_option(G.OPT_VARIANT, variant)
        render = pkg.Render(mgpu, (8, 8), sc.words, capacity=max(sc.words.size, 1024))
        dev = torch.from_numpy(rays).cuda()
        for flags in (O.F_PAUSE_ADAPTIVE, O.F_PAUSE_ADAPTIVE | O.F_MISC_BOOL):
            render.uniforms.flags = flags
            render.upload_uniforms()
            buf = render.alloc_hits(rays.shape[0]).fill_(-1)
            render.trace_rays(dev, hits=buf)
            mgpu.sync()
            want = O.trace_rays(sc.words, rays, flags=flags, threads=8)
            assert_hits_equal(pkg.render.hits_to_numpy(buf), want, f"deep lattice rays, depth {depth} flags {flags}")
            assert np.isin(want["normal_bits"], S.TWO_AXIS_TIES).any(), "the set should contain steps that tie on two axes"
            assert (((want["info"] >> 8) & 0xFF)[want["value"] != 0xFF000000] > 16).any(), "the set should end rays below level 16"
    finally:
        mgpu.set_option(G.OPT_VARIANT, G.VARIANT_STACK)
        mgpu.set_option(G.OPT_TREE_DEPTH, 16)


@pytest.mark.parametrize("ge", [1, 0], ids=["ge", "gt"])
def test_replay_kernel(pkg, O, ge):
    """trace_stack_replay_kernel<..., GE>: a resting lattice view of the depth-16 scene, dealt from the learned table; every
    frame of the settling, of the learning and after it is the oracle's, and frames were replayed"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sc = S.scene(16)
    u = sc.uniforms(O, O.F_PAUSE_ADAPTIVE | (O.F_MISC_BOOL if ge else 0), size=REPLAY_SIZE)
    want = O.trace_frame(sc.words, u, threads=8)
    want32 = np.ascontiguousarray(want).reshape(-1).view(np.uint32)
    g = pkg.Gpu(0)  # a context of the test's own: the static deal on, its counters at zero
    try:
        g.set_option(pkg.gpu.OPT_VARIANT, pkg.gpu.VARIANT_STACK)
        g.set_option(pkg.gpu.OPT_STATIC_DEAL, 1)
        render = pkg.Render(g, REPLAY_SIZE, sc.words, capacity=max(sc.words.size, 1024))
        set_uniforms_from_oracle(render, u)
        buf = render.alloc_hits(want.size)
        for k in range(SETTLE + DEAL_LEARN + 2):
            buf.fill_(-1)
            render.render(hits=buf)
            g.sync()
            got = pkg.render.hits_to_numpy(buf)
            if not np.array_equal(got.view(np.uint32).reshape(-1), want32):
                assert_hits_equal(got, want, f"replay GE {ge}, frame {k}")  # (says where)
                raise AssertionError(f"replay GE {ge}, frame {k}: records differ")
        st = g.deal_status()
        assert st["replayed"] > 0, st
    finally:
        g.close()
