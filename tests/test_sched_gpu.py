"""The device half of the strip schedule against tests/sched_ref.py, through Gpu.schedule_status: the
cost classes post_kernel measures against the oracle's step counts, the eight lists strip_hist_kernel + strip_order_kernel build
against the restatement from the device's own classes and shares (and, without it: every strip in exactly one list, classes
never rising along a list, no list beyond its cap), over the sixteen learning frames of a resting view, with culled and
skipped strips left out, under the motion floor, and for tiles.  Records do not depend on the schedule, so nothing else sees a
mistake here.  Exact integers only: no test looks at a time."""
import math

import numpy as np
import pytest

import sched_ref as S
from conftest import assert_hits_equal, set_uniforms_from_oracle
from pass_frame import own_gpu  # noqa: F401  (a context of this module's own: the options set here stay here)

pytestmark = pytest.mark.gpu

EQUAL = [8192 * k for k in range(9)]
OUTSIDE = ((0.2, 0.1, -1.2), (0.0, 0.0, 1.0))   # close: the cube fills most of the frame
SKY_AROUND = ((0.3, 0.2, -3.0), (0.0, 0.0, 1.0))  # a cube with sky all around
LOOKING_AWAY = ((1.5, 0.0, 0.0), (1.0, 0.0, 0.0))  # the cube lies behind the camera: every ray misses it


@pytest.fixture
def sgpu(pkg, own_gpu):
    """the module's context, STACK variant, every option a test may touch back at its default afterwards"""
    G = pkg.gpu
    own_gpu.set_option(G.OPT_VARIANT, G.VARIANT_STACK)
    own_gpu.set_option(G.OPT_SCHEDULE, 2)  # (drops what the test before left in the slots: every test starts a layout anew)
    yield own_gpu
    own_gpu.sync()
    for opt, v in ((G.OPT_CULL, 2), (G.OPT_FUSED_SHADOWS, 2), (G.OPT_BLOCK_SHAPE, 3), (G.OPT_SCHEDULE_MOTION, 0x1204), (G.OPT_SCHEDULE, 2)):
        own_gpu.set_option(opt, v)


@pytest.fixture(scope="module")
def terrain(pkg):
    """the depth-10 terrain and a grazing pose inside the cube (no culling pass: the lists are the stored ones)"""
    cam, look = pkg.scenes.terrain_camera(0, 10)
    words = pkg.scenes.terrain(seed=0, max_depth=10, cam=cam, lod_c=150.0, max_words=2_000_000)
    words.setflags(write=False)
    return words, cam, look


class View:
    """a Render and a record buffer that is poisoned before every frame"""

    def __init__(self, pkg, gpu, words, u, n_records=None):
        self.pkg, self.gpu = pkg, gpu
        size = (int(u.dimensions[0]), int(u.dimensions[1]))
        self.render = pkg.Render(gpu, size, words, capacity=max(words.size, 1024))
        set_uniforms_from_oracle(self.render, u)
        self.buf = self.render.alloc_hits(n_records if n_records is not None else size[0] * size[1])

    def frame(self, poison=True, what="", **how):
        """trace one frame (how: tiles=(tw, th, first, stride) or rgba=tensor) and return its records; poison left behind
        means that a strip was in no list"""
        if poison:
            self.buf.fill_(-1)  # 0xFF bytes
        if "tiles" in how:
            self.render.render_tiles(*how["tiles"], hits=self.buf)
        else:
            self.render.render(hits=self.buf, rgba=how.get("rgba"))
        self.gpu.sync()
        got = self.pkg.render.hits_to_numpy(self.buf)
        left = np.flatnonzero(got["info"] == 0xFFFFFFFF)
        assert left.size == 0, f"{what}: {left.size} records were never written (a dropped strip), first {left[:4].tolist()}"
        return got


def blocks(w, h, bw_log2=3):
    return -(-w // (1 << bw_log2)) * -(-h // (64 >> bw_log2))


def test_a_slot_without_buffers_is_refused(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg.Gpu(0)  # (a context that has traced nothing, so not the module's)
    try:
        for slot in (0, 1):
            with pytest.raises(pkg._lib.SvoError, match="no buffers"):
                g.schedule_status(slot)
    finally:
        g.close()


# ---- cost classes against the oracle ----

def measured_frame(view, gpu, pkg, **how):
    """Trace, drop the schedule, trace the same view again into the same records: a ray the second frame defers to the post
    pass then has its final record in place when the classes are measured, and that frame had no schedule to reuse."""
    view.frame(**how)
    gpu.set_option(pkg.gpu.OPT_SCHEDULE, 2)
    got = view.frame(poison=False, **how)
    return got, gpu.schedule_status()


PARTIAL = (197, 131)  # 25 x 17 blocks of 8 x 8, 13 x 33 of 16 x 4: the last column and the last row are partial at both shapes


def partial_on_both_edges(size, shape):
    return size[0] % (1 << shape) != 0 and size[1] % (64 >> shape) != 0


@pytest.mark.parametrize("size,shape", [((256, 256), 3), ((200, 136), 3), (PARTIAL, 3), ((256, 256), 4), ((200, 136), 4), (PARTIAL, 4)])
def test_cost_classes_match_the_oracle(pkg, sgpu, O, monu9_words, size, shape):
    """256 x 256: whole blocks.  200 x 136: 25 x 17 whole blocks of 8 x 8, and 13 x 34 of 16 x 4 whose last column is half a block.
    197 x 131: blocks that the frame cuts on the right and at the bottom at both shapes -- the pixels such a block does not have
    must count nothing."""
    assert partial_on_both_edges(size, shape) == (size == PARTIAL)
    sgpu.set_option(pkg.gpu.OPT_CULL, 0)
    sgpu.set_option(pkg.gpu.OPT_BLOCK_SHAPE, shape)
    u = O.make_uniforms(pos=OUTSIDE[0], look=OUTSIDE[1], width=size[0], height=size[1], flags=O.F_PAUSE_ADAPTIVE)
    want = O.trace_frame(monu9_words, u, threads=8)
    got, st = measured_frame(View(pkg, sgpu, monu9_words, u), sgpu, pkg)
    assert_hits_equal(got, want, f"{size}, blocks 2^{shape} wide")
    classes = S.cost_classes(want, shape)
    assert st["n_strips"] == blocks(*size, shape) == classes.size and st["cap"] == S.list_cap(classes.size)
    assert len(np.unique(classes)) > 8, "the view should spread over the classes"
    bad = np.flatnonzero(st["classes"] != classes)
    assert bad.size == 0, f"{bad.size} strips' classes differ, first {bad[:8].tolist()}: got {st['classes'][bad[:8]].tolist()} want {classes[bad[:8]].tolist()}"
    assert st["bpr"] == -(-size[0] // (1 << shape))  # one rectangle: ranked column by column
    S.check_stored_lists(st, f"{size}")


@pytest.mark.parametrize("size", [(200, 136), PARTIAL])
def test_cost_classes_of_a_shaded_frame_add_the_shadow_rays(pkg, sgpu, O, monu9_words, size):
    """fused shadow rays: a lane's chain is the primary ray plus its shadow ray, and so is its cost; whole blocks, and blocks cut
    on the right and at the bottom"""
    import torch
    sgpu.set_option(pkg.gpu.OPT_CULL, 0)
    sgpu.set_option(pkg.gpu.OPT_FUSED_SHADOWS, 1)
    W, H = size
    assert partial_on_both_edges(size, 3) == (size == PARTIAL)
    u = O.make_uniforms(pos=OUTSIDE[0], look=OUTSIDE[1], width=W, height=H, flags=O.F_PAUSE_ADAPTIVE | O.F_SHADOWS)
    prim, sec = O.secondary_frame(monu9_words, u, 1, threads=8)
    view = View(pkg, sgpu, monu9_words, u)
    img = torch.empty(W * H, dtype=torch.int32, device=view.buf.device)
    got, st = measured_frame(view, sgpu, pkg, rgba=img)
    assert_hits_equal(got, prim, "shaded frame, primary records")
    classes, alone = S.cost_classes(prim, 3, shadow=sec[0]), S.cost_classes(prim, 3)
    assert (classes != alone).sum() > 20, "the shadow rays should change classes on this view"
    assert np.array_equal(st["classes"], classes)
    S.check_stored_lists(st, "shaded")


def test_cost_classes_of_explicit_rays_with_a_ragged_last_strip(pkg, sgpu, O, monu9_words):
    import torch
    rng = np.random.default_rng(5)
    n = 1000  # 15 strips and 40 rays
    d = rng.normal(size=(n, 3))
    rays = np.concatenate([rng.uniform(-0.9, 0.9, (n, 3)), d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)
    want, u = O.trace_rays(monu9_words, rays, flags=O.F_PAUSE_ADAPTIVE), O.make_uniforms(width=64, height=64, flags=O.F_PAUSE_ADAPTIVE)
    view = View(pkg, sgpu, monu9_words, u, n_records=n)
    dev = torch.from_numpy(rays).to(view.buf.device)
    for k in range(2):
        if k:
            sgpu.set_option(pkg.gpu.OPT_SCHEDULE, 2)
        view.render.trace_rays(dev, hits=view.buf)
        sgpu.sync()
    assert_hits_equal(pkg.render.hits_to_numpy(view.buf), want, "explicit rays")
    st = sgpu.schedule_status()
    assert st["n_strips"] == 16 and st["bpr"] == 0
    assert np.array_equal(st["classes"], S.cost_classes(want))
    S.check_stored_lists(st, "explicit rays")


# ---- the lists against the restatement, from the device's own classes and shares ----

@pytest.mark.parametrize("size", [(8, 8), (504, 8), (512, 8), (520, 8), (256, 256), (512, 512), (136, 1928), (1920, 1080)],
                         ids=lambda s: f"{blocks(*s)}_strips")
def test_lists_match_the_restatement(pkg, sgpu, O, terrain, size):
    """1 strip; 63, 64, 65 (a wave's width); 1 024; 4 096 and 4 097 = 17 x 241 (the builder's chunk grows from 64 strips to 128:
    two of a workgroup's four waves own nothing); 32 400 (a wave walks several 64-strip groups)"""
    words, cam, look = terrain
    u = O.make_uniforms(pos=cam, look=look, width=size[0], height=size[1], flags=O.F_PAUSE_ADAPTIVE)
    view = View(pkg, sgpu, words, u)
    n = blocks(*size)
    for k in range(3):  # the frame that measures and builds with equal shares, then two that step the shares and rebuild
        view.frame(what=f"{size}, frame {k}")
        st = sgpu.schedule_status()
        assert (st["n_strips"], st["cap"], st["bpr"]) == (n, S.list_cap(n), -(-size[0] // 8)), st
        assert st["valid"] and not st["order_filtered"] and st["balance_frames"] == k
        if k == 0:
            assert st["balance"][:9].tolist() == EQUAL
        S.check_shares(st["balance"])
        S.check_stored_lists(st, f"{size}, frame {k}")
    if n >= 1024:
        assert len(np.unique(st["classes"])) > 8, "the view should spread over the classes"


def test_tiles_are_ranked_in_strip_order(pkg, sgpu, O, terrain):
    words, cam, look = terrain
    u = O.make_uniforms(pos=cam, look=look, width=256, height=128, flags=O.F_PAUSE_ADAPTIVE)
    view = View(pkg, sgpu, words, u, n_records=4 * 64 * 64)
    for k in range(3):
        view.frame(what=f"tiles, frame {k}", tiles=(64, 64, 0, 2))  # rank 0 of 2: four 64 x 64 rectangles
        st = sgpu.schedule_status()
        assert st["n_strips"] == 256 and st["bpr"] == 0
        S.check_stored_lists(st, f"tiles, frame {k}")


def test_a_view_of_sky_only(pkg, sgpu, O, monu9_words):
    """every ray misses the cube: one class, or strips culled before the trace -- the lists hold exactly the others"""
    for cull in (0, 2):
        sgpu.set_option(pkg.gpu.OPT_CULL, cull)
        u = O.make_uniforms(pos=LOOKING_AWAY[0], look=LOOKING_AWAY[1], width=256, height=144, flags=O.F_PAUSE_ADAPTIVE)
        view = View(pkg, sgpu, monu9_words, u)
        for k in range(2):
            got = view.frame(what=f"sky, cull {cull}, frame {k}")
            assert not got["info"].any()
            st = sgpu.schedule_status()
            used = st["classes_now"] if st["order_filtered"] else st["classes"]
            assert set(np.unique(used).tolist()) <= {0, S.OUT} and not st["classes"].any()
            if st["order_filtered"]:  # (lists built before the trace are cut into equal eighths)
                st["balance"] = np.array(EQUAL, dtype=np.uint32)
            S.check_lists(st, used, f"sky, cull {cull}, frame {k}")
            assert int(st["lengths"].sum()) == int((used != S.OUT).sum())


# ---- the learning frames of a resting view ----

def test_learning_frames_keep_every_strip_listed_and_restore_the_best_shares(pkg, sgpu, O, terrain):
    words, cam, look = terrain
    u = O.make_uniforms(pos=cam, look=look, width=256, height=256, flags=O.F_PAUSE_ADAPTIVE)
    view = View(pkg, sgpu, words, u)
    first = kept = None
    for k in range(1 + S.LEARN_FRAMES + 2):
        got = view.frame(what=f"frame {k}")
        first = got if first is None else first
        assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), f"frame {k}: records differ from the first frame's"
        st = sgpu.schedule_status()
        bal = st["balance"]
        S.check_shares(bal)
        S.check_stored_lists(st, f"frame {k}")
        assert st["balance_frames"] == k
        if 1 <= k <= S.LEARN_FRAMES:
            assert bal[20] != 0 and bal[18] <= k, f"frame {k}: no frame time noted"
            S.check_shares(bal[21:30])
        if k == S.LEARN_FRAMES:  # update 16: the shares a resting view keeps are the best ones seen
            assert bal[:9].tolist() == bal[21:30].tolist()
            kept = st
        if k > S.LEARN_FRAMES:
            assert bal[:9].tolist() == kept["balance"][:9].tolist() and np.array_equal(st["lengths"], kept["lengths"])
            assert all(np.array_equal(st["lists"][j, :st["lengths"][j]], kept["lists"][j, :kept["lengths"][j]]) for j in range(8))


# ---- filtered lists: culled and skipped strips ----

def test_culled_strips_are_in_no_list(pkg, sgpu, O, monu9_words):
    sgpu.set_option(pkg.gpu.OPT_CULL, 1)
    W, H = 256, 144
    u = O.make_uniforms(pos=SKY_AROUND[0], look=SKY_AROUND[1], width=W, height=H, flags=O.F_PAUSE_ADAPTIVE)
    want = O.trace_frame(monu9_words, u, threads=8)
    view = View(pkg, sgpu, monu9_words, u)
    n = blocks(W, H)
    measured = None
    for k in range(2):
        assert_hits_equal(view.frame(what=f"culled, frame {k}"), want, f"culled, frame {k}")
        st = sgpu.schedule_status()
        assert st["order_filtered"] and st["n_strips"] == n
        now = st["classes_now"]
        assert np.array_equal(now, sgpu.strip_classes(n))
        culled = now == S.OUT
        assert 64 < culled.sum() < n - 64, "the view should have more than a wave's width of culled and of unculled strips"
        # this frame's lists were built before its trace, in equal eighths: in screen order on the first frame, by the classes
        # the first frame measured on the second
        assert np.array_equal(now, np.where(culled, S.OUT, 0 if measured is None else measured))
        S.check_lists(dict(st, balance=np.array(EQUAL, dtype=np.uint32)), now, f"culled, frame {k}")
        measured = st["classes"].copy()
    assert measured.any()


def skip_views(O, terrain, w, h, flags):
    """the terrain seen from outside (the frame's last pixel is sky: the ragged last strip holds no ray) and from the grazing
    pose inside (it is ground: that strip holds one)"""
    words, cam, look = terrain
    return (("outside", O.make_uniforms(pos=SKY_AROUND[0], look=SKY_AROUND[1], width=w, height=h, flags=flags), True),
            ("inside", O.make_uniforms(pos=cam, look=look, width=w, height=h, flags=flags), False))


def test_skip_mask_with_a_ragged_last_strip(pkg, sgpu, O, terrain):
    """secondary rays as explicit rays with a skip mask (slot 1): 129 x 129 pixels = 260 strips and one slot"""
    sgpu.set_option(pkg.gpu.OPT_FUSED_SHADOWS, 0)
    W = H = 129
    n = W * H
    for name, u, last_empty in skip_views(O, terrain, W, H, O.F_PAUSE_ADAPTIVE):
        render = pkg.Render(sgpu, (W, H), terrain[0], capacity=terrain[0].size)
        set_uniforms_from_oracle(render, u)
        prev = None
        for n_secondary in (1, 1, 2):  # (2: another layout, 521 strips, the last holding two slots)
            hits, _ = render.render_secondary(n_secondary)
            sgpu.sync()
            hit = (pkg.render.hits_to_numpy(hits)["info"] >> 16) & 1
            skip = np.tile(hit == 0, n_secondary).astype(np.uint8)
            st = sgpu.schedule_status(slot=1)
            assert st["order_filtered"] and st["n_strips"] == (n * n_secondary + 63) // 64 and st["bpr"] == 0
            if n_secondary == 2:
                prev = None
            want = S.skip_classes(skip, n * n_secondary, prev)
            assert (want[-1] == S.OUT) == last_empty, f"{name}: the last pixel was meant to {'miss' if last_empty else 'hit'}"
            assert np.array_equal(st["classes_now"], want), f"{name}, {n_secondary} secondary rays"
            S.check_lists(dict(st, balance=np.array(EQUAL, dtype=np.uint32)), want, f"{name}, {n_secondary} secondary rays")
            prev = st["classes"].copy()


def test_shadow_pass_of_a_shaded_frame_skips_its_empty_strips(pkg, sgpu, O, terrain):
    """slot 1 of a shaded two-pass frame: one shadow-ray slot per pixel, skipped where the primary ray hit nothing"""
    import torch
    sgpu.set_option(pkg.gpu.OPT_FUSED_SHADOWS, 0)
    W = H = 129
    prev = None  # (the slot's layout is the same for both views: the second view's first frame is ordered by the first view's costs)
    for name, u, last_empty in skip_views(O, terrain, W, H, O.F_PAUSE_ADAPTIVE | O.F_SHADOWS):
        view = View(pkg, sgpu, terrain[0], u)
        img = torch.empty(W * H, dtype=torch.int32, device=view.buf.device)
        for k in range(2):
            got = view.frame(what=f"{name}, frame {k}", rgba=img)
            skip = (((got["info"] >> 16) & 1) == 0).astype(np.uint8)
            st = sgpu.schedule_status(slot=1)
            want = S.skip_classes(skip, W * H, prev)
            assert st["n_strips"] == 261 and (want[-1] == S.OUT) == last_empty
            assert np.array_equal(st["classes_now"], want), f"{name}, frame {k}"
            S.check_lists(dict(st, balance=np.array(EQUAL, dtype=np.uint32)), want, f"{name}, frame {k}")
            prev = st["classes"].copy()


# ---- the motion floor ----

def test_motion_floor_raises_strips_near_long_ones(pkg, sgpu, O, terrain):
    words, cam, look = terrain
    option = 0x1204
    sgpu.set_option(pkg.gpu.OPT_SCHEDULE_MOTION, option)
    W, H = 512, 256
    view, floored, raised = None, 0, 0
    for k in range(7):  # yaw a quarter of a degree a frame
        a = math.radians(0.25 * k)
        lk = (look[0] * math.cos(a) + look[2] * math.sin(a), look[1], look[2] * math.cos(a) - look[0] * math.sin(a))
        u = O.make_uniforms(pos=cam, look=lk, width=W, height=H, flags=O.F_PAUSE_ADAPTIVE)
        if view is None:
            view = View(pkg, sgpu, words, u)
        else:
            set_uniforms_from_oracle(view.render, u)
        view.frame(what=f"yaw, frame {k}")
        st = sgpu.schedule_status()
        if st["floored"] and st["age"] == 0:  # this frame's post pass measured, floored and built
            floored += 1
            want = S.danger_floor(st["classes"], st["bpr"], *S.motion_option(option))
            raised += int((want != st["classes"]).sum())
            assert st["bpr"] == 64 and np.array_equal(st["classes_now"], want), f"frame {k}: floored classes differ"
            S.check_lists(st, st["classes_now"], f"yaw, frame {k}")
        elif st["age"] == 0:
            S.check_stored_lists(st, f"yaw, frame {k}")
    assert floored >= 2, "the moving frames should have been floored"
    assert raised > 0, "the floor raised no strip on this view: the test shows nothing"
