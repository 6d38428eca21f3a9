"""A resting view's static deal on the GPU (SVO_OPT_STATIC_DEAL): the frames the replay kernel traces from its table
are the frames the claiming kernel traces -- bit for bit, on every frame of the learning and after it -- and the table holds every
strip exactly once.  The hit buffer is poisoned before every frame: a strip no wave traced leaves poison.  Small frames of the
depth-10 terrain (camera inside the cube: no culling pass, so the lists are the stored ones) and of small.vox."""
import numpy as np
import pytest

from conftest import assert_hits_equal, set_uniforms_from_oracle

pytestmark = pytest.mark.gpu

LIST_LEARN, DEAL_LEARN = 16, 16  # kBalanceLearnFrames, kDealLearnFrames
SETTLE = 1 + LIST_LEARN          # the frame that builds the lists, then the frames that learn their shares


@pytest.fixture
def dgpu(pkg):
    """a context of the test's own: the options it sets stay here, and the deal's counters start at zero"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg.Gpu(0)
    g.set_option(pkg.gpu.OPT_VARIANT, pkg.gpu.VARIANT_STACK)
    yield g
    g.close()


@pytest.fixture(scope="module")
def off_gpu(pkg):
    """a context with the option off: the claiming kernel's frames"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg.Gpu(0)
    g.set_option(pkg.gpu.OPT_VARIANT, pkg.gpu.VARIANT_STACK)
    g.set_option(pkg.gpu.OPT_STATIC_DEAL, 0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def scene(pkg, O):
    """the terrain, two cameras inside it, and the oracle's frames (computed once, never written to)"""
    cam, look = pkg.scenes.terrain_camera(0, 10)
    words = pkg.scenes.terrain(seed=0, max_depth=10, cam=cam, lod_c=150.0, max_words=2_000_000)
    cam_b = (cam[0] + 0.013, cam[1] + 0.004, cam[2] - 0.009)
    frames = {}

    def want(size, which="a"):
        key = (size, which)
        if key not in frames:
            u = O.make_uniforms(pos=cam if which == "a" else cam_b, look=look, width=size[0], height=size[1], flags=O.F_PAUSE_ADAPTIVE)
            rec = O.trace_frame(words, u, threads=8)
            rec.setflags(write=False)
            frames[key] = (u, rec)
        return frames[key]
    return words, want


class Frames:
    """a Render whose every frame goes into a poisoned buffer and is compared with the records wanted"""

    def __init__(self, pkg, gpu, words, size, u):
        self.pkg, self.gpu = pkg, gpu
        self.render = pkg.Render(gpu, size, words, capacity=max(words.size, 1024))
        set_uniforms_from_oracle(self.render, u)
        self.buf = None

    def look(self, u):
        set_uniforms_from_oracle(self.render, u)

    def trace(self, n, want, what, tiles=None):
        want32 = np.ascontiguousarray(want).reshape(-1).view(np.uint32)
        for k in range(n):
            if self.buf is None or self.buf.numel() != want32.size:
                self.buf = self.render.alloc_hits(want32.size // 4)
            self.buf.fill_(-1)  # 0xFF bytes
            if tiles:
                self.render.render_tiles(*tiles, hits=self.buf)
            else:
                self.render.render(hits=self.buf)
            self.gpu.sync()
            got = self.pkg.render.hits_to_numpy(self.buf)
            if not np.array_equal(got.reshape(-1).view(np.uint32), want32):
                assert_hits_equal(got, want, f"{what}, frame {k}")  # (says where)
                raise AssertionError(f"{what}, frame {k}: records differ")


def check_table(status, n_strips):
    rows = [r[:list(r).index(0xFFFFFFFF)] for r in status["table"]]
    assert sorted(int(s) for r in rows for s in r) == list(range(n_strips)), "the table does not hold every strip exactly once"


def reference(pkg, off_gpu, scene, size, which="a", tiles=None):
    """the frame as the oracle and as the claiming kernel (option off) give it"""
    words, want = scene
    u, rec = want(size, which)
    if tiles:
        tw, th, first, stride = tiles
        tx = size[0] // tw
        rec = np.stack([rec[(t // tx) * th:(t // tx + 1) * th, (t % tx) * tw:(t % tx + 1) * tw] for t in range(first, tx * (size[1] // th), stride)])
    off = Frames(pkg, off_gpu, words, size, u)
    off.trace(SETTLE + 2, rec, "option off", tiles)
    assert off_gpu.deal_status()["replayed"] == 0
    return words, u, rec


def test_resting_frame_replays_bit_exact_and_deals_every_strip_once(pkg, dgpu, off_gpu, scene):
    size = (512, 256)  # 2 048 strips: fewer than the device has waves, so the grid shrinks
    words, u, rec = reference(pkg, off_gpu, scene, size)
    f = Frames(pkg, dgpu, words, size, u)
    f.trace(SETTLE, rec, "before the deal")
    assert dgpu.deal_status()["replayed"] == 0
    f.trace(DEAL_LEARN, rec, "learning the deal")
    st = dgpu.deal_status(table=True, stamps=True)
    assert st["replayed"] == DEAL_LEARN and st["step"] == DEAL_LEARN and st["verdict"] in (1, 2) and st["device_seeds"] == 1, st
    assert st["rows"] == 4 * 512 and st["row_cap"] >= 4
    check_table(st, 2048)
    assert (st["stamps"][:, 1] != 0).all()  # every wave left its end stamp
    f.trace(3, rec, "resting")
    after = dgpu.deal_status()
    # a view whose replay never beat its claims is traced by the claiming kernel again, from the frame the host has seen that on
    assert after["replayed"] == DEAL_LEARN + (3 if st["verdict"] == 1 else 0) and after["claims"] == (st["verdict"] == 2), after
    assert after["moves"] == st["moves"] and after["step"] == DEAL_LEARN


def test_rows_beyond_the_cap_stay_with_claims(pkg, dgpu, off_gpu, scene):
    size = (512, 256)
    words, u, rec = reference(pkg, off_gpu, scene, size)
    dgpu.set_option(pkg.gpu.OPT_GRID_BLOCKS, 8)  # 2 048 strips on 32 waves
    try:
        f = Frames(pkg, dgpu, words, size, u)
        f.trace(SETTLE + 3, rec, "8 workgroups")
        st = dgpu.deal_status()
        assert st["replayed"] == 0 and st["seeded"] == 0, st
    finally:
        dgpu.set_option(pkg.gpu.OPT_GRID_BLOCKS, 0)


def test_frame_with_fewer_strips_than_waves(pkg, dgpu, off_gpu, scene):
    size = (64, 64)  # 64 strips on 64 waves, 8 a list: the shares leave some rows empty
    words, u, rec = reference(pkg, off_gpu, scene, size)
    f = Frames(pkg, dgpu, words, size, u)
    f.trace(SETTLE + DEAL_LEARN + 3, rec, "64 x 64")
    st = dgpu.deal_status(table=True)
    assert st["step"] == DEAL_LEARN and st["replayed"] >= DEAL_LEARN, st
    check_table(st, 64)


def test_small_vox_seen_from_outside_is_never_replayed(pkg, dgpu, O, small_words):
    # the default camera stands outside the cube: the culling pass builds this frame's lists, there are no stored ones to deal from
    u = O.make_uniforms(width=256, height=256, flags=O.F_PAUSE_ADAPTIVE)
    rec = O.trace_frame(small_words, u, threads=4)
    f = Frames(pkg, dgpu, small_words, (256, 256), u)
    f.trace(SETTLE + 3, rec, "small.vox")
    st = dgpu.deal_status()
    assert st["replayed"] == 0 or st["seeded"] == 1, st


def test_camera_move_resize_and_tree_write_drop_the_table(pkg, dgpu, off_gpu, scene):
    size = (256, 128)
    words, u, rec = reference(pkg, off_gpu, scene, size)
    _, want = scene
    u_b, rec_b = want(size, "b")
    f = Frames(pkg, dgpu, words, size, u)
    f.trace(SETTLE + DEAL_LEARN + 2, rec, "camera a")
    st = dgpu.deal_status()
    assert st["seeds"] == 1 and st["step"] == DEAL_LEARN and st["replayed"] >= DEAL_LEARN, st
    f.look(u_b)
    f.trace(1, rec_b, "camera b, first frame")
    assert dgpu.deal_status()["seeded"] == 0
    f.trace(DEAL_LEARN + 2, rec_b, "camera b, at rest")
    st = dgpu.deal_status(table=True)
    # (the lists of the first frame at rest were built under the motion floor; the exact ones that follow differ, and the compare
    # on the device then seeds once more)
    assert st["seeds"] == 2 and st["device_seeds"] in (2, 3) and st["step"] == DEAL_LEARN, st
    check_table(st, 512)
    # a write to the node buffer (one word, the value it has): the lists are rebuilt and the deal starts over
    f.render.scatter_nodes(np.array([0], dtype=np.uint32), words[:1])
    f.trace(1, rec_b, "after the write")
    assert dgpu.deal_status()["seeded"] == 0
    f.trace(3, rec_b, "after the write, at rest")
    assert dgpu.deal_status()["seeds"] == 3
    # another frame size: a new layout, new lists, and in time a new table
    size2 = (512, 256)
    u2, rec2 = want(size2, "a")
    f.look(u2)
    f.trace(SETTLE, rec2, "resized")
    assert dgpu.deal_status()["seeds"] == 3
    f.trace(3, rec2, "resized, settled")
    st = dgpu.deal_status(table=True)
    assert st["seeds"] == 4 and st["rows"] == 4 * 512, st
    check_table(st, 2048)
    # the option off drops it, too
    dgpu.set_option(pkg.gpu.OPT_STATIC_DEAL, 0)
    f.trace(2, rec2, "option off")
    st = dgpu.deal_status()
    assert st["seeded"] == 0
    dgpu.set_option(pkg.gpu.OPT_STATIC_DEAL, 1)


def test_backstop_rebuild_keeps_the_learned_deal(pkg, dgpu, off_gpu, scene):
    size = (256, 128)
    words, u, rec = reference(pkg, off_gpu, scene, size)
    f = Frames(pkg, dgpu, words, size, u)
    f.trace(SETTLE + DEAL_LEARN + 1, rec, "learning")
    learnt = dgpu.deal_status(table=True)
    f.trace(70, rec, "resting past the schedule's 64-frame backstop")
    st = dgpu.deal_status(table=True)
    assert st["seeds"] == 1 and st["device_seeds"] == 1 and st["step"] == DEAL_LEARN and st["moves"] == learnt["moves"], st
    assert np.array_equal(st["table"], learnt["table"]) and st["learn_left"] == 0
    if learnt["verdict"] == 1:
        assert st["replayed"] == learnt["replayed"] + 70


def test_tiles_of_a_sharded_frame(pkg, dgpu, off_gpu, scene):
    size, tiles = (256, 128), (64, 64, 0, 2)  # rank 0 of 2: four 64 x 64 tiles, 256 strips
    words, u, rec = reference(pkg, off_gpu, scene, size, tiles=tiles)
    f = Frames(pkg, dgpu, words, size, u)
    f.trace(SETTLE + DEAL_LEARN + 3, rec, "tiles", tiles)
    st = dgpu.deal_status(table=True)
    assert st["step"] == DEAL_LEARN and st["replayed"] >= DEAL_LEARN, st
    check_table(st, 256)
