"""The host frame the GPU tree passes share (csrc/svo_ctx.h): one context runs every pass that keeps a
workspace, hands out each pass's times and is closed, which is where all of its owning members are released together;
a second context then builds the same tree."""
import numpy as np
import pytest

import build_ref as B

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
