"""The inputs of the trace-kernel matrix (tests/trace_matrix_scenes.py) can tell a wrong kernel from a right one: conditions on
the scenes, checked on the CPU oracle alone.  A tie-break that went wrong changes records and counter words; the deep trees end
rays below the default stack's last level; the sun leaves enough pixels on either side of the shadow test; some ray runs into
the step limit; and two frames saturate a counter.  Each test prints the counts it measured (pytest -s shows them)."""
import numpy as np
import pytest

import trace_matrix_scenes as S

STEP_LIMIT = 0xFF000000


@pytest.fixture(scope="module", params=S.DEPTHS, ids=lambda d: f"depth{d}")
def scene(request):
    return S.scene(request.param)


def hit_bit(rec):
    return ((rec["info"] >> 16) & 1).astype(bool)


def test_tree_is_small_and_as_deep_as_it_says(pkg, scene):
    n = scene.words.size
    print(f"depth {scene.depth}: {scene.coords.shape[0]} voxels, {n} words")
    assert 2000 <= n <= 5000
    assert pkg.scenes.max_depth(scene.words) == scene.depth


def test_tie_break_changes_records(O, scene):
    gt = O.trace_frame(scene.words, scene.uniforms(O, O.F_PAUSE_ADAPTIVE), threads=4).reshape(-1)
    ge = O.trace_frame(scene.words, scene.uniforms(O, O.F_PAUSE_ADAPTIVE | O.F_MISC_BOOL), threads=4).reshape(-1)
    differ = int(np.count_nonzero((gt.view(np.uint32).reshape(-1, 4) != ge.view(np.uint32).reshape(-1, 4)).any(axis=1)))
    print(f"depth {scene.depth}: {differ} of {gt.size} rays' records differ between > and >=")
    assert differ >= 20


@pytest.mark.parametrize("shadows", [False, True], ids=["primary", "shadows"])
def test_tie_break_changes_counters(O, scene, shadows):
    base = O.F_SHADOWS if shadows else 0
    gt = O.count_frame(scene.words, scene.uniforms(O, base))
    ge = O.count_frame(scene.words, scene.uniforms(O, base | O.F_MISC_BOOL))
    assert np.array_equal(gt >> 4, scene.words >> 4) and np.array_equal(ge >> 4, scene.words >> 4)
    differ = int(np.count_nonzero(gt != ge))
    print(f"depth {scene.depth}, shadows {shadows}: {differ} counter words differ between > and >=")
    assert differ >= 50


@pytest.mark.parametrize("ge", [0, 1])
def test_rays_end_below_the_default_stack(O, scene, ge):
    rec = O.trace_frame(scene.words, scene.uniforms(O, S.flags_of(O, ge, 0, 0)), threads=4).reshape(-1)
    steps, depth = rec["info"] & 0xFF, (rec["info"] >> 8) & 0xFF
    limit = rec["value"] == STEP_LIMIT
    assert (steps[limit] == 101).all() and (depth[limit] == 100).all()
    deep = float(np.count_nonzero((depth > 16) & ~limit)) / rec.size
    print(f"depth {scene.depth}, ge {ge}: {deep:.1%} of the rays end below level 16, {int(limit.sum())} at the step limit, "
          f"deepest {int(depth[~limit].max())}")
    if not ge:  # (under >= the depth-21 frame has none: the condition is on the scene, and > meets it in all four)
        assert limit.any(), "no ray reaches the step limit"
    assert int(depth[~limit].max()) == scene.depth
    if scene.depth > 16:
        assert deep >= 0.25
    else:
        assert deep == 0.0


@pytest.mark.parametrize("ge", [0, 1])
def test_shadow_test_has_both_outcomes(O, scene, ge):
    u = scene.uniforms(O, S.flags_of(O, ge, 0, 1))
    prim, sec = O.secondary_frame(scene.words, u, 1, threads=4)
    hit = hit_bit(prim) & (prim["value"] != STEP_LIMIT)
    shadowed = hit & hit_bit(sec[0])
    lit = hit & ~hit_bit(sec[0])
    print(f"depth {scene.depth}, ge {ge}: {int(lit.sum())} lit / {int(shadowed.sum())} shadowed hit pixels")
    assert lit.sum() >= 100 and shadowed.sum() >= 100


@pytest.mark.parametrize("ge", [0, 1])
def test_counters_saturate_in_two_frames(O, scene, ge):
    u = scene.uniforms(O, S.flags_of(O, ge, 1, 0))
    two = O.count_frame(O.count_frame(scene.words, u), u)
    print(f"depth {scene.depth}, ge {ge}: {int(np.count_nonzero(two & 15))} words counted, {int(np.count_nonzero((two & 15) == 15))} at 15")
    assert (two & 15).max() == 15


@pytest.mark.parametrize("depth", [17, 21])
def test_deep_lattice_rays_tie(O, depth):
    sc = S.scene(depth)
    rays = sc.lattice_rays()
    for flags in (O.F_PAUSE_ADAPTIVE, O.F_PAUSE_ADAPTIVE | O.F_MISC_BOOL):
        rec = O.trace_rays(sc.words, rays, flags=flags, threads=4)
        multi = int(np.isin(rec["normal_bits"], S.TWO_AXIS_TIES).sum())
        deep = int(np.count_nonzero((((rec["info"] >> 8) & 0xFF) > 16) & (rec["value"] != STEP_LIMIT)))
        print(f"depth {depth}, flags {flags}: {multi} rays end on a two-axis tie, {deep} below level 16, {int(hit_bit(rec).sum())} hit")
        assert multi > 0 and deep >= 100  # (the bar the frames' pixel classes have)
    gt = O.trace_rays(sc.words, rays, flags=O.F_PAUSE_ADAPTIVE, threads=4)
    differ = int(np.count_nonzero(gt["value"] != rec["value"]))
    print(f"depth {depth}: {differ} of {rays.shape[0]} lattice rays end on another word under >=")
    assert differ >= 20, "the lattice rays should notice the tie-break"  # (the frames' bar)
