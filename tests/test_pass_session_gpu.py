"""Sessions of tree passes on one context against their restatements (tests/pass_session_ops.py): about 100 calls a session --
four kinds of build, edits by cell list and by shapes, compactions, simplifications in and out of place, structure stamps, the
five queries, refused calls, frames -- on a context that is never renewed and a second one that shares its node buffer on a
stream of its own, both with their options at the defaults (static deal on).  About a third of the writes go through the sharing
context, and the frames behind a write are traced by the context that did not write.  After every mutating call: the return
value, node_length and the words up to the model's highest length, then two 64x64 frames bit-exact against the oracle on the
model's words (the second from stored lists).  After every query: every returned tensor equal to the restatement's arrays in
order and dtype, one in five by a raw call into sentinel-filled buffers whose tail must stay.  After every refused call: the
library's message, the words and node_length as they were.  In a rest of the owner: every frame bit-exact and the static deal
replaying when and only when session_ops.Tracker says the ops determine it.  Nothing that depends on a measured time is
asserted.  A failure names the session, the op and the twelve ops before it: a prefix of the session replays it.

The second table (tests/pass_session_ops2.py) adds four sessions, seed301..seed303 and worst_combinations, of 70 to 85 calls
with the same discipline: combine_nodes with all six ops from a third Render on a context of its own, from a bare tensor and
from the pair of an out-of-place simplification of the scene (a combine mutates: return value, node_length, the words, the
source's words unchanged, two frames by the context that did not write); drop_floating (its triple; when it drops a leaf it is
a write like any other, when it drops none a query that is always followed by a comparison of the words); surface_rects and
label_components as queries, one in five raw into sentinel-filled buffers; and the refusals of REFUSALS2, after which the
source of a combine holds what it held."""
import collections
import ctypes as C
import time

import numpy as np
import pytest

import pass_session_ops as P
import pass_session_ops2 as P2
import session_ops as S
from conftest import assert_hits_equal, set_uniforms_from_oracle
from pass_frame import SLACK, SentinelOut

pytestmark = pytest.mark.gpu

HALT = []  # a HIP error met by an earlier case: nothing more is started on the GPU in this run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return S.build_driver(tmp_path_factory.mktemp("pass_session_plan"))


@pytest.fixture
def contexts(pkg):
    """a context of the case's own, the second one that shares its node buffer (on a stream of its own), and a third one
    with a node buffer of its own for the sources of the combines"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if HALT:
        pytest.fail(f"not started: an earlier session met a device error ({HALT[0]})")
    owner, other, third = pkg.Gpu(0), pkg.Gpu(0), pkg.Gpu(0)
    other.use_own_stream()
    third.use_own_stream()
    yield owner, other, third
    third.close()
    other.close()
    owner.close()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


class PassSession:
    def __init__(self, pkg, O, driver, name, steps, gpus):
        import torch
        self.torch, self.pkg, self.O, self.name, self.steps = torch, pkg, O, name, steps
        self.gpu, self.gpu2, self.gpu3 = gpus
        self.views = P.Views(O)
        self.plan = S.Tracker(self.views).plan(P.owner_ops(steps)[0], driver)
        self.next_frame = 0
        self.render = pkg.Render(self.gpu, (64, 64), np.full(8, P.B.EMPTY, dtype=np.uint32), capacity=P.CAPACITY)
        self.gpu.sync()
        self.share = pkg.Render.share_nodes(self.gpu2, self.render)
        self.source = pkg.Render(self.gpu3, (64, 64), np.full(8, P.B.EMPTY, dtype=np.uint32), capacity=P2.SRC_CAPACITY)
        offsets, index, colours = P.tree_structure()
        self.structure = pkg.Structure(offsets, index, colours)
        self.words = np.full(8, P.B.EMPTY, dtype=np.uint32)  # the model's words after the last mutating step, up to its high-water
        self.length = 8
        self.version = 0  # counts the model's trees: the oracle's frames are kept per tree and pose
        self.oracle = {}
        self.replayed = 0
        self.queries = 0
        self.at = 0
        self.tally = collections.Counter()

    def context(self, deal=True):
        lo = max(0, self.at - 12)
        lines = [f"session {self.name}, op {self.at}: {self.steps[self.at]['op']!r}; the ops before it:"]
        lines += [f"  {k}: {self.steps[k]['op']!r}" for k in range(lo, self.at)]
        if deal:
            try:
                lines.append(f"  deal: {self.gpu.deal_status()}")
            except self.pkg.SvoError as e:
                lines.append(f"  deal: {e}")
        return "\n".join(lines)

    def run(self):
        began = time.perf_counter()
        try:
            slowest = (0.0, 0)
            for self.at, step in enumerate(self.steps):
                op, t0 = step["op"], time.perf_counter()
                if op.kind == "frame":
                    self.frames(self.render, self.gpu, step["pose"], op.args[1], f"{op!r}", owner=True)
                elif step["refused"]:
                    self.refused(step)
                elif step["mutates"]:
                    self.mutate(step)
                else:
                    self.query(step)
                assert self.gpu.tree_depth == step["declared"] and self.gpu2.tree_depth == step["declared"], "the declared depth moved"
                slowest = max(slowest, (time.perf_counter() - t0, self.at))
            assert self.next_frame == len(self.plan)
            print(f"{self.name}: {time.perf_counter() - began:.1f} s (the slowest op, {slowest[1]}: {slowest[0]:.2f} s), {dict(self.tally)}")
        except AssertionError as e:
            raise AssertionError(f"{e}\n{self.context()}") from None
        except self.pkg.SvoError as e:  # (nothing more is asked of the device, the deal's state included)
            HALT.append(f"{self.name}, op {self.at}: {e}")
            raise self.pkg.SvoError(f"{e}\n{self.context(deal=False)}") from None

    # ---- the two contexts ----

    def through(self, via):
        """(the Render a call goes through, its context, the other Render, its context), node_length handed over"""
        a, b = (self.share, self.render) if via else (self.render, self.share)
        a.node_length = b.node_length = self.length
        if via:
            self.gpu.sync()  # (a write does not wait for the frames other contexts still have in flight)
        else:
            self.gpu2.sync()
        return (a, self.gpu2, b, self.gpu) if via else (a, self.gpu, b, self.gpu2)

    def nodes(self, what):
        for r in (self.render, self.share):
            assert r.node_length == self.length, f"{what}: node_length {r.node_length}, want {self.length}"
        got, want = self.render.read_nodes(self.words.size), self.words
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} of {want.size} words differ, first at {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"
        self.tally["node buffers compared"] += 1

    # ---- frames ----

    def frames(self, render, gpu, pose, n, what, owner):
        u = self.views.uniforms(pose)
        key = (self.version, pose)
        if key not in self.oracle:
            if len(self.oracle) > 8:
                self.oracle.clear()
            self.oracle[key] = self.O.trace_frame(self.words[:self.length], u, threads=8)
        want = self.oracle[key]
        for r in (self.render, self.share):
            if getattr(r, "_pose", None) != pose:
                set_uniforms_from_oracle(r, u)
                r._pose = pose
        for k in range(n):
            hits = render.render()
            gpu.sync()
            got = self.pkg.render.hits_to_numpy(hits)
            if not np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32)):
                assert_hits_equal(got, want, f"{what}: frame {k}")  # (says where; NaN payloads may differ)
            self.tally["frames"] += 1
            self.tally["records that hit"] += int(((want["info"] >> 16) & 1).sum())
            if owner:
                self.deal(f"{what}: frame {k}")

    def deal(self, what):
        """the static deal of the owner after one of its frames, by session_ops.Tracker's facts (test_session_gpu.py)"""
        F = self.plan[self.next_frame]
        self.next_frame += 1
        L = F["launches"][0]
        d = self.gpu.deal_status()
        if L["deal_grow"]:
            self.replayed = 0  # (the slot started over with new buffers)
        step, allowed = d["replayed"] - self.replayed, L["replay"]
        self.replayed = d["replayed"]
        self.tally["frames replayed"] += step
        self.tally["frames that had to be replayed"] += allowed == 1
        self.tally["frames that must not be replayed"] += allowed == 0
        if allowed is None:
            assert step in (0, 1), f"{what}: replayed advanced by {step}"
        else:
            why = "its facts forbid a replay" if allowed == 0 else f"frame {L['deal_run']} of an accepted rest is replayed"
            assert step == allowed, f"{what}: replayed advanced by {step}; {why}"

    # ---- calls ----

    def mutate(self, step):
        pkg, a, want, op = self.pkg, step["action"], step["want"], step["op"]
        r, g, other, other_gpu = self.through(step["via"])
        kind = op.kind
        if kind == "build":
            form = op.args[0]
            if form == "list":
                ret = r.build_nodes(a["coords"], a["depth"], a["colours"])
            elif form == "dense":
                ret = r.build_nodes_dense(a["grid"])
            else:
                ret = r.build_nodes_mesh(a["vq"], a["triangles"], a["depth"], a["colours"], quantized=True, solid=a["solid"],
                                         fill_colour=P.FILL, merge=a["merge"])
        elif kind == "edit":
            ret = r.edit_nodes(a["coords"], a["depth"], a["colours"])
        elif kind == "region":
            ret = r.edit_region(self.shapes(a["shapes"]), a["depth"])
        elif kind == "compact":
            ret = r.compact_nodes(prune=a["prune"])
        elif kind == "simplify":
            ret = r.simplify_nodes(merge=a["merge"], cut_level=a["cut_level"], min_level=a["min_level"])
        elif kind == "stamp":
            ret = self.stamp(r, a, want, f"{op!r}")
        elif kind == "combine":
            src, held = self.combine_source(r, other, a, f"{op!r}")
            ret = r.combine_nodes(src, a["op"], a["depth"], at=a["at"], at_level=a["at_level"])
            held(f"{op!r}")
        elif kind == "drop":
            got = r.drop_floating(a["depth"], a["anchor"], a["same_value"])
            assert got == want["triple"], f"{op!r} returned {got}, want {want['triple']}"
            ret = r.node_length
        else:
            raise ValueError(op)
        assert ret == want["ret"] == r.node_length, f"{op!r} returned {ret}, node_length {r.node_length}, want {want['ret']}"
        self.words, self.length = step["words"], step["length"]
        self.version += 1
        self.render.node_length = self.share.node_length = self.length
        self.nodes(f"after {op!r}")
        # two frames by the context that did not write
        self.frames(other, other_gpu, step["pose"], 2, f"behind {op!r}", owner=step["via"])
        self.tally["writes"] += 1
        self.tally["writes through the sharing context"] += step["via"]

    def combine_source(self, r, other, a, what):
        """(what combine_nodes takes as the source, a check that the source still holds its words) for a["form"]: the third
        Render holding the words, a bare tensor of them, the pair of the scene's own out-of-place simplification, or -- for
        the refusal -- the Render on the other context of the pair, which shares the node buffer"""
        form, words = a["form"], a["src"]
        if form == "sharing":
            return other, lambda what: None  # (the words of the node buffer are compared after every refusal)
        if form == "render":
            self.source.write_nodes(words)
            self.source.node_length = words.size

            def held(what):
                assert self.source.node_length == words.size, f"{what}: the source's node_length moved"
                assert np.array_equal(self.source.read_nodes(words.size), words), f"{what}: the source's words changed"
            return self.source, held
        if form == "pair":
            t, n = r.simplify_nodes(merge=a["merge"], cut_level=a["cut_level"], out_of_place=True)
            assert n == words.size == len(t) and r.node_length == self.length, f"{what}: the out-of-place simplification has {n} words, want {words.size}"
            self.same((t,), (words,), f"{what}: the out-of-place simplification")
            src = (t, n)
        else:
            t = self.torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(r.gpu.torch_device)
            self.torch.cuda.current_stream(r.gpu.torch_device).synchronize()
            src = t

        def held(what):
            assert np.array_equal(u32(t), words), f"{what}: the source's words changed"
        return src, held

    def shapes(self, shapes):
        R = self.pkg.region
        return [R.box(s[1], s[2], s[3], s[4]) if s[0] == "box" else R.ball(s[1], s[2], s[3], s[4]) for s in shapes]

    def stamp(self, r, a, want, what):
        depth = a["depth"]
        if a["form"] == "place":
            return r.place_structures(self.structure, a["origins"], depth, a["rots"])
        if a["form"] == "scatter":
            origins, rots = r.scatter_structures(self.structure, a["origin"], a["size"], a["one_in"], seed=a["seed"], depth=depth)
            self.same((origins, rots), (want["origins"], want["rots"]), f"{what}: the sites")
            return r.node_length
        tops, values = r.column_tops(a["origin"], a["size"], depth, with_values=True)
        self.same((tops, values), (want["tops"], want["values"]), f"{what}: column_tops")
        origins, rots = r.structure_sites(tops, values, a["origin"], a["one_in"], a["seed"])
        self.same((origins, rots), (want["origins"], want["rots"]), f"{what}: structure_sites")
        coords, colours = r.stamp_structures(self.structure, origins, depth, rots)
        self.same((coords, colours), (want["coords"], want["colours"]), f"{what}: stamp_structures")
        return r.edit_nodes(coords, depth, colours)

    def same(self, got, want, what):
        """device int32 tensors against the restatement's arrays: shape, dtype and every entry, in order"""
        assert len(got) == len(want), what
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == self.torch.int32 and g.is_cuda, f"{what}: result {k} is {g.dtype} on {g.device}"
            w = np.asarray(w)
            assert tuple(g.shape) == w.shape, f"{what}: result {k} has shape {tuple(g.shape)}, want {w.shape}"
            h = u32(g)
            bad = np.flatnonzero(h.reshape(-1) != w.astype(np.int64).reshape(-1) & 0xFFFFFFFF)
            assert bad.size == 0, f"{what}: result {k}: {bad.size} entries differ, first at {bad[:5]}"
        self.tally["result arrays compared"] += len(got)

    def query(self, step):
        a, op, out = step["action"], step["op"], step["want"].get("out")
        r, g, _, _ = self.through(False)
        kind, what = op.kind, f"{op!r}"
        self.queries += kind != "simplify"
        raw = kind not in ("simplify", "drop") and self.queries % 5 == 0
        if kind == "simplify":  # out of place: the buffer is only read, and no rest ends
            words, n = r.simplify_nodes(merge=a["merge"], cut_level=a["cut_level"], min_level=a["min_level"], out_of_place=True)
            assert n == step["want"]["words"].size == len(words) and r.node_length == self.length, what
            self.same((words,), (step["want"]["words"],), what)
        elif kind == "list":
            xyz, val, lev = out
            if raw:
                self.raw_list(self.pkg._lib.ListParams, "svo_nodes_list_voxels", "max_voxels", 1 if a["expand"] else 0, a["depth"],
                              (xyz, val, lev), what)
            got = r.list_voxels(a["depth"], a["expand"], a["with_levels"])
            self.same(got, (xyz, val, lev) if a["with_levels"] else (xyz, val), what)
        elif kind in ("surface", "quads"):
            xyz, val, lev, face = out
            if raw:
                self.raw_list(self.pkg._lib.SurfaceParams, "svo_nodes_list_surface", "max_entries", a["flags"], a["depth"],
                              (xyz, val, lev, face), what)
            if a["quads"]:
                self.same(r.surface_quads(a["depth"], a["closed"]), (xyz, val, face, lev), what)
            else:
                self.same(r.list_surface(a["depth"], a["closed"], a["keep_hidden"], with_levels=True), (xyz, val, face, lev), what)
        elif kind == "sample":
            if raw:
                self.raw_sample(a, out, what)
            self.same(r.sample_voxels(a["cells"], a["depth"], with_levels=True, with_indices=True), out, what)
        elif kind == "dense":
            if raw:
                p = self.pkg._lib.SampleParams()
                p.depth, p.n_words = step["depth"], self.length
                self.raw_box(out.size, (out,), what, lambda t: self.pkg._lib.lib().svo_nodes_sample_dense(
                    self.gpu._h, C.byref(p), (C.c_uint32 * 3)(*a["origin"]), (C.c_uint32 * 3)(*a["size"]), t[0].data_ptr()))
            self.same((r.sample_dense(a["origin"], a["size"], step["depth"]),), (out,), what)
        elif kind == "tops":
            if raw:
                p = self.pkg._lib.TopsParams()
                p.depth, p.n_words = step["depth"], self.length
                p.y_lo, p.y_hi = (0, 1 << step["depth"]) if a["y_range"] is None else a["y_range"]
                self.raw_box(out[0].size, out, what, lambda t: self.pkg._lib.lib().svo_nodes_column_tops(
                    self.gpu._h, C.byref(p), (C.c_uint32 * 2)(*a["origin"]), (C.c_uint32 * 2)(*a["size"]), t[0].data_ptr(), t[1].data_ptr()))
            self.same(r.column_tops(a["origin"], a["size"], step["depth"], a["y_range"], with_values=True), out, what)
        elif kind == "rects":
            if raw:
                self.raw_rects(a, out, what)
            self.same(r.surface_rects(a["depth"], a["closed"], a["rounds"], a["any_value"]), out, what)
        elif kind == "components":
            label, ids, n, indices, sizes = step["want"]["out"]
            if raw:
                self.raw_components(a, (label, ids, indices), n, what)
            got = r.label_components(a["depth"], a["same_value"], True, a["with_indices"], a["with_sizes"])
            assert len(got) == 3 + a["with_indices"] + a["with_sizes"] and got[2] == n, f"{what}: {got[2]} components, want {n}"
            self.same(got[:2] + ((got[3],) if a["with_indices"] else ()), (label, ids) + ((indices,) if a["with_indices"] else ()), what)
            if a["with_sizes"]:
                t = got[-1]
                assert t.dtype == self.torch.int64 and t.is_cuda and tuple(t.shape) == sizes.shape, f"{what}: sizes are {t.dtype}, {tuple(t.shape)}"
                assert np.array_equal(t.cpu().numpy(), sizes), f"{what}: the sizes differ"
                self.tally["result arrays compared"] += 1
        elif kind == "drop":  # one that drops nothing: a query, and always held to have written nothing
            got = r.drop_floating(a["depth"], a["anchor"], a["same_value"])
            assert got == step["want"]["triple"], f"{what} returned {got}, want {step['want']['triple']}"
            assert r.node_length == self.length, f"{what}: node_length moved to {r.node_length}"
            self.nodes(f"after {what}: nothing floats, nothing is written")
        else:
            raise ValueError(op)
        self.tally["queries"] += 1
        self.tally["raw queries into sentinel buffers"] += raw
        if self.queries % 7 == 0:
            self.nodes(f"after {what}: a query writes nothing")

    def raw_list(self, params, call, cap_field, flags, depth, want, what):
        """the count query, then the fill into buffers SLACK entries longer than the count: the tail keeps the sentinel"""
        n_want = len(want[1])
        p = params()
        p.flags, p.depth, p.n_words = flags, self.gpu.tree_depth if depth is None else depth, self.length
        n = C.c_uint64(0xAAAA)
        fn = getattr(self.pkg._lib.lib(), call)
        nulls = (None,) * len(want)
        self.gpu.check(fn(self.gpu._h, C.byref(p), *nulls, C.byref(n)))
        assert n.value == n_want, f"{what}: the count query gives {n.value}, want {n_want}"
        out = SentinelOut(self.gpu, [(n_want + SLACK, 3)] + [n_want + SLACK] * (len(want) - 1))
        setattr(p, cap_field, n_want)
        if n_want:
            self.gpu.check(fn(self.gpu._h, C.byref(p), *[t.data_ptr() for t in out.t], C.byref(n)))
            self.gpu.sync()
        assert n.value == n_want and out.untouched_from(n_want), f"{what}: the fill wrote behind its {n_want} entries"
        for got, w in zip(out.host(), want):
            assert np.array_equal(got[:n_want], w), f"{what}: the raw call's entries differ"

    def raw_rects(self, a, want, what):
        """svo_nodes_merge_surface: the count query, then the fill into buffers SLACK entries longer than the count"""
        rects, values = want
        n_want = len(values)
        p = self.pkg._lib.SurfaceMergeParams()
        p.flags = (1 if a["closed"] else 0) | (8 if a["any_value"] else 0)
        p.depth, p.rounds, p.n_words = self.gpu.tree_depth if a["depth"] is None else a["depth"], a["rounds"], self.length
        n = C.c_uint64(0xAAAA)
        fn = self.pkg._lib.lib().svo_nodes_merge_surface
        self.gpu.check(fn(self.gpu._h, C.byref(p), None, None, C.byref(n)))
        assert n.value == n_want, f"{what}: the count query gives {n.value}, want {n_want}"
        out = SentinelOut(self.gpu, [(n_want + SLACK, 6), n_want + SLACK])
        p.max_entries = n_want
        if n_want:
            self.gpu.check(fn(self.gpu._h, C.byref(p), *[t.data_ptr() for t in out.t], C.byref(n)))
            self.gpu.sync()
        assert n.value == n_want and out.untouched_from(n_want), f"{what}: the fill wrote behind its {n_want} entries"
        for got, w in zip(out.host(), (rects, values)):
            assert np.array_equal(got[:n_want], w), f"{what}: the raw call's entries differ"

    def raw_components(self, a, want, n_components, what):
        """svo_nodes_label_components into buffers SLACK entries longer than the listing's count"""
        n_want = len(want[0])
        p = self.pkg._lib.ComponentsParams()
        p.flags, p.depth = (1 if a["same_value"] else 0), self.gpu.tree_depth if a["depth"] is None else a["depth"]
        p.n_words, p.max_entries = self.length, n_want
        n, c = C.c_uint64(0xAAAA), C.c_uint64(0xAAAA)
        out = SentinelOut(self.gpu, [n_want + SLACK] * 3)
        ptrs = [t.data_ptr() for t in out.t] if n_want else [None] * 3
        self.gpu.check(self.pkg._lib.lib().svo_nodes_label_components(self.gpu._h, C.byref(p), *ptrs, C.byref(n), C.byref(c)))
        self.gpu.sync()
        assert (n.value, c.value) == (n_want, n_components), f"{what}: the raw call gives {n.value} entries in {c.value} components, want {n_want} in {n_components}"
        assert out.untouched_from(n_want), f"{what}: the raw call wrote behind its {n_want} entries"
        for got, w in zip(out.host(), want):
            assert np.array_equal(got[:n_want], np.asarray(w).astype(np.uint32)), f"{what}: the raw call's entries differ"

    def raw_box(self, n, want, what, call):
        """a dense result of n entries per array into flat buffers SLACK entries longer"""
        out = SentinelOut(self.gpu, [n + SLACK] * len(want))
        self.gpu.check(call(out.t))
        self.gpu.sync()
        assert out.untouched_from(n), f"{what}: the raw call wrote behind its {n} entries"
        for got, w in zip(out.host(), want):
            assert np.array_equal(got[:n], np.asarray(w).reshape(-1)), f"{what}: the raw call's entries differ"

    def raw_sample(self, a, want, what):
        n = len(a["cells"])
        p = self.pkg._lib.SampleParams()
        p.depth, p.n_words = self.gpu.tree_depth if a["depth"] is None else a["depth"], self.length
        cells = self.torch.as_tensor(np.asarray(a["cells"], dtype=np.int64).astype(np.int32), device=self.gpu.torch_device)
        out = SentinelOut(self.gpu, [n + SLACK] * 3)
        self.gpu.check(self.pkg._lib.lib().svo_nodes_sample(self.gpu._h, C.byref(p), cells.data_ptr(), n, *[t.data_ptr() for t in out.t]))
        self.gpu.sync()
        assert out.untouched_from(n), f"{what}: the raw call wrote behind its {n} entries"
        for got, w in zip(out.host(), want):
            assert np.array_equal(got[:n], w), f"{what}: the raw call's entries differ"

    def refused(self, step):
        pkg, a, op = self.pkg, step["action"], step["op"]
        kind = op.args[0]
        _, cls, fragment = step["refused"]
        r, g, other, _ = self.through(step["via"])
        held = None
        if step["refused"][0] == "combine":
            src, held = self.combine_source(r, other, a, f"{op!r}")
        calls = {
            "combine_finer": lambda: r.combine_nodes(src, a["op"], a["depth"]),
            "max_words_combine": lambda: r.combine_nodes(src, a["op"], a["depth"], max_words=a["max_words"]),
            "combine_overlap": lambda: r.combine_nodes(src, a["op"], a["depth"]),
            "source_malformed": lambda: r.combine_nodes(src, a["op"], a["depth"]),
            "rects_depth": lambda: r.surface_rects(a["depth"]),
            "components_depth": lambda: r.label_components(a["depth"]),
            "max_entries_rects": lambda: self.raw_short(r, "rects", a),
            "max_entries_components": lambda: self.raw_short(r, "components", a),
            "max_words_build": lambda: r.build_nodes(a["coords"], a["depth"], a["colours"], max_words=a["max_words"]),
            "max_words_edit": lambda: r.edit_nodes(a["coords"], a["depth"], a["colours"], max_words=a["max_words"]),
            "max_words_region": lambda: r.edit_region(self.shapes(a["shapes"]), a["depth"], max_words=a["max_words"]),
            "edit_depth": lambda: r.edit_nodes(a["coords"], a["depth"], a["colours"]),
            "region_depth": lambda: r.edit_region(self.shapes(a["shapes"]), a["depth"]),
            "list_depth": lambda: r.list_voxels(a["depth"]),
            "surface_depth": lambda: r.list_surface(a["depth"]),
            "dense_box": lambda: r.sample_dense(a["origin"], a["size"], a["depth"]),
            "simplify_min_level": lambda: r.simplify_nodes(merge=a["merge"], cut_level=a["cut_level"], min_level=a["min_level"]),
        }
        if kind.startswith("malformed"):  # one interior pointer off the multiple of 8 for the call, then back
            calls[kind] = {"compact": r.compact_nodes, "simplify": r.simplify_nodes, "list": lambda: r.list_voxels(a["depth"]),
                           "surface": lambda: r.list_surface(a["depth"]), "rects": lambda: r.surface_rects(a["depth"], rounds=2),
                           "components": lambda: r.label_components(a["depth"], with_indices=True),
                           "combine": lambda: r.combine_nodes(src, a["op"], a["depth"])}[step["refused"][0]]
            r.scatter_nodes([a["at"]], [a["bad"]])
        try:
            with pytest.raises(getattr(pkg, cls)) as e:
                calls[kind]()
        finally:
            if kind.startswith("malformed"):
                r.scatter_nodes([a["at"]], [a["good"]])
        assert fragment in str(e.value), f"{op!r}: the refusal says {e.value}, want '{fragment}'"
        assert r.node_length == self.length, f"{op!r}: a refused call moved node_length to {r.node_length}"
        self.nodes(f"after {op!r}: a refused call writes nothing")
        if held:
            held(f"after {op!r}")
        self.tally["refused calls"] += 1


    def raw_short(self, r, which, a):
        """the raw entry point with outputs of max_entries = the count less one: refused, and nothing written to them"""
        n, c = C.c_uint64(0), C.c_uint64(0)
        cap = a["max_entries"]
        if which == "rects":
            p = self.pkg._lib.SurfaceMergeParams()
            p.flags, p.depth, p.rounds, p.n_words, p.max_entries = 0, a["depth"], a["rounds"], self.length, cap
            out = SentinelOut(r.gpu, [(cap + SLACK, 6), cap + SLACK])
            rc = self.pkg._lib.lib().svo_nodes_merge_surface(r.gpu._h, C.byref(p), *[t.data_ptr() for t in out.t], C.byref(n))
        else:
            p = self.pkg._lib.ComponentsParams()
            p.flags, p.depth, p.n_words, p.max_entries = 0, a["depth"], self.length, cap
            out = SentinelOut(r.gpu, [cap + SLACK] * 3)
            rc = self.pkg._lib.lib().svo_nodes_label_components(r.gpu._h, C.byref(p), *[t.data_ptr() for t in out.t], C.byref(n), C.byref(c))
        try:
            r.gpu.check(rc)
        finally:
            r.gpu.sync()
            assert out.untouched_from(0), f"{which}: a call refused for max_entries wrote to its outputs"


@pytest.mark.parametrize("name", P2.ALL_NAMES)
def test_pass_session(pkg, O, driver, contexts, name):
    PassSession(pkg, O, driver, name, P2.session(name), contexts).run()
