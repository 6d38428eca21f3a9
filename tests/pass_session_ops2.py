"""The pass sessions' second table (tests/test_pass_session_host.py, tests/test_pass_session_gpu.py): the passes that came after
pass_session_ops.py was written -- combine_nodes, surface_rects, label_components and drop_floating -- as ops of the same
generator and the same host model, answered from the restatements alone (combine_ref, surface_ref with surface_merge_ref,
components_ref, sample_ref for the cross-checks).  Nothing of pass_session_ops.py changes: its tables, its seven sessions and
their op lines (tests/golden/pass_session_ops.txt) stay as they are, and only the sessions of this module draw from PASSES2,
SHARED2 and REFUSALS2.  Nothing here touches a GPU.

The new ops (the old ones: pass_session_ops.py):
  combine(op, source, at_level, at, depth, via)   mutates.  source: render/<tree> (a third Render on a context of its own that
                                    holds the tree) | tensor/<tree> (a bare device tensor of words) | pair/merge, pair/cut<level>
                                    (the (tensor, length) pair of an out-of-place simplify_nodes of the scene itself: the op's
                                    first call is that simplification).  <tree>: ball | list/<seed>/<n> | empty (8 words)
  rects(depth, closed, rounds, any_value)         query: surface_rects
  components(depth, same_value, with_indices, with_sizes)   query: label_components
  drop(anchor, same_value, via)     drop_floating; mutates only if it drops a leaf (writes: 1 then, else 0)
  refused(kind, seed, via)          the kinds of REFUSALS2; the malformed_* kinds write one word by svo_nodes_scatter before the
                                    call and put it back after, source_malformed hands in a host-built source with one interior
                                    pointer off the multiple of 8

The sessions: three seeded ones (seed301..seed303) and worst_combinations(), 70 to 85 ops each on trees of depth 5 and 6, with
one stretch over a scan tile in groups followed by a tree under 512 groups.
"""
import functools

import numpy as np

import build_ref as B
import combine_ref as X
import compact_ref as K
import components_ref as Q
import list_ref as L
import pass_session_ops as P
import region_ref as G
import sample_ref as SM
import simplify_ref as R
import surface_merge_ref as MR
import surface_ref as F
from pass_session_ops import CAPACITY, REST_POSE, TILE, Gen, Model, Refusal, groups_of
from session_ops import Op

SRC_CAPACITY = 1 << 17  # words of the third Render, which holds the sources
PASSES2 = ("combine", "rects", "components", "drop")
ALL_PASSES = P.PASSES + PASSES2
MUTATING2 = ("combine", "drop")  # (drop: when it drops a leaf)
ALL_MUTATING = P.MUTATING + MUTATING2
# which of the new passes share what with which (csrc/svo_ctx.h, svo_combine.hip, svo_surface_merge.hip, svo_components.hip):
# a refusal of a new pass is followed directly by a call of each of the others of its groups
SHARED2 = {
    # svo_combine.hip scans its flags in place by svo_scan_u32, whose tile sums are the context's (scan_tiles), as the region
    # edit, the edit and the builder's sort do; it marks, checks and commits its frontier by the kernels of svo_frontier.h
    # (region_mark, region_check, region_fill, region_write), which are the region edit's
    "scan_tiles, svo_frontier.h": ("combine", "region", "edit", "build"),
    # svo_surface_merge.hip owns a svo_surface_state (a svo_list_plan, its svo_tree_walk and status words) that runs the
    # surface pass's code (svo_surface_list_quads), and sorts in the builder's workspace (svo_build_sort_u64)
    "svo_surface_state, svo_build_sort_u64": ("rects", "surface", "build"),
    # svo_components.hip owns a svo_list_plan with a svo_tree_walk and status words of its own, run by the listing's code
    # (svo_list_plan_count, svo_list_plan_offsets)
    "svo_list_plan": ("components", "list"),
}
# refusal kind -> (the pass refused, the error class's name, a fragment of the library's message)
REFUSALS2 = {
    "combine_finer": ("combine", "SvoError", "finer there than the combine"),
    "max_words_combine": ("combine", "SvoError", "the combined tree needs"),
    "combine_overlap": ("combine", "SvoError", "the source overlaps the node buffer"),
    "malformed_combine": ("combine", "SvoError", "malformed tree: an interior pointer"),
    "source_malformed": ("combine", "SvoError", "malformed source: an interior pointer"),
    "rects_depth": ("rects", "SvoError", "deeper than depth ="),
    "components_depth": ("components", "SvoError", "deeper than depth ="),
    "malformed_rects": ("rects", "SvoError", "is not a multiple of 8"),
    "malformed_components": ("components", "SvoError", "is not a multiple of 8"),
    # the raw entry points with room for one entry fewer than the count
    "max_entries_rects": ("rects", "SvoError", "more than max_entries ="),
    "max_entries_components": ("components", "SvoError", "more than max_entries ="),
}
ALL_REFUSALS = {**P.REFUSALS, **REFUSALS2}
SEEDS2 = (301, 302, 303)
SOLID = 0x00C0DE  # the one-leaf source of the refusals: a paint by it opens every interior word of the scene


def partners2(kind):
    """the passes that share state or helpers with the pass that refusal `kind` of REFUSALS2 refuses (itself among them)"""
    p = REFUSALS2[kind][0]
    return sorted({q for group in SHARED2.values() if p in group for q in group})


def all_pairs2():
    """the (mutating pass, pass) pairs in which at least one side is a new pass"""
    return [(a, b) for a in ALL_MUTATING for b in ALL_PASSES if a in PASSES2 or b in PASSES2]


def all_refusal_pairs2():
    return [(kind, b) for kind in REFUSALS2 for b in partners2(kind)]


def old_refusal_pairs2():
    """the (refusal kind of the first table, new pass) pairs: a new pass directly behind every refusal of a pass it shares
    state or helpers with"""
    return [(kind, q) for kind, (p, _, _) in P.REFUSALS.items() for q in PASSES2 if any(p in group and q in group for group in SHARED2.values())]


# ---- the sources ----

@functools.lru_cache(maxsize=None)
def ball_tree(s, centre2=None, radius2=None):
    """a two-coloured solid ball in the depth-s grid, built and merged, as combine_ref.ball_source makes its depth-7 one"""
    side = 1 << s
    cells = X.ball_cells(s, (side,) * 3 if centre2 is None else centre2, int(0.78 * side) if radius2 is None else radius2)
    built = B.build(cells, s, np.where(cells[:, 0] < side // 2, 0x40C0FF, 0xFF8020))
    return R.simplify(built, built.size)[0]


def list_tree(s, seed, n):
    rng = np.random.default_rng(seed)
    return B.build(rng.integers(0, 1 << s, (n, 3)), s, rng.integers(1, 1 << 24, n))


def empty_tree():
    return np.full(8, B.EMPTY, dtype=np.uint32)


def solid_tree():
    return np.full(8, (B.VOXEL_OFFSET + SOLID) << 4, dtype=np.uint32)


def source_grid(src, s):
    grid = SM.sample_dense(src, src.size, (0, 0, 0), (1 << s,) * 3, s)
    assert not (grid == SM.FINER).any(), "a source finer than its cube"
    return grid


# ---- the model ----

class Model2(Model):
    def combine(self, src, op, at_level, at, depth=None):
        depth = self.depth if depth is None else depth
        try:
            new = X.combine(self.buf, self.length, src, op, depth, at_level, at)[0]
        except X.Refused:
            raise Refusal("combine_finer") from None
        assert depth == self.depth
        s = depth - at_level
        self._declare(depth)
        n = self._store(new)
        self.grid = X.apply_cells(self.grid, source_grid(src, s), op, at, s)
        return n

    def rects(self, depth, closed, rounds, any_value):
        d = self.d(depth)
        try:
            quads = F.list_surface(self.buf, self.length, d, F.QUADS | (F.CLOSED_BOUNDARY if closed else 0))
        except L.TooDeep:
            raise Refusal("rects_depth") from None
        return MR.merge_rects(quads, d, rounds, any_value), int(np.unique(quads[2]).size)

    def components(self, depth, same_value):
        """(labels, ids, n_components, indices, sizes): the first three by components_ref.labels; the indices by sample_ref at
        the entries' cells; the sizes from the grid of the per-cell contracts, whose own labelling must give the same partition"""
        d = self.d(depth)
        try:
            label, ids, n, index = Q.labels(self.buf, self.length, d, same_value)
        except L.TooDeep:
            raise Refusal("components_depth") from None
        xyz, value, level = L.list_voxels(self.buf, self.length, d)
        f = d - self.depth
        cell = xyz.astype(np.int64) >> f
        indices = SM.sample(self.buf, self.length, xyz.astype(np.int64), d)[2]
        assert np.array_equal(indices.astype(np.int64), index.astype(np.int64)), "components_ref and sample_ref stop on different words"
        sizes = np.zeros(n, dtype=np.int64)
        g = self.grid
        if not same_value:
            lab, total = Q.label_grid((g != 0).astype(np.int64))
            of_entry = lab[tuple(cell.T)]
            assert total == n and Q.same_partition(of_entry, ids), "the grid's components are not the words'"
            u, first = np.unique(of_entry, return_index=True)
            assert (u > 0).all()
            sizes[ids[first]] = np.bincount(lab.reshape(-1), minlength=total + 1)[u]
        else:
            w = np.int64(1) << (self.depth - np.minimum(level.astype(np.int64), self.depth))
            for e in range(value.size):  # the cells of the entry's cube that hold its value: all of them
                c = cell[e]
                cube = g[c[0]:c[0] + w[e], c[1]:c[1] + w[e], c[2]:c[2] + w[e]]
                assert (cube == value[e]).all()
                sizes[ids[e]] += cube.size
        return label, ids, n, indices, sizes << (3 * f)

    def drop(self, anchor, same_value):
        """((components, dropped components, dropped leaves), the dropped leaves' word indices, the grid afterwards): the triple
        and the grid by components_ref.drop_floating on the grid, the leaves by components_ref.labels on the words"""
        grid, n, n_dropped = Q.drop_floating(self.grid, anchor, same_value)
        label, ids, n_words, index = Q.labels(self.buf, self.length, self.depth, same_value)
        assert n_words == n, "the grid's components are not the words'"
        xyz = L.list_voxels(self.buf, self.length, self.depth)[0].astype(np.int64)
        gone = grid[tuple(xyz.T)] == 0
        assert np.unique(ids[gone]).size == n_dropped and not np.isin(ids[~gone], ids[gone]).any()
        return (n, n_dropped, int(gone.sum())), index[gone].astype(np.int64), grid.astype(np.uint32)

    def commit_drop(self, indices, grid):
        self.buf[indices] = B.EMPTY
        self.grid = grid
        return self.length


# ---- the generator ----

class Gen2(Gen):
    def __init__(self, pkg, seed, needs=(), refusal_needs=()):
        super().__init__(pkg, seed, needs, refusal_needs)
        self.m = Model2(pkg)

    # -- the new ops --

    def source(self, name, s):
        """the words of the source tree `name` at depth s"""
        parts = name.split("/")
        if parts[0] == "ball":
            return ball_tree(s)
        if parts[0] == "list":
            return list_tree(s, int(parts[1], 16), int(parts[2]))
        return {"empty": empty_tree, "solid": solid_tree}[parts[0]]()

    def draw_tree(self):
        k = int(self.rng.integers(0, 5))
        return ("ball", "ball", f"list/{self.seed():#x}/{int(self.rng.integers(10, 200))}", f"list/{self.seed():#x}/{int(self.rng.integers(10, 200))}", "empty")[k]

    def combine(self, op=None, source=None, at_level=None, at=None, via=None, words=None):
        """source: <form>/<tree>, or with `words` given any name for them"""
        m = self.m
        op = X.OPS[int(self.rng.integers(0, 6))] if op is None else op
        if source is None:
            form = ("render", "tensor", "pair")[int(self.rng.integers(0, 3))]
            if form == "pair":
                source = "pair/merge" if self.rng.random() < 0.5 else f"pair/cut{int(self.rng.integers(2, m.depth + 1))}"
            else:
                source = f"{form}/{self.draw_tree()}"
        form, tree = source.split("/", 1)
        if form == "pair":
            at_level, at = 0, (0, 0, 0)
        if at_level is None:
            at_level = int(self.rng.integers(0, 3))
        if at is None:
            at = tuple(int(v) for v in self.rng.integers(0, 1 << at_level, 3))
        via = self.via() if via is None else via
        self.before()
        self._canonical_in = m.canonical()
        action = {"via": via, "op": op, "form": form, "at_level": at_level, "at": at, "depth": m.depth}
        if form == "pair":
            cut = None if tree == "merge" else int(tree[3:])
            action.update(merge=cut is None, cut_level=cut)
            words = R.simplify(m.buf, m.length, cut is None, cut, 0)[0]
            calls = ["simplify", "combine"]
        else:
            words = self.source(tree, m.depth - at_level) if words is None else words
            calls = ["combine"]
        assert words.size <= SRC_CAPACITY
        action["src"] = words
        self.note(calls[0])
        ret = m.combine(words, op, at_level, at)
        return self.record(Op("combine", op, source, at_level, at, m.depth, via), calls, action, want={"ret": ret}, mutates=True)

    def q_rects(self, depth=-1, closed=None, rounds=None, any_value=None):
        m = self.m
        depth = self.query_depth() if depth == -1 else depth
        closed = bool(self.rng.random() < 0.5) if closed is None else closed
        rounds = int(self.rng.integers(1, 5)) if rounds is None else rounds
        any_value = bool(self.rng.random() < 0.3) if any_value is None else any_value
        self.before()
        self._canonical_in = m.canonical()
        self.note("rects")
        out, levels = m.rects(depth, closed, rounds, any_value)
        return self.record(Op("rects", depth, closed, rounds, any_value), ["rects"],
                           {"depth": depth, "closed": closed, "rounds": rounds, "any_value": any_value, "levels": levels}, want={"out": out})

    def q_components(self, depth=-1, same_value=None, with_indices=None, with_sizes=None):
        m = self.m
        depth = self.query_depth() if depth == -1 else depth
        same_value = bool(self.rng.random() < 0.4) if same_value is None else same_value
        with_indices = bool(self.rng.random() < 0.6) if with_indices is None else with_indices
        with_sizes = bool(self.rng.random() < 0.6) if with_sizes is None else with_sizes
        self.before()
        self._canonical_in = m.canonical()
        self.note("components")
        return self.record(Op("components", depth, same_value, with_indices, with_sizes), ["components"],
                           {"depth": depth, "same_value": same_value, "with_indices": with_indices, "with_sizes": with_sizes},
                           want={"out": m.components(depth, same_value)})

    def anchors(self):
        """the floor first or an explicit box first, by the draw; then boxes that hold less and less"""
        side = 1 << self.m.depth
        lo = tuple(int(v) for v in self.rng.integers(0, side // 2, 3))
        box = (lo, tuple(v + side // 3 for v in lo))
        rest = [((0, side - 2, 0), (side, side + 3, side)), ((-2, -2, -2), (1, 1, 1))]  # (the ceiling; one corner, clipped)
        return ([None, box] if self.rng.random() < 0.5 else [box, None]) + rest

    def drop(self, anchor=-1, same_value=None, via=None, must=False):
        """must: of the anchors the first one that drops a leaf, if any does"""
        m = self.m
        if same_value is None:
            same_value = bool(self.rng.random() < 0.35 and np.unique(m.grid).size <= 200)
        self.before()
        self._canonical_in = m.canonical()
        for a in (self.anchors() if anchor == -1 else [anchor]):
            triple, indices, grid = m.drop(a, same_value)
            if triple[2] or not must:
                break
        drops = triple[2] > 0
        via = bool(drops and (self.via() if via is None else via))
        self.note("drop")
        ret = m.commit_drop(indices, grid)
        return self.record(Op("drop", a, same_value, via), ["drop"], {"via": via, "anchor": a, "same_value": same_value, "depth": m.depth,
                           "writes": int(drops)}, want={"ret": ret, "triple": triple}, mutates=drops)

    # -- the new refusals --

    def refused(self, kind, via=None):
        if kind in P.REFUSALS:
            return super().refused(kind, via)
        m = self.m
        seed = self.seed()
        via = bool((self.via() if via is None else via) and REFUSALS2[kind][0] == "combine")
        action = {"via": via, "kind": kind, "depth": m.depth}
        state = (m.length, m.high, m.declared, m.depth)
        words = m.buf[:m.length]
        try:
            if kind == "combine_finer":  # a paint by one leaf, one level above the scene's: a scene with a voxel of its depth is finer
                if m.depth < 2:
                    return False
                action.update(op="paint", form="render", src=solid_tree(), depth=m.depth - 1)
                X.combine(words, m.length, action["src"], "paint", m.depth - 1)
                return False
            elif kind == "max_words_combine":
                src = list_tree(m.depth, seed, 150)
                need = X.combine(words, m.length, src, "over", m.depth)[0].size
                if need <= m.length:
                    return False
                action.update(op="over", form="tensor", src=src, max_words=need - 1)
            elif kind == "combine_overlap":  # the Render on the other context of the pair, which shares the node buffer
                action.update(op="over", form="sharing", src=None)
            elif kind == "source_malformed":  # an over follows every interior pointer of the source's root group
                src = ball_tree(m.depth).copy()
                ptr = src[:8].astype(np.int64) >> 4
                ok = np.flatnonzero((ptr < B.VOXEL_OFFSET) & (ptr + 12 <= src.size))
                if not len(ok):
                    return False
                src[ok[0]] += 4 << 4
                action.update(op="over", form="tensor", src=src)
                X.combine(words, m.length, src, "over", m.depth)
                return False
            elif kind in ("rects_depth", "components_depth"):
                action.update(depth=m.depth - 1)
                L.list_voxels(words, m.length, m.depth - 1)
                return False
            elif kind.startswith("malformed"):
                reached = K.compact(m.buf, m.length, False)[1].astype(np.int64)  # (the old places of the reachable words)
                ptr = m.buf[reached].astype(np.int64) >> 4
                ok = reached[(ptr < B.VOXEL_OFFSET) & (ptr + 12 <= m.length)]
                if not len(ok):
                    return False
                at = int(ok[np.random.default_rng(seed).integers(0, len(ok))])
                good = int(m.buf[at])
                action.update(at=at, good=good, bad=good + (4 << 4), writes=2)
                bad = words.copy()
                bad[at] = action["bad"]
                if kind == "malformed_combine":
                    action.update(op="paint", form="tensor", src=solid_tree())
                    X.combine(bad, m.length, action["src"], "paint", m.depth)
                else:
                    L.list_voxels(bad, m.length, m.depth)
                return False
            elif kind in ("max_entries_rects", "max_entries_components"):
                if kind == "max_entries_rects":
                    action.update(closed=False, rounds=2, any_value=False)
                    count = len(m.rects(m.depth, False, 2, False)[0][1])
                else:
                    action.update(same_value=False)
                    count = len(L.list_voxels(words, m.length, m.depth)[1])
                if not count:
                    return False
                action.update(max_entries=count - 1)
        except (X.Refused, X.Malformed, L.TooDeep, K.Malformed):
            pass
        assert state == (m.length, m.high, m.declared, m.depth)
        self.before()
        return self.record(Op("refused", kind, seed, via), [], action, refused=REFUSALS2[kind])

    # -- drawing --

    def emit(self, name):
        if name == "drop":
            return self.drop(must=True)
        if name == "combine":  # (its first call the combine: no pair, which begins with the simplification)
            return self.combine(source=f"{('render', 'tensor')[int(self.rng.integers(0, 2))]}/{self.draw_tree()}")
        if name in PASSES2:
            return {"rects": self.q_rects, "components": self.q_components}[name]()
        return super().emit(name)

    def floats(self):
        """whether some anchor drops a leaf: a component that does not hold the cell (0, 0, 0)"""
        g = self.m.grid
        return bool(Q.label_grid((g != 0).astype(np.int64))[1] > (1 if g[0, 0, 0] else 0))

    def step(self):
        """the next op: what settles a need of this session if one can be settled now (of several, one that writes and is
        itself waited for behind), else a free draw from both tables"""
        r = self.rng.random()
        if self.m.length > CAPACITY // 3:
            return self.compact(True)
        waited = {a for a, _ in self.needs}
        if self.last_refusal is not None:
            mine = [b for k, b in self.refusal_needs if k == self.last_refusal]
            if mine:
                return self.emit(sorted(mine, key=lambda b: b not in waited)[0])
        if self.last is not None:
            mine = [b for a, b in self.needs if a == self.last]
            if mine:
                return self.emit(sorted(mine, key=lambda b: b not in waited)[0])
        if r < 0.88 and (self.needs or self.refusal_needs):
            if self.needs and (not self.refusal_needs or r < 0.4):
                need = self.needs[0]
                if need[0] == "drop" and not self.floats():
                    return self.edit()  # (nothing floats: voxels strewn in, for the next draw)
                self.emit(need[0])
                if self.last != need[0] and self.needs and self.needs[0] == need:
                    self.needs.append(self.needs.pop(0))  # (no such write on this tree: later)
                return None
            if self.refused(self.refusal_needs[0][0]) is False:
                self.refusal_needs.append(self.refusal_needs.pop(0))  # (not on this tree: later)
                return self.emit("edit")
            return None
        if r < 0.93:
            return self.frame()
        if r < 0.95:
            kind = tuple(ALL_REFUSALS)[int(self.rng.integers(0, len(ALL_REFUSALS)))]
            return self.refused(kind) or None
        return self.emit(ALL_PASSES[int(self.rng.integers(3, len(ALL_PASSES)))])

    def every_new_pass(self):
        """each of the four new entry points on a tree of the size that stands, behind a combine that appended to it"""
        self.combine(source=f"render/list/{self.seed():#x}/120", op="over", at_level=0)
        self.q_rects(self.m.depth)
        self.q_components(self.m.depth, with_indices=True, with_sizes=True)
        self.drop(must=True)


def make_session2(pkg, seed, needs=(), refusal_needs=()):
    """about 70 ops: a depth-6 tree over a scan tile in groups with every new pass on it, a small tree with every new pass
    again in the workspaces the large tree grew, then trees at depth 5 and 6 until every pair of this session stood side by side"""
    g = Gen2(pkg, seed, needs, refusal_needs)
    g.build("list", 6, g.seed(), 5000)
    g.every_new_pass()
    g.build("list", 5, g.seed(), 60)
    g.every_new_pass()
    builds = (("dense", 5, g.seed(), 1500), ("solid", 5, 1, 1), ("list", 6, g.seed(), 2500), ("mesh", 5, 1, 0))
    for k in range(len(builds)):
        if not (g.needs or g.refusal_needs):
            break
        g.phase(builds[(k + seed) % len(builds)], 14)
    guard = 0
    while (g.needs or g.refusal_needs) and guard < 200:
        g.step()
        guard += 1
    g.frame()
    return g.steps


def worst_combinations(pkg):
    """The new passes beside their nasty neighbours, on one context."""
    g = Gen2(pkg, 9)
    m = g.m
    # rests of the owner: behind a write of either new writer the deal must not replay, behind a call that writes nothing it
    # goes on replaying.  session_ops.Tracker knows a replay for certain only in the first DEAL_LEARN frames of an accepted
    # rest, so the three calls that write nothing stand once inside that window, between frames that must be replayed, and
    # once each directly behind a 34-frame rest, where a replay may go on and the ops alone do not say that it does
    g.build("list", 5, 41, 2000, False)
    g.frame(REST_POSE, 34)
    g.combine("over", "render/ball", 1, (1, 0, 1), via=False)
    g.frame(REST_POSE, 2)
    g.frame(REST_POSE, 34)
    g.combine("carve", "tensor/list/0x2a/150", 0, (0, 0, 0), via=True)
    g.frame(REST_POSE, 34)
    assert g.drop(None, False, via=True)["mutates"]
    g.frame(REST_POSE, 8)
    assert not g.drop(None, False)["mutates"]           # (everything that floated is gone)
    g.frame(REST_POSE, 2)
    g.q_rects(5, False, 2, False)
    g.frame(REST_POSE, 2)
    g.q_components(5, False, True, True)
    g.frame(REST_POSE, 2)
    g.frame(REST_POSE, 34)
    g.drop(None, False)
    g.frame(REST_POSE, 34)
    g.q_rects(None, True, 1, True)
    g.frame(REST_POSE, 34)
    g.q_components(None, True, False, False)
    g.frame(REST_POSE, 3)

    # combine -> drop -> compact(prune) -> components -> rects on one tree, then on what an in-place cut leaves
    def chain(op, source, anchor):
        g.combine(op, source, 0, (0, 0, 0), via=False)
        g.drop(anchor, False, via=False)
        g.compact(True, False)
        g.q_components(m.depth, False, True, True)
        g.q_rects(m.depth, True, 3, False)

    g.edit(seed=43, n=200, via=False)
    chain("under", "tensor/ball", None)
    g.simplify(merge=False, cut_level=4, via=False)
    chain("paint", "render/list/0x2b/190", ((0, 0, 0), (16, 32, 16)))
    # the scene's own out-of-place simplification as the source, directly behind an in-place simplify
    g.simplify(merge=True, cut_level=None, via=False)
    g.combine("keep", "pair/cut3", via=False)
    g.q_rects(None, False, 4, True)
    g.combine("replace", "pair/merge", via=True)
    # each new pass directly behind every refusal of an old pass it shares with: a combine behind a region edit refused for
    # max_words, a rects behind a malformed surface, ...
    g.build("list", 5, 46, 1500, False)
    for kind, b in old_refusal_pairs2():
        assert g.refused(kind) is not False, kind
        g.emit(b)
    # a pillar on the floor carved through by a ball: the piece above floats, and a drop removes exactly that piece
    g.build("list", 5, 44, 0, False)
    pillar = [("box", (20, 0, 20), (28, 30, 28), 0x909090, G.MODE_SET), ("box", (22, 18, 22), (26, 22, 26), 0x20C020, G.MODE_SET)]
    g.region(shapes=pillar, records=[G.box(s[1], s[2], s[3], s[4]) for s in pillar], via=False)
    g.combine("carve", "tensor/cutter", 1, (1, 0, 1), via=False, words=ball_tree(4, (16, 16, 16), 14))
    step = g.q_components(5, False, True, True)
    assert step["want"]["out"][2] == 2, "the carve leaves no floating piece"
    step = g.drop(None, False, via=True)
    assert step["want"]["triple"][:2] == (2, 1) and not (m.grid[:, 13:, :] != 0).any() and (m.grid[:, :3, :] != 0).any()
    g.drop(None, True)
    # the 8-word empty tree as scene and as source, directly before and after the tree over a scan tile
    g.build("list", 6, 45, 0, True)
    g.q_rects(6, True, 2, False)
    g.q_components(None, True, True, True)
    g.drop(None, False)
    g.combine("over", "render/empty", 0, (0, 0, 0), via=False)
    g.combine("under", "tensor/list/0x2d/5000", 0, (0, 0, 0), via=False)
    assert groups_of(m.length) > TILE
    g.q_rects(6, False, 2, False)
    g.q_components(6, False, True, False)
    g.drop(((0, 0, 0), (64, 64, 20)), False, via=False)
    g.combine("paint", "render/ball", 0, (0, 0, 0), via=True)
    g.combine("keep", "tensor/empty", 0, (0, 0, 0), via=False)
    g.q_components(6, False, True, True)
    g.compact(True, False)
    assert m.length == 8
    g.q_rects(None, False, 1, True)
    g.q_components(6, True, False, True)
    g.drop(None, True)
    g.combine("replace", "render/empty", 2, (3, 0, 1), via=True)
    g.frame("corner", 2)
    return g.steps


NAMES2 = tuple(f"seed{seed}" for seed in SEEDS2) + ("worst_combinations",)
ALL_NAMES = P.NAMES + NAMES2


@functools.lru_cache(maxsize=None)
def session(name):
    """the steps of a session of either module, generated and modelled once per process; seeded session k of this module has
    every len(SEEDS2)-th new pair to put side by side, from the k-th on"""
    if name in P.NAMES:
        return P.session(name)
    pkg = P._package()
    if name == "worst_combinations":
        return worst_combinations(pkg)
    k = NAMES2.index(name)
    return make_session2(pkg, SEEDS2[k], all_pairs2()[k::len(SEEDS2)], all_refusal_pairs2()[k::len(SEEDS2)])
