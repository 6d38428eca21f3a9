"""Sessions of tree passes on one context (tests/test_pass_session_host.py, tests/test_pass_session_gpu.py): a seeded generator of
pass calls, the hand-written session worst_transitions(), and a host model that answers every call from the restatements alone
(build_ref, edit_ref, region_ref, compact_ref, simplify_ref, list_ref, surface_ref, sample_ref, structure_ref, voxelize_ref,
solid_ref).  Nothing here touches a GPU; the package is needed for mesh.icosphere and mesh.quantize_vertices, which run on the host.

An op is a session_ops.Op and reprs to one line.  `via` on a mutating op: through the second context that shares the node buffer.
  build(form, depth, a, b, via)   form: list (a: seed, b: n) | dense (a: seed, b: n) | mesh (a: subdivisions) | solid (a: subdivisions, b: merge)
  edit(seed, n, depth, via)       region(seed, k, depth, via)       compact(prune, via)
  simplify(merge, cut_level, min_level, out_of_place, via)
  stamp(form, seed, via)          form: steps (column_tops, structure_sites, stamp_structures, edit_nodes) | scatter (the one call)
                                        | place (place_structures at origins of the seed's)
  list(depth, expand, with_levels)   surface(depth, closed, keep_hidden)   quads(depth, closed)   sample(seed, n, depth)
  dense(origin, size)   tops(origin_xz, size_xz, y_range)       depth None: the depth the context has declared
  frame(pose, repeat)             traced by the owner
  refused(kind, seed, via)        a call the model predicts will be refused (REFUSALS); the malformed kinds write one word by
                                  svo_nodes_scatter before the call and put it back after

A session is generated and modelled in one go, because what an op means depends on the tree it meets (cells already present, one
word short of what the call needs): session(name) returns its steps, one dict per op with the concrete inputs of the call,
what it must return, the words the device must hold after it and what the host test tallies.  The model also keeps a second state,
a dense grid of cell values that only the per-cell contracts update; after every mutating op the words, sampled, must equal it.

The passes that came later -- combine, rects (surface_rects), components (label_components) and drop (drop_floating), their
refusal kinds and the sessions seed301..seed303 and worst_combinations() -- stand in pass_session_ops2.py, which reuses Gen and
Model.  PASSES, SHARED, REFUSALS and the seven sessions here stay as they are: a name added to them would reshuffle
all_pairs() and with it every session, and tests/golden/pass_session_ops.txt pins their op lines.
"""
import collections
import functools
import os

import numpy as np

import build_ref as B
import compact_ref as K
import edit_ref as E
import list_ref as L
import region_ref as G
import sample_ref as SM
import simplify_ref as R
import solid_ref as Z
import structure_ref as T
import surface_ref as F
import voxelize_ref as V
from conftest import GOLDEN
from session_ops import OUTSIDE, Op

CAPACITY = 1 << 19
DECLARED = 16          # SVO_OPT_TREE_DEPTH's default: no tree of a session is deeper, so the declared depth never rises
TILE, SMALL = 4096, 512  # groups: a scan tile (kTile, csrc/svo_scan.h); what counts as a small input
FILL = 0x00BEEF        # the interior of a solid mesh
POSES = {"close": OUTSIDE["close"], "far": OUTSIDE["far"], "corner": ((1.3, 1.1, -1.5), (-0.6, -0.5, 0.7))}
REST_POSE = "close"    # the cube fills the frame: SVO_OPT_CULL = 2 filters nothing, so the static deal may replay

PASSES = ("build", "build_dense", "build_mesh", "edit", "region", "compact", "simplify",
          "list", "surface", "sample", "dense", "tops", "structure")
MUTATING = PASSES[:7]
# which passes share what (csrc/svo_ctx.h): a refusal of one is followed directly by a call of each of the others
SHARED = {
    "svo_tree_walk": ("compact", "simplify", "list"),
    "svo_list_plan": ("list", "surface", "structure"),
    "svo_build_leaves": ("build", "build_mesh", "edit"),
    "scan_tiles": ("build", "build_dense", "build_mesh", "edit", "region", "compact", "simplify", "list", "surface"),
}
# refusal kind -> (the pass refused, the error class's name, a fragment of the library's message)
REFUSALS = {
    "max_words_build": ("build", "SvoError", "max_words"),
    "max_words_edit": ("edit", "SvoError", "max_words"),
    "max_words_region": ("region", "SvoError", "max_words"),
    "edit_depth": ("edit", "SvoError", "is an interior node at depth"),
    "region_depth": ("region", "SvoError", "which is an interior node at depth"),
    "list_depth": ("list", "SvoError", "deeper than depth ="),
    "surface_depth": ("surface", "SvoError", "deeper than depth ="),
    "dense_box": ("dense", "SvoError", "the box leaves the grid"),
    "simplify_min_level": ("simplify", "SvoError", "min_level must be 0 without"),
    # beyond the calls that are refused for what they ask: a tree that is refused for what it holds.  One reachable interior
    # pointer is moved off the multiple of 8 by svo_nodes_scatter, the pass is called, the word is put back.  These are the
    # refusals that leave a status word set on the device (SVO_WALK_ALIGN), which the next call's reset has to clear.
    "malformed_compact": ("compact", "SvoError", "is not a multiple of 8"),
    "malformed_simplify": ("simplify", "SvoError", "is not a multiple of 8"),
    "malformed_list": ("list", "SvoError", "is not a multiple of 8"),
    "malformed_surface": ("surface", "SvoError", "is not a multiple of 8"),
}
DISCOVERY = ("compact", "list", "simplify", "surface")  # the passes that run svo_tree_discover and its checks
SEEDS = (201, 202, 203, 204, 205, 206)


def partners(kind):
    """the passes that share a workspace with the pass that refusal `kind` refuses (itself among them)"""
    p = REFUSALS[kind][0]
    if kind.startswith("malformed"):
        return list(DISCOVERY)
    return sorted({q for group in SHARED.values() if p in group for q in group})


def all_pairs():
    return [(a, b) for a in MUTATING for b in PASSES]


def all_refusal_pairs():
    return [(kind, b) for kind in REFUSALS for b in partners(kind)]


@functools.lru_cache(maxsize=None)
def tree_structure():
    """tree.vox of tests/golden/structures_vox.npz by the restatement: (offsets, index, colours)"""
    z = np.load(os.path.join(GOLDEN, "structures_vox.npz"))
    return T.load_structure(tuple(int(v) for v in z["tree_size"]), z["tree_xyzi"], z["tree_palette"])


def groups_of(n_words):
    return n_words // 8


# ---- the model ----

class Refusal(Exception):
    """the model's verdict on a call: refused, with the fragment the library's message must carry"""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


class Model:
    """The words the device must hold (up to the highest length reached), node_length, the declared depth, and the dense grid
    of cell values at the depth of the last build that only the per-cell contracts update."""

    def __init__(self, pkg):
        self.pkg = pkg
        self.buf = np.full(CAPACITY, B.EMPTY, dtype=np.uint32)
        self.length = self.high = 8
        self.declared = DECLARED
        self.depth = 5
        self.grid = np.zeros((32,) * 3, dtype=np.uint32)
        self.over = False  # a call that was not refused went over the capacity

    def words(self):
        return self.buf[:self.length]

    def d(self, depth):
        return self.declared if depth is None else depth

    def canonical(self):
        return np.array_equal(K.compact(self.buf, self.length, False)[0], self.words())

    # -- the writes: each takes the concrete inputs, returns what the call returns and leaves both states updated --

    def _store(self, new, freed=False):
        """new words from word 0; freed: the tail up to the old length holds the empty word"""
        if new.size > CAPACITY:
            self.over = True
            raise OverflowError(new.size)
        self.buf[:new.size] = new
        if freed and new.size < self.length:
            self.buf[new.size:self.length] = B.EMPTY
        self.length = new.size
        self.high = max(self.high, new.size)
        return new.size

    def _declare(self, depth):
        self.declared = max(self.declared, depth)

    def build(self, coords, depth, colours, merge=False):
        self._declare(depth)
        n = self._store(B.build(coords, depth, colours))
        if merge:  # (the wrapper's simplify_nodes() after the build: the tail it frees holds the empty word)
            n = self._store(R.simplify(self.buf, n)[0], freed=True)
        # the cells: the last voxel of a cell wins; a merge changes no cell
        self.depth, self.grid = depth, np.zeros((1 << depth,) * 3, dtype=np.uint32)
        keys, col, index = E.distinct(coords, depth, colours) if len(coords) else (None, np.zeros(0), np.zeros(0, dtype=np.int64))
        c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)[index]
        self.grid[c[:, 0], c[:, 1], c[:, 2]] = col
        return n

    def edit(self, coords, depth, colours):
        try:
            new = E.edit(self.buf, self.length, coords, depth, colours)
        except E.Refused:
            raise Refusal("edit_depth") from None
        before, n_before = self.words().copy(), self.length
        self._declare(depth)
        n = self._store(new)
        self._cells_edit(before, n_before, coords, depth, colours)
        return n

    def _cells_edit(self, before, n_before, coords, depth, colours):
        """the edit per cell: the last entry of a cell wins, colour 0 empties, and a coarser leaf met on the way down is split
        into EMPTY children, so the rest of its cube is empty afterwards"""
        f = self.depth - depth
        keys, col, index = E.distinct(coords, depth, colours)
        c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)[index]
        level = SM.sample(before, n_before, c << f, self.depth)[1].astype(np.int64)
        g = self.grid
        for cell, l in zip(c[level < depth], level[level < depth]):
            s = depth - l
            lo, w = (cell >> s) << (s + f), 1 << (s + f)
            g[lo[0]:lo[0] + w, lo[1]:lo[1] + w, lo[2]:lo[2] + w] = 0
        w = 1 << f
        for cell, v in zip(c << f, col):
            g[cell[0]:cell[0] + w, cell[1]:cell[1] + w, cell[2]:cell[2] + w] = v

    def region(self, records, depth):
        sh = G.shapes(records)
        try:
            new, _ = G.edit(self.buf, self.length, sh, depth)
        except G.Refused:
            raise Refusal("region_depth") from None
        assert depth == self.depth
        self._declare(depth)
        n = self._store(new)
        self.grid = G.apply_cells(self.grid, depth, sh)
        return n

    def compact(self, prune):
        return self._store(K.compact(self.buf, self.length, prune)[0], freed=True)

    def simplify(self, merge, cut_level, min_level, out_of_place):
        try:
            R.check_params(merge, cut_level, min_level or 0)
        except ValueError:
            raise Refusal("simplify_min_level") from None
        out = R.simplify(self.buf, self.length, merge, cut_level, min_level or 0)[0]
        if out_of_place:
            return out
        if cut_level is not None:
            self.grid = R.cut_cells(self.buf, self.length, self.depth, cut_level)
        # (a merge: every cell samples to what it sampled before -- merged_cells -- so the grid stays)
        return self._store(out, freed=True)

    def cells_differ(self):
        """the words sampled over the whole grid against the grid of the per-cell contracts: (cells that differ, FINER cells,
        the levels of the coloured leaves)"""
        side = 1 << self.depth
        got, level, _ = SM.sample(self.buf, self.length, SM.box_cells((0, 0, 0), (side,) * 3), self.depth)
        levels = tuple(int(v) for v in np.unique(level[(got != 0) & (got < SM.FINER)]))
        return int((got.reshape(self.grid.shape) != self.grid).sum()), int((got == SM.FINER).sum()), levels

    # -- the queries --

    def list(self, depth, expand):
        try:
            return L.list_voxels(self.buf, self.length, self.d(depth), expand)
        except L.TooDeep:
            raise Refusal("list_depth") from None

    def surface(self, depth, flags):
        try:
            return F.list_surface(self.buf, self.length, self.d(depth), flags)
        except L.TooDeep:
            raise Refusal("surface_depth") from None

    def sample(self, cells, depth):
        return SM.sample(self.buf, self.length, cells, self.d(depth))

    def dense(self, origin, size):
        try:
            return SM.sample_dense(self.buf, self.length, origin, size, self.depth)
        except ValueError:
            raise Refusal("dense_box") from None

    def tops(self, origin, size, y_range):
        lo, hi = (0, 1 << self.depth) if y_range is None else y_range
        return T.column_tops_skipping(self.buf, self.length, origin, size, self.depth, lo, hi)


# ---- the generator ----

def mesh_voxels(pkg, depth, subdivisions, solid):
    """(vq, triangles, triangle colours, the voxel list of the wrapper: the interior in FILL, then the surface)"""
    v, t = pkg.mesh.icosphere(subdivisions, 0.55, (0.05, -0.1, 0.2))
    vq = pkg.mesh.quantize_vertices(v, depth)
    colours = 0x010000 + np.arange(len(t))
    coords, cell_colours = V.voxelize(vq, t, depth, colours)[:2]
    coords, cell_colours = coords.astype(np.int64), cell_colours.astype(np.int64)
    if solid:
        res = Z.solid(vq, t, depth)
        assert res.n_open == 0
        inner = res.cells.astype(np.int64)
        coords = np.concatenate([inner, coords])
        cell_colours = np.concatenate([np.full(len(inner), FILL, dtype=np.int64), cell_colours])
    return vq, t, colours, coords, cell_colours


class Gen:
    """Draws ops, models them and keeps the steps.  `needs`: the (pass A, pass B) pairs and (refusal kind, pass B) pairs this
    session has to put side by side; the rest of its ops are drawn freely."""

    def __init__(self, pkg, seed, needs=(), refusal_needs=()):
        self.pkg, self.rng = pkg, np.random.default_rng(seed)
        self.m = Model(pkg)
        self.steps = []
        self.pose = REST_POSE
        self.needs, self.refusal_needs = list(needs), list(refusal_needs)
        self.last = None          # the pass of the in-place write or refusal kind directly before, if the last op was one
        self.last_refusal = None

    # -- bookkeeping --

    def record(self, op, calls, action, want=None, refused=None, mutates=False, groups_in=None):
        m = self.m
        step = {"op": op, "calls": calls, "action": action, "want": want, "refused": refused, "mutates": mutates, "via": bool(action.get("via")),
                "writes": action.get("writes", 1 if mutates else 0),  # calls that reach svo_store_note_write
                "groups_in": self._groups_in if groups_in is None else groups_in, "canonical_in": self._canonical_in,
                "length": m.length, "high": m.high, "declared": m.declared, "depth": m.depth, "pose": self.pose,
                "words": None, "cells_differ": None, "levels": None}
        if mutates:
            step["words"] = m.buf[:m.high].copy()
            differ, finer, step["levels"] = m.cells_differ()
            step["cells_differ"] = (differ, finer)
        self.steps.append(step)
        # what is side by side
        if refused:
            self.last, self.last_refusal = None, op.args[0]
        elif op.kind == "frame":
            self.last = self.last_refusal = None
        else:
            self.last, self.last_refusal = (calls[-1] if mutates else None), None
        return step

    def before(self):
        self._groups_in, self._canonical_in = groups_of(self.m.length), None

    def via(self):
        return bool(self.rng.random() < 0.34)

    def seed(self):
        return int(self.rng.integers(0, 1 << 16))

    def note(self, first_call):
        """an op whose first call is `first_call` comes now: strike what it settles"""
        if self.last_refusal is not None and (self.last_refusal, first_call) in self.refusal_needs:
            self.refusal_needs.remove((self.last_refusal, first_call))
        if self.last is not None and (self.last, first_call) in self.needs:
            self.needs.remove((self.last, first_call))

    # -- builds --

    def build(self, form, depth, a, b=0, via=None):
        via = self.via() if via is None else via
        m, pkg = self.m, self.pkg
        self.before()
        op = Op("build", form, depth, a, b, via)
        call = {"list": "build", "dense": "build_dense", "mesh": "build_mesh", "solid": "build_mesh"}[form]
        self.note(call)
        side = 1 << depth
        if form in ("list", "dense"):
            rng = np.random.default_rng(a)
            coords, colours = rng.integers(0, side, (b, 3)), rng.integers(1, 1 << 24, b)
            action = {"via": via, "coords": coords, "colours": colours, "depth": depth}
            if form == "dense":
                grid = np.zeros((side,) * 3, dtype=np.uint32)
                keys, col, index = E.distinct(coords, depth, colours)
                grid[tuple(coords[index].T)] = col
                coords, colours = B.dense_to_voxels(grid)
                action = {"via": via, "grid": grid, "depth": depth}
            n = m.build(coords, depth, colours)
        else:
            vq, t, tri_colours, coords, colours = mesh_voxels(pkg, depth, a, form == "solid")
            action = {"via": via, "vq": vq, "triangles": t, "colours": tri_colours, "depth": depth, "solid": form == "solid", "merge": bool(b)}
            n = m.build(coords, depth, colours, merge=bool(b))
        return self.record(op, [call], action, want={"ret": n}, mutates=True, groups_in=groups_of(n))

    # -- edits --

    def edit_inputs(self, seed, n, depth):
        """a third of the cells already present, a quarter of all removed; below the grid's depth: random cells"""
        m = self.m
        rng = np.random.default_rng(seed)
        side = 1 << depth
        coords = rng.integers(0, side, (n, 3))
        if depth == m.depth:
            present = np.argwhere(m.grid != 0)
            k = min(n // 3, len(present))
            if k:
                coords[:k] = present[rng.choice(len(present), k, replace=False)]
            coords[-1] = coords[0]  # (one cell twice: the last entry wins)
        colours = np.where(rng.random(n) < 0.25, 0, rng.integers(1, 1 << 24, n))
        return coords, colours

    def edit(self, seed=None, n=None, depth=None, via=None):
        m = self.m
        seed = self.seed() if seed is None else seed
        n = int(self.rng.integers(30, 400)) if n is None else n
        depth = m.depth if depth is None else depth
        via = self.via() if via is None else via
        self.before()
        self._canonical_in = None
        coords, colours = self.edit_inputs(seed, n, depth)
        op = Op("edit", seed, n, depth, via)
        self.note("edit")
        ret = m.edit(coords, depth, colours)
        return self.record(op, ["edit"], {"via": via, "coords": coords, "colours": colours, "depth": depth}, want={"ret": ret}, mutates=True)

    def region_records(self, seed, k, depth):
        """k boxes and balls in all three modes, some boxes empty after clipping: (what the wrapper takes, the records of the
        restatement, clipped as the wrapper clips)"""
        rng = np.random.default_rng(seed)
        side = 1 << depth
        shapes, records = [], []
        for i in range(k):
            mode = int(rng.integers(1, 4))
            colour = 0 if rng.random() < 0.3 else int(rng.integers(1, 1 << 24))
            if rng.random() < 0.5:
                lo = rng.integers(-4, side, 3)
                hi = lo + rng.integers(1, max(2, side // 3), 3)
                if i == 1:
                    lo, hi = np.array([side, 0, 0]), np.array([side + 5, 4, 4])  # empty after clipping
                shapes.append(("box", tuple(int(v) for v in lo), tuple(int(v) for v in hi), colour, mode))
                a, b = np.maximum(lo, 0), np.minimum(hi, side)
                if (a < b).all():
                    records.append(G.box(a.tolist(), b.tolist(), colour, mode))
            else:
                c2 = rng.integers(0, 2 * side + 1, 3)
                r2 = int(rng.integers(1, max(2, side // 2)))
                shapes.append(("ball", tuple(float(v) / 2 for v in c2), r2 / 2, colour, mode))
                records.append(G.ball(c2.tolist(), r2, colour, mode))
        return shapes, records

    def region(self, seed=None, k=None, depth=None, via=None, shapes=None, records=None):
        m = self.m
        depth = m.depth if depth is None else depth
        via = self.via() if via is None else via
        if shapes is None:
            seed = self.seed() if seed is None else seed
            k = int(self.rng.integers(1, 7)) if k is None else k
            shapes, records = self.region_records(seed, k, depth)
            while not records:
                seed += 1
                shapes, records = self.region_records(seed, k, depth)
        self.before()
        op = Op("region", seed, k, depth, via)
        self.note("region")
        ret = m.region(records, depth)
        return self.record(op, ["region"], {"via": via, "shapes": shapes, "depth": depth}, want={"ret": ret}, mutates=True)

    def compact(self, prune=None, via=None):
        prune = bool(self.rng.random() < 0.6) if prune is None else prune
        via = self.via() if via is None else via
        self.before()
        self._canonical_in = self.m.canonical()
        self.note("compact")
        ret = self.m.compact(prune)
        return self.record(Op("compact", prune, via), ["compact"], {"via": via, "prune": prune}, want={"ret": ret}, mutates=True)

    def simplify(self, merge=None, cut_level=-1, min_level=None, out_of_place=False, via=None):
        m = self.m
        if merge is None:
            merge = bool(self.rng.random() < 0.7)
        if cut_level == -1:
            cut_level = None if merge and self.rng.random() < 0.6 else int(self.rng.integers(2, m.depth + 1))
        if min_level is None and merge and self.rng.random() < 0.3:
            min_level = int(self.rng.integers(2, m.depth))
        via = (self.via() if via is None else via) and not out_of_place
        self.before()
        self._canonical_in = m.canonical()
        self.note("simplify")
        op = Op("simplify", merge, cut_level, min_level, out_of_place, via)
        ret = m.simplify(merge, cut_level, min_level, out_of_place)
        action = {"via": via, "merge": merge, "cut_level": cut_level, "min_level": min_level, "out_of_place": out_of_place}
        if out_of_place:
            step = self.record(op, ["simplify"], action, want={"words": ret})
            self.last = None  # (no write)
            return step
        return self.record(op, ["simplify"], action, want={"ret": ret}, mutates=True)

    def stamp(self, form=None, seed=None, via=None):
        """a few trees on the ground of a rectangle (or, `place`, at origins of the seed's)"""
        m = self.m
        form = ("steps", "scatter", "place")[int(self.rng.integers(0, 3))] if form is None else form
        seed = self.seed() if seed is None else seed
        via = self.via() if via is None else via
        rng = np.random.default_rng(seed)
        side = 1 << m.depth
        offsets, _, colours = tree_structure()
        self.before()
        self._canonical_in = m.canonical()
        action = {"via": via, "form": form, "depth": m.depth, "seed": seed}
        want = {}
        if form == "place":
            k = int(rng.integers(1, 5))
            origins = rng.integers(-3, side + 3, (k, 3)).astype(np.int32)
            rots = rng.integers(0, 4, k).astype(np.uint32)
            calls = ["structure", "edit"]
            action.update(origins=origins, rots=rots)
        else:
            o = rng.integers(0, side // 2, 2)
            s = rng.integers(side // 4, side // 2 + 1, 2)
            top, value = m.tops(o.tolist(), s.tolist(), None)
            columns = int((top != T.TOP_NONE).sum())
            if not columns:
                return None
            one_in = max(1, columns // 6)
            origins, rots = T.sites(top, value, o.tolist(), one_in, seed)
            while not len(origins) and one_in > 1:
                one_in = max(1, one_in // 2)
                origins, rots = T.sites(top, value, o.tolist(), one_in, seed)
            if not len(origins):
                return None
            calls = ["tops", "structure", "edit"]
            action.update(origin=tuple(o.tolist()), size=tuple(s.tolist()), one_in=one_in)
            want.update(tops=top, values=value, origins=origins, rots=rots)
        xyz, colour, _ = T.stamp(offsets, colours, origins, rots, m.depth)
        if not len(xyz):
            return None
        want.update(coords=xyz, colours=colour)
        self.note(calls[0])
        want["ret"] = m.edit(xyz.astype(np.int64), m.depth, colour.astype(np.int64))
        return self.record(Op("stamp", form, seed, via), calls, action, want=want, mutates=True)

    # -- queries --

    def query_depth(self):
        return None if self.rng.random() < 0.3 else self.m.depth

    def q_list(self, depth=-1, expand=None, with_levels=None):
        m = self.m
        depth = self.query_depth() if depth == -1 else depth
        expand = bool(depth is not None and self.rng.random() < 0.4) if expand is None else expand
        with_levels = bool(self.rng.random() < 0.5) if with_levels is None else with_levels
        self.before()
        self._canonical_in = m.canonical()
        self.note("list")
        return self.record(Op("list", depth, expand, with_levels), ["list"], {"depth": depth, "expand": expand, "with_levels": with_levels},
                           want={"out": m.list(depth, expand)})

    def q_surface(self, quads=None, depth=-1):
        m = self.m
        depth = self.query_depth() if depth == -1 else depth
        quads = bool(self.rng.random() < 0.4) if quads is None else quads
        closed = bool(self.rng.random() < 0.5)
        keep = bool(not quads and self.rng.random() < 0.4)
        self.before()
        self._canonical_in = m.canonical()
        self.note("surface")
        flags = (F.CLOSED_BOUNDARY if closed else 0) | (F.KEEP_HIDDEN if keep else 0) | (F.QUADS if quads else 0)
        op = Op("quads", depth, closed) if quads else Op("surface", depth, closed, keep)
        return self.record(op, ["surface"], {"depth": depth, "closed": closed, "keep_hidden": keep, "quads": quads, "flags": flags},
                           want={"out": m.surface(depth, flags)})

    def q_sample(self, seed=None, n=None, depth=-1):
        m = self.m
        seed = self.seed() if seed is None else seed
        n = int(self.rng.integers(1, 300)) if n is None else n
        depth = self.query_depth() if depth == -1 else depth
        rng = np.random.default_rng(seed)
        d = m.d(depth)
        cells = rng.integers(0, 1 << m.depth, (n, 3)) << (d - m.depth)
        cells += rng.integers(0, 1 << (d - m.depth), (n, 3)) if d > m.depth else 0
        k = min(n // 4, 8)  # cells outside the grid, negative ones among them
        if k:
            cells[:k] = rng.integers(-3, (1 << d) + 3, (k, 3))
            cells[0] = (1 << d, 0, 0)
            cells[k - 1] = (0, -1, 0)
        self.before()
        self._canonical_in = m.canonical()
        self.note("sample")
        return self.record(Op("sample", seed, n, depth), ["sample"], {"cells": cells, "depth": depth}, want={"out": m.sample(cells, depth)})

    def q_dense(self, whole=None):
        m = self.m
        side = 1 << m.depth
        if whole is None:
            whole = self.rng.random() < 0.3 and m.depth < 7
        origin = (0, 0, 0) if whole else tuple(int(v) for v in self.rng.integers(0, side - 9, 3))
        size = (side,) * 3 if whole else tuple(int(v) for v in self.rng.integers(1, 10, 3))
        self.before()
        self.note("dense")
        return self.record(Op("dense", origin, size), ["dense"], {"origin": origin, "size": size}, want={"out": m.dense(origin, size)})

    def q_tops(self):
        m = self.m
        side = 1 << m.depth
        o = tuple(int(v) for v in self.rng.integers(0, side // 2, 2))
        s = tuple(int(v) for v in self.rng.integers(1, side // 2 + 1, 2))
        y_range = None
        if self.rng.random() < 0.5:
            lo = int(self.rng.integers(0, side - 1))
            y_range = (lo, int(self.rng.integers(lo + 1, side + 1)))
        self.before()
        self._canonical_in = m.canonical()
        self.note("tops")
        return self.record(Op("tops", o, s, y_range), ["tops"], {"origin": o, "size": s, "y_range": y_range}, want={"out": m.tops(o, s, y_range)})

    def frame(self, pose=None, repeat=None):
        if pose is None:
            pose = tuple(POSES)[int(self.rng.integers(0, len(POSES)))]
        repeat = (1, 2)[int(self.rng.integers(0, 2))] if repeat is None else repeat
        self.pose = pose
        self.before()
        return self.record(Op("frame", pose, repeat), [], {}, groups_in=0)

    # -- refusals --

    def refused(self, kind, via=None):
        """a call the model refuses; False when the tree as it stands gives no such refusal"""
        m = self.m
        seed = self.seed()
        via = (self.via() if via is None else via) and REFUSALS[kind][0] in MUTATING
        side = 1 << m.depth
        action = {"via": via, "kind": kind, "depth": m.depth}
        state = (m.length, m.high, m.declared, m.depth)
        probe = Model.__new__(Model)  # the call on a copy of the words: what it would need, or its refusal
        probe.__dict__.update(m.__dict__, buf=m.buf.copy(), grid=m.grid.copy())
        try:
            if kind == "max_words_build":
                rng = np.random.default_rng(seed)
                n = int(rng.integers(50, 400))
                coords, colours = rng.integers(0, side, (n, 3)), rng.integers(1, 1 << 24, n)
                action.update(coords=coords, colours=colours, max_words=B.build(coords, m.depth, colours).size - 1)
            elif kind == "max_words_edit":
                coords, colours = self.edit_inputs(seed, 60, m.depth)
                need = probe.edit(coords, m.depth, colours)
                if need <= m.length:
                    return False
                action.update(coords=coords, colours=colours, max_words=need - 1)
            elif kind == "max_words_region":
                shapes, records = self.region_records(seed, 4, m.depth)
                need = probe.region(records, m.depth) if records else 0
                if need <= m.length:
                    return False
                action.update(shapes=shapes, max_words=need - 1)
            elif kind == "edit_depth":
                present = np.argwhere(m.grid != 0)
                if m.depth < 2 or not len(present):
                    return False
                coords = present[np.random.default_rng(seed).choice(len(present), min(20, len(present)), replace=False)] >> 1
                action.update(coords=coords, colours=np.full(len(coords), 0x123456), depth=m.depth - 1)
                probe.edit(coords, m.depth - 1, action["colours"])
                return False
            elif kind == "region_depth":
                half = side // 2
                shapes = [("box", (0, 0, 0), (half, half, half), 0x00FF00, G.MODE_VOXELS)]
                action.update(shapes=shapes, depth=m.depth - 1)
                G.edit(m.buf, m.length, G.shapes([G.box((0, 0, 0), (half,) * 3, 0x00FF00, G.MODE_VOXELS)]), m.depth - 1)
                return False
            elif kind == "list_depth":
                action.update(depth=m.depth - 1)
                probe.list(m.depth - 1, False)
                return False
            elif kind == "surface_depth":
                action.update(depth=m.depth - 1)
                L.list_voxels(m.buf, m.length, m.depth - 1)
                return False
            elif kind == "dense_box":
                action.update(origin=(side - 2, 0, 1), size=(4, 3, 2))
                probe.dense(action["origin"], action["size"])
                return False
            elif kind == "simplify_min_level":
                action.update(merge=False, cut_level=2, min_level=3)
                probe.simplify(False, 2, 3, False)
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
                probe.buf[at] = action["bad"]
                {"compact": lambda: probe.compact(True), "simplify": lambda: probe.simplify(True, None, None, False),
                 "list": lambda: probe.list(m.depth, False), "surface": lambda: probe.surface(m.depth, 0)}[REFUSALS[kind][0]]()
                return False
        except (Refusal, G.Refused, L.TooDeep, K.Malformed):
            pass
        except OverflowError:
            return False
        assert state == (m.length, m.high, m.declared, m.depth)
        self.before()
        return self.record(Op("refused", kind, seed, via), [], action, refused=REFUSALS[kind])

    # -- drawing --

    def emit(self, name):
        """an op whose first call is pass `name`, of a size like the tree's; None when the tree gives none"""
        m = self.m
        if name == "build":
            return self.build("list", m.depth, self.seed(), self.size_like())
        if name == "build_dense":
            return self.build("dense", m.depth, self.seed(), self.size_like())
        if name == "build_mesh":
            if groups_of(m.length) > TILE and m.depth == 6:
                return self.build("solid", 6, 2, 0)
            if groups_of(m.length) < SMALL:
                return self.build("mesh", 4, 0)
            return self.build(*(("mesh", 5, 1, 0), ("solid", 5, 1, 1), ("solid", 5, 1, 0))[int(self.rng.integers(0, 3))])
        if name == "structure":
            return self.stamp("place")
        return {"edit": self.edit, "region": self.region, "compact": self.compact, "simplify": self.simplify, "list": self.q_list,
                "surface": self.q_surface, "sample": self.q_sample, "dense": self.q_dense, "tops": self.q_tops}[name]()

    def size_like(self):
        g = groups_of(self.m.length)
        if g > TILE:
            return 5000
        if g < SMALL:
            return int(self.rng.integers(20, 80))
        return int(self.rng.integers(1500, 5001))

    def step(self):
        """the next op: what settles a need of this session if one can be settled now, else a free draw"""
        r = self.rng.random()
        if self.last_refusal is not None:
            mine = [b for k, b in self.refusal_needs if k == self.last_refusal]
            if mine:
                return self.emit(mine[0])
        if self.last is not None:
            mine = [b for a, b in self.needs if a == self.last]
            if mine:
                return self.emit(mine[0])
        if r < 0.55 and (self.needs or self.refusal_needs):
            if self.needs and (not self.refusal_needs or r < 0.3):
                return self.emit(self.needs[0][0])
            if self.refused(self.refusal_needs[0][0]) is False:
                self.refusal_needs.append(self.refusal_needs.pop(0))  # (not on this tree: later)
                return self.emit("edit")
            return None
        if r < 0.75:
            return self.frame()
        if r < 0.8:
            kind = tuple(REFUSALS)[int(self.rng.integers(0, len(REFUSALS)))]
            return self.refused(kind) or None
        if r < 0.84:
            return self.stamp()
        return self.emit(PASSES[int(self.rng.integers(3, len(PASSES)))])

    def phase(self, build, n_ops):
        """a build, then n_ops steps on what it made"""
        self.build(*build)
        end = len(self.steps) + n_ops
        for _ in range(4 * n_ops):
            if len(self.steps) >= end:
                break
            self.step()

    def every_pass(self):
        """each of the thirteen entry points once on a tree of the size that stands"""
        for name in ("edit", "region", "list", "surface", "sample", "dense"):  # (the queries meet what the edits appended)
            self.emit(name)
        self.refused("dense_box")
        for name in ("tops", "compact", "edit", "simplify"):
            self.emit(name)
        self.stamp("steps") or self.stamp("place")
        self.stamp("place")
        for name in ("build_mesh", "build_dense", "build"):
            self.emit(name)

    def rest(self, then):
        """a rest of 34 frames of the owner, long enough for the static deal's replay, directly before `then`"""
        self.frame(REST_POSE, 34)
        then()
        self.frame(REST_POSE, 2)


def make_session(pkg, seed, needs=(), refusal_needs=()):
    """about 100 ops: a depth-6 tree over a scan tile in groups with every pass on it, a small tree with every pass again, then
    trees at depth 5 and 6 under free draws; every second session a depth-7 stretch; rests before writes of every kind"""
    g = Gen(pkg, seed, needs, refusal_needs)
    k = seed % 6
    g.build("list", 6, g.seed(), 5000)
    g.edit(n=300)
    g.every_pass()                      # above a tile (the last three builds keep the size)
    g.build("list", 5, g.seed(), 60)
    g.every_pass()                      # under 512 groups, in the workspaces the large tree grew
    g.phase(("dense", 5, g.seed(), 1500 + 500 * k), 14)
    rests = (lambda: g.edit(via=False), lambda: g.region(via=False), lambda: g.compact(via=False), lambda: g.simplify(merge=True, cut_level=None, via=False),
             lambda: g.build("list", 5, g.seed(), 2000, False), lambda: g.edit(via=True),
             lambda: g.simplify(merge=True, cut_level=None, out_of_place=True))
    g.rest(rests[k])
    g.rest(rests[(k + 3) % 7])
    if seed % 2:
        g.phase(("list", 7, g.seed(), 10000), 6)
    g.phase(("list", 6, g.seed(), 1500 + 600 * k), 10)
    g.phase(("solid", 6, 2, 1), 8)
    guard = 0
    while (g.needs or g.refusal_needs) and guard < 120:
        g.step()
        guard += 1
    g.frame()
    return g.steps


def worst_transitions(pkg):
    """The nasty neighbours side by side, on one context."""
    g = Gen(pkg, 7)
    level_boxes = [("box", (0, 0, 0), (16, 16, 16), 0x101010, 3), ("box", (16, 16, 16), (24, 24, 24), 0x202020, 3),
                   ("box", (24, 24, 24), (28, 28, 28), 0x303030, 3), ("box", (28, 28, 28), (30, 30, 30), 0x404040, 3)]
    # a solid merged at the build, then voxels put into the merged solid by cell list: the documented colour trap
    g.build("solid", 6, 2, 1, False)
    g.frame(REST_POSE, 2)
    rng = np.random.default_rng(1)
    inner = np.argwhere(g.m.grid == FILL)
    coords = inner[rng.choice(len(inner), 40, replace=False)]
    g.before()
    g.note("edit")
    ret = g.m.edit(coords, 6, np.full(40, 0xFF0000))
    g.record(Op("edit", "into the merged solid", 40, 6, False), ["edit"], {"via": False, "coords": coords, "colours": np.full(40, 0xFF0000), "depth": 6},
             want={"ret": ret}, mutates=True)
    # the same by shapes, which carry the colour down; leaves of every level from 2 to 6
    g.region(shapes=level_boxes, records=[G.box(s[1], s[2], s[3], s[4]) for s in level_boxes], via=False)
    g.q_list(6, False, True)
    # a cut, then a region edit at full depth, then an edit at the cut's level
    g.simplify(merge=False, cut_level=4, via=False)
    g.region(seed=11, k=5, via=False)
    g.simplify(merge=True, cut_level=3, via=True)
    g.edit(seed=12, n=50, depth=3, via=False)
    g.compact(True, False)
    # an out-of-place simplify between two replayed frames of a rest
    g.build("list", 6, 21, 5000, False)
    g.frame(REST_POSE, 24)
    g.simplify(merge=True, cut_level=None, out_of_place=True)
    g.frame(REST_POSE, 4)
    g.simplify(merge=False, cut_level=4, out_of_place=True)
    g.frame(REST_POSE, 6)
    # a compaction through the sharing context during a rest of the owner
    g.edit(seed=22, n=300, via=False)
    g.frame(REST_POSE, 34)
    g.compact(True, True)
    g.frame(REST_POSE, 34)
    g.simplify(merge=True, cut_level=None, out_of_place=True)
    g.frame(REST_POSE, 3)
    # a refusal of each pass directly before a call of each other pass that shares a workspace with it
    for kind in REFUSALS:
        for b in partners(kind):
            if groups_of(g.m.length) > 3 * TILE or g.m.length > CAPACITY // 3:
                g.build("list", 6, g.seed(), 3000, False)
            if g.refused(kind) is False:
                g.build("list", 6, g.seed(), 3000, False)
                assert g.refused(kind) is not False, kind
            assert g.emit(b) is not None
    # the depth-7 tree directly before and after the 8-word empty tree
    g.build("list", 7, 31, 10000, False)
    g.q_surface(False, 7)
    g.build("list", 7, 32, 0, True)
    g.q_list(7, True, True)
    g.q_surface(True, None)
    g.compact(True, False)
    g.simplify(merge=True, cut_level=None, via=False)
    g.q_tops()
    g.build("list", 7, 33, 10000, True)
    g.compact(False, True)
    g.frame("corner", 2)
    return g.steps


NAMES = tuple(f"seed{seed}" for seed in SEEDS) + ("worst_transitions",)


@functools.lru_cache(maxsize=None)
def _package():
    import __graft_entry__ as entry
    return entry.build()


@functools.lru_cache(maxsize=None)
def session(name):
    """the steps of a session, generated and modelled once per process (the host test and the GPU test share them); seeded
    session k has every len(SEEDS)-th pair to put side by side, from the k-th on"""
    pkg = _package()
    if name == "worst_transitions":
        return worst_transitions(pkg)
    k = NAMES.index(name)
    return make_session(pkg, SEEDS[k], all_pairs()[k::len(SEEDS)], all_refusal_pairs()[k::len(SEEDS)])


def owner_ops(steps):
    """The session as the owner's trace path sees it, in session_ops ops for session_ops.Tracker: a camera where the pose changes,
    one render per frame the owner traces, one write per call that reaches svo_store_note_write.  A frame op is the owner's; the
    two frames behind a mutating op are traced by the context that did not write.  Returns (ops, per step the number of owner
    frames)."""
    ops, frames, pose = [Op("flags", True, False, False)], [], None
    for s in steps:
        op, n = s["op"], 0
        ops += [Op("write", "edit", s["via"], 0)] * s["writes"]
        if (op.kind == "frame" or (s["mutates"] and s["via"])) and s["pose"] != pose:
            pose = s["pose"]
            ops.append(Op("camera", pose))
        if op.kind == "frame":
            n = op.args[1]
        elif s["mutates"] and s["via"]:
            n = 2
        if n:
            ops.append(Op("frame", "render", None, n))
        frames.append(n)
    return ops, frames


class Views:
    """what session_ops.Tracker asks of its pools: the uniforms of a pose"""

    def __init__(self, O):
        self.O, self._u = O, {}

    def uniforms(self, pose, size=(64, 64), flags=1):
        key = (pose, size, flags)
        if key not in self._u:
            pos, look = POSES[pose]
            self._u[key] = self.O.make_uniforms(pos=pos, look=look, width=size[0], height=size[1], flags=flags)
        return self._u[key]


def tallies(steps):
    t = collections.Counter()
    for s in steps:
        t["ops"] += 1
        t[s["op"].kind] += 1
        t["refused"] += s["refused"] is not None
        t["through the sharing context"] += s["via"]
        t["mutating"] += s["mutates"]
    return t
