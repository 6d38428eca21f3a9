"""Whole sessions on one context (tests/test_session_host.py, tests/test_session_gpu.py): a seeded generator of calls, the
hand-written session worst_transitions(), a host model that answers every call from the CPU oracle alone, and the translation of a
session into the lines tests/schedule_plan_driver.cpp reads, so that the strip schedule's state after every frame is predicted by
the policy in csrc/svo_sched.h and not by the glue that is under test.  Nothing here touches a GPU.

An op is a small record that reprs to one line:
  camera(pose)  size(w, h)  flags(pause_adaptive, shadows, misc_bool)  option(name, value)
  frame(kind, arg, repeat)   kind: render | tile (arg: rect) | tiles (arg: tw, th, first, stride) | shaded (arg: rect or None)
                                   | secondary (arg: n) | rays (arg: n, seed)
  write(kind, via_share, arg)  kind: scatter_same | scatter_colour | tree (arg: pool name) | edit | scan  (arg: a seed otherwise)
"""
import os
import subprocess

import numpy as np

import edit_ref as E
import trace_matrix_scenes as M
from conftest import load_vox_fixture

F_PAUSE, F_SHADOWS, F_MISC = 1, 8, 16
VOXEL_OFFSET = 1 << 27
LIST_LEARN, DEAL_LEARN, MAX_AGE = 16, 16, 64  # kBalanceLearnFrames, kDealLearnFrames, kSchedMaxAge

SIZES = ((64, 64), (96, 64), (67, 45), (197, 131), (256, 128),
         (328, 203),   # 68 224 items: the deferred-ray buffer regrows
         (520, 512))   # 4 160 strips: the schedule slot regrows (at most twice a session)
BIG = (520, 512)
REPEATS = (1, 2, 3, 17, 34)
OPTION_VALUES = {
    "CULL": (0, 1, 2), "SCHEDULE": (0, 1, 2), "STATIC_DEAL": (0, 1), "FUSED_SHADOWS": (0, 1, 2), "GRID_BLOCKS": (0, 1, 5, 64),
    "REFILL_MIN": (1, 32, 64), "BLOCK_SHAPE": (3, 4), "CAMERA_SHORTCUT": (0, 1), "SCHEDULE_MOTION": (0, 0x1204), "VARIANT": (0, 1),
    "TREE_DEPTH": (16, 17), "SCAN_CLEARS_COUNTERS": (0, 1),
}
DEFAULTS = {"CULL": 2, "SCHEDULE": 2, "STATIC_DEAL": 1, "FUSED_SHADOWS": 2, "GRID_BLOCKS": 0, "REFILL_MIN": 32, "BLOCK_SHAPE": 3,
            "CAMERA_SHORTCUT": 1, "SCHEDULE_MOTION": 0x1204, "VARIANT": 1, "TREE_DEPTH": 16, "SCAN_CLEARS_COUNTERS": 0}
FRAME_KINDS = ("render", "tile", "tiles", "shaded", "secondary", "rays")
WRITE_KINDS = ("scatter_same", "scatter_colour", "tree", "edit", "scan")
RAY_COUNTS = (1, 63, 64, 65, 1000, 4133)

# ---- the pools ----
TREES = ("small", "monu9", "terrain", "deep17")
TREE_DEPTH = {"small": 3, "monu9": 7, "terrain": 10, "deep17": 17}
# pose -> (pos, look); in_a / in_b are filled in from the package's terrain camera (test_deal_gpu's pair)
OUTSIDE = {
    "close": ((0.2, 0.1, -1.2), (0.0, 0.0, 1.0)),       # CULL_POSES[0]: the cube fills most of the frame
    "far": ((2.5, 1.5, -6.0), (-0.4, -0.25, 1.0)),      # CULL_POSES[2]
    "graze": ((0.0, 1.0005, -2.0), (0.0, 0.0, 1.0)),    # CULL_POSES[4]: grazing the face y = 1
    "away": ((1.5, 0.0, 0.0), (1.0, 0.0, 0.0)),         # CULL_POSES[8]: the cube lies behind the camera
    "defer": ((0.0, 0.0, -1.5), (0.0, 0.0, 1.5)),       # camera_inverse[0] *= 1e-30: the whole frame takes the deferred list
}
INSIDE = {"plane": ((0.0, 0.0, -0.2), (0.3, 0.1, 1.0))}  # exactly on the x = 0 and y = 0 centre planes
# Which poses a tree is seen from.  A pose is listed for a tree only when the oracle hits the model on 5 % .. 95 % of the rays at
# every size of SIZES (test_session_host.py holds the pools to that), except the poses declared below.
POSES = {
    "terrain": ("in_a", "in_b", "graze", "far", "away", "defer"),
    "monu9": ("in_a", "in_b", "plane", "close", "far", "away", "defer"),
    "small": ("close", "graze", "far", "away", "defer"),
    "deep17": ("lattice",),
}
SKY_ONLY = ("away",)      # every ray misses the cube
SKY_MOSTLY = ("far",)     # the cube covers a few blocks: exempt from the 5 % floor, but some ray must hit the model
DEFERRED = ("defer",)
FORCED_CULL = ("far", "graze", "away")  # the poses OPT_CULL = 1 is there for: 20 never-entered blocks and more at 256 x 128
IS_OUTSIDE = tuple(OUTSIDE)


def pose_ok(pose, size):
    """SVO_OPT_CULL = 2 culls when 40 % of a coarse grid of rays look past the cube; a pose is used only at sizes where that share
    is at most 20 % or at least 60 %.  The grazing pose misses with half of its rays in the two square frames."""
    return not (pose == "graze" and size[0] * 3 < size[1] * 4)


class Op(tuple):
    """(kind, args...); reprs to one line"""

    def __new__(cls, kind, *args):
        return super().__new__(cls, (kind,) + args)

    kind = property(lambda self: self[0])
    args = property(lambda self: tuple(self[1:]))

    def __repr__(self):
        return f"{self[0]}({', '.join(hex(a) if isinstance(a, int) and a > 4200 else repr(a) for a in self[1:])})"


def rects_of(size):
    """ragged rectangles of a frame: off the block grid, 1 x 1 in the last corner, a single row, an inner block"""
    w, h = size
    return ((3, 5, w - 7, h - 9), (w - 1, h - 1, 1, 1), (0, min(7, h - 1), w, 1), (w // 3, h // 4, w // 2 + 1, h // 3 + 1))


def tilings_of(size):
    """(tw, th) that cut the frame into whole tiles, more than one of them"""
    w, h = size
    out = [(w // a, h // b) for a in (1, 2, 4) for b in (1, 2, 4, 5, 8) if w % a == 0 and h % b == 0 and a * b > 1]
    return tuple(out)


# ---- the generator ----

class _Gen:
    def __init__(self, rng):
        self.rng = rng
        self.ops = []
        self.tree, self.pose, self.size, self.flags = "terrain", "in_a", (64, 64), (True, False, False)
        self.opt = dict(DEFAULTS)
        self.frames = 0
        self.big_used = 0

    def pick(self, seq, p=None):
        return seq[int(self.rng.choice(len(seq), p=p))]

    def emit(self, kind, *args):
        self.ops.append(Op(kind, *args))

    def camera(self):
        self.pose = self.pick([p for p in POSES[self.tree] if pose_ok(p, self.size)])
        self.emit("camera", self.pose)

    def resize(self):
        sizes = [s for s in SIZES if s != self.size and (s != BIG or self.big_used < 2) and pose_ok(self.pose, s)]
        self.size = self.pick(sizes)
        self.big_used += self.size == BIG
        self.emit("size", *self.size)

    def set_flags(self, pause=None):
        pause = bool(self.rng.random() < 0.7) if pause is None else pause
        self.flags = (pause, bool(self.rng.random() < 0.5), bool(self.rng.random() < 0.3))
        self.emit("flags", *self.flags)

    def option(self, name=None, value=None):
        name = self.pick(sorted(OPTION_VALUES)) if name is None else name
        values = OPTION_VALUES[name]
        if name == "TREE_DEPTH" and self.tree == "deep17":
            values = (17,)  # (a declared 16 over the depth-17 tree: the refusal, which refusal() scripts)
        value = self.pick(values) if value is None else value
        self.opt[name] = value
        self.emit("option", name, value)

    def frame(self, kind=None, repeat=None):
        kind = self.pick(FRAME_KINDS, p=(0.38, 0.12, 0.10, 0.16, 0.10, 0.14)) if kind is None else kind
        counting = not self.flags[0]
        if repeat is None:
            repeat = self.pick(REPEATS, p=(0.34, 0.25, 0.2, 0.13, 0.08))
        if self.frames > 400:
            repeat = min(repeat, 3)
        if counting and repeat > 3 and (self.size[0] * self.size[1] > 96 * 64 or kind != "render"):
            repeat = 3  # (every counting frame is an oracle frame of its own: the long stretch is a small plain one)
        if self.size[0] * self.size[1] > 256 * 128:
            repeat = min(repeat, 17)
        arg = None
        if kind == "tile":
            arg = self.pick(rects_of(self.size))
        elif kind == "tiles":
            tilings = tilings_of(self.size)
            if not tilings:
                kind = "render"
            else:
                tw, th = self.pick(tilings)
                n = (self.size[0] // tw) * (self.size[1] // th)
                first = int(self.rng.integers(0, min(n, 2)))
                arg = (tw, th, first, int(self.rng.integers(1, 4)))
        elif kind == "shaded":
            arg = self.pick(rects_of(self.size)) if self.rng.random() < 0.25 else None
        elif kind == "secondary":
            arg = 1 if counting else int(self.rng.integers(1, 4))  # (the oracle counts the shadow ray only)
        elif kind == "rays":
            arg = (self.pick(RAY_COUNTS), int(self.rng.integers(0, 1 << 16)))
        self.frames += repeat
        self.emit("frame", kind, arg, repeat)

    def write(self, kind=None, via_share=None):
        kind = self.pick(WRITE_KINDS, p=(0.25, 0.25, 0.2, 0.15, 0.15)) if kind is None else kind
        via_share = bool(self.rng.random() < 0.35) if via_share is None else via_share
        if kind == "tree":
            self.new_tree(self.pick([t for t in TREES if t != self.tree]), via_share)
        elif kind == "scan":
            self.emit("write", "scan", via_share, 0)
        else:
            self.emit("write", kind, via_share, int(self.rng.integers(0, 1 << 16)))

    def new_tree(self, tree, via_share=False):
        if self.tree == "deep17" and self.opt["TREE_DEPTH"] == 17 and self.rng.random() < 0.5:
            self.option("TREE_DEPTH", 16)  # back to the default stack (else the shallow tree stays on the deep one)
        self.tree = tree
        self.emit("write", "tree", via_share, tree)
        self.camera()
        if tree == "deep17" and self.opt["TREE_DEPTH"] < 17:
            if self.opt["VARIANT"] == 1 and self.rng.random() < 0.6:
                self.refusal()
            self.option("TREE_DEPTH", 17)

    def refusal(self):
        """a depth-17 tree under a declared depth of 16 on the STACK family: the frame is refused when it is waited for"""
        if not self.flags[0]:
            self.set_flags(pause=True)  # (what a refused frame counted is nobody's to say)
        self.frame("render", 1)

    def rest(self):
        """a plain static rest: list learning, deal learning, replay"""
        self.set_flags(pause=True)
        for name, value in (("VARIANT", 1), ("STATIC_DEAL", 1), ("GRID_BLOCKS", 0)):
            if self.opt[name] != value:
                self.option(name, value)
        if self.opt["SCHEDULE"] == 0:
            self.option("SCHEDULE", 2)
        if self.tree == "deep17" or self.opt["TREE_DEPTH"] != 16:
            if self.tree == "deep17":
                self.new_tree(self.pick(("terrain", "monu9")))
            if self.opt["TREE_DEPTH"] != 16:
                self.option("TREE_DEPTH", 16)
        if self.pose in IS_OUTSIDE and self.opt["CULL"] != 0:
            self.pose = self.pick([p for p in POSES[self.tree] if p not in IS_OUTSIDE] or ["close"])
            self.emit("camera", self.pose)
            if self.pose in IS_OUTSIDE:
                self.option("CULL", 0)
        if self.size[0] * self.size[1] > 256 * 128:
            self.size = self.pick([s for s in SIZES[:5] if pose_ok(self.pose, s)])
            self.emit("size", *self.size)
        self.frames += 37
        self.emit("frame", "render", None, 34)
        self.emit("frame", "render", None, 3)
        what = self.rng.random()
        if what < 0.3:
            self.write(self.pick(("scatter_same", "scatter_colour", "edit")), via_share=bool(self.rng.random() < 0.5))
        elif what < 0.5:
            self.option(self.pick(("REFILL_MIN", "CAMERA_SHORTCUT", "GRID_BLOCKS", "BLOCK_SHAPE")))
        elif what < 0.65:
            self.set_flags(pause=False)
            self.frame("render", 1)
            self.set_flags(pause=True)
        self.frame("render", 3)

    def step(self):
        what = self.pick(("camera", "size", "flags", "option", "frame", "write", "rest"), p=(0.13, 0.10, 0.08, 0.21, 0.35, 0.10, 0.03))
        if what == "rest" and self.frames > 330:
            what = "frame"
        {"camera": self.camera, "size": self.resize, "flags": self.set_flags, "option": self.option, "frame": self.frame,
         "write": self.write, "rest": self.rest}[what]()


def make_session(seed, n_ops=150):
    """n_ops ops (a few more when the last step was a scripted run) drawn with default_rng(seed); deterministic, no GPU"""
    g = _Gen(np.random.default_rng(seed))
    while len(g.ops) < n_ops:
        g.step()
    return g.ops


SEEDS = [101, 102, 103, 104, 105, 106, 107, 108]


def worst_transitions():
    """The interleavings that a stale table, a list of the wrong parity or a replay that no longer fits would need, chained on
    one context; a rest long enough for the schedule's 64-frame backstop among them."""
    o = []

    def add(kind, *args):
        o.append(Op(kind, *args))
    add("flags", True, False, False)
    add("size", 256, 128)
    add("camera", "in_a")
    # a rest into replay, a counting frame in the middle of it, the rest again
    add("frame", "render", None, 34)
    add("frame", "render", None, 3)
    add("flags", False, False, False)
    add("frame", "render", None, 1)
    add("flags", True, False, False)
    add("frame", "render", None, 34)
    add("frame", "render", None, 34)   # past the schedule's backstop (age 64) with the deal in place
    add("frame", "render", None, 3)
    # explicit rays on slot 0 between pixel frames of the resting view
    add("frame", "rays", (1000, 7), 1)
    add("frame", "render", None, 2)
    add("frame", "rays", (65, 8), 2)
    add("frame", "render", None, 17)
    # a write through a sharing context while the owner rests, then an option change, each followed by the same view
    add("write", "scatter_same", True, 11)
    add("frame", "render", None, 3)
    add("write", "scatter_colour", True, 12)
    add("frame", "render", None, 17)
    add("option", "REFILL_MIN", 1)
    add("frame", "render", None, 2)
    add("option", "GRID_BLOCKS", 64)
    add("frame", "render", None, 17)
    add("option", "GRID_BLOCKS", 0)
    add("option", "REFILL_MIN", 32)
    add("write", "edit", False, 13)
    add("frame", "render", None, 2)
    # a culled frame, then an unculled frame of another size; culled, then inside
    add("option", "CULL", 1)
    add("camera", "graze")
    add("frame", "render", None, 2)
    add("option", "CULL", 0)
    add("size", 197, 131)
    add("frame", "render", None, 2)
    add("option", "CULL", 2)
    add("camera", "far")
    add("frame", "render", None, 3)
    add("camera", "in_b")
    add("frame", "render", None, 2)
    # resize down, then up past the deferred buffer's first size; a shaded two-pass frame (slot 1) straight after the regrow
    add("size", 67, 45)
    add("frame", "render", None, 2)
    add("option", "FUSED_SHADOWS", 0)
    add("flags", True, True, False)
    add("size", 328, 203)
    add("frame", "shaded", None, 2)
    add("camera", "defer")
    add("frame", "shaded", None, 2)
    add("frame", "render", None, 1)
    # slot-1 frames, then a slot-0 rest
    add("camera", "in_a")
    add("size", 96, 64)
    add("frame", "secondary", 3, 2)
    add("frame", "shaded", (3, 5, 89, 55), 1)
    add("frame", "render", None, 34)
    add("frame", "render", None, 3)
    add("option", "FUSED_SHADOWS", 1)
    add("frame", "shaded", None, 2)
    add("frame", "secondary", 2, 1)
    add("frame", "render", None, 2)
    # counting frames with shadow rays, then the scan, with and without the counters cleared
    add("flags", False, True, False)
    add("size", 64, 64)
    add("frame", "shaded", None, 2)
    add("frame", "render", None, 17)
    add("write", "scan", False, 0)
    add("option", "SCAN_CLEARS_COUNTERS", 1)
    add("write", "scan", True, 0)
    add("frame", "secondary", 1, 1)
    add("option", "SCAN_CLEARS_COUNTERS", 0)
    add("flags", True, False, True)
    # the slot regrows (4 160 strips), tiles, scheduling off and on, the other block shape
    add("size", 520, 512)
    add("frame", "render", None, 2)
    add("frame", "tiles", (260, 128, 1, 3), 2)
    add("option", "SCHEDULE", 0)
    add("frame", "render", None, 2)
    add("option", "SCHEDULE", 1)
    add("frame", "render", None, 2)
    add("option", "BLOCK_SHAPE", 4)
    add("frame", "render", None, 2)
    add("option", "SCHEDULE", 2)
    add("option", "BLOCK_SHAPE", 3)
    add("size", 256, 128)
    # another tree through the sharing context; the depth-17 tree: refused under a declared 16, then the deep stack, then RESTART
    add("write", "tree", True, "monu9")
    add("camera", "close")
    add("frame", "render", None, 3)
    add("write", "tree", False, "deep17")
    add("camera", "lattice")
    add("frame", "render", None, 1)      # refused
    add("option", "TREE_DEPTH", 17)
    add("frame", "render", None, 3)
    add("frame", "shaded", None, 1)
    add("option", "VARIANT", 0)
    add("frame", "render", None, 2)
    add("option", "VARIANT", 1)
    add("frame", "tile", (3, 5, 249, 119), 2)
    add("write", "tree", False, "small")
    add("camera", "graze")
    add("option", "TREE_DEPTH", 16)     # the depth option changes kernel families between two frames
    add("frame", "render", None, 2)
    add("option", "TREE_DEPTH", 17)
    add("frame", "render", None, 2)
    add("option", "TREE_DEPTH", 16)
    add("option", "SCHEDULE_MOTION", 0)
    add("camera", "close")
    add("frame", "render", None, 2)
    add("option", "SCHEDULE_MOTION", 0x1204)
    add("write", "tree", False, "terrain")
    add("camera", "in_a")
    add("frame", "render", None, 1)
    add("camera", "in_b")
    add("frame", "render", None, 1)      # floored
    add("frame", "render", None, 2)      # the exact rebuild at rest
    return o


def sessions():
    """name -> ops: the committed seeds and the hand-written session"""
    out = {f"seed{seed}": make_session(seed) for seed in SEEDS}
    out["worst_transitions"] = worst_transitions()
    return out


# ---- trees, poses, rays ----

class Pools:
    """the trees (never written to), their poses' uniforms and explicit rays; needs the package's host code and the oracle"""

    def __init__(self, pkg, O):
        self.pkg, self.O = pkg, O
        self.words = {}
        for name in ("small", "monu9"):
            size, xyzi, pal, n, _ = load_vox_fixture(name)
            self.words[name] = pkg.CpuOctree.from_voxels(size, xyzi, pal).to_octree_words()
        cam, look = pkg.scenes.terrain_camera(0, 10)
        self.words["terrain"] = pkg.scenes.terrain(seed=0, max_depth=10, cam=cam, lod_c=150.0, max_words=2_000_000)
        self.words["deep17"] = np.array(M.scene(17).words)
        for w in self.words.values():
            w.setflags(write=False)
        self.poses = dict(OUTSIDE)
        self.poses.update(INSIDE)
        self.poses["in_a"] = (cam, look)
        self.poses["in_b"] = ((cam[0] + 0.013, cam[1] + 0.004, cam[2] - 0.009), look)
        self.capacity = max(w.size for w in self.words.values()) + (1 << 16)  # (room for what the edits append)
        self._u = {}

    def uniforms(self, pose, size, flags):
        key = (pose, size, flags)
        if key not in self._u:
            O = self.O
            if pose == "lattice":
                u = M.scene(17).uniforms(O, flags, size)
            else:
                pos, look = self.poses[pose]
                u = O.make_uniforms(pos=pos, look=look, width=size[0], height=size[1], flags=flags)
                if pose == "defer":
                    u.camera_inverse[0] *= 1e-30
            self._u[key] = u
        return self._u[key]

    def central_ray(self, pose):
        if pose == "lattice":
            return tuple(float(v) for v in M.scene(17).origin) + M.FORWARD
        pos, look = self.poses[pose]
        d = np.array(look, dtype=np.float64)
        return tuple(pos) + tuple(d / np.linalg.norm(d))

    def rays(self, tree, n, seed):
        """n explicit rays: random ones into and inside the cube (the depth-17 tree: its lattice rays), the first few replaced
        by NaN, inf and zero directions"""
        rng = np.random.default_rng(seed)
        if tree == "deep17":
            rays = M.scene(17).lattice_rays(max(n, 64))[:n].copy()
        else:
            d = rng.normal(size=(n, 3))
            rays = np.concatenate([rng.uniform(-1.4, 1.4, (n, 3)), d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)
        edge = np.array([[np.nan, 0, 0, 1, 0, 0], [0, 0, -2, np.nan, 0, 1], [0, 0, -2, 0, 0, np.inf], [np.inf, 0, 0, -1, 0, 0],
                         [0.0, 0.0, 0.0, 0, 0, 0], [0.1, 0.2, 0.3, 0, -1, 0], [0, 5, 0, 0, 1, 0]], dtype=np.float32)
        k = min(n - 1, edge.shape[0]) if n > 1 else 0
        rays[n - k:] = edge[:k]
        return rays


def cull_facts(u):
    """(outside, miss share) of svo_abi.cpp's cull_worthwhile, restated: the camera's position from camera_inverse, and the share
    of a 12 x 8 grid of rays that look past the cube (None where the function gives up: a w of 0)"""
    ci = [float(np.float32(v)) for v in u.camera_inverse]
    w = ci[15]
    if not abs(w) > 1e-20:
        return False, None
    o = [ci[12] / w, ci[13] / w, ci[14] / w]
    if not (abs(o[0]) > 1.001 or abs(o[1]) > 1.001 or abs(o[2]) > 1.001):
        return False, None
    miss = 0
    for j in range(8):
        for i in range(12):
            cx, cy = (i + 0.5) / 12 * 2.0 - 1.0, -((j + 0.5) / 8 * 2.0 - 1.0)
            d4 = [ci[r] * cx + ci[4 + r] * cy + ci[8 + r] + ci[12 + r] for r in range(4)]
            if not abs(d4[3]) > 1e-20:
                return True, None
            t0, t1 = -1e300, 1e300
            for k in range(3):
                d = d4[k] / d4[3] - o[k]
                if d == 0.0:
                    if abs(o[k]) > 1.0:
                        t1 = -1e300
                    continue
                a, b = (-1.0 - o[k]) / d, (1.0 - o[k]) / d
                t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
            if not (t1 >= 0.0 and t0 <= t1):
                miss += 1
    return True, miss / 96.0


_cull_facts = {}


def culls(u, mode):
    """does a pixel frame of these uniforms run the culling pass under SVO_OPT_CULL = mode?"""
    if mode == 0:
        return False
    key = bytes(u)
    if key not in _cull_facts:
        _cull_facts[key] = cull_facts(u)
    outside, miss = _cull_facts[key]
    if not outside:
        return False
    if mode == 1:
        return True
    return miss is not None and miss * 96 * 10 >= 96 * 4 - 1e-9


# ---- the launches of a session, and what the policy says about them ----

def work_rect(rect, shape):
    x0, y0, w, h = rect
    bw, bh = 1 << shape, 64 >> shape
    bpr = -(-w // bw)
    bprect = bpr * -(-h // bh)
    return dict(mode=0, x0=x0, y0=y0, w=w, h=h, shape=shape, bpr=bpr, bprect=bprect, n_rects=1, tiles_x=1, first=0, stride=0, n_items=bprect * 64)


def work_tiles(size, tiles, shape):
    tw, th, first, stride = tiles
    d = work_rect((0, 0, tw, th), shape)
    tiles_x = size[0] // tw
    n = tiles_x * (size[1] // th)
    n_rects = (n - first + stride - 1) // stride if first < n else 0
    d.update(mode=1, n_rects=n_rects, tiles_x=tiles_x, first=first, stride=stride, n_items=n_rects * d["bprect"] * 64)
    return d


def work_rays(n):
    return dict(mode=2, x0=0, y0=0, w=0, h=0, shape=0, bpr=1, bprect=1, n_rects=0, tiles_x=1, first=0, stride=0, n_items=n)


def deal_row_cap(order_cap, grid_blocks):
    """svo_deal.h: deal_row_cap"""
    if grid_blocks < 8 or ((grid_blocks + 7) // 8) * 4 > 1024:
        return 0
    w_min = (grid_blocks // 8) * 4
    longest = -(-order_cap // w_min)
    cap = 2
    while cap < 2 * longest + 1:
        cap *= 2
    return cap if cap <= 256 else 0


ROW_FIELDS = ("reset_shares", "feed_balance", "prior_costs", "measure", "reuse_costs", "build_lists", "floor", "balance_update",
              "valid", "order_filtered", "age", "balance_frames", "floored")
STATE_FIELDS = ("valid", "order_filtered", "age", "balance_frames", "floored")


class Tracker:
    """Follows a session without tracing anything: the uniforms, options, store version and work layouts the glue compares, and
    from them every STACK launch as a line of schedule_plan_driver.cpp.  plan(ops, driver) returns one record per frame (a
    repeat counts), each with its launches; after the driver has run, every launch carries the policy's row and what the static
    deal may do."""

    def __init__(self, pools):
        self.P = pools
        self.opt = dict(DEFAULTS)
        self.period = 2
        self.tree, self.pose, self.size, self.flags = "terrain", "in_a", (64, 64), F_PAUSE
        self.version = 2  # svo_nodes_alloc and the first svo_nodes_write have reached note_write
        self.epoch = 0    # SVO_OPT_SCHEDULE set: both slots lose their schedule, as if their layouts were new
        self.cams, self.layouts = {}, {}
        self.cap = [0, 0]
        self.defer_items = 0
        self.dropped = [False, False]
        self.launches, self.frames = [], []
        self.since = []  # ops since the last frame

    def uniforms(self):
        return self.P.uniforms(self.pose, self.size, self.flags)

    def stack(self):
        return self.opt["VARIANT"] == 1

    def apply(self, index, op):
        """a call that is no frame"""
        kind, a = op.kind, op.args
        self.since.append(op)
        if kind == "camera":
            self.pose = a[0]
        elif kind == "size":
            self.size = (a[0], a[1])
        elif kind == "flags":
            self.flags = (F_PAUSE if a[0] else 0) | (F_SHADOWS if a[1] else 0) | (F_MISC if a[2] else 0)
        elif kind == "option":
            self.opt[a[0]] = a[1]
            if a[0] == "SCHEDULE":
                if a[1]:
                    self.period = a[1]
                self.epoch += 1
                self.dropped = [True, True]
        elif kind == "write":
            if a[0] != "scan":
                self.version += 1  # (the scan writes counters only and does not reach note_write)
            if a[0] == "tree":
                self.tree = a[2]
        else:
            raise ValueError(op)

    def launch(self, slot, work, u, skip=False, count_rays=False, fused=False):
        n_strips = (work["n_items"] + 63) // 64
        sched = int(self.opt["SCHEDULE"] != 0)
        pixel = work["mode"] != 2
        filt = int(bool(sched and (skip or (pixel and culls(u, self.opt["CULL"])))))
        grow = int(bool(sched and self.cap[slot] < n_strips))
        if grow:
            self.cap[slot] = max(4096, n_strips)
        regrow = self.defer_items < work["n_items"]
        if regrow:
            self.defer_items = max(1 << 16, work["n_items"])
        cam = self.cams.setdefault(bytes(u), len(self.cams) + 1)
        layout = self.layouts.setdefault((self.epoch,) + tuple(sorted(work.items())), len(self.layouts) + 1)
        counting = (pixel or count_rays) and not (self.flags & F_PAUSE)
        deep = self.opt["TREE_DEPTH"] > 16
        blocks = -(-n_strips // 4)
        if self.opt["GRID_BLOCKS"]:
            blocks = min(blocks, self.opt["GRID_BLOCKS"])
        elif blocks > 1024:
            blocks = None  # (the device's own grid may be the smaller one)
        L = dict(slot=slot, work=work, n_strips=n_strips, sched=sched, filt=filt, grow=grow, defer_regrow=regrow, cam=cam,
                 version=self.version, counting=counting, fused=fused, skip=skip, deep=deep, blocks=blocks,
                 motion=self.opt["SCHEDULE_MOTION"], has_buffers=self.cap[slot] > 0,
                 plain=bool(self.opt["STATIC_DEAL"] and slot == 0 and pixel and not skip and not counting and not fused and not deep),
                 dropped=self.dropped[slot] and not sched,
                 line=(cam, self.version, layout, work["mode"], slot, work["n_rects"], filt, sched, self.opt["SCHEDULE_MOTION"],
                       self.period, 1, grow))
        if sched:
            self.dropped[slot] = False
        self.launches.append(L)
        return L

    def frame(self, index, op, rep):
        kind, arg, _ = op.args
        u = self.uniforms()
        shape = self.opt["BLOCK_SHAPE"]
        stack = self.stack()
        fusable = stack and self.opt["FUSED_SHADOWS"] != 0
        if kind in ("render", "tile", "shaded", "secondary"):
            rect = tuple(arg) if kind in ("tile", "shaded") and arg is not None else (0, 0) + self.size
            work = work_rect(rect, shape)
            pixels = rect[2] * rect[3]
        elif kind == "tiles":
            rect = None
            work = work_tiles(self.size, arg, shape)
            pixels = work["n_rects"] * arg[0] * arg[1]
        else:
            rect, work, pixels = None, work_rays(arg[0]), 0
        F = dict(index=index, rep=rep, op=op, kind=kind, arg=arg, u=u, tree=self.tree, pose=self.pose, size=self.size, flags=self.flags,
                 rect=rect, work=work, pixels=pixels, stack=stack, opt=dict(self.opt), since=self.since, launches=[],
                 refused=stack and TREE_DEPTH[self.tree] > (16 if self.opt["TREE_DEPTH"] <= 16 else 22),
                 counting=kind != "rays" and not (self.flags & F_PAUSE))
        self.since = []
        shadows = kind == "shaded" and bool(self.flags & F_SHADOWS)
        fused = (shadows or kind == "secondary") and fusable
        F["fused"], F["two_pass"] = fused, False
        if stack:
            F["launches"].append(self.launch(0, work, u, fused=fused))
        second = 0
        if shadows and not fused:
            second = pixels
        elif kind == "secondary":
            second = pixels * (arg - (1 if fused else 0))
        if second:
            F["two_pass"] = True
            if stack:
                F["launches"].append(self.launch(1, work_rays(second), u, skip=True, count_rays=True))
        self.frames.append(F)
        return F

    def plan(self, ops, driver):
        for i, op in enumerate(ops):
            if op.kind == "frame":
                for rep in range(op.args[2]):
                    self.frame(i, op, rep)
            else:
                self.apply(i, op)
        rows = run_driver(driver, [L["line"] for L in self.launches])
        built, prev_bf, run = [None, None], [0, 0], 0
        for L, row in zip(self.launches, rows):
            s = L["slot"]
            if L["grow"]:
                built[s], prev_bf[s] = None, 0
                if s == 0:
                    run = 0
            L["row"] = row
            L["want_state"] = {f: row[f] for f in STATE_FIELDS}
            if L["dropped"]:
                L["want_state"]["valid"] = 0  # (the option dropped the schedule; with scheduling off no frame has built one since)
            if s == 0:
                at_rest = built[0] == (L["cam"], L["version"])
                ok = L["plain"] and L["sched"] and not L["filt"] and row["lists"] == "L" and at_rest and prev_bf[0] >= LIST_LEARN
                cap = None if L["blocks"] is None else deal_row_cap((L["n_strips"] + 3) // 4 + 32, L["blocks"])
                L["deal_grow"] = bool(L["grow"])
                if not ok or cap == 0:
                    run, L["replay"] = 0, 0          # DealFacts forbid it: the table is dropped
                elif cap is None or run < 0:
                    run, L["replay"] = -1, None      # (a grid this model does not know: either)
                else:
                    run += 1
                    L["replay"] = 1 if run <= DEAL_LEARN else None  # learning: replayed; then the device's verdict decides
                L["deal_run"] = run
            if row["measure"] or row["reuse_costs"]:
                built[s] = (L["cam"], L["version"])
            prev_bf[s] = row["balance_frames"]
        return self.frames


def run_driver(driver, lines):
    stdin = "".join(" ".join(str(v) for v in line) + "\n" for line in lines)
    out = subprocess.run([driver], input=stdin, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    rows = []
    for text in out:
        _, a, b, c = text.split("|")
        a, vals = a.split(), [int(v) for v in b.split() + c.split()]
        row = dict(zip(ROW_FIELDS, [int(v) for v in a[1:]] + vals))
        row["lists"] = a[0]
        rows.append(row)
    return rows


def build_driver(directory):
    """compile tests/schedule_plan_driver.cpp, unchanged, into `directory`"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(str(directory), "schedule_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(os.path.dirname(here), "octree-tracer_amd", "csrc"),
                           os.path.join(here, "schedule_plan_driver.cpp"), "-o", exe])
    return exe


# ---- the model ----

class Model:
    """The node words the device must hold and, from the oracle alone, what every call must return.  The oracle's answers are kept
    by (tree words, uniforms, call): the records of a frame do not depend on the hit counters (test_session_host.py checks that),
    so a counting stretch costs one count_frame a frame and a rest of 34 frames one oracle frame."""

    def __init__(self, pools, O, threads=8):
        self.P, self.O, self.threads = pools, O, threads
        self.buf = np.zeros(pools.capacity, dtype=np.uint32)
        first = pools.words["terrain"]
        self.buf[:first.size] = first
        self.length = first.size
        self.tree = "terrain"
        self.structure = 0  # changes with every write to the tree (the counters apart)
        self.cache = {}
        self.saturated = False
        self.scans = []

    def words(self):
        return self.buf[:self.length]

    def _ask(self, call, u, fn):
        key = (self.structure, bytes(u), call)
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def records(self, u, rect):
        """(h, w) records of a rectangle of the frame"""
        return self._ask(("trace", rect), u, lambda: self.O.trace_frame(self.words(), u, tile=rect, threads=self.threads))

    def resolve(self, op, pose):
        """the concrete write of a write op on the words as they are, seen from `pose`: (what, ...) for the model and for the
        device alike"""
        kind, _, arg = op.args
        w = self.words()
        if kind == "tree":
            return ("write", self.P.words[arg], arg)
        if kind == "scan":
            return ("scan",)
        rng = np.random.default_rng(arg)
        if kind == "scatter_same":
            at = rng.integers(0, self.length, 1)
            return ("scatter", at.astype(np.uint32), w[at].copy())
        if kind == "scatter_colour":
            leaves = np.flatnonzero((w >> 4) > VOXEL_OFFSET)
            at = rng.choice(leaves, min(64, leaves.size), replace=False)
            return ("scatter", at.astype(np.uint32), ((VOXEL_OFFSET + rng.integers(1, 1 << 24, at.size)) << 4).astype(np.uint32))
        if kind == "edit":
            depth = TREE_DEPTH[self.tree]
            side = 1 << depth
            centre = np.array([side // 2] * 3)
            # a cluster where the view's central ray meets the model, so that the edit shows
            ray = np.array(self.P.central_ray(pose), dtype=np.float32)
            rec = self.O.trace_rays(w, ray[None])[0]
            if (rec["info"] >> 16) & 1 and np.isfinite(rec["t"]):
                p = ray[:3].astype(np.float64) + ray[3:].astype(np.float64) * float(rec["t"])
                centre = np.clip(((p + 1.0) * 0.5 * side).astype(np.int64), 0, side - 1)
            n = 48
            coords = np.clip(centre + rng.integers(-3, 4, (n, 3)), 0, side - 1)
            colours = np.where(rng.random(n) < 0.25, 0, rng.integers(1, 1 << 24, n))
            return ("edit", coords.astype(np.int32), depth, colours.astype(np.int32))
        raise ValueError(op)

    def write(self, action, clears=False):
        """apply a resolved write; returns the scan's sorted lists for a scan"""
        what = action[0]
        if what == "scan":
            sub, unsub = self.O.scan(self.words(), node_length=self.length)
            lists = (np.sort(sub[1:1 + sub[0]]), np.sort(unsub[1:1 + unsub[0]]))
            self.scans.append((lists[0].size, lists[1].size))
            if clears:
                self.buf[:self.length] &= ~np.uint32(15)
            return lists
        if what == "write":
            self.buf[:action[1].size] = action[1]
            self.length = max(self.length, action[1].size)
            self.tree = action[2]
        elif what == "scatter":
            self.buf[action[1]] = action[2]
        elif what == "edit":
            new = E.edit(self.buf, self.length, action[1], action[2], action[3])
            self.buf[:new.size] = new
            self.length = new.size
        self.structure += 1
        return None

    def frame(self, F):
        """what frame F must return: dict(records, secondary, image, rays); a counting frame advances the words"""
        O, u, kind, arg = self.O, F["u"], F["kind"], F["arg"]
        out = {}
        if kind == "rays":
            rays = self.P.rays(F["tree"], arg[0], arg[1])
            out["rays"] = rays
            out["records"] = self._ask(("rays", arg), u, lambda: O.trace_rays(self.words(), rays, flags=F["flags"], threads=self.threads))
            return out
        rect = F["rect"]
        if kind == "tiles":
            tw, th, first, stride = arg
            tx = F["size"][0] // tw
            full = self.records(u, (0, 0) + F["size"])
            rects = [((t % tx) * tw, (t // tx) * th, tw, th) for t in range(first, tx * (F["size"][1] // th), stride)]
            out["records"] = np.stack([full[y:y + h, x:x + w] for x, y, w, h in rects])
        else:
            rects = [rect]
            if kind == "secondary":
                prim, sec = self._ask(("secondary", rect, arg), u, lambda: O.secondary_frame(self.words(), u, arg, tile=rect, threads=self.threads))
                out["records"], out["secondary"] = prim, sec
            else:
                out["records"] = self.records(u, rect)
            if kind == "shaded":
                img = self._ask(("shade", rect), u, lambda: O.shade_frame(self.words(), u, tile=rect, threads=self.threads))
                out["image"] = np.floor(np.clip(img, 0, 1) * 255.0 + 0.5).astype(np.int32)
        if F["counting"]:
            # shader.wgsl:276: the shadow ray counts like a primary one -- of a shaded frame when the shadows flag is set, of
            # render_secondary always (its ray 0); a plain frame traces none
            cu = O.Uniforms.from_buffer_copy(bytes(u))
            if kind == "secondary":
                cu.flags = u.flags | F_SHADOWS
            elif kind != "shaded":
                cu.flags = u.flags & ~F_SHADOWS
            words = self.words()
            for r in rects:
                words = O.count_frame(words, cu, tile=r)
            self.buf[:self.length] = words
            self.saturated = self.saturated or bool(((words & 15) == 15).any())
        return out


def block_records(records, work, strip):
    """the records behind strip `strip` of a pixel layout: records is (h, w) or (n_rects, h, w)"""
    rec = records if records.ndim == 3 else records[None]
    r, b = divmod(strip, work["bprect"])
    by, bx = divmod(b, work["bpr"])
    bw, bh = 1 << work["shape"], 64 >> work["shape"]
    return rec[r, by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw]


def all_zero(rec):
    return not np.ascontiguousarray(rec).view(np.uint32).any()
