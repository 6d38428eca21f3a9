"""Whole sessions on one context, frame by frame against the oracle (tests/session_ops.py): about 150 calls a session -- cameras,
sizes, flags, options, six kinds of frame, writes to the tree through the context and through a second one that shares its node
buffer -- on a context that is never renewed, so that what trace_launch keeps between frames (two schedule slots, the static deal,
the deferred-ray lists and their parity, the claim counters, the top table, the buffers that regrow) is exercised in combination
and deep into its life.  After every call: records bit-exact in a poisoned buffer with an untouched tail, shaded images within 1
of the oracle's, the node words after every counting frame, write and scan, the schedule slot's state equal to what the policy of
svo_sched.h gives for the frame (tests/schedule_plan_driver.cpp, unchanged), its lists complete (or, filtered, short of exactly
the strips that hold nothing), and the deal replaying when and only when its facts allow.  Nothing that depends on a measured time
is asserted.  A failure names the session, the op and the twelve ops before it: a prefix of the session replays it."""
import collections

import numpy as np
import pytest

import sched_ref as R
import session_ops as S
from conftest import assert_hits_equal, set_uniforms_from_oracle
from test_deal_gpu import check_table

pytestmark = pytest.mark.gpu

EQUAL = np.array([8192 * k for k in range(9)], dtype=np.uint32)
SLACK = 64  # records behind an output's end that must keep the poison
HALT = []   # a HIP error met by an earlier case: nothing more is started on the GPU in this run


@pytest.fixture(scope="module")
def pools(pkg, O):
    return S.Pools(pkg, O)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return S.build_driver(tmp_path_factory.mktemp("session_plan"))


@pytest.fixture
def contexts(pkg):
    """a context of the case's own, and the second one that shares its node buffer (on a stream of its own)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if HALT:
        pytest.fail(f"not started: an earlier session met a device error ({HALT[0]})")
    owner, other = pkg.Gpu(0), pkg.Gpu(0)
    other.use_own_stream()
    yield owner, other
    other.close()
    owner.close()


class Session:
    def __init__(self, pkg, O, pools, driver, name, ops, gpus):
        import torch
        self.torch, self.pkg, self.O, self.P, self.name, self.ops = torch, pkg, O, pools, name, ops
        self.gpu, self.gpu2 = gpus
        self.frames = S.Tracker(pools).plan(ops, driver)
        self.model = S.Model(pools, O)
        G = pkg.gpu
        for opt, v in S.DEFAULTS.items():
            self.gpu.set_option(getattr(G, "OPT_" + opt), v)
        self.opt = dict(S.DEFAULTS)
        self.render = pkg.Render(self.gpu, (64, 64), pools.words["terrain"], capacity=pools.capacity)
        self.share = None
        self.compute = pkg.Compute(self.gpu, self.render)
        self.pose, self.size, self.flags = "in_a", (64, 64), S.F_PAUSE
        self.upload()
        self.bufs = {}
        self.replayed = 0
        self.traced = False
        self.at = 0
        self.tally = collections.Counter()

    def upload(self):
        set_uniforms_from_oracle(self.render, self.P.uniforms(self.pose, self.size, self.flags))

    def out(self, what, n):
        """a poisoned int32 device buffer for n entries of `what` (4 words each for records) and SLACK more"""
        words = 4 if what != "rgba" else 1
        key = (what, n)
        if key not in self.bufs:
            if len(self.bufs) > 24:
                self.bufs.clear()
            self.bufs[key] = self.torch.empty(((n + SLACK), words) if words > 1 else (n + SLACK,), dtype=self.torch.int32,
                                              device=self.gpu.torch_device)
        self.bufs[key].fill_(-1)  # 0xFF bytes
        return self.bufs[key]

    def context(self):
        lo = max(0, self.at - 12)
        lines = [f"session {self.name}, op {self.at}: {self.ops[self.at]!r}; the ops before it:"]
        lines += [f"  {k}: {self.ops[k]!r}" for k in range(lo, self.at)]
        try:
            for slot in (0, 1):
                st = self.gpu.schedule_status(slot)
                lines.append(f"  schedule slot {slot}: " + ", ".join(f"{f}={st[f]}" for f in self.gpu.SCHEDULE_INFO))
        except self.pkg.SvoError as e:
            lines.append(f"  schedule: {e}")
        try:
            lines.append(f"  deal: {self.gpu.deal_status()}")
        except self.pkg.SvoError as e:
            lines.append(f"  deal: {e}")
        return "\n".join(lines)

    def run(self):
        k = 0
        try:
            for self.at, op in enumerate(self.ops):
                if op.kind == "frame":
                    for rep in range(op.args[2]):
                        F = self.frames[k]
                        k += 1
                        assert (F["index"], F["rep"]) == (self.at, rep)
                        self.frame(F, f"frame {rep} of {op!r}")
                else:
                    self.apply(op)
            print(f"{self.name}: {dict(self.tally)}")
        except AssertionError as e:
            raise AssertionError(f"{e}\n{self.context()}") from None
        except self.pkg.SvoError as e:
            HALT.append(f"{self.name}, op {self.at}: {e}")
            raise

    # ---- calls that are no frame ----

    def apply(self, op):
        kind, a = op.kind, op.args
        if kind == "camera":
            self.pose = a[0]
            self.upload()
        elif kind == "size":
            self.size = (a[0], a[1])
            self.upload()
        elif kind == "flags":
            self.flags = (S.F_PAUSE if a[0] else 0) | (S.F_SHADOWS if a[1] else 0) | (S.F_MISC if a[2] else 0)
            self.upload()
        elif kind == "option":
            self.gpu.set_option(getattr(self.pkg.gpu, "OPT_" + a[0]), a[1])
            if a[0] == "SCAN_CLEARS_COUNTERS":  # (the one option a write through the sharing context looks at)
                self.gpu2.set_option(self.pkg.gpu.OPT_SCAN_CLEARS_COUNTERS, a[1])
            self.opt[a[0]] = a[1]
        elif kind == "write":
            self.write(op)

    def write(self, op):
        what, via_share, _ = op.args
        action = self.model.resolve(op, self.pose)
        r = self.render
        if via_share:
            if self.share is None:
                self.share = self.pkg.Render.share_nodes(self.gpu2, self.render)
            r = self.share
            r.node_length = self.render.node_length
            self.gpu.sync()  # (a write does not wait for the frames other contexts still have in flight)
        lists = self.model.write(action, clears=bool(self.opt["SCAN_CLEARS_COUNTERS"]))
        if action[0] == "scan":
            compute = self.pkg.Compute(self.gpu2, r) if via_share else self.compute
            compute.update(int(self.render.node_length))
            sub, unsub = compute.read_lists()
            assert np.array_equal(np.sort(sub), lists[0]), f"the scan's subdivide list: {sub.size} entries, want {lists[0].size}"
            assert np.array_equal(np.sort(unsub), lists[1]), f"the scan's unsubdivide list: {unsub.size} entries, want {lists[1].size}"
        elif action[0] == "write":
            r.write_nodes(action[1])
        elif action[0] == "scatter":
            r.scatter_nodes(action[1], action[2])
        elif action[0] == "edit":
            r.edit_nodes(action[1], action[2], action[3])
        self.render.node_length = max(self.render.node_length, r.node_length)
        self.nodes(f"after {op!r}")

    def nodes(self, what):
        assert self.render.node_length == self.model.length, f"{what}: node_length {self.render.node_length}, want {self.model.length}"
        got, want = self.render.read_nodes(self.model.length), self.model.words()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} node words differ, first at {bad[:5].tolist()}: got {got[bad[:5]].tolist()} want {want[bad[:5]].tolist()}"
        self.tally["node buffers compared"] += 1

    # ---- frames ----

    def frame(self, F, what):
        pkg, r, kind, arg = self.pkg, self.render, F["kind"], F["arg"]
        want = None if F["refused"] else self.model.frame(F)
        n = arg[0] if kind == "rays" else F["pixels"]
        hits = self.out("hits", n)
        img = sec = None
        tile = F["rect"] if kind in ("tile", "shaded", "secondary") and F["rect"] != (0, 0) + F["size"] else None
        if kind in ("render", "tile"):
            r.render(hits=hits, tile=tile)
        elif kind == "tiles":
            r.render_tiles(*arg, hits=hits)
        elif kind == "shaded":
            img = self.out("rgba", n)
            r.render(hits=hits, tile=tile, rgba=img)
        elif kind == "secondary":
            sec = self.out("secondary", n * arg)
            r.render_secondary(arg, tile=tile, hits=hits, secondary=sec)
        else:
            rays = self.torch.from_numpy(self.P.rays(F["tree"], arg[0], arg[1])).to(self.gpu.torch_device)
            r.trace_rays(rays, hits=hits)
        self.tally["frames"] += 1
        if F["refused"]:
            with pytest.raises(pkg.SvoError, match="deeper than"):
                self.gpu.sync()
            self.tally["refused frames"] += 1
            self.nodes(f"{what}: after the refusal")
        else:
            self.gpu.sync()
            self.records(hits, want["records"], n, f"{what}: records")
            if sec is not None:
                self.records(sec, want["secondary"], n * arg, f"{what}: secondary records")
            if img is not None:
                got = img.cpu().numpy().view(np.uint8).reshape(-1, 4)
                assert (got[n:] == 0xFF).all(), f"{what}: the image's tail was written"
                diff = np.abs(got[:n].astype(np.int32) - want["image"].reshape(-1, 4))
                assert diff.max() <= 1, f"{what}: {int((diff > 1).any(axis=1).sum())} pixels of the image are off by more than 1 (most {diff.max()})"
                self.tally["images compared"] += 1
            if F["counting"]:
                self.nodes(f"{what}: counters")
        if F["launches"]:
            self.traced = True
        for L in F["launches"]:
            self.schedule(F, L, want, what)
        if self.traced:
            self.deal(F, what)

    def records(self, buf, want, n, what):
        got = self.pkg.render.hits_to_numpy(buf)
        assert (got[n:].view(np.uint32) == 0xFFFFFFFF).all(), f"{what}: the buffer's tail was written"
        want = np.ascontiguousarray(want).reshape(-1)
        if not np.array_equal(got[:n].view(np.uint32), want.view(np.uint32)):
            left = np.flatnonzero(got[:n]["info"] == 0xFFFFFFFF)
            assert left.size == 0, f"{what}: {left.size} records were never written, first {left[:4].tolist()}"
            assert_hits_equal(got[:n], want, what)  # (says where; NaN payloads may differ)
        self.tally["records compared"] += n
        self.tally["records that hit"] += int(((want["info"] >> 16) & 1).sum())

    def schedule(self, F, L, want, what):
        slot = L["slot"]
        what = f"{what}, slot {slot}"
        if not L["has_buffers"]:
            return
        st = self.gpu.schedule_status(slot)
        got = {f: int(st[f]) for f in S.STATE_FIELDS}
        assert got == L["want_state"], f"{what}: the slot holds {got}, the policy's row gives {L['want_state']} (row {L['row']})"
        self.tally[f"slot {slot} states compared"] += 1
        if not L["sched"]:
            return
        row = L["row"]
        if row["measure"] or row["reuse_costs"] or L["filt"]:
            assert st["n_strips"] == L["n_strips"], f"{what}: {st['n_strips']} strips, want {L['n_strips']}"
        if L["filt"]:
            now = st["classes_now"]
            R.check_lists(dict(st, balance=EQUAL), now, what)
            out = np.flatnonzero(now == R.OUT)
            self.tally["filtered lists checked"] += 1
            self.tally["strips left out"] += out.size
            if want is None:
                return
            if slot == 0:
                for s in out:
                    assert S.all_zero(S.block_records(want["records"], L["work"], int(s))), f"{what}: strip {s} is in no list, but a ray of it enters the cube"
            else:  # a skip mask: exactly the strips none of whose pixels hit anything
                miss = ((want["records"].reshape(-1)["info"] >> 16) & 1) == 0
                skip = np.tile(miss, L["work"]["n_items"] // miss.size).astype(np.uint8)
                empty = R.skip_classes(skip, L["work"]["n_items"]) == R.OUT
                assert np.array_equal(now == R.OUT, empty), f"{what}: the strips left out are not the ones without a ray"
                rec = want.get("secondary")
                if rec is not None:
                    flat = np.ascontiguousarray(rec).reshape(-1)[-L["work"]["n_items"]:]
                    for s in out:
                        assert S.all_zero(flat[64 * s:64 * s + 64]), f"{what}: strip {s} is in no list, but holds a record"
        elif row["build_lists"]:
            R.check_stored_lists(st, what, motion=L["motion"])
            self.tally["stored lists checked"] += 1

    def deal(self, F, what):
        d = self.gpu.deal_status()
        L = next((L for L in F["launches"] if L["slot"] == 0), None)
        if L is not None and L["deal_grow"]:
            self.replayed = 0  # (the slot started over with new buffers)
        step, allowed = d["replayed"] - self.replayed, (L["replay"] if L is not None else 0)
        self.replayed = d["replayed"]
        self.tally["frames replayed"] += step
        self.tally["frames that had to be replayed"] += allowed == 1
        if allowed is None:
            assert step in (0, 1), f"{what}: replayed advanced by {step}"
        else:
            why = "its facts forbid a replay" if allowed == 0 else f"frame {L['deal_run']} of an accepted rest is replayed"
            assert step == allowed, f"{what}: replayed advanced by {step}; {why}"
        if L is not None and d["seeded"] and d["rows"]:
            check_table(self.gpu.deal_status(table=True), L["n_strips"])
            self.tally["deal tables checked"] += 1


@pytest.mark.parametrize("name", list(S.sessions()))
def test_session(pkg, O, pools, driver, contexts, name):
    Session(pkg, O, pools, driver, name, S.sessions()[name], contexts).run()
