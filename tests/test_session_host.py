"""What makes the session tests (tests/test_session_gpu.py) worth running, held on the host: the committed seeds and
worst_transitions() together use every call and every option value, contain the interleavings the trace path's state can get wrong,
drive the schedule's policy (svo_sched.h, through tests/schedule_plan_driver.cpp, unchanged) into every corner it has per slot,
rest long enough for the static deal, and look at the trees from poses that hit them.  Without these conditions the GPU test could
pass while checking nothing.  The tallies are printed (-s shows them)."""
import collections

import numpy as np
import pytest

import session_ops as S


@pytest.fixture(scope="module")
def pools(pkg, O):
    return S.Pools(pkg, O)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return S.build_driver(tmp_path_factory.mktemp("session_plan"))


@pytest.fixture(scope="module")
def plans(pools, driver):
    """name -> the frames of the session, every launch with the policy's row"""
    return {name: S.Tracker(pools).plan(ops, driver) for name, ops in S.sessions().items()}


def test_generator_is_deterministic():
    for seed in S.SEEDS:
        a, b = S.make_session(seed), S.make_session(seed)
        assert a == b and len(a) >= 150
        assert all("\n" not in repr(op) and len(repr(op)) < 100 for op in a)
        frames = sum(op.args[2] for op in a if op.kind == "frame")
        assert frames <= 460, f"seed {seed}: {frames} frames"
        assert sum(op == S.Op("size", *S.BIG) for op in a) <= 2
    assert len(S.SEEDS) == 8 and len(set(S.SEEDS)) == 8


def test_every_op_kind_and_option_value_occurs():
    kinds, values = collections.Counter(), collections.Counter()
    for ops in S.sessions().values():
        for op in ops:
            kinds[op.kind] += 1
            if op.kind == "frame":
                kinds["frame:" + op.args[0]] += 1
                kinds[f"repeat:{op.args[2]}"] += 1
            elif op.kind == "write":
                kinds["write:" + op.args[0]] += 1
                kinds["write via the sharing context"] += op.args[1]
                if op.args[0] == "tree":
                    kinds["tree:" + op.args[2]] += 1
            elif op.kind == "option":
                values[op.args] += 1
            elif op.kind == "camera":
                kinds["pose:" + op.args[0]] += 1
            elif op.kind == "size":
                kinds[f"size:{op.args}"] += 1
            elif op.kind == "flags":
                kinds["flags:" + "".join("PSM"[k] if v else "-" for k, v in enumerate(op.args))] += 1
    print("op kinds:", dict(sorted(kinds.items())))
    print("option values:", {f"{n}={v}": c for (n, v), c in sorted(values.items())})
    want = ["camera", "size", "flags", "option", "frame", "write", "write via the sharing context"]
    want += ["frame:" + k for k in S.FRAME_KINDS] + ["write:" + k for k in S.WRITE_KINDS] + [f"repeat:{r}" for r in S.REPEATS]
    want += ["tree:" + t for t in S.TREES] + [f"size:{s}" for s in S.SIZES]
    want += ["pose:" + p for p in sorted({p for ps in S.POSES.values() for p in ps})]
    for k in want:
        assert kinds[k] >= 3, f"{k} occurs {kinds[k]} times"
    for k in ("flags:P--", "flags:---"):  # at rest and counting
        assert sum(c for f, c in kinds.items() if f.startswith("flags:") and (f[6] == "P") == (k[6] == "P")) >= 3
    for name, vs in S.OPTION_VALUES.items():
        for v in vs:
            assert values[(name, v)] >= 3, f"option {name} = {v} occurs {values[(name, v)]} times"


def eligible(F):
    return any(L["slot"] == 0 and L.get("replay") != 0 for L in F["launches"])


def slot0(F):
    return next((L for L in F["launches"] if L["slot"] == 0), None)


def transitions(frames):
    """the critical transitions a session's frames contain"""
    found = collections.Counter()
    items = lambda F: F["size"][0] * F["size"][1]
    same_view = lambda A, B: bytes(A["u"]) == bytes(B["u"]) and A["tree"] == B["tree"]
    for k in range(1, len(frames)):
        A, B = frames[k - 1], frames[k]
        C = frames[k + 1] if k + 1 < len(frames) else None
        a0, b0 = slot0(A), slot0(B)
        writes = [op for op in B["since"] if op.kind == "write" and op.args[0] != "scan"]
        if C and eligible(A) and B["counting"] and B["stack"] and not C["counting"] and same_view(A, C):
            found["a counting frame between two frames of a replayed rest"] += 1
        if C and A["kind"] != "rays" and B["kind"] == "rays" and C["kind"] != "rays" and B["stack"] and C["stack"]:
            found["explicit rays on slot 0 between pixel frames"] += 1
        if a0 and b0 and a0["filt"] and not b0["filt"] and b0["work"]["mode"] != 2 and A["size"] != B["size"]:
            found["a culled frame, then an unculled frame of another size"] += 1
        if B["two_pass"] and len(B["launches"]) == 2 and B["kind"] == "shaded" and (any(L["defer_regrow"] for L in A["launches"] + B["launches"])):
            found["a shaded two-pass frame after a resize that regrew the deferred buffer"] += 1
        if eligible(A) and same_view(A, B) and any(op.args[1] for op in writes):
            found["a write through the sharing context while the owner rests"] += 1
        if A["stack"] and B["stack"] and A["opt"]["TREE_DEPTH"] != B["opt"]["TREE_DEPTH"]:
            found["a tree-depth option change between two frames"] += 1
        if a0 and b0 and a0["filt"] and a0["work"]["mode"] != 2 and not b0["filt"] and B["pose"] not in S.IS_OUTSIDE:
            found["culled, then inside"] += 1
        if len(A["launches"]) == 2 and B["kind"] == "render" and len(B["launches"]) == 1 and not B["counting"]:
            found["a slot-1 frame, then a slot-0 rest"] += 1
        if same_view(A, B) and B["since"] and all(op.kind == "option" for op in B["since"]) and A["stack"] and B["stack"]:
            found["an option change during a rest"] += 1
        if eligible(A) and same_view(A, B) and writes:
            found["a write during a replay-eligible rest"] += 1
        if A["refused"] and not B["refused"]:
            found["a refused frame, then one that is not"] += 1
        if not A["stack"] and B["stack"] or A["stack"] and not B["stack"]:
            found["RESTART and STACK frames side by side"] += 1
    sizes = [items(F) for k, F in enumerate(frames) if k == 0 or F["size"] != frames[k - 1]["size"]]
    found["resize down, then up"] = sum(a > b < c for a, b, c in zip(sizes, sizes[1:], sizes[2:]))
    return found


CRITICAL = [
    "a counting frame between two frames of a replayed rest",
    "explicit rays on slot 0 between pixel frames",
    "a culled frame, then an unculled frame of another size",
    "a shaded two-pass frame after a resize that regrew the deferred buffer",
    "a write through the sharing context while the owner rests",
    "a tree-depth option change between two frames",
    "resize down, then up",
    "culled, then inside",
    "a slot-1 frame, then a slot-0 rest",
    "an option change during a rest",
    "a write during a replay-eligible rest",
    "a refused frame, then one that is not",
    "RESTART and STACK frames side by side",
]


def test_critical_transitions_occur(plans):
    total = collections.Counter()
    for name, frames in plans.items():
        found = transitions(frames)
        total.update(found)
        print(f"{name}: {dict(found)}")
    print("transitions:", dict(total))
    for t in CRITICAL:
        assert total[t] >= 1, f"no session holds: {t}"
    assert all(transitions(plans["worst_transitions"])[t] >= 1 for t in CRITICAL), "the hand-written session is meant to hold them all"


def reached(rows):
    """which corners of the policy a slot's rows reach"""
    out = collections.Counter()
    before = None
    for r in rows:
        out["lists " + r["lists"]] += 1
        out["reset_shares"] += r["reset_shares"]
        out["prior_costs"] += r["prior_costs"]
        out["measure"] += r["measure"]
        out["reuse_costs"] += r["reuse_costs"]
        out["floored build"] += bool(r["build_lists"] and r["floor"])
        out["balance_update 16"] += r["balance_update"] == S.LIST_LEARN
        out["complete rebuild after a filtered frame"] += bool(before and before["order_filtered"] and r["build_lists"])
        out["age at the backstop"] += bool(before and before["age"] >= S.MAX_AGE and r["age"] == 0)
        before = r
    return out


def test_plan_rows_reach_every_corner_per_slot(plans):
    got = [collections.Counter(), collections.Counter()]
    for frames in plans.values():
        for slot in (0, 1):
            got[slot].update(reached([L["row"] for F in frames for L in F["launches"] if L["slot"] == slot]))
    print("plan rows, slot 0:", dict(got[0]))
    print("plan rows, slot 1:", dict(got[1]))
    for corner in ("lists L", "lists F", "lists -", "reset_shares", "prior_costs", "measure", "reuse_costs", "floored build", "balance_update 16",
                   "complete rebuild after a filtered frame", "age at the backstop"):
        assert got[0][corner] >= 1, f"slot 0 never reaches: {corner}"
    # Slot 1 is traced by trace_common and trace_secondary only, always with a skip mask: every scheduled frame of it is filtered,
    # so it stores no lists, builds none in its post pass and feeds nothing back.  What the glue can reach there is asked for, and
    # the rest is asserted absent -- a change of the glue that opens it shows here.
    for corner in ("lists F", "lists -", "reset_shares", "prior_costs", "measure"):
        assert got[1][corner] >= 1, f"slot 1 never reaches: {corner}"
    for corner in ("lists L", "reuse_costs", "floored build", "balance_update 16", "complete rebuild after a filtered frame"):
        assert got[1][corner] == 0, f"slot 1 reached {corner}: the model of the glue is out of date"


def test_sessions_rest_long_enough_for_the_deal(plans):
    rests = {}
    for name, frames in plans.items():
        runs = [L["deal_run"] for F in frames for L in F["launches"] if L["slot"] == 0]
        rests[name] = max(runs, default=0)
    print("longest accepted static rest past its list learning, per session:", rests)
    # 1 frame builds the lists and 16 learn their shares before the deal's run starts: a run of 16 + 3 is a rest of 1 + 16 + 16 + 3
    assert sum(r >= S.DEAL_LEARN + 3 for r in rests.values()) >= 3
    assert rests["worst_transitions"] >= S.MAX_AGE, "one session rests past the schedule's backstop with the deal in place"


def test_tree_depths(pkg, pools):
    for name, words in pools.words.items():
        assert pkg.scenes.max_depth(words) == S.TREE_DEPTH[name], name
        assert words.size % 8 == 0


def test_pools_hit_their_trees(pools, O):
    shares, misses = {}, {}
    for tree, poses in S.POSES.items():
        words = pools.words[tree]
        for pose in poses:
            for size in S.SIZES:
                if not S.pose_ok(pose, size):
                    continue
                u = pools.uniforms(pose, size, S.F_PAUSE)
                rec = O.trace_frame(words, u, threads=8)
                share = float(((rec["info"] >> 16) & 1).mean())
                shares[(tree, pose, size)] = share
                if pose in S.SKY_ONLY:
                    assert share == 0.0
                elif pose in S.SKY_MOSTLY:
                    assert 0.0 < share < 0.95, (tree, pose, size, share)
                elif pose not in S.DEFERRED:
                    assert 0.05 <= share <= 0.95, (tree, pose, size, share)
                else:
                    assert share > 0.05, (tree, pose, size, share)
                if pose in S.FORCED_CULL and size == (256, 128):
                    never = np.array([[S.all_zero(rec[y:y + 8, x:x + 8]) for x in range(0, 256, 8)] for y in range(0, 128, 8)])
                    misses[(tree, pose)] = int(never.sum())
                    assert never.sum() >= 20, (tree, pose, int(never.sum()))
    print("hit shares (min .. max over the sizes):",
          {f"{t}/{p}": (round(min(v for k, v in shares.items() if k[:2] == (t, p)), 3), round(max(v for k, v in shares.items() if k[:2] == (t, p)), 3))
           for t, ps in S.POSES.items() for p in ps})
    print("never-entered 8x8 blocks at 256x128:", {f"{t}/{p}": n for (t, p), n in misses.items()})


def test_automatic_culling_is_never_a_close_call(pools):
    """OPT_CULL = 2 asks for 40 % of a 12 x 8 grid of rays to look past the cube: every pose is far from that, so the model's
    restatement and the glue cannot disagree by a rounding"""
    seen = {}
    for pose in sorted({p for ps in S.POSES.values() for p in ps}):
        for size in S.SIZES:
            if not S.pose_ok(pose, size):
                continue
            outside, miss = S.cull_facts(pools.uniforms(pose, size, S.F_PAUSE))
            assert outside == (pose in S.IS_OUTSIDE), pose
            if outside:
                assert miss is not None and (miss <= 0.2 or miss >= 0.6), (pose, size, miss)
                seen.setdefault(pose, []).append(round(miss, 3))
    print("miss shares of the outside poses:", seen)


def test_model_on_the_oracle_alone(pools, O, plans):
    """every session through the model, no GPU: the counting stretches saturate a counter and fill both scan lists, and a frame's
    records do not depend on the counters (the model keeps them by tree, not by counter state)"""
    saturated, scans, checked = 0, [], 0
    for name, ops in S.sessions().items():
        model, frames, k = S.Model(pools, O), plans[name], 0
        pose, clears = "in_a", False
        for i, op in enumerate(ops):
            if op.kind == "frame":
                for rep in range(op.args[2]):
                    F = frames[k]
                    k += 1
                    assert (F["index"], F["rep"]) == (i, rep)
                    assert F["pose"] in S.POSES[F["tree"]] and S.pose_ok(F["pose"], F["size"]), (name, i, op)
                    if F["refused"]:
                        continue
                    want = model.frame(F)
                    if F["counting"] and rep == op.args[2] - 1 and F["kind"] == "render" and checked < 6:
                        again = O.trace_frame(model.words(), F["u"], threads=8)
                        assert np.array_equal(again.view(np.uint32), want["records"].view(np.uint32)), "records depend on the counters"
                        checked += 1
            elif op.kind == "write":
                model.write(model.resolve(op, pose), clears=clears)
            elif op.kind == "camera":
                pose = op.args[0]
            elif op.args[:1] == ("SCAN_CLEARS_COUNTERS",):
                clears = bool(op.args[1])
        saturated += model.saturated
        scans += model.scans
        print(f"{name}: counter saturated {model.saturated}, scan lists {model.scans}, {len(model.cache)} oracle answers")
    assert saturated >= 3 and checked >= 3
    assert any(s > 0 and u > 0 for s, u in scans), "no scan found both lists non-empty"
