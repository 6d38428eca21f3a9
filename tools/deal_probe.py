"""Developer probe of the static deal (SVO_OPT_STATIC_DEAL) on the benchmark frame: for every learning frame the
distribution of the waves' end times (5th / 50th / 95th percentile and the last wave, us after the frame's start), the strips per
wave and the strips moved by the step; then the resting frame's kernel time with the option off and on, alternating in one process.
usage: python tools/deal_probe.py [--lod 1500] [--w 1920 --h 1080] [--reps 100] [--rounds 3] [--scene-file words.npy]
SVO_DEAL_PAIRS_DIV=n in the environment sweeps the pairs a step moves (a list's waves / n)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lod", type=float, default=1500.0)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-words", type=int, default=125_000_000)
    ap.add_argument("--scene-file", default=None, help="the scene's words as .npy: loaded when there, else written after the build")
    a = ap.parse_args()
    pkg = entry.load_package()
    t0 = time.time()
    cam, look = pkg.scenes.terrain_camera(0, 16)
    if a.scene_file and os.path.exists(a.scene_file):
        words = np.load(a.scene_file)
    else:
        words = pkg.scenes.terrain(seed=0, max_depth=16, cam=cam, lod_c=a.lod, max_words=a.max_words)
        if a.scene_file:
            np.save(a.scene_file, words)
    print(f"scene: {words.size} words in {time.time() - t0:.1f}s", flush=True)
    gpu = pkg.Gpu(0)
    render = pkg.Render(gpu, (a.w, a.h), words, capacity=words.size)
    render.set_flags(pause_adaptive=True, shadows=False)
    render.update(pkg.Settings(), pkg.Character(cam, look))
    hits = render.alloc_hits(a.w * a.h)

    def frames(n):
        gpu.set_option(pkg.gpu.OPT_TIMING, n)
        for _ in range(n):
            render.render(hits=hits)
        gpu.sync()
        return gpu.timing_collect()

    frames(40)  # clocks settle; the lists are built and their shares learnt
    ref = hits.cpu().numpy().copy()
    st = gpu.deal_status()
    print("before:", json.dumps({k: st[k] for k in ("replayed", "seeds", "step", "verdict", "rows", "row_cap")}))
    # the option off and on again: the view's deal is seeded on the next frame and learnt over the frames that follow
    gpu.set_option(pkg.gpu.OPT_STATIC_DEAL, 0)
    frames(2)
    gpu.set_option(pkg.gpu.OPT_STATIC_DEAL, 1)
    for k in range(18):
        ms = frames(1)[0]
        st = gpu.deal_status(table=True, stamps=True)
        if not st["rows"]:
            print(f"frame {k}: not replayed ({ms * 1e3:.1f} us)")
            continue
        end = st["stamps"][:, 1].astype(np.int64)
        rel = (end - end.max()) * 0.01 + st["last_ticks"] * 0.01  # us after the start stamp (while a step follows every frame)
        p5, p50, p95 = np.percentile(rel, [5, 50, 95])
        lens = (st["table"] != 0xFFFFFFFF).cumprod(axis=1).sum(axis=1)
        print(f"frame {k}: kernel {ms * 1e3:6.1f} us | wave ends p5 {p5:6.1f} p50 {p50:6.1f} p95 {p95:6.1f} last {rel.max():6.1f} (p95-p5 {p95 - p5:5.1f}) | "
              f"strips/wave min {lens.min()} mean {lens.mean():.2f} max {lens.max()} | step {st['step']} moved {st['last_moves']} "
              f"best {st['best_ticks'] * 0.01:.1f} verdict {st['verdict']}", flush=True)
    st = gpu.deal_status()
    print("learnt:", json.dumps({k: v for k, v in st.items()}))
    assert np.array_equal(hits.cpu().numpy(), ref), "records changed"
    # the resting frame, option off / on alternating
    res = {0: [], 1: []}
    for r in range(a.rounds):
        for on in (0, 1):
            gpu.set_option(pkg.gpu.OPT_STATIC_DEAL, on)
            frames(20 if on else 3)  # (on: the table is seeded and learnt again -- the verdict included)
            ms = frames(a.reps)
            res[on].append(float(np.median(ms)))
            print(f"round {r} option {on}: kernel median {np.median(ms) * 1e3:.1f} us, mean {np.mean(ms) * 1e3:.1f} us, replayed {gpu.deal_status()['replayed']}", flush=True)
    off, on = np.median(res[0]), np.median(res[1])
    print(json.dumps({"off_ms": round(off, 5), "on_ms": round(on, 5), "on_vs_off_pct": round((on / off - 1) * 100, 2),
                      "off_spread_pct": round((max(res[0]) - min(res[0])) / off * 100, 2), "pairs_div": os.environ.get("SVO_DEAL_PAIRS_DIV", "16")}))
    assert np.array_equal(hits.cpu().numpy(), ref), "records changed"


if __name__ == "__main__":
    main()
