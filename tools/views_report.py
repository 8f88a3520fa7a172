#!/usr/bin/env python3
"""The views report (needs a GPU; there is no fallback). Writes profiles/views_report.json (or --out).

camera_change   on the headline scene (cornell_direct_1920x1080_8x8), per repetition and as median / min / max, in ms
                of host wall time around calls that end in a device synchronise (the frame's copy to the host):
                a frame on a resident handle; set_camera to another view plus that frame; release plus a fresh
                GpuRenderer (flatten, upload) plus that frame. All at the engine's default batch (2^23 samples), so a
                fresh handle's first frame allocates the same level state in every variant.
render_multi    a process that calls render_multi on cornell_direct_800_4x4 and then on the headline scene (the same
                world under another camera): the second call's wall time and phases. With --parent-root also in the
                parent commit's tree, where that second call releases and uploads.
strip           64 views of the cornell world at 240 x 135, at 4 x 4 and at 8 x 8 steps, on one handle: the strip
                (render_views) against 64 x (set_camera + render), alternating, --reps repetitions each, batches of
                2^27 samples for both (the strip is one batch); medians, spreads (max - min), whether the two are
                bit-identical, and the project's gain rule: the strip stays only if the sequence's median exceeds its
                median by more than three times the larger spread.
no_regression   with --parent-root: bench.py --gpus 1 in the parent's tree and in this one, alternating, --bench-runs
                runs each: the headline ms_per_step of every run, medians and spreads; passes when this tree's median
                does not exceed the parent's by more than the larger spread.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_ray_tracer_amd import build  # noqa: E402
from fast_ray_tracer_amd import runtime  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADLINE = "cornell_direct_1920x1080_8x8"


def scene_of(name):
    return runtime.Scene(build.build_scene(os.path.join(GOLDEN, "scenes", name + ".c")),
                         asset_root=os.path.join(GOLDEN, "assets"))


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3),
            "max": round(max(values), 3), "spread": round(max(values) - min(values), 3),
            "runs": [round(v, 3) for v in values]}


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def turntable(scene, k, n, **args):
    """View k of n on an arc in front of the cornell room's opening, looking at its centre."""
    a = (k / max(1, n - 1) - 0.5) * 0.5
    return scene.view((1.2 * math.sin(a), 0.15 * math.cos(3 * a), -2.0 - 0.6 * math.cos(a)), (0.0, 0.0, 0.0), **args)


def camera_change(reps):
    scene = scene_of(HEADLINE)
    views = [turntable(scene, k, 4) for k in (1, 2)]
    r = runtime.GpuRenderer(scene)
    r.render()
    r.render()
    frame, moved, fresh = [], [], []
    for i in range(reps):
        frame.append(ms(r.render)[0])
        v = views[i % 2]
        moved.append(ms(lambda: (r.set_camera(v), r.render()))[0])

        def reupload():
            nonlocal r
            r.close()
            r = runtime.GpuRenderer(scene)
            r.set_camera(v)
            return r.render()
        fresh.append(ms(reupload)[0])
        r.render()  # (the next repetition's resident frame is a warm one again)
    r.close()
    return {"scene": HEADLINE, "batch_samples": 1 << 23, "frame_ms": spread(frame),
            "set_camera_plus_frame_ms": spread(moved), "release_prepare_frame_ms": spread(fresh)}


RM_PROBE = """
import json, os, sys, time
sys.path.insert(0, os.getcwd())
from fast_ray_tracer_amd import build
from fast_ray_tracer_amd.runtime import Scene, render_multi, render_multi_phases
g = os.path.join(os.getcwd(), "tests", "golden")
sc = [Scene(build.build_scene(os.path.join(g, "scenes", n + ".c")), asset_root=os.path.join(g, "assets"))
      for n in ("cornell_direct_800_4x4", "cornell_direct_1920x1080_8x8")]
render_multi(sc[0], devices="0")
t0 = time.perf_counter()
c = render_multi(sc[1], devices="0")
dt = 1e3 * (time.perf_counter() - t0)
ph = render_multi_phases()
print("RM", json.dumps({"second_call_ms": round(dt, 2), "upload_ms": ph["upload"], "flatten_ms": ph["flatten"],
                        "render_rows_and_copy_ms": ph["render_rows_and_copy"], "release_ms": ph["release"],
                        "canvas_sum": float(c[:, :, :3].sum())}))
"""


def render_multi_change(root, runs):
    out = []
    for _ in range(runs):
        p = subprocess.run([sys.executable, "-c", RM_PROBE], cwd=root, capture_output=True, text=True, timeout=600)
        lines = [ln[3:] for ln in p.stdout.splitlines() if ln.startswith("RM ")]
        if p.returncode != 0 or not lines:
            raise RuntimeError("render_multi probe failed in %s: %s" % (root, p.stderr[-2000:]))
        out.append(json.loads(lines[-1]))
    return {"second_call_ms": spread([o["second_call_ms"] for o in out]), "runs": out}


def strip_against_sequence(steps, nviews, reps):
    base = scene_of("cornell_direct_240x135_8x8")
    views = [turntable(base, k, nviews, usteps=steps, vsteps=steps) for k in range(nviews)]
    batch = 1 << 27
    r = runtime.GpuRenderer(base)

    def sequence():
        frames = []
        for v in views:
            r.set_camera(v)
            frames.append(r.render(batch_samples=batch))
        return np.stack(frames)

    def strip():
        return r.render_views(views, batch_samples=batch)

    r.set_camera(views[0])
    a, b = sequence(), strip()  # (warm-up of both: level state, code objects; and the comparison)
    identical = bool(np.array_equal(a, b))
    t_seq, t_strip = [], []
    for _ in range(reps):
        t_strip.append(ms(strip)[0])
        t_seq.append(ms(sequence)[0])
    _, st = r.render_views(views, batch_samples=batch, stats=True)
    r.close()
    s, q = spread(t_strip), spread(t_seq)
    gain = q["median"] - s["median"]
    bar = 3.0 * max(s["spread"], q["spread"])
    return {"views": nviews, "width": views[0].width, "height": views[0].height, "steps": steps,
            "samples": nviews * views[0].width * views[0].height * steps * steps, "batch_samples": batch,
            "bit_identical": identical, "strip_ms": s, "sequence_ms": q, "gain_ms": round(gain, 3),
            "three_spreads_ms": round(bar, 3), "strip_stays": bool(identical and gain > bar),
            "speedup": round(q["median"] / s["median"], 2),
            "strip_stats_frame": {"render_ms": round(st.render_ms, 3),
                                  "kernel_ms": st.as_dict()["kernel_ms"], "launches": st.as_dict()["kernel_launches"]}}


def bench_once(root, steps, warmup):
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], cwd=root, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise RuntimeError("bench.py failed in %s: %s" % (root, p.stderr[-2000:]))
    return float(json.loads(lines[-1])["ms_per_step"])


def no_regression(parent, runs, steps, warmup):
    mine, theirs = [], []
    for _ in range(runs):
        theirs.append(bench_once(parent, steps, warmup))
        mine.append(bench_once(ROOT, steps, warmup))
    a, b = spread(theirs), spread(mine)
    return {"bench": "bench.py --gpus 1 --steps %d --warmup %d" % (steps, warmup), "parent_ms_per_step": a,
            "this_ms_per_step": b, "allowed_ms": max(a["spread"], b["spread"]),
            "passes": bool(b["median"] <= a["median"] + max(a["spread"], b["spread"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_report.json"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (A/B parts)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--only", default="strip,camera_change,render_multi,no_regression")
    args = ap.parse_args()
    if runtime.host_lib().frt_device_count() <= 0:
        raise SystemExit("views_report: no HIP device visible (the report is measured on the GPU)")
    if args.parent_root:
        args.parent_root = os.path.abspath(args.parent_root)
    parts = args.only.split(",")
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")

    if "strip" in parts:
        out["strip"] = {}
        for steps in (4, 8):
            out["strip"]["%dx%d" % (steps, steps)] = strip_against_sequence(steps, args.views, args.reps)
            print("strip", steps, json.dumps(out["strip"]["%dx%d" % (steps, steps)]), flush=True)
            save()
    if "camera_change" in parts:
        out["camera_change"] = camera_change(3)
        print("camera_change", json.dumps(out["camera_change"]), flush=True)
        save()
    if "render_multi" in parts:
        out["render_multi_camera_change"] = {"this": render_multi_change(ROOT, 3)}
        if args.parent_root:
            out["render_multi_camera_change"]["parent"] = render_multi_change(args.parent_root, 3)
        print("render_multi", json.dumps(out["render_multi_camera_change"]), flush=True)
        save()
    if "no_regression" in parts and args.parent_root:
        out["no_regression"] = no_regression(args.parent_root, args.bench_runs, args.bench_steps, args.bench_warmup)
        print("no_regression", json.dumps(out["no_regression"]), flush=True)
        save()


if __name__ == "__main__":
    main()
