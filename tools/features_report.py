#!/usr/bin/env python3
"""The feature-buffers report (needs a GPU; there is no fallback). Writes profiles/features_report.json (or --out).

headline        cornell_direct_1920x1080_8x8 on one resident handle, whole-frame batches (2^27 samples), --reps
                repetitions alternating a statistics features pass and a statistics colour frame in one process:
                the pass's render_ms and its three kernel times (trace kernel_ms[5], prepare kernel_ms[6],
                k_feature_resolve sub_ms[10]) beside the colour frame's kernel_ms[5], [6] and render_ms; medians and
                spreads (max - min), as tools/views_report.py reports them. Host wall time around the two calls
                without statistics as well (each ends in the copy of its buffers to the host).
strip           64 views of the cornell world at 240 x 135, 8 x 8 steps, on one handle: render_feature_views against
                64 x (set_camera + render_features), alternating, wall time; whether the two are bit-identical.
no_regression   with --parent-root (a built checkout of the parent commit): bench.py --gpus 1 in the parent's tree and
                in this one, alternating, --bench-runs runs each; the rule of profiles/r09_ab_refactor.txt: the
                medians differ by no more than the larger run-to-run spread. --ab-text writes the runs as text.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fast_ray_tracer_amd import runtime  # noqa: E402
from views_report import HEADLINE, ms, scene_of, spread, turntable  # noqa: E402

BATCH = 1 << 27


def headline(reps):
    r = runtime.GpuRenderer(scene_of(HEADLINE))
    for _ in range(2):  # (warm-up of both: level state, code objects)
        r.render(batch_samples=BATCH)
        r.render_features(batch_samples=BATCH)
    feat = {k: [] for k in ("render_ms", "trace_ms", "prepare_ms", "resolve_ms", "wall_ms")}
    col = {k: [] for k in ("render_ms", "trace_primary_ms", "prepare_ms", "wall_ms")}
    launches = None
    for _ in range(reps):
        _, st = r.render_features(batch_samples=BATCH, stats=True)
        feat["render_ms"].append(st.render_ms)
        feat["trace_ms"].append(st.kernel_ms[5])
        feat["prepare_ms"].append(st.kernel_ms[6])
        feat["resolve_ms"].append(st.sub_ms[10])
        launches = {"trace": int(st.kernel_launches[5]), "prepare": int(st.kernel_launches[6]),
                    "k_feature_resolve": int(st.sub_launches[10])}
        _, st = r.render(batch_samples=BATCH, stats=True)
        col["render_ms"].append(st.render_ms)
        col["trace_primary_ms"].append(st.kernel_ms[5])
        col["prepare_ms"].append(st.kernel_ms[6])
        feat["wall_ms"].append(ms(lambda: r.render_features(batch_samples=BATCH))[0])
        col["wall_ms"].append(ms(lambda: r.render(batch_samples=BATCH))[0])
    f = r.render_features(batch_samples=BATCH)
    r.close()
    return {"scene": HEADLINE, "batch_samples": BATCH, "reps": reps,
            "features": {k: spread(v) for k, v in feat.items()}, "features_launches": launches,
            "colour_frame": {k: spread(v) for k, v in col.items()},
            "coverage_mean": float(f["coverage"].mean()), "depth_max": float(f["depth"].max())}


def strip_against_sequence(nviews, reps, steps=8):
    base = scene_of("cornell_direct_240x135_8x8")
    views = [turntable(base, k, nviews, usteps=steps, vsteps=steps) for k in range(nviews)]
    r = runtime.GpuRenderer(base)

    def sequence():
        out = []
        for v in views:
            r.set_camera(v)
            f = r.render_features(batch_samples=BATCH)
            out.append((f["depth"].base, f["node"].base))
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def strip():
        f = r.render_feature_views(views, batch_samples=BATCH)
        return f["depth"].base, f["node"].base

    r.set_camera(views[0])
    a, b = sequence(), strip()
    identical = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    t_seq, t_strip = [], []
    for _ in range(reps):
        t_strip.append(ms(strip)[0])
        t_seq.append(ms(sequence)[0])
    _, st = r.render_feature_views(views, batch_samples=BATCH, stats=True)
    r.close()
    s, q = spread(t_strip), spread(t_seq)
    return {"views": nviews, "width": views[0].width, "height": views[0].height, "steps": steps,
            "samples": nviews * views[0].width * views[0].height * steps * steps, "batch_samples": BATCH,
            "bit_identical": identical, "strip_ms": s, "sequence_ms": q,
            "speedup": round(q["median"] / s["median"], 2),
            "strip_stats_frame": {"render_ms": round(st.render_ms, 3), "trace_ms": round(st.kernel_ms[5], 3),
                                  "prepare_ms": round(st.kernel_ms[6], 3), "resolve_ms": round(st.sub_ms[10], 3)}}


def bench_once(root, steps, warmup):
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], cwd=root, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise RuntimeError("bench.py failed in %s: %s" % (root, p.stderr[-2000:]))
    return json.loads(lines[-1])


def no_regression(parent, runs, steps, warmup, text):
    mine, theirs, lines = [], [], []
    for i in range(runs):
        for who, root, into in (("parent", parent, theirs), ("result", ROOT, mine)):
            res = bench_once(root, steps, warmup)
            into.append(float(res["ms_per_step"]))
            lines.append("%s %d ms_per_step %7.3f value %.3f" % (who, i + 1, res["ms_per_step"], res.get("value", 0.0)))
            print(lines[-1], flush=True)
    a, b = spread(theirs), spread(mine)
    allowed = max(a["spread"], b["spread"])
    diff = abs(b["median"] - a["median"])
    within = bool(diff <= allowed)
    lines.append("ms_per_step: parent median %.3f max-min %.3f | result median %.3f max-min %.3f | difference %.3f "
                 "(result %s) against the larger spread %.3f: %s"
                 % (a["median"], a["spread"], b["median"], b["spread"], diff, "+" if b["median"] > a["median"] else "-",
                    allowed, "within" if within else "NOT within"))
    if text:
        with open(text, "w") as f:
            f.write("# feature buffers: the parent commit, built from a checkout of its own, against the result;\n"
                    "# python bench.py --gpus 1 --steps %d --warmup %d, %d runs per build, alternating (parent first in\n"
                    "# each pair), one session. The device code of render_frame's kernels is the same in both builds.\n"
                    "# Rule: the medians differ by no more than the larger of the two run-to-run spreads (max-min).\n"
                    % (steps, warmup, runs))
            f.write("\n".join(lines) + "\n")
    return {"bench": "bench.py --gpus 1 --steps %d --warmup %d" % (steps, warmup), "parent_ms_per_step": a,
            "this_ms_per_step": b, "allowed_ms": allowed, "difference_ms": round(diff, 3), "passes": within}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_report.json"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (the A/B part)")
    ap.add_argument("--ab-text", default=None, help="also write the A/B runs as text (profiles/features_ab_bench.txt)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--only", default="headline,strip,no_regression")
    args = ap.parse_args()
    if runtime.host_lib().frt_device_count() <= 0:
        raise SystemExit("features_report: no HIP device visible (the report is measured on the GPU)")
    parts = args.only.split(",")
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")

    if "headline" in parts:
        out["headline"] = headline(args.reps)
        print("headline", json.dumps(out["headline"]), flush=True)
        save()
    if "strip" in parts:
        out["strip"] = strip_against_sequence(args.views, args.reps)
        print("strip", json.dumps(out["strip"]), flush=True)
        save()
    if "no_regression" in parts and args.parent_root:
        out["no_regression"] = no_regression(os.path.abspath(args.parent_root), args.bench_runs, args.bench_steps,
                                             args.bench_warmup, args.ab_text)
        print("no_regression", json.dumps(out["no_regression"]), flush=True)
        save()


if __name__ == "__main__":
    main()
