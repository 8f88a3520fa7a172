#!/usr/bin/env python3
"""The reprojection report (needs a GPU; there is no fallback). Writes profiles/reproject_report.json (or --out).
Medians of --reps with spread max - min, each part measured in one process. Every device step (the kernel part, the
wall part, each quality scene, each bench.py run) is a child process under a time limit of its own, one at a time; a
step that fails or runs into its limit is killed and ends the report there, with the parts before it saved.

kernel          cornell_direct_1920x1080_8x8: k_accum_reproject (HIP events) on device-resident buffers, for the
                identical camera and for a pan of about 8 pixels, against the time its unique bytes need at the copy
                rate measured on this part: one read of each view's features, one read and one write of the state,
                computed from the shapes.
wall            a temporal().render(view, frames=1) step (views alternating, so every step reprojects) against
                render_accumulated(1) plus render_features() of the same view.
quality         the stochastic goldens at the seeds of tests/test_gpu_stochastic.py, view A the golden's own and view
                B panned by about three pixels: RMSE at B, against the mean of 64 frames at B, of one frame, of four
                frames at A reprojected plus that frame, and of five frames at B.
no_regression   with --parent-root (a built checkout of the parent commit): bench.py --gpus 1 in both trees,
                alternating; --ab-text writes the runs as text.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fast_ray_tracer_amd import runtime  # noqa: E402
from features_report import no_regression  # noqa: E402
from views_report import HEADLINE, ms, scene_of, spread  # noqa: E402

QUALITY_SCENES = ("cornell_gi_64", "cornell_gi_24", "cornell_caustics_64", "cornell_shipped_48_4x4")
SEEDS = (0x5EED, 0xC0FFEE, 11, 12)
COPY_RATE_TBS = 6.29  # measured copy rate of the MI355X (read + write counted), the roofline of DESIGN.md
REFERENCE_FRAMES = 64


def panned(scene, pixels):
    """The scene's own camera moved sideways by about `pixels` pixels of a surface as far away as the point it looks
    at (taken as far from the eye as the world's origin is) and 3 % of that distance forwards (the cornell goldens'
    eye lies on the face of the slab behind it: a view moved sideways alone starts inside), looking the same way."""
    cam = runtime.flat_camera(scene)
    inv = np.array(cam.inv).reshape(4, 4)
    eye, left, up, fwd = inv[:3, 3], inv[:3, 0], inv[:3, 1], -inv[:3, 2]
    dist = max(1.0, float(np.linalg.norm(eye)))
    shift = pixels * cam.pixel_size / cam.canvas_distance * dist
    at = eye + shift * left + 0.03 * dist * fwd
    return scene.view(tuple(at), tuple(at + dist * fwd), up=tuple(up))


def state_bytes(npx):
    """The model's unique bytes: both views' features (64 + 8 per pixel each), the state read and written (60)."""
    return npx * (2 * (8 * 8 + 2 * 4) + 2 * (7 * 8 + 4))


def kernel(reps):
    import torch
    scene = scene_of(HEADLINE)
    view_b = panned(scene, 8.0)
    r = runtime.GpuRenderer(scene)
    h, w = scene.height, scene.width
    feats = []
    for v in (scene, view_b):
        r.set_camera(v)
        geom = torch.empty((h, w, 8), dtype=torch.float64, device="cuda")
        ids = torch.empty((h, w, 2), dtype=torch.int32, device="cuda")
        r.render_features_into(geom.data_ptr(), ids.data_ptr())
        feats.append((geom, ids))
    r.set_camera(scene)
    src, dst = runtime.Accumulator((h, w), device=0), runtime.Accumulator((h, w), device=0)
    r._accumulate(src, 2, 0x5EED, 0, None, False)
    ptr = [(g.data_ptr(), i.data_ptr()) for g, i in feats]
    runs, counts = {"identical": [], "pan_8": []}, {}
    for rep in range(reps + 1):  # (the first is the warm-up)
        for tag, cur, cf in (("identical", scene, ptr[0]), ("pan_8", view_b, ptr[1])):
            st = runtime.reproject(dst, src, scene, ptr[0], cur, cf, stats=True)
            counts[tag] = {k: v for k, v in st.as_dict().items() if k in ("reprojected", "missed", "no_history")}
            if rep:
                runs[tag].append(st.kernel_ms)
    src.close()
    dst.close()
    r.close()
    nbytes = state_bytes(w * h)
    model_ms = nbytes / (COPY_RATE_TBS * 1e12) * 1e3
    out = {"scene": HEADLINE, "width": w, "height": h, "reps": reps, "unique_bytes": nbytes,
           "copy_rate_tb_s": COPY_RATE_TBS, "model_ms": round(model_ms, 4), "outcomes": counts}
    for tag, v in runs.items():
        out[tag + "_ms"] = spread(v)
        out[tag + "_over_model"] = round(out[tag + "_ms"]["median"] / model_ms, 2)
    return out


def wall(reps):
    scene = scene_of(HEADLINE)
    views = [scene, panned(scene, 8.0)]
    r = runtime.GpuRenderer(scene)
    t = r.temporal()
    temporal, plain = [], []

    def by_hand(v):
        r.set_camera(v)
        r.render_accumulated(1)
        r.render_features()

    for v in views:
        t.render(v)
        by_hand(v)
    for k in range(reps):
        v = views[k % 2]
        temporal.append(ms(lambda: t.render(v, frames=1))[0])
        plain.append(ms(lambda: by_hand(v))[0])
    t.close()
    r.close()
    return {"scene": HEADLINE, "reps": reps, "temporal_step_wall_ms": spread(temporal),
            "render_accumulated_1_plus_features_wall_ms": spread(plain)}


def _rmse(img, ref):
    return float(np.sqrt(np.mean((img[..., :3] - ref[..., :3]) ** 2)))


def quality_scene(name):
    scene = scene_of(name)
    view_b = panned(scene, 3.0)
    r = runtime.GpuRenderer(scene)
    rows = {"one_frame": [], "four_at_a_reprojected_plus_one": [], "five_at_b": []}
    outcomes = None
    r.set_camera(view_b)
    ref = r.render_accumulated(REFERENCE_FRAMES, seed=1000)[0]
    for seed in SEEDS:
        t = r.temporal(seed=seed)
        t.render(scene, frames=4)
        mean, _, info = t.render(view_b, frames=1, stats=True)
        t.close()
        outcomes = {k: info["reproject"][k] for k in ("reprojected", "missed", "no_history")}
        rows["four_at_a_reprojected_plus_one"].append(_rmse(mean, ref))
        rows["one_frame"].append(_rmse(r.render(seed=(seed + 4) & 0xFFFFFFFFFFFFFFFF), ref))
        rows["five_at_b"].append(_rmse(r.render_accumulated(5, seed=seed)[0], ref))
    r.close()
    return {"shape": list(ref.shape), "seeds": list(SEEDS), "reference_frames": REFERENCE_FRAMES, "pan_pixels": 3.0,
            "outcomes_last_seed": outcomes,
            "rmse": {k: {"mean": float(np.mean(v)), "per_seed": [round(x, 6) for x in v]} for k, v in rows.items()}}


def child(step, reps, seconds):
    """One device step in a process of its own under its time limit; its result, or the end of the report."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(reps)]
    try:
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired:
        raise SystemExit("reproject_report: %s ran into its limit of %d s; nothing more is started" % (step, seconds))
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        raise SystemExit("reproject_report: %s failed (exit %d); nothing more is started\n%s"
                         % (step, p.returncode, p.stderr[-2000:]))
    return json.loads(lines[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_report.json"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (the A/B part)")
    ap.add_argument("--ab-text", default=None, help="also write the A/B runs as text (profiles/reproject_ab_bench.txt)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--scenes", default=",".join(QUALITY_SCENES))
    ap.add_argument("--only", default="kernel,wall,quality,no_regression")
    ap.add_argument("--child", default=None, help="(internal) run one device step and print its result")
    args = ap.parse_args()
    if args.child:
        step = args.child
        res = (kernel(args.reps) if step == "kernel" else wall(args.reps) if step == "wall"
               else quality_scene(step.split(":", 1)[1]))
        print("RESULT " + json.dumps(res), flush=True)
        return
    if runtime.host_lib().frt_device_count() <= 0:
        raise SystemExit("reproject_report: no HIP device visible (the report is measured on the GPU)")
    parts = args.only.split(",")
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")

    for part in ("kernel", "wall"):
        if part in parts:
            out[part] = child(part, args.reps, 400)
            print(part, json.dumps(out[part]), flush=True)
            save()
    if "quality" in parts:
        out.setdefault("quality", {})
        for name in [s for s in args.scenes.split(",") if s]:
            out["quality"][name] = child("quality:" + name, args.reps, 600)
            print(name, json.dumps({k: round(v["mean"], 6) for k, v in out["quality"][name]["rmse"].items()}),
                  json.dumps(out["quality"][name]["outcomes_last_seed"]), flush=True)
            save()
    if "no_regression" in parts and args.parent_root:
        out["no_regression"] = no_regression(os.path.abspath(args.parent_root), args.bench_runs, args.bench_steps,
                                             args.bench_warmup, None)
        if args.ab_text:
            nr = out["no_regression"]
            with open(args.ab_text, "w") as f:
                f.write("# temporal reprojection: the parent commit, built from a checkout of its own, against the\n"
                        "# result; python %s,\n"
                        "# %d runs per build, alternating (parent first in each pair), one session. The device code\n"
                        "# of render_frame's kernels is the same in both builds. Rule: the medians differ by no more\n"
                        "# than the larger of the two run-to-run spreads (max-min).\n"
                        % (nr["bench"], args.bench_runs))
                for who in ("parent", "this"):
                    f.write("%s ms_per_step runs %s median %.3f max-min %.3f\n"
                            % (who, nr[who + "_ms_per_step"]["runs"], nr[who + "_ms_per_step"]["median"],
                               nr[who + "_ms_per_step"]["spread"]))
                f.write("difference %.3f against the larger spread %.3f: %s\n"
                        % (nr["difference_ms"], nr["allowed_ms"], "within" if nr["passes"] else "NOT within"))
        print("no_regression", json.dumps(out["no_regression"]), flush=True)
        save()


if __name__ == "__main__":
    main()
