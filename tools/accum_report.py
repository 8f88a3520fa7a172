#!/usr/bin/env python3
"""The accumulation report (needs a GPU; there is no fallback). Writes profiles/accum_report.json (or --out).

time            cornell_direct_1920x1080_8x8: --reps repetitions (medians and spreads, max - min, one process) of
                k_accum_add and k_accum_resolve (the accumulator's HIP events), of the variance-guided pass on device
                buffers at its defaults (k_denoise_var_pack, each a-trous launch and their sum) and, beside it in the
                same loop, of the fixed-width pass (k_denoise_pack, k_denoise_atrous) on the same frame. Then the host
                wall time of render_accumulated(frames=4) against four render() calls and a numpy mean.
quality         the stochastic goldens at the seeds of tests/test_gpu_stochastic.py: RMSE and image-mean bias against
                the mean of the golden's reference renders, of one frame (seed s), of the plain mean of 4 frames
                (seeds s .. s + 3), of the fixed-width denoise at its defaults on that mean and of the variance-guided
                denoise on it at sigma_color 1, 2 (the default) and 4; means over the seeds. The same at 1 x 1 steps
                (one sample per pixel) on the same cameras.
no_regression   with --parent-root (a built checkout of the parent commit): bench.py --gpus 1 in both trees,
                alternating; --ab-text writes the runs as text.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fast_ray_tracer_amd import runtime  # noqa: E402
from features_report import no_regression  # noqa: E402
from views_report import GOLDEN, HEADLINE, ms, scene_of, spread  # noqa: E402

QUALITY_SCENES = ("cornell_gi_64", "cornell_gi_24", "cornell_caustics_64", "cornell_shipped_48_4x4")
SEEDS = (0x5EED, 0xC0FFEE, 11, 12)
SIGMAS = (1.0, 2.0, 4.0)
FRAMES = 4


def timing(reps):
    import torch
    scene = scene_of(HEADLINE)
    r = runtime.GpuRenderer(scene)
    h, w = scene.height, scene.width
    frame = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
    mean = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
    var = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
    geom = torch.empty((h, w, 8), dtype=torch.float64, device="cuda")
    ids = torch.empty((h, w, 2), dtype=torch.int32, device="cuda")
    out = torch.empty_like(frame)
    out_var = torch.empty_like(frame)
    r.render_features_into(geom.data_ptr(), ids.data_ptr())
    acc = runtime.Accumulator((h, w), device=0)
    keys = (["accum_add_ms", "accum_resolve_ms", "var_pack_ms", "var_atrous_ms", "var_total_ms", "plain_pack_ms",
             "plain_atrous_ms", "plain_total_ms"] + ["var_atrous_%d_ms" % i for i in range(5)] +
            ["plain_atrous_%d_ms" % i for i in range(5)])
    runs = {k: [] for k in keys}
    for rep in range(reps + 1):  # (the first is the warm-up: scratch, code objects)
        acc.reset()
        for k in range(2):
            r.render_into(frame.data_ptr(), seed=0x5EED + k)
            acc.add(frame.data_ptr())
        ast = acc.resolve_into(mean.data_ptr(), var.data_ptr())
        vst = runtime._denoise_var(mean.data_ptr(), var.data_ptr(), geom.data_ptr(), ids.data_ptr(), True, w, h, 1,
                                   None, "device", 0, out.data_ptr(), out_var.data_ptr())
        pst = runtime._denoise(mean.data_ptr(), geom.data_ptr(), ids.data_ptr(), True, w, h, 1, None, "device", 0,
                               out.data_ptr())
        if rep == 0:
            continue
        runs["accum_add_ms"].append(ast.add_ms)
        runs["accum_resolve_ms"].append(ast.resolve_ms)
        for tag, st in (("var", vst), ("plain", pst)):
            runs[tag + "_pack_ms"].append(st.pack_ms)
            runs[tag + "_atrous_ms"].append(st.atrous_ms)
            runs[tag + "_total_ms"].append(st.pack_ms + st.atrous_ms)
            for i in range(5):
                runs["%s_atrous_%d_ms" % (tag, i)].append(st.atrous_iter_ms[i])
    nonzero_var = float((var[..., :3] > 0).double().mean().item())
    acc.close()

    # the whole call against frames copied to the host and averaged there
    def on_host():
        frames = [r.render(seed=0x5EED + k) for k in range(FRAMES)]
        return np.mean(frames, axis=0)

    r.render_accumulated(FRAMES)
    on_host()
    dev, host = [], []
    for _ in range(reps):
        dev.append(ms(lambda: r.render_accumulated(FRAMES))[0])
        host.append(ms(on_host)[0])
    r.close()
    return {"scene": HEADLINE, "width": w, "height": h, "reps": reps, "frames_accumulated": 2,
            "pixels_with_variance": round(nonzero_var, 4), "device": {k: spread(x) for k, x in runs.items()},
            "render_accumulated_%d_wall_ms" % FRAMES: spread(dev),
            "render_x%d_numpy_mean_wall_ms" % FRAMES: spread(host)}


def _err(img, mean):
    d = img[:, :, :3] - mean
    return float(np.sqrt(np.mean(d ** 2))), float(img[:, :, :3].mean() - mean.mean())


def _quality_rows(r, mean_ref):
    rows = {}

    def put(tag, img):
        rmse, bias = _err(img, mean_ref)
        rows.setdefault(tag, {"rmse": [], "bias": []})
        rows[tag]["rmse"].append(rmse)
        rows[tag]["bias"].append(bias)

    for seed in SEEDS:
        put("one_frame", r.render(seed=seed))
        mean, var = r.render_accumulated(FRAMES, seed=seed)
        f = r.render_features(seed=seed)
        put("mean_%d" % FRAMES, mean)
        put("denoise_on_mean", runtime.denoise(mean, f))
        for sc in SIGMAS:
            put("denoise_var_sigma_%g" % sc, runtime.denoise_var(mean, var, f, params={"sigma_color": sc})[0])
    return {tag: {"rmse": float(np.mean(v["rmse"])), "bias": float(np.mean(v["bias"])),
                  "rmse_per_seed": [round(x, 6) for x in v["rmse"]]} for tag, v in rows.items()}


def quality(out, save, scenes):
    index = json.load(open(os.path.join(GOLDEN, "golden.json")))
    for name in scenes:
        refs = np.load(os.path.join(GOLDEN, index[name]["canvas"]))["refs"]
        mean_ref = refs.mean(axis=0)
        scene = scene_of(name)
        r = runtime.GpuRenderer(scene)
        full = _quality_rows(r, mean_ref)
        r.set_camera(runtime.View(scene, scene.camera, 1, 1, scene.jitter, scene.drand48_state, name + "@1x1"))
        one = _quality_rows(r, mean_ref)
        r.close()
        out[name] = {"references": int(refs.shape[0]), "shape": list(mean_ref.shape), "seeds": list(SEEDS),
                     "frames": FRAMES, "golden_steps": full, "one_sample": one}
        print(name, json.dumps({k: round(v["rmse"], 5) for k, v in full.items()}),
              json.dumps({k: round(v["rmse"], 5) for k, v in one.items()}), flush=True)
        save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_report.json"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (the A/B part)")
    ap.add_argument("--ab-text", default=None, help="also write the A/B runs as text (profiles/accum_ab_bench.txt)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--scenes", default=",".join(QUALITY_SCENES))
    ap.add_argument("--only", default="time,quality,no_regression")
    args = ap.parse_args()
    if runtime.host_lib().frt_device_count() <= 0:
        raise SystemExit("accum_report: no HIP device visible (the report is measured on the GPU)")
    parts = args.only.split(",")
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")

    if "time" in parts:
        out["time"] = timing(args.reps)
        print("time", json.dumps(out["time"]), flush=True)
        save()
    if "quality" in parts:
        out.setdefault("quality", {})
        quality(out["quality"], save, [s for s in args.scenes.split(",") if s])
    if "no_regression" in parts and args.parent_root:
        out["no_regression"] = no_regression(os.path.abspath(args.parent_root), args.bench_runs, args.bench_steps,
                                             args.bench_warmup, None)
        if args.ab_text:
            nr = out["no_regression"]
            with open(args.ab_text, "w") as f:
                f.write("# accumulation and the variance-guided denoise: the parent commit, built from a checkout of its\n"
                        "# own, against the result; python %s, %d runs per build, alternating (parent first in each\n"
                        "# pair), one session. Rule: a difference of the medians inside three times the larger of the two\n"
                        "# run-to-run spreads (max-min) is no difference.\n" % (nr["bench"], args.bench_runs))
                for who in ("parent", "this"):
                    f.write("%s ms_per_step runs %s median %.3f max-min %.3f\n"
                            % (who, nr[who + "_ms_per_step"]["runs"], nr[who + "_ms_per_step"]["median"],
                               nr[who + "_ms_per_step"]["spread"]))
                rule = 3.0 * nr["allowed_ms"]
                f.write("difference %.3f against three times the larger spread %.3f: %s\n"
                        % (nr["difference_ms"], rule, "within" if nr["difference_ms"] <= rule else "NOT within"))
        print("no_regression", json.dumps(out["no_regression"]), flush=True)
        save()


if __name__ == "__main__":
    main()
