#!/usr/bin/env python3
"""The denoise report (needs a GPU; there is no fallback). Writes profiles/denoise_report.json (or --out).

time            cornell_direct_1920x1080_8x8: the frame and its feature buffers rendered once into device memory, then
                --reps repetitions of the device pass on them at the defaults (5 iterations): k_denoise_pack, each
                a-trous launch and their sum from the pass's HIP events, medians and spreads (max - min). The same
                pass from host buffers (upload and read-back apart), render_denoised beside render (host wall time
                around calls that end in the frame's copy to the host), and the host pass on one CPU.
                (The LDS-staged kernel's A/B, measured before it was dropped: profiles/denoise_lds_experiment.json.)
quality         the stochastic goldens at the seeds of tests/test_gpu_stochastic.py: RMSE and mean absolute difference
                of the GPU frame to the mean of the golden's reference renders, before and after the filter at the
                defaults, and the image-mean bias; per seed and as means. Then, for every scene alike (nothing is
                tuned per scene), the mean RMSE ratio at sigma_color 1, 1/4, 1/16 and 1/64 and at 1, 2, 3 and 5
                iterations: what the defaults' footprint costs on frames that are already converged. And the
                defaults once more on the same cameras at 1 x 1 steps (one sample per pixel: the noisy input the
                filter is for), against the same reference means ("one_sample").
no_regression   with --parent-root (a built checkout of the parent commit): bench.py --gpus 1 in both trees,
                alternating; the rule of profiles/r09_ab_refactor.txt. --ab-text writes the runs as text.
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
SWEEP = ([("sigma_color=%g" % sc, {"sigma_color": sc}) for sc in (1.0, 0.25, 0.0625, 0.015625)] +
         [("iterations=%d" % n, {"iterations": n}) for n in (1, 2, 3, 5)])


def timing(reps):
    import torch
    scene = scene_of(HEADLINE)
    r = runtime.GpuRenderer(scene)
    h, w = scene.height, scene.width
    frame = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
    geom = torch.empty((h, w, 8), dtype=torch.float64, device="cuda")
    ids = torch.empty((h, w, 2), dtype=torch.int32, device="cuda")
    out = torch.empty_like(frame)
    r.render_into(frame.data_ptr())
    r.render_features_into(geom.data_ptr(), ids.data_ptr())
    torch.cuda.synchronize()

    def device_pass():
        return runtime._denoise(frame.data_ptr(), geom.data_ptr(), ids.data_ptr(), True, w, h, 1, None, "device", 0,
                                out.data_ptr())

    device_pass()  # (warm-up: the scratch, the code objects)
    result = out.cpu().numpy()
    keys = ["pack_ms", "atrous_ms", "total_ms"] + ["atrous_%d_ms" % i for i in range(5)]
    runs = {k: [] for k in keys}
    valid = 0
    for _ in range(reps):
        st = device_pass()
        valid = int(st.valid_pixels)
        runs["pack_ms"].append(st.pack_ms)
        runs["atrous_ms"].append(st.atrous_ms)
        runs["total_ms"].append(st.pack_ms + st.atrous_ms)
        for i in range(5):
            runs["atrous_%d_ms" % i].append(st.atrous_iter_ms[i])
    device = {k: spread(x) for k, x in runs.items()}

    # host buffers: upload and read-back apart
    h_frame, h_geom, h_ids = frame.cpu().numpy(), geom.cpu().numpy(), ids.cpu().numpy()
    hostbuf = {k: [] for k in ("upload_ms", "pack_ms", "atrous_ms", "readback_ms", "wall_ms")}
    runtime.denoise(h_frame, (h_geom, h_ids))
    for _ in range(reps):
        t, (res, st) = ms(lambda: runtime.denoise(h_frame, (h_geom, h_ids), stats=True))
        for k in ("upload_ms", "pack_ms", "atrous_ms", "readback_ms"):
            hostbuf[k].append(getattr(st, k))
        hostbuf["wall_ms"].append(t)
    same_host_buffers = bool(np.array_equal(res.view(np.uint64), result.view(np.uint64)))

    # the whole call beside a plain frame
    r.render()
    r.render_denoised()
    plain, den = [], []
    for _ in range(reps):
        plain.append(ms(r.render)[0])
        den.append(ms(r.render_denoised)[0])
    _, fst = r.render_features(stats=True)
    r.close()

    # the host pass, one thread
    host = []
    for _ in range(min(reps, 3)):
        res, st = runtime.denoise(h_frame, (h_geom, h_ids), backend="host", stats=True)
        host.append(st.host_ms)
    return {"scene": HEADLINE, "width": w, "height": h, "iterations": 5, "reps": reps, "valid_pixels": valid,
            "device_buffers": device,
            "host_buffers": {k: spread(x) for k, x in hostbuf.items()}, "host_buffers_identical": same_host_buffers,
            "render_wall_ms": spread(plain), "render_denoised_wall_ms": spread(den),
            "features_render_ms": round(fst.render_ms, 3), "host_pass_ms": spread(host),
            "host_identical": bool(np.array_equal(res.view(np.uint64), result.view(np.uint64)))}


def quality():
    index = json.load(open(os.path.join(GOLDEN, "golden.json")))
    out = {}
    for name in QUALITY_SCENES:
        refs = np.load(os.path.join(GOLDEN, index[name]["canvas"]))["refs"]
        mean = refs.mean(axis=0)
        r = runtime.GpuRenderer(scene_of(name))
        rows, sweep = [], {key: [] for key, _ in SWEEP}
        for seed in SEEDS:
            frame = r.render(seed=seed)
            f = r.render_features(seed=seed)
            den, st = runtime.denoise(frame, f, stats=True)
            row = {"seed": seed, "valid_pixels": int(st.valid_pixels)}
            for tag, img in (("before", frame), ("after", den)):
                d = img[:, :, :3] - mean
                row["rmse_" + tag] = float(np.sqrt(np.mean(d ** 2)))
                row["mad_" + tag] = float(np.abs(d).mean())
                row["bias_" + tag] = float(img[:, :, :3].mean() - mean.mean())
            rows.append(row)
            for key, params in SWEEP:
                d = runtime.denoise(frame, f, params=params)[:, :, :3] - mean
                sweep[key].append(float(np.sqrt(np.mean(d ** 2))) / row["rmse_before"])
        # the same camera at one sample per pixel
        scene = r.scene
        r.set_camera(runtime.View(scene, scene.camera, 1, 1, scene.jitter, scene.drand48_state, name + "@1x1"))
        one = {"rmse_before": [], "rmse_after": [], "mad_before": [], "mad_after": []}
        for seed in SEEDS:
            frame = r.render(seed=seed)
            den = runtime.denoise(frame, r.render_features(seed=seed))
            for tag, img in (("before", frame), ("after", den)):
                d = img[:, :, :3] - mean
                one["rmse_" + tag].append(float(np.sqrt(np.mean(d ** 2))))
                one["mad_" + tag].append(float(np.abs(d).mean()))
        one = {k: float(np.mean(v)) for k, v in one.items()}
        one["rmse_ratio"] = one["rmse_after"] / one["rmse_before"]
        one["mad_ratio"] = one["mad_after"] / one["mad_before"]
        r.close()
        summary = {k: float(np.mean([row[k] for row in rows])) for k in rows[0] if k not in ("seed", "valid_pixels")}
        summary["rmse_ratio"] = summary["rmse_after"] / summary["rmse_before"]
        summary["mad_ratio"] = summary["mad_after"] / summary["mad_before"]
        # what a single reference render is from the mean of the others: the noise floor of this comparison
        k = refs.shape[0]
        summary["rmse_ref_to_mean_of_others"] = float(np.mean(
            [np.sqrt(np.mean((refs[i] - np.delete(refs, i, axis=0).mean(axis=0)) ** 2)) for i in range(k)]))
        out[name] = {"references": int(k), "shape": list(mean.shape), "seeds": rows, "mean": summary, "one_sample": one,
                     "rmse_ratio_sweep": {key: round(float(np.mean(v)), 4) for key, v in sweep.items()}}
        print(name, json.dumps(summary), json.dumps(out[name]["rmse_ratio_sweep"]), json.dumps(one),
              flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_report.json"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (the A/B part)")
    ap.add_argument("--ab-text", default=None, help="also write the A/B runs as text")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--only", default="time,quality,no_regression")
    args = ap.parse_args()
    if runtime.host_lib().frt_device_count() <= 0:
        raise SystemExit("denoise_report: no HIP device visible (the report is measured on the GPU)")
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
        out["quality"] = quality()
        save()
    if "no_regression" in parts and args.parent_root:
        out["no_regression"] = no_regression(os.path.abspath(args.parent_root), args.bench_runs, args.bench_steps,
                                             args.bench_warmup, None)
        if args.ab_text:
            nr = out["no_regression"]
            with open(args.ab_text, "w") as f:
                f.write("# denoise: the parent commit, built from a checkout of its own, against the result;\n"
                        "# python %s, %d runs per build, alternating (parent first in each pair), one session.\n"
                        "# Rule: the medians differ by no more than the larger of the two run-to-run spreads (max-min).\n"
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
