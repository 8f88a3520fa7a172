#!/usr/bin/env python3
"""The fast shading mode's mismatch report (needs a GPU; there is no fallback).

For every deterministic canvas golden: the parity and the fast32 frame of one handle, and per scene
  max_abs_vs_reference   max |fast32 - golden canvas|
  max_abs_vs_parity      max |fast32 - parity|
  ppm_mismatch_fraction  share of the 16-bit PPM channel values (encode_ppm) that differ from the golden canvas's
  ppm_max_step           the largest such difference in quantised steps
  parity_* : the same figures of the parity frame, for comparison
  sub_ms                 k_shade_lit / k_shade_lit32 of an instrumented frame of each mode
cornell_shipped_48_4x4 (a stochastic light cache) against parity at the same seed. With --headline also
cornell_direct_1920x1080_8x8 and cornell_shipped_1920x1080_8x8: the whole frame in one batch, 5 warm-up and 20 timed
frames per mode, the modes alternated frame by frame in one process; HIP-event frame times (frt_frame_stats.render_ms)
and the shading kernels' sub_ms, each as median / min / max.

Writes profiles/fast32_mismatch.json (or --out).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_ray_tracer_amd import build  # noqa: E402
from fast_ray_tracer_amd.runtime import GpuRenderer, Scene, ppm_values  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

SHIPPED_SMALL = "cornell_shipped_48_4x4"
HEADLINE = ("cornell_direct_1920x1080_8x8", "cornell_shipped_1920x1080_8x8")
KERNEL = {"parity": "k_shade_lit", "fast32": "k_shade_lit32"}


def golden_index():
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        return json.load(f)


def load_scene(name):
    return Scene(build.build_scene(os.path.join(GOLDEN, "scenes", name + ".c")),
                 asset_root=os.path.join(GOLDEN, "assets"))


def against(img, ref):
    got, want = ppm_values(img), ppm_values(ref)
    return {"max_abs": float(np.abs(img - ref).max()), "ppm_mismatch_fraction": float((got != want).mean()),
            "ppm_max_step": int(np.abs(got - want).max())}


def scene_report(name, reference):
    r = GpuRenderer(load_scene(name))
    try:
        frames, sub = {}, {}
        for mode in ("parity", "fast32"):
            img, st = r.render(stats=True, precision=mode)
            d = st.as_dict()
            if d["errors"]:
                raise RuntimeError("%s (%s): engine errors %s" % (name, mode, d["errors"]))
            frames[mode] = img[:, :, :3]
            sub[mode] = {KERNEL[mode]: round(d["sub_ms"].get(KERNEL[mode], 0.0), 4), "lit_nodes": d["lit_nodes"]}
    finally:
        r.close()
    out = {"finite": bool(np.isfinite(frames["fast32"]).all()),
           "max_abs_vs_parity": float(np.abs(frames["fast32"] - frames["parity"]).max()),
           "channels_differing_from_parity": float((frames["fast32"] != frames["parity"]).mean()), "sub_ms": sub}
    if reference is not None:
        f, p = against(frames["fast32"], reference), against(frames["parity"], reference)
        out.update({"max_abs_vs_reference": f["max_abs"], "ppm_mismatch_fraction": f["ppm_mismatch_fraction"],
                    "ppm_max_step": f["ppm_max_step"], "parity_max_abs_vs_reference": p["max_abs"],
                    "parity_ppm_mismatch_fraction": p["ppm_mismatch_fraction"], "parity_ppm_max_step": p["ppm_max_step"]})
    else:
        f = against(frames["fast32"], frames["parity"])
        out.update({"ppm_mismatch_fraction_vs_parity": f["ppm_mismatch_fraction"],
                    "ppm_max_step_vs_parity": f["ppm_max_step"]})
    return out


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def headline_report(name, warmup, steps, batch_samples):
    import torch
    scene = load_scene(name)
    r = GpuRenderer(scene)
    shard = torch.zeros((scene.height, scene.width, 4), dtype=torch.float64, device="cuda")
    times = {m: {"frame_ms": [], KERNEL[m]: [], "shade": []} for m in KERNEL}
    frames = {}
    try:
        for k in range(warmup + steps):
            for mode in ("parity", "fast32"):  # (alternated: both modes see the same clocks and the same neighbours)
                st = r.render_into(shard.data_ptr(), batch_samples=batch_samples, stats=True, precision=mode)
                d = st.as_dict()
                if d["errors"]:
                    raise RuntimeError("%s (%s): engine errors %s" % (name, mode, d["errors"]))
                if k >= warmup:
                    times[mode]["frame_ms"].append(d["render_ms"])
                    times[mode][KERNEL[mode]].append(d["sub_ms"][KERNEL[mode]])
                    times[mode]["shade"].append(d["kernel_ms"]["shade"])
                if k == warmup + steps - 1:
                    frames[mode] = shard.cpu().numpy()[:, :, :3].copy()
    finally:
        r.close()
        del shard
    f = against(frames["fast32"], frames["parity"])
    return {"frames": steps, "warmup": warmup, "batch_samples": batch_samples,
            "parity": {k: spread(v) for k, v in times["parity"].items()},
            "fast32": {k: spread(v) for k, v in times["fast32"].items()},
            "finite": bool(np.isfinite(frames["fast32"]).all()), "max_abs_vs_parity": f["max_abs"],
            "ppm_mismatch_fraction_vs_parity": f["ppm_mismatch_fraction"], "ppm_max_step_vs_parity": f["ppm_max_step"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--headline", action="store_true", help="also time the two 1920x1080 8x8 frames in both modes")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch-samples", type=int, default=1 << 27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast32_mismatch.json"))
    args = ap.parse_args()

    index = golden_index()
    report = {"scenes": {}}
    for name in sorted(n for n, e in index.items() if "canvas" in e and not e.get("stochastic")):
        reference = np.load(os.path.join(GOLDEN, index[name]["canvas"]))["canvas"]
        report["scenes"][name] = scene_report(name, reference)
        print(name, json.dumps(report["scenes"][name]), flush=True)
    worst = max(report["scenes"], key=lambda n: report["scenes"][n]["max_abs_vs_reference"])
    worst_ppm = max(report["scenes"], key=lambda n: report["scenes"][n]["ppm_mismatch_fraction"])
    report["worst"] = {"scene": worst, "max_abs_vs_reference": report["scenes"][worst]["max_abs_vs_reference"],
                       "ppm_scene": worst_ppm,
                       "ppm_mismatch_fraction": report["scenes"][worst_ppm]["ppm_mismatch_fraction"],
                       "ppm_max_step": max(s["ppm_max_step"] for s in report["scenes"].values())}
    report["stochastic_vs_parity"] = {SHIPPED_SMALL: scene_report(SHIPPED_SMALL, None)}
    print(SHIPPED_SMALL, json.dumps(report["stochastic_vs_parity"][SHIPPED_SMALL]), flush=True)
    if args.headline:
        report["headline"] = {}
        for name in HEADLINE:
            report["headline"][name] = headline_report(name, args.warmup, args.steps, args.batch_samples)
            print(name, json.dumps(report["headline"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("worst:", json.dumps(report["worst"]))


if __name__ == "__main__":
    main()
