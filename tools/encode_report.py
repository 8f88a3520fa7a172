#!/usr/bin/env python3
"""The device image encode's report (needs a GPU; there is no fallback).

For every golden canvas and the three modes (ppm_scaled, ppm_clamped, png): the values the device left undecided,
whether the device's bytes equal the host pass's, and (ppm_scaled) whether they hash to the reference's ppm_sha256.
The selftest's worst deviation of the device's sRGB curve from the host libm's (frt_encode_selftest, 2^20 values).
With --headline also cornell_direct_1920x1080_8x8: one render_multi frame (a page-locked canvas) encoded per mode by
the host pass and by the device, alternated call by call in one process (1 warm-up and --steps timed rounds); the
host pass's wall time, and the device's four phases (upload, kernels, read-back, host patching) and their sum, each as
median / min / max; the same from a pageable copy of the canvas, from a random canvas of that size (the rendered frame
is mostly dark and skips pow there; every random value takes the pow branch) and from device memory (render_encoded:
no upload).

Writes profiles/encode_report.json (or --out).
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_ray_tracer_amd import build  # noqa: E402
from fast_ray_tracer_amd import runtime  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MODES = runtime.ENCODE_MODES
HEADLINE = "cornell_direct_1920x1080_8x8"
PHASES = ("upload_ms", "kernel_ms", "readback_ms", "patch_ms")


def ppm_bytes(values):
    h, w = values.shape[:2]
    return b"P6\n%d %d\n65535\n" % (w, h) + values.astype(">u2").tobytes() + b"\n"


def golden_report(name, entry):
    canvas = np.load(os.path.join(GOLDEN, entry["canvas"]))["canvas"]
    out = {}
    for mode in MODES:
        host, _ = runtime.encode16(canvas, mode, backend="host")
        dev, st = runtime.encode16(canvas, mode, backend="device")
        out[mode] = {"backend": st["backend"], "decline": st["decline"], "values": st["values"],
                     "undecided": st["undecided"], "equals_host": bool(np.array_equal(host, dev))}
        if mode == "ppm_scaled" and "ppm_sha256" in entry:
            out[mode]["reference_sha256"] = hashlib.sha256(ppm_bytes(dev)).hexdigest() == entry["ppm_sha256"]
    return out


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def timed_rounds(canvas, steps):
    """host and device encodes of one host canvas, alternated; per mode the host's wall ms and the device's phases"""
    out = {}
    for mode in MODES:
        host_ms, dev = [], {k: [] for k in PHASES + ("sum_ms", "wall_ms")}
        undecided = equal = None
        for k in range(steps + 1):
            t0 = time.perf_counter()
            hv, hst = runtime.encode16(canvas, mode, backend="host")
            t1 = time.perf_counter()
            dv, st = runtime.encode16(canvas, mode, backend="device")
            t2 = time.perf_counter()
            if st["backend"] != "device":
                raise RuntimeError("%s: the device declined: %s" % (mode, st))
            undecided, equal = st["undecided"], bool(np.array_equal(hv, dv))
            if k == 0:  # (the warm-up round: the device's buffers grow to this size in it)
                first = round(sum(st[p] for p in PHASES), 4)
                continue
            host_ms.append(hst["host_ms"])
            for p in PHASES:
                dev[p].append(st[p])
            dev["sum_ms"].append(sum(st[p] for p in PHASES))
            dev["wall_ms"].append((t2 - t1) * 1e3)  # (the call from Python, its output array and conversion included)
        out[mode] = {"host_ms": spread(host_ms), "device": {k: spread(v) for k, v in dev.items()},
                     "device_warmup_round_sum_ms": first, "undecided": undecided, "equals_host": equal}
    return out


def headline_report(steps):
    scene = runtime.Scene(build.build_scene(os.path.join(GOLDEN, "scenes", HEADLINE + ".c")),
                          asset_root=os.path.join(GOLDEN, "assets"))
    canvas = runtime.render_multi(scene, devices="0")
    out = {"scene": HEADLINE, "steps": steps, "width": scene.width, "height": scene.height,
           "values": 3 * scene.width * scene.height,
           "share_of_values_on_the_pow_branch": float((canvas[:, :, :3] >= 0.0031308).mean()),
           "page_locked_canvas": timed_rounds(canvas, steps), "pageable_canvas": timed_rounds(canvas.copy(), steps)}
    # (the rendered frame is mostly dark: for scale, a canvas whose every value takes the pow branch)
    rnd = np.zeros(canvas.shape)
    rnd[:, :, :3] = np.random.default_rng(1).random(canvas[:, :, :3].shape) * 1.2 + 0.01
    out["random_canvas_same_size"] = timed_rounds(rnd, steps)
    host = {mode: runtime.encode16(canvas, mode, backend="host")[0] for mode in MODES}
    del canvas
    runtime.release_render_multi()
    r = runtime.GpuRenderer(scene)
    try:
        res = {}
        for mode in MODES:
            ph = {k: [] for k in PHASES + ("sum_ms",)}
            for k in range(steps + 1):
                v, st = r.render_encoded(mode, batch_samples=1 << 27)
                if st["backend"] != "device":
                    raise RuntimeError("%s: the device declined: %s" % (mode, st))
                if k:
                    for p in PHASES:
                        ph[p].append(st[p])
                    ph["sum_ms"].append(sum(st[p] for p in PHASES))
            res[mode] = {"device": {k: spread(x) for k, x in ph.items()}, "undecided": st["undecided"],
                         "equals_host_of_render_multi_frame": bool(np.array_equal(v, host[mode]))}
        out["device_resident_canvas"] = res
    finally:
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--headline", action="store_true", help="also time the encode of a 1920x1080 frame")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_report.json"))
    args = ap.parse_args()

    with open(os.path.join(GOLDEN, "golden.json")) as f:
        index = json.load(f)
    report = {"margin": "2^-40", "goldens": {}}
    for name in sorted(n for n, e in index.items() if "canvas" in e):
        report["goldens"][name] = golden_report(name, index[name])
        print(name, json.dumps(report["goldens"][name]), flush=True)
    g = report["goldens"].values()
    report["goldens_summary"] = {
        "canvases": len(report["goldens"]),
        "all_equal_host": all(m["equals_host"] for e in g for m in e.values()),
        "all_on_device": all(m["backend"] == "device" for e in g for m in e.values()),
        "all_reference_sha256": all(e["ppm_scaled"].get("reference_sha256", True) for e in g),
        "undecided_total": {mode: sum(e[mode]["undecided"] for e in g) for mode in MODES}}
    bad, out = runtime.encode_selftest(1 << 20, 0x5EED)
    report["selftest"] = {"n": 1 << 20, "failed": bad, "worst_srgb_deviation": out[0],
                          "worst_srgb_deviation_log2": float(np.log2(out[0])) if out[0] > 0 else None,
                          "worst_pow_deviation": out[1], "values_differing_from_host": int(out[2]),
                          "bound": "2^-44"}
    print("selftest", json.dumps(report["selftest"]), flush=True)
    if args.headline:
        report["headline"] = headline_report(args.steps)
        print("headline", json.dumps(report["headline"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("summary:", json.dumps(report["goldens_summary"]))


if __name__ == "__main__":
    main()
