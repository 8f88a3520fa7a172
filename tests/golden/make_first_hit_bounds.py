#!/usr/bin/env python3
"""Write tests/golden/first_hit_bounds.json: the largest deviations of the CPU oracle's first hits
(oracle.first_hits) from the extended-precision reference (tests/first_hit_ref.py) over the decided samples of every
view of tests/first_hit_views.py, per leaf type: |t_ref - t| / max(1, t) and |n_ref - n|; and the undecided share
of every view. No GPU. tests/test_first_hit_cpu.py recomputes them and requires each to be at most what is recorded
here; tests/test_first_hit.py holds the device to the same figures (the toroid: 4 x).

The figures are recorded rounded up to two significant digits, so a libm whose cbrt / acos / cos (the toroid's
solve_cubic) differ in the last place from the recording machine's still reproduces them.

Every type but the toroid must stay within 1e-9 in t, the bound tests/test_features.py derives for the sphere at the
same discriminant clearance; the toroid's figure is what the reference's quartic solver gives.

  python tests/golden/make_first_hit_bounds.py
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def round_up(x):
    """x rounded up to two significant digits."""
    if x <= 0.0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return float("%de%d" % (math.ceil(x / 10.0 ** e), e))


def measure():
    import first_hit_views as views
    types, undecided, hits = {}, {}, {}
    for key in views.KEYS:
        r = views.reference_of(key)
        mask_ok, leaf_ok, dev = views.deviations(r, *views.oracle_of(key))
        assert mask_ok and leaf_ok, key
        undecided[key] = float(r["undecided"].mean())
        hits[key] = {k: v["hits"] for k, v in dev.items()}
        for name, d in dev.items():
            cur = types.setdefault(name, {"t": 0.0, "normal": 0.0})
            cur["t"], cur["normal"] = max(cur["t"], d["t"]), max(cur["normal"], d["normal"])
    types = {name: {k: round_up(v) for k, v in d.items()} for name, d in types.items()}
    undecided = {key: round_up(v) for key, v in undecided.items()}
    return {"types": types, "undecided": undecided}, hits


def main():
    bounds, hits = measure()
    for name, d in sorted(bounds["types"].items()):
        print("%-16s t %.3e  normal %.3e" % (name, d["t"], d["normal"]))
        assert name == "toroid" or d["t"] <= 1e-9, (name, d)
    for key, share in bounds["undecided"].items():
        print("%-40s undecided %.4f  decided hits %s" % (key, share, hits[key]))
    with open(os.path.join(HERE, "first_hit_bounds.json"), "w") as f:
        json.dump(bounds, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
