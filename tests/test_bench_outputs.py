"""bench.py --dump-outputs and the plain / --full split: the rows a dump holds (CPU), and one plain run of the
benchmark on a small golden scene (GPU): its JSON line carries the headline only and its dumped canvas is the
reference's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden_canvas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

FULL_ONLY = ("shipped", "gi", "scaling_proxy", "cpu_baseline", "roofline", "roofline_shadow_pass",
             "render_multi_wall_ms")


def test_dump_rows_takes_every_row_that_fits():
    rows = bench.dump_rows(1080, 1920 * 4 * 8, limit=1 << 30)
    assert rows.tolist() == list(range(1080))


def test_dump_rows_samples_within_the_limit_and_repeats():
    row_bytes = 1920 * 4 * 8
    rows = bench.dump_rows(1080, row_bytes)
    assert 0 < len(rows) < 1080  # (the headline canvas, 66.4 MB, is over the limit)
    assert len(rows) * (row_bytes + 8) + 2 * 4096 <= bench.DUMP_LIMIT_BYTES
    assert (len(rows) + 1) * (row_bytes + 8) + 2 * 4096 > bench.DUMP_LIMIT_BYTES  # (as many as fit)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 1080
    assert rows.tolist() == bench.dump_rows(1080, row_bytes).tolist()
    with pytest.raises(RuntimeError):
        bench.dump_rows(4, bench.DUMP_LIMIT_BYTES)


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_canvas(built, tmp_path):
    name = "cornell_direct_64_4x4"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--scene", name, "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["unit"] == "Mrays/s" and out["value"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert not [k for k in FULL_ONLY if k in out]
    canvas = np.load(tmp_path / "canvas.npy")
    rows = np.load(tmp_path / "canvas_rows.npy")
    assert canvas.dtype == np.float64 and canvas.shape == (64, 64, 4)
    assert rows.dtype == np.float64 and rows.tolist() == list(range(64))
    # the parity bound of the deterministic goldens (tests/test_gpu_parity.py)
    assert np.abs(canvas[:, :, :3] - load_golden_canvas(name)).max() <= 1e-4
