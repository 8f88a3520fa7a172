"""csrc/frt_cam_index.hpp on the host: the multiply-shift division that level 0's camera index math uses where a batch
fits 32 bits (frt_camera.hpp camera_sample), and the rule that says when it does (frt_engine.hip batch_camera_index).
The header is plain C++, so tests/cam_index_check.cpp includes it and is compiled here with the host compiler alone.

Divisors 1, 2, 3, 9, 63, 64, 65, 1919, 1920 and 2^31 - 1; dividends 0, 2^32 - 1, and for every k <= 32 the multiples
of the divisor next to 2^k, each with the values one below and one above it. Quotient and remainder must equal / and
%. The rule must refuse a batch whose last pixel index is 2^32 (and admit the headline frame)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "fast_ray_tracer_amd", "csrc")


def test_multiply_shift_division_and_the_32_bit_rule(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++ or clang++) to build tests/cam_index_check.cpp with")
    exe = tmp_path / "cam_index_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe),
                    os.path.join(HERE, "cam_index_check.cpp")], check=True, capture_output=True, text=True, timeout=120)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert p.stdout.strip().splitlines()[-1].startswith("OK ")
