"""The host-side fit behind the shared sweep's model thresholds (kiez_amd/csrc/kz_floor.h: kz_theta_fit, kz_floor_r2) under
AddressSanitizer + UBSan: tests/host/theta_fit_sanitize.cpp is a program of its own (the header has no HIP dependency), built with
g++ and run as a child process -- no sanitized code is loaded into this interpreter.  It fits an exact line, a probe with constant
|t_c|^2, probes with non-finite values and with zero rows, and counts saturated and short rows on constructed probes."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_theta_fit_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "theta_fit_sanitize"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                            "-Werror", str(ROOT / "tests" / "host" / "theta_fit_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "0 failures" in run.stdout, run.stdout[-2000:]
