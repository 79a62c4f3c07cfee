"""The plan of a whole fit / kneighbors (kiez_amd/csrc/kz_fit_plan.h: which searches kz_fit runs, whether the forward lists come out
of the fit, which tail kz_kneighbors runs, the buffer sizes, every refusal) has no HIP dependency: tests/host/fit_plan_sanitize.cpp
enumerates it over small n, K, kinds and flags against the documented rules written out independently, under AddressSanitizer +
UBSan on the CPU build (tests/test_host_sanitize.py: the same recipe for the other host-only headers)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_fit_plan_follows_the_documented_rules_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "fit_plan_sanitize"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                            "-Werror", str(ROOT / "tests" / "host" / "fit_plan_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "0 failures" in run.stdout and " plans checked" in run.stdout, run.stdout[-2000:]
    assert int(run.stdout.split(" plans checked")[0].split()[-1]) > 100000


def test_plan_constants_agree_with_the_binding():
    """The limits the plan header names are the ones the Python side documents."""
    from kiez_amd import _native as N
    text = (ROOT / "kiez_amd" / "csrc" / "kz_fit_plan.h").read_text()
    assert f"KZ_FIT_SPLIT_MAX_K1 = {N.MAX_FUSED_NEIGHBORS};" in text
    assert f"KZ_FIT_FUSED_MAX_K = {N.RESCALE_SELECT_FUSED_MAX_K};" in text
    assert f"KZ_FIT_MAX_K = {N.MAX_NEIGHBORS - 1};" in text
