"""CPU-only: the host code of every film stage (csrc/<stage>_host.cpp with the scaffold they share, csrc/film_stage_host.cpp: the
checks, the defaults and the CPU twins of libdenoise, libadaptive, libhistory, libpost, libmetrics and libupscale) under
AddressSanitizer + UndefinedBehaviorSanitizer, in the manner of tests/test_film_sanitizers.py: compiled from source into a stand-alone
driver (tests/sanitize/<stage>_driver.cpp) that also checks what it computes; and, in the same manner, the CPU twin of the first-bounce
plan (csrc/first_plan_host.cpp with csrc/pt_first_plan.h, tests/sanitize/first_plan_driver.cpp).  Nothing loaded into python runs under
a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ascendpathtracing_amd", "csrc")
FP = ["-ffp-contract=off", "-fno-fast-math"]          # the product's own arithmetic flags (csrc/Makefile)
# stage -> the least number of its own checks the driver must report
MIN_CHECKS = {"denoise": 10000, "adaptive": 10000, "history": 10000, "post": 10000, "metrics": 10000, "upscale": 10000}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("stage", list(MIN_CHECKS))
def test_stage_host_code_under_asan_and_ubsan(stage, tmp_path):
    exe = str(tmp_path / f"{stage}_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *FP, os.path.join(ROOT, "tests", "sanitize", f"{stage}_driver.cpp"), os.path.join(CSRC, f"{stage}_host.cpp"),
                    os.path.join(CSRC, "film_stage_host.cpp"), "-o", exe, "-lm", "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > MIN_CHECKS[stage]      # the driver's own checks ran
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_first_plan_twin_under_asan_and_ubsan(tmp_path):
    """The edge shapes (1 x 1, one row, one column, 2^24 squared, beyond 2^24, 2^32 - 1 squared), members of the test family written out as
    numbers, every refusing premise and non-finite entry; the driver checks the record's invariants, the members' records and the mask."""
    exe = str(tmp_path / "first_plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *FP, os.path.join(ROOT, "tests", "sanitize", "first_plan_driver.cpp"), os.path.join(CSRC, "first_plan_host.cpp"),
                    "-o", exe, "-lm", "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 100000      # the driver's own checks ran
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
