"""CPU-only: the host code of guided film upscaling (csrc/upscale_host.cpp: apt_film_upscale_host, apt_film_upscale_patch_host,
apt_film_upscale_default_host) under AddressSanitizer + UndefinedBehaviorSanitizer, in the manner of tests/test_history_sanitizers.py:
compiled from source into a stand-alone driver (tests/sanitize/upscale_driver.cpp) that also checks what it computes.  Nothing loaded
into python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ascendpathtracing_amd", "csrc")
FP = ["-ffp-contract=off", "-fno-fast-math"]          # the product's own arithmetic flags (csrc/Makefile)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_upscale_host_code_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "upscale_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *FP, os.path.join(ROOT, "tests", "sanitize", "upscale_driver.cpp"), os.path.join(CSRC, "upscale_host.cpp"), "-o", exe,
                    "-lm", "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 10000      # the driver's own checks ran
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
