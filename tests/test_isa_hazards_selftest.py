"""CPU: the hazard scan of tests/test_isa_hazards.py (no TRANS result read by the very next VALU instruction) on the code object of the
seeded-divide self-test (csrc/selftest_seeded.hip), which `make asm` lists next to the render and material kernels."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_selftest_unit_has_no_trans_hazard_and_holds_its_kernel():
    csrc = os.path.join(ROOT, "ascendpathtracing_amd", "csrc")
    listing = os.path.join(csrc, "selftest_seeded.s")
    # (this unit alone: the whole `asm` target takes minutes and tests/test_isa_hazards.py runs it)
    flags = subprocess.run(["make", "-s", "-C", csrc, "--eval=print-flags: ; @echo $(HIPCC) $(HIPFLAGS)", "print-flags"],
                           check=True, capture_output=True, text=True).stdout.split()
    subprocess.run(flags + ["--cuda-device-only", "-S", "selftest_seeded.hip", "-o", listing], cwd=csrc, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(listing).read()
    assert "selftest_div3_seeded_kernel" in text and "v_rsq_f32" in text
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "check_hazards.py"), listing], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
