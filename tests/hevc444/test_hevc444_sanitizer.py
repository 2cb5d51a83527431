"""ASan + UBSan over the HEVC CPU encoder in fullcolor and the host entropy
path over the 4:4:4 level layout: native/tests/hevc444_asan_main.cpp, a
stand-alone host program built and run by `make -C native asan-hevc444`."""

import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))


def test_hevc444_host_code_under_asan_ubsan():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "native"),
                        "asan-hevc444"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "hevc444 sanitizer harness ok" in r.stdout
    # the worst-case bytes per CTU it reports stay under half the HIP
    # pipeline's fullcolor CABAC stride (4096 bytes per CTU)
    figures = [float(v) for line in r.stdout.splitlines()
               if line.startswith("fullcolor qp0")
               for v in re.findall(r"([\d.]+) \(", line)]
    assert len(figures) == 6
    assert max(figures) <= 2048, figures
