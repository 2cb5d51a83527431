"""ASan + UBSan over the host code of HEVC P pictures (CPU encoder chains
and the host entropy path with P jobs): native/tests/hevcp_asan_main.cpp, a
stand-alone host program built and run by `make -C native asan-hevcp`."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))


def test_hevc_p_host_code_under_asan_ubsan():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "native"),
                        "asan-hevcp"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "hevcp sanitizer harness ok" in r.stdout
