import os
import shutil
import sys
import tempfile
from pathlib import Path

import pytest

# make the repo root importable regardless of invocation directory
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture()
def sock_dir():
    """Per-test directory with a SHORT path, for AF_UNIX sockets.

    sockaddr_un.sun_path holds 108 bytes and pytest's tmp_path (base temp
    dir + user + run + test name) can exceed that on its own, so tests
    that bind unix sockets use this instead of tmp_path."""
    base = next((d for d in (tempfile.gettempdir(), "/tmp", "/dev/shm",
                             "/var/tmp")
                 if len(d) <= 32 and os.path.isdir(d)
                 and os.access(d, os.W_OK | os.X_OK)), None)
    if base is None:
        pytest.fail("no writable temp directory with a path short enough "
                    "for AF_UNIX sockets")
    d = tempfile.mkdtemp(prefix="sk-", dir=base)
    yield Path(d)
    shutil.rmtree(d, ignore_errors=True)


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires an AMD GPU (MI355X); skipped in CPU CI")


def pytest_collection_modifyitems(config, items):
    """Skip gpu-marked tests automatically when no HIP device is present,
    unless the run explicitly selects them (-m gpu)."""
    if config.getoption("-m") and "gpu" in config.getoption("-m"):
        return
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU available")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
