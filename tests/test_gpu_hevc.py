"""HIP HEVC pipeline (gfx950) correctness on a real MI355X.

The GPU pipeline must be BYTE-IDENTICAL to the CPU striped HEVC pipeline
(same deterministic mode decision, same integer transforms, same CABAC
byte emitter), and its streams must reconstruct bit-exactly under the
from-spec Python decoder. HIPFLUX_CPU_HEVC_ENTROPY isolates the rows
kernel from the CABAC kernel when chasing a mismatch."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
from hevc_ref_decoder import Decoder
from pipeline_content import assert_planes_equal, dump_planes


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


def psnr(a, b):
    mse = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).mean()
    return 10 * math.log10(255 * 255 / max(mse, 1e-12))


def make_frames(w, h, n, seed=42):
    rng = np.random.default_rng(seed)
    base = np.zeros((h, w, 4), np.uint8)
    base[:, :, 0] = np.linspace(0, 255, w, dtype=np.uint8)[None, :]
    base[:, :, 1] = np.linspace(0, 255, h, dtype=np.uint8)[:, None]
    base[:, :, 2] = 80
    base[:, :, 3] = 255
    band = min(16, h // 4)
    base[h // 2:h // 2 + band, :] = rng.integers(
        0, 256, (band, w, 4), dtype=np.uint8)
    frames = []
    for i in range(n):
        f = base.copy()
        x = (16 + i * 24) % max(1, w - 48)
        f[16:48, x:x + 48, 0] = 255
        f[16:48, x:x + 48, 2] = 0
        frames.append(np.ascontiguousarray(f))
    return frames


def encode(kind, frames, w, h, qp, stripe_h=64):
    return _native._pipeline_encode(kind, frames, w, h, qp, stripe_h, 2)


def flatten(per_frame):
    out = {}
    for fr in per_frame:
        for data, y, hgt, key in fr:
            assert key, "HEVC stripes are all-intra (always keyframes)"
            out.setdefault(y, b"")
            out[y] += bytes(data)
    return out


@pytest.mark.parametrize("qp", [18, 30, 42])
def test_gpu_byte_identical_to_cpu(qp):
    require_gpu()
    w, h, n = 320, 192, 4
    frames = make_frames(w, h, n)
    gpu = encode("gpu", frames, w, h, qp)
    cpu = encode("cpu", frames, w, h, qp)
    rows_g, rows_c = flatten(gpu), flatten(cpu)
    assert set(rows_g) == set(rows_c) == {0, 64, 128}
    for y in rows_c:
        assert rows_g[y] == rows_c[y], (
            f"qp={qp} stripe y={y}: GPU stream differs from CPU "
            f"({len(rows_g[y])} vs {len(rows_c[y])} bytes)")


def test_gpu_multislice_width_byte_identical():
    """Width >= 1280 triggers multiple slice segments per CTU row."""
    require_gpu()
    w, h = 1280, 128
    frames = make_frames(w, h, 2)
    gpu = flatten(encode("gpu", frames, w, h, 30))
    cpu = flatten(encode("cpu", frames, w, h, 30))
    for y in cpu:
        assert gpu[y] == cpu[y], f"stripe y={y} differs"


def test_gpu_odd_dims_byte_identical():
    require_gpu()
    w, h = 322, 150   # conformance-window cropping + clamped source reads
    frames = make_frames(w, h, 2)
    gpu = flatten(encode("gpu", frames, w, h, 28))
    cpu = flatten(encode("cpu", frames, w, h, 28))
    for y in cpu:
        assert gpu[y] == cpu[y], f"stripe y={y} differs"


def test_gpu_stream_decodes_bit_exact():
    require_gpu()
    w, h, n = 320, 192, 3
    frames = make_frames(w, h, n)
    out, dump = _native._pipeline_encode("gpu", frames, w, h, 26, 64, 2, True)
    rows = flatten(out)
    for y, stream in rows.items():
        decoded = Decoder().decode(stream)
        assert len(decoded) == n
        # the kernel's recon planes hold the last frame: equal to what
        # the decoder makes of it, in all three planes
        assert_planes_equal(dump_planes(dump, h), y, decoded[-1],
                            f"stripe y={y}")
    # and the recon resembles the source (last frame's top stripe)
    dy = Decoder().decode(rows[0])[-1][0]
    src_y, _, _ = _native.bgrx_to_yuv420(frames[-1].tobytes(), w, h)
    src = np.frombuffer(src_y, np.uint8).reshape(h, w)[:64]
    assert psnr(dy, src) > 30


def test_gpu_noise_4k_stripe_decodes():
    """One 4K-width stripe of pure noise (worst case) stays byte-identical
    and decodable — exercises the 4-segment row split and escape coding."""
    require_gpu()
    rng = np.random.default_rng(7)
    w, h = 3840, 64
    frames = [np.ascontiguousarray(
        rng.integers(0, 256, (h, w, 4), dtype=np.uint8))]
    gpu = flatten(encode("gpu", frames, w, h, 30))
    cpu = flatten(encode("cpu", frames, w, h, 30))
    assert gpu[0] == cpu[0]
    assert Decoder().decode(gpu[0])


def test_cpu_entropy_fallback_byte_identical():
    """HIPFLUX_CPU_HEVC_ENTROPY (host CABAC over GPU levels) must produce
    the same bytes as the GPU CABAC kernel — run in a subprocess since the
    env var is read at pipeline construction."""
    require_gpu()
    code = r"""
import numpy as np, sys
sys.path.insert(0, "tests")
from hipflux import _native
rng = np.random.default_rng(5)
w, h = 320, 128
frames = [np.ascontiguousarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8))]
out = _native._pipeline_encode("gpu", frames, w, h, 30, 64, 2)
blob = b"".join(bytes(d) for fr in out for d, y, hh, k in fr)
sys.stdout.buffer.write(blob)
"""
    env = dict(os.environ)
    env.pop("HIPFLUX_CPU_HEVC_ENTROPY", None)
    a = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       env=env, cwd=os.path.dirname(os.path.dirname(
                           os.path.abspath(__file__))))
    assert a.returncode == 0, a.stderr.decode()
    env["HIPFLUX_CPU_HEVC_ENTROPY"] = "1"
    b = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       env=env, cwd=os.path.dirname(os.path.dirname(
                           os.path.abspath(__file__))))
    assert b.returncode == 0, b.stderr.decode()
    assert a.stdout == b.stdout, (
        f"GPU CABAC kernel vs host entropy differ "
        f"({len(a.stdout)} vs {len(b.stdout)} bytes)")
