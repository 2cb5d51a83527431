"""HEVC fullcolor (Main 4:4:4) on the HIP pipeline, on a real MI355X.

The GPU stream must be byte-identical to the CPU pipeline's (same mode
decision, integer transforms and CABAC), and its recon planes must equal
what the from-spec decoder (hevc444_ref_decoder.Decoder444) reconstructs
from the stream, for all three full-size planes. Every comparison is
exact."""

import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
from hevc444_ref_decoder import Decoder444
from pipeline_content import frames_for

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


@functools.lru_cache(maxsize=None)
def noise_frame(w, h, seed=7):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    f.setflags(write=False)
    return f


def encode(kind, frames, w, h, qp, stripe_h=64, fullcolor=True, **kw):
    return _native._pipeline_encode(kind, list(frames), w, h, qp, stripe_h, 2,
                                    fullcolor=fullcolor, **kw)


def per_frame(out):
    """[[(y, bytes) per stripe] per frame]"""
    return [[(y, bytes(d)) for d, y, hh, key in fr] for fr in out]


def assert_same_bytes(gpu, cpu, what):
    g, c = per_frame(gpu), per_frame(cpu)
    assert len(g) == len(c)
    for fi, (fg, fc) in enumerate(zip(g, c)):
        assert [y for y, _ in fg] == [y for y, _ in fc]
        for (y, a), (_, b) in zip(fg, fc):
            assert a == b, (f"{what}: frame {fi} stripe y={y} differs "
                            f"({len(a)} vs {len(b)} bytes)")


# ---- 1. GPU bytes == CPU bytes ----------------------------------------------

@pytest.mark.parametrize("qp", [18, 30, 42])
def test_bytes_equal_cpu(qp):
    require_gpu()
    w, h, n = 320, 192, 3
    fr = frames_for(w, h, n)
    gpu = encode("gpu", fr, w, h, qp)
    assert [len(f) for f in gpu] == [3] * n
    assert_same_bytes(gpu, encode("cpu", fr, w, h, qp), f"qp {qp}")


def test_bytes_equal_cpu_odd_size():
    """321x149: clamped source reads in all three planes, crop in units
    of one sample, a 21-row last stripe."""
    require_gpu()
    w, h = 321, 149
    fr = frames_for(w, h, 2)
    assert_same_bytes(encode("gpu", fr, w, h, 28),
                      encode("cpu", fr, w, h, 28), "321x149")


def test_bytes_equal_cpu_two_segments_per_row():
    """Width 1280 splits each CTU row into two slice segments."""
    require_gpu()
    w, h = 1280, 16
    fr = frames_for(w, h, 1)
    gpu = encode("gpu", fr, w, h, 30, stripe_h=16)
    assert_same_bytes(gpu, encode("cpu", fr, w, h, 30, stripe_h=16),
                      "1280x16")
    data = per_frame(gpu)[0][0][1]
    assert data.count(b"\x00\x00\x00\x01\x26\x01") == 2   # two IDR NALs


@pytest.mark.parametrize("qp", [0, 51])
def test_bytes_equal_cpu_noise(qp):
    """256x16 noise at the QP extremes: the largest CABAC payload per CTU
    (output stride sizing) and escape codes in 16x16 chroma."""
    require_gpu()
    w, h = 256, 16
    fr = (noise_frame(w, h),)
    gpu = encode("gpu", fr, w, h, qp, stripe_h=16)
    assert_same_bytes(gpu, encode("cpu", fr, w, h, qp, stripe_h=16),
                      f"noise qp {qp}")
    assert Decoder444().decode(per_frame(gpu)[0][0][1])


# ---- 2. GPU recon == decoder, all three planes -------------------------------

@pytest.mark.parametrize("w,h,qp", [(320, 192, 26), (321, 149, 34)])
def test_recon_equals_decoder(w, h, qp):
    require_gpu()
    fr = frames_for(w, h, 2)
    out, dump = encode("gpu", fr, w, h, qp, dump=True)
    assert dump["cpitch"] == dump["ypitch"]
    yh = (h + 15) & ~15
    planes = [np.frombuffer(dump[k], np.uint8).reshape(yh, dump["ypitch"])
              for k in ("y", "cb", "cr")]
    modes, cbfs = set(), [set(), set(), set()]
    for y0, data in per_frame(out)[-1]:
        dec = Decoder444()
        got = dec.decode(data)
        assert dec.sps["chroma_format_idc"] == 3
        assert dec.sps["profile_idc"] == 4
        sh = dec.sps["h"]
        for name, plane, want in zip("y cb cr".split(), planes, got[0]):
            assert want.shape == (sh, w)
            assert np.array_equal(plane[y0:y0 + sh, :w], want), \
                f"stripe y={y0} plane {name}"
        modes |= {c[0] for c in dec.ctus}
        for i in range(3):
            cbfs[i] |= {c[1 + i] for c in dec.ctus}
    assert modes == {0, 1, 10, 26}, sorted(modes)
    assert all(s == {0, 1} for s in cbfs), cbfs


# ---- 3. damage gating --------------------------------------------------------

def test_encode_mask_gates_stripes():
    require_gpu()
    w, h = 320, 192
    fr = frames_for(w, h, 3)
    mask = [[True, True, True], [True, False, True], [False, True, True]]
    gpu = encode("gpu", fr, w, h, 30, encode_mask=mask)
    for fi, f in enumerate(per_frame(gpu)):
        assert [y for y, _ in f] == \
            [y for y, m in zip((0, 64, 128), mask[fi]) if m]
    assert_same_bytes(gpu, encode("cpu", fr, w, h, 30, encode_mask=mask),
                      "masked")


# ---- 4. pipelining -----------------------------------------------------------

def test_depth2_equals_depth1():
    require_gpu()
    w, h = 320, 192
    fr = frames_for(w, h, 3)
    d1 = per_frame(encode("gpu", fr, w, h, 30))
    d2 = per_frame(encode("gpu", fr, w, h, 30, pipeline_depth=2))
    assert all(len(f) == 3 for f in d1)
    assert d1 == d2


# ---- 5. host entropy over GPU levels ----------------------------------------

def test_cpu_entropy_fallback_byte_identical():
    """HIPFLUX_CPU_HEVC_ENTROPY (host CABAC over the 4:4:4 level layout)
    gives the same bytes as the CABAC kernel. Fresh child processes: the
    variable is read when the pipeline is built."""
    require_gpu()
    code = r"""
import numpy as np, sys
from hipflux import _native
rng = np.random.default_rng(5)
w, h = 320, 128
frames = [np.ascontiguousarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8))]
out = _native._pipeline_encode("gpu", frames, w, h, 30, 64, 2, fullcolor=True)
blob = b"".join(bytes(d) for fr in out for d, y, hh, k in fr)
sys.stdout.buffer.write(blob)
"""
    env = dict(os.environ)
    env.pop("HIPFLUX_CPU_HEVC_ENTROPY", None)
    a = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       env=env, cwd=REPO)
    assert a.returncode == 0, a.stderr.decode()
    env["HIPFLUX_CPU_HEVC_ENTROPY"] = "1"
    b = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       env=env, cwd=REPO)
    assert b.returncode == 0, b.stderr.decode()
    assert len(a.stdout) > 1000
    assert a.stdout == b.stdout, (
        f"CABAC kernel vs host entropy differ "
        f"({len(a.stdout)} vs {len(b.stdout)} bytes)")
    dec = Decoder444()
    dec.decode(a.stdout[:a.stdout.index(b"\x00\x00\x00\x01\x40\x01", 4)])
    assert dec.sps["chroma_format_idc"] == 3


# ---- 6. engine ---------------------------------------------------------------

@pytest.mark.parametrize("gpu_frontend", [False, True])
def test_engine_emits_main444(gpu_frontend):
    require_gpu()
    w, h = 128, 64
    s = _native.CaptureSettings()
    s.capture_width = w
    s.capture_height = h
    s.target_fps = 30
    s.output_mode = 2
    s.video_fullcolor = True
    s.use_cpu = False
    s.gpu_id = 0
    s.capture_backend = "synthetic:noise"
    s.video_fullframe = True
    s.stripe_height = 64
    s.gpu_frontend = gpu_frontend
    got = []
    done = threading.Event()

    def cb(data, frame_id, y, width, height, key, *a):
        if key and not done.is_set():
            got.append((bytes(data), y, width, height))
            done.set()

    cap = _native.ScreenCapture()
    cap.start_capture(cb, s)
    arrived = done.wait(10)
    pipeline = cap.pipeline
    frontend = cap.frontend
    cap.stop_capture()
    assert arrived, "no keyframe stripe arrived"
    assert pipeline == "hip-hevc", pipeline
    assert frontend == ("hip" if gpu_frontend else "host")
    data, y, width, height = got[0]
    assert (y, width, height) == (0, w, h)
    dec = Decoder444()
    frames = dec.decode(data[10:])
    assert dec.sps["chroma_format_idc"] == 3 and dec.sps["profile_idc"] == 4
    assert [p.shape for p in frames[0]] == [(h, w)] * 3


# ---- 7. 4:2:0 guard ----------------------------------------------------------

def test_420_still_equals_cpu():
    require_gpu()
    w, h = 320, 192
    fr = frames_for(w, h, 2)
    gpu = _native._pipeline_encode("gpu", list(fr), w, h, 30, 64, 2)
    cpu = _native._pipeline_encode("cpu", list(fr), w, h, 30, 64, 2)
    assert_same_bytes(gpu, cpu, "4:2:0")
    dec = Decoder444()
    dec.decode(per_frame(gpu)[0][0][1])
    assert dec.sps["chroma_format_idc"] == 1 and dec.sps["profile_idc"] == 1
