"""gpu_frontend end to end through ScreenCapture on a real MI355X: the
same synthetic desktop capture (frames and cursor are a pure function of
the acquire count) encoded once with the host front end and once with the
device one must emit byte-identical stripes, for every HIP pipeline and
both scale modes, with damage gating on."""

import threading

import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native

N_FRAMES = 8


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


def run(output_mode, gpu_frontend, **scale):
    s = _native.CaptureSettings()
    s.capture_width = 256
    s.capture_height = 128
    s.target_fps = 60
    s.output_mode = output_mode
    s.use_cpu = False
    s.gpu_id = 0
    s.capture_backend = "synthetic:desktop"
    s.capture_cursor = True
    s.video_fullframe = False       # damage gating, default threshold
    s.damage_block_duration = 2     # so that gating bites within 8 frames
    s.video_cbr_mode = False
    s.video_crf = 24
    s.stripe_height = 32
    s.gpu_frontend = gpu_frontend
    for k, v in scale.items():
        setattr(s, k, v)
    assert s.damage_block_threshold == 15
    got = []
    done = threading.Event()

    def cb(data, frame_id, y, width, height, key, *a):
        # frame N_FRAMES arriving means frames 0..N_FRAMES-1 are complete
        if frame_id >= N_FRAMES:
            done.set()
        else:
            got.append((frame_id, y, bytes(data)))

    cap = _native.ScreenCapture()
    cap.start_capture(cb, s)
    ok = done.wait(20)
    pipeline = cap.pipeline
    frontend_ms = cap.last_frontend_ms
    frontend = cap.frontend
    cap.stop_capture()
    assert ok, "capture did not reach the frame count"
    assert pipeline.startswith("hip"), pipeline
    assert frontend_ms > 0
    assert frontend == ("hip" if gpu_frontend else "host")
    return got


@pytest.mark.parametrize("output_mode", [0, 1, 2])
@pytest.mark.parametrize("scale", [dict(capture_scale=0.5),
                                   dict(capture_scale_div=2)],
                         ids=["bilinear0.5", "box2"])
def test_gpu_frontend_stream_identical(output_mode, scale):
    require_gpu()
    host = run(output_mode, False, **scale)
    dev = run(output_mode, True, **scale)
    assert {f for f, _, _ in host} == set(range(N_FRAMES))
    assert len(host) == len(dev)
    for (hf, hy, hd), (df, dy, dd) in zip(host, dev):
        assert (hf, hy) == (df, dy)
        assert hd == dd, f"frame {hf} stripe y={hy} differs"
    # gating really gated: fewer stripes than frames x stripe rows
    assert len(host) < N_FRAMES * (64 // 32)
