"""Host side of the capture front end: DamageTracker.apply_dirty against
update(), the overlay code moved to cpu/overlay.h against a numpy mirror
of its formulas and origin math, and the refactored bilinear downscale
against the numpy mirror of its fixed-point math. No GPU needed."""

import numpy as np
import pytest

hipflux = pytest.importorskip("hipflux")
if not hipflux.native_available():
    pytest.skip("hipflux native module not built", allow_module_level=True)

from hipflux import _native

import frontend_mirror as fm

W, H = 250, 90


@pytest.mark.parametrize("threshold", [0, 15])
@pytest.mark.parametrize("duration", [1, 3])
def test_apply_dirty_matches_update(threshold, duration):
    """Flags derived in numpy and fed to apply_dirty give the ages and
    still-frame count update() computes from the frames themselves, after
    every frame of a six-frame sequence (50x37: partial last blocks)."""
    w, h = 50, 37
    rng = np.random.default_rng(100 * threshold + duration)
    a = _native._DamageTracker()
    b = _native._DamageTracker()
    a.reset(w, h)
    b.reset(w, h)
    assert (a.blocks_x, a.blocks_y) == (4, 3)
    # keep clear of 0/255 so every +-delta below lands exactly
    cur = rng.integers(100, 156, (h, w, 4), dtype=np.uint8)
    prev = None
    seen_dirty = seen_clean = False
    for f in range(6):
        if f in (1, 2, 4):   # frames 3 and 5 repeat their predecessor
            for _ in range(3):
                x, y, c = rng.integers(0, w), rng.integers(0, h), \
                    rng.integers(0, 4)
                # at, just above, and far above the threshold
                delta = int(rng.choice([threshold, threshold + 1, 40]))
                sign = int(rng.choice([-1, 1]))
                cur[y, x, c] = int(cur[y, x, c]) + sign * delta
        buf, stride = fm.padded(cur)
        a.update(buf, stride, threshold, duration)
        if prev is None:
            b.apply_dirty(None, duration)
        else:
            flags = fm.block_flags(cur, prev, threshold)
            seen_dirty |= bool(flags.any())
            seen_clean |= not flags.all()
            b.apply_dirty(flags.reshape(-1), duration)
        assert np.array_equal(a.ages(), b.ages()), f
        assert a.consecutive_still_frames() == b.consecutive_still_frames(), f
        prev = cur.copy()
    assert seen_dirty and seen_clean
    # frame 5 repeats frame 4: a still frame
    assert a.consecutive_still_frames() >= 1


def _cpu_overlay(frame, wm=None, location=0, frame_idx=0, cursor=None):
    h, w, _ = frame.shape
    fe = _native._frontend_cpu(w, h)
    if wm is not None:
        fe.set_watermark(wm.tobytes(), wm.shape[1], wm.shape[0], location)
    buf, stride = fm.padded(frame)
    cur = None
    if cursor is not None:
        argb, cx, cy = cursor
        cur = (argb.tobytes(), argb.shape[1], argb.shape[0], cx, cy)
    r = fe.process(buf, stride, cursor=cur, frame_idx=frame_idx,
                   damage=False)
    assert (r["w"], r["h"]) == (w, h)
    return np.frombuffer(r["frame"], np.uint8).reshape(h, w, 4)


# location 6 on a 250x90 frame with a 40x20 mark: sx = 210, sy = 70, so x
# reflects between frame 69 (207) and 70 (209), y between 34 (68) and 35
# (69); 139 -> 140 wraps x back to 0
@pytest.mark.parametrize("location,frame_idx", [
    (1, 0), (2, 0), (3, 0), (4, 0), (5, 0),
    (6, 0), (6, 34), (6, 35), (6, 69), (6, 70), (6, 139), (6, 140)])
def test_watermark_matches_numpy(location, frame_idx):
    rng = np.random.default_rng(7)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    wm = fm.make_watermark(rng, 40, 20)
    got = _cpu_overlay(frame, wm, location, frame_idx)
    exp = fm.blend_watermark(frame, wm, location, frame_idx)
    assert not np.array_equal(exp, frame)
    assert np.array_equal(got, exp)
    assert np.array_equal(got[..., 3], frame[..., 3])


def test_watermark_origin_reflects():
    """The mirror's own bounce, pinned to hand-computed origins."""
    assert fm.watermark_origin(6, W, H, 40, 20, 69) == (207, 1)
    assert fm.watermark_origin(6, W, H, 40, 20, 70) == (209, 0)
    assert fm.watermark_origin(6, W, H, 40, 20, 34) == (102, 68)
    assert fm.watermark_origin(6, W, H, 40, 20, 35) == (105, 69)


@pytest.mark.parametrize("location", [2, 4])
def test_oversized_watermark_clips(location):
    """A 300x100 mark on 250x90: negative origin, clipped on all sides."""
    rng = np.random.default_rng(8)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    wm = fm.make_watermark(rng, 300, 100)
    got = _cpu_overlay(frame, wm, location)
    assert np.array_equal(got, fm.blend_watermark(frame, wm, location, 0))


@pytest.mark.parametrize("cx,cy", [(-5, -7), (247, 86), (100, 40),
                                   (-12, 3), (250, 0)])
def test_cursor_matches_numpy(cx, cy):
    rng = np.random.default_rng(9)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    argb = fm.make_cursor(rng)
    got = _cpu_overlay(frame, cursor=(argb, cx, cy))
    exp = fm.blend_cursor(frame, argb, cx, cy)
    if -12 < cx < W:
        assert not np.array_equal(exp, frame)
    assert np.array_equal(got, exp)


def test_watermark_then_cursor_order():
    rng = np.random.default_rng(10)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    wm = fm.make_watermark(rng, 40, 20)
    argb = fm.make_cursor(rng)
    got = _cpu_overlay(frame, wm, 1, 0, cursor=(argb, 20, 20))
    exp = fm.blend_cursor(fm.blend_watermark(frame, wm, 1, 0), argb, 20, 20)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("w,h", [(157, 93), (64, 48), (17, 5)])
def test_refactored_bilinear_matches_numpy(w, h):
    rng = np.random.default_rng(21)
    src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    for scale in (0.25, 0.3, 0.5, 2 / 3, 0.8125, 0.9):
        data, ow, oh = _native._bilinear_downscale(src.tobytes(), w, h, scale)
        exp = fm.bilinear(src, scale)
        assert (oh, ow) == exp.shape[:2], scale
        got = np.frombuffer(data, np.uint8).reshape(oh, ow, 4)
        assert np.array_equal(got, exp), scale


@pytest.mark.parametrize("div", [2, 3, 4])
def test_cpu_twin_box_matches_numpy(div):
    rng = np.random.default_rng(22)
    src = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    fe = _native._frontend_cpu(W, H, scale_div=div)
    buf, stride = fm.padded(src)
    r = fe.process(buf, stride, damage=False)
    exp = fm.box(src, div)
    got = np.frombuffer(r["frame"], np.uint8).reshape(r["h"], r["w"], 4)
    assert np.array_equal(got, exp)


def test_gpu_frontend_setting_falls_back_on_cpu_pipeline():
    """gpu_frontend with a CPU pipeline: the engine says so once, takes the
    host front end, and the stream is the one it emits without the
    setting; last_frontend_ms is filled on the host path."""
    import threading

    def run(flag):
        s = _native.CaptureSettings()
        s.capture_width = 256
        s.capture_height = 128
        s.capture_scale = 0.5
        s.capture_cursor = True
        s.target_fps = 60
        s.output_mode = 0
        s.use_cpu = True
        s.gpu_id = -1
        s.capture_backend = "synthetic:desktop"
        s.damage_block_duration = 2
        s.stripe_height = 32
        s.gpu_frontend = flag
        got, done = [], threading.Event()

        def cb(data, frame_id, y, *a):
            if frame_id >= 4:
                done.set()
            else:
                got.append((frame_id, y, bytes(data)))

        cap = _native.ScreenCapture()
        cap.start_capture(cb, s)
        ok = done.wait(10)
        name, ms, where = cap.pipeline, cap.last_frontend_ms, cap.frontend
        cap.stop_capture()
        assert ok and name == "cpu-jpeg" and where == "host"
        assert ms > 0
        return got

    assert _native.CaptureSettings().gpu_frontend is False
    assert run(True) == run(False)
