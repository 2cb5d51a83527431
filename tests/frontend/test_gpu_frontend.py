"""Capture front end on a real MI355X: GpuFrontEnd.process (upload,
overlay, downscale and 16x16 block diff kernels) against _frontend_cpu,
the engine's host code, byte for byte: scaled frame, size, block ages and
still-frame count after every frame.

Sizes are the small, non-multiple-of-16 ones at which these kernels can go
wrong: 250x90 (16x6 blocks, last column and row 10 px), 64x48 and 17x5.
The source stride is always width*4 + 12 with noise in the pad bytes."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native

import frontend_mirror as fm

W, H = 250, 90


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


class Pair:
    """The device front end and its host twin, fed the same calls."""

    def __init__(self, w, h, **kw):
        require_gpu()
        self.gpu = _native.GpuFrontEnd(w, h, **kw)
        self.cpu = _native._frontend_cpu(w, h, **kw)

    def set_watermark(self, wm, location):
        for fe in (self.gpu, self.cpu):
            fe.set_watermark(wm.tobytes(), wm.shape[1], wm.shape[0],
                             location)

    def step(self, frame, cursor=None, tag="", **kw):
        """Process one (h, w, 4) frame on both; assert equality; return
        the host twin's result."""
        h, w, _ = frame.shape
        buf, stride = fm.padded(frame)
        cur = None
        if cursor is not None:
            argb, cx, cy = cursor
            cur = (argb.tobytes(), argb.shape[1], argb.shape[0], cx, cy)
        g = self.gpu.process(buf, stride, cursor=cur, width=w, height=h, **kw)
        c = self.cpu.process(buf, stride, cursor=cur, width=w, height=h, **kw)
        assert (g["w"], g["h"]) == (c["w"], c["h"]), tag
        gf = np.frombuffer(g["frame"], np.uint8)
        cf = np.frombuffer(c["frame"], np.uint8)
        assert gf.size == c["w"] * c["h"] * 4, tag
        bad = np.flatnonzero(gf != cf)
        assert bad.size == 0, (
            f"{tag}: {bad.size} bytes differ, first at byte {bad[:1]}")
        assert np.array_equal(g["ages"], c["ages"]), tag
        assert g["still_frames"] == c["still_frames"], tag
        return c


SCALES = [dict(scale=s) for s in (0.25, 0.3, 0.5, 0.67, 0.9)] + \
         [dict(scale_div=d) for d in (2, 3, 4)]


@pytest.mark.parametrize("w,h", [(250, 90), (64, 48), (17, 5)])
@pytest.mark.parametrize("mode", SCALES, ids=lambda m: "-".join(
    f"{k}{v}" for k, v in m.items()))
def test_gpu_scale(w, h, mode):
    """Bilinear and box downscale, all four bytes, random content; a
    second frame with a few changed pixels runs the diff at that size."""
    rng = np.random.default_rng(w * 7 + h)
    p = Pair(w, h, **mode)
    frame = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    r = p.step(frame, tag="frame 0")
    if "scale" in mode:
        exp = fm.bilinear(frame, mode["scale"])
    else:
        exp = fm.box(frame, mode["scale_div"])
    assert (r["h"], r["w"]) == exp.shape[:2]
    assert np.array_equal(
        np.frombuffer(r["frame"], np.uint8).reshape(exp.shape), exp)
    frame = frame.copy()
    frame[h // 2, w // 2] ^= 0x80
    frame[h - 1, w - 1] ^= 0x80
    p.step(frame, tag="frame 1")


def test_gpu_scale_none_keeps_frame():
    rng = np.random.default_rng(3)
    p = Pair(W, H)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    r = p.step(frame)
    assert r["frame"] == frame.tobytes()


@pytest.mark.parametrize("cx,cy", [(-5, -7), (247, 86), (100, 40)])
def test_gpu_cursor(cx, cy):
    rng = np.random.default_rng(11)
    p = Pair(W, H)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    argb = fm.make_cursor(rng)
    r = p.step(frame, cursor=(argb, cx, cy))
    exp = fm.blend_cursor(frame, argb, cx, cy)
    assert not np.array_equal(exp, frame)
    assert r["frame"] == exp.tobytes()
    # same position, new shape: the image must be uploaded again
    argb2 = fm.make_cursor(np.random.default_rng(12))
    r = p.step(frame, cursor=(argb2, cx, cy), tag="new shape")
    assert r["frame"] == fm.blend_cursor(frame, argb2, cx, cy).tobytes()


@pytest.mark.parametrize("location,frame_idx,size", [
    (1, 0, (40, 20)), (2, 0, (40, 20)), (3, 0, (40, 20)), (4, 0, (40, 20)),
    (5, 0, (40, 20)), (6, 35, (40, 20)), (6, 70, (40, 20)),
    (2, 0, (300, 100)), (4, 0, (300, 100))])
def test_gpu_watermark(location, frame_idx, size):
    """Locations 1..6; the 300x100 mark has a negative origin and is
    clipped on all sides of the 250x90 frame."""
    rng = np.random.default_rng(13)
    p = Pair(W, H)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    wm = fm.make_watermark(rng, *size)
    p.set_watermark(wm, location)
    r = p.step(frame, frame_idx=frame_idx)
    exp = fm.blend_watermark(frame, wm, location, frame_idx)
    assert not np.array_equal(exp, frame)
    assert r["frame"] == exp.tobytes()


# block kinds on the 16x6 grid of 250x90, with the pixel touched in each:
# the far corner of the partial blocks, so an edge slip shows
INTERIOR = [((2, 1), (40, 20)), ((5, 2), (95, 47))]
LASTCOL = [((15, 1), (249, 30)), ((15, 3), (249, 63))]
LASTROW = [((3, 5), (50, 89)), ((8, 5), (140, 89))]
CORNER = ((15, 5), (249, 89))


@pytest.mark.parametrize("variant", [0, 1])
def test_gpu_damage_threshold_edges(variant):
    """Threshold 15, duration 3, five frames. Frame f (1..4) changes one
    byte of channel f-1 (B, G, R, X) by exactly 16 in one interior, one
    last-column and one last-row block, and by exactly 15 in another of
    each; the corner block alternates 16 / 15 per frame. The variant
    swaps which blocks (and which corner frames) get 16."""
    rng = np.random.default_rng(14)
    p = Pair(W, H)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    sites = INTERIOR + LASTCOL + LASTROW + [CORNER]
    for _, (x, y) in sites:
        frame[y, x] = 100
    bx = 16
    r = p.step(frame, threshold=15, duration=3, tag="frame 0")
    assert (r["ages"] == 3).all()
    expect = np.full(16 * 6, 3, np.int64)
    for f in range(1, 5):
        ch = f - 1
        frame = frame.copy()
        dirty = []
        for kind in (INTERIOR, LASTCOL, LASTROW):
            (b16, p16), (b15, p15) = kind if variant == 0 else kind[::-1]
            frame[p16[1], p16[0], ch] += 16
            frame[p15[1], p15[0], ch] += 15
            dirty.append(b16)
        (cb, (cx, cy)) = CORNER
        if (f + variant) % 2:
            frame[cy, cx, ch] += 16
            dirty.append(cb)
        else:
            frame[cy, cx, ch] += 15
        r = p.step(frame, threshold=15, duration=3, tag=f"frame {f}")
        expect = np.maximum(expect - 1, 0)
        for (i, j) in dirty:
            expect[j * bx + i] = 3
        assert np.array_equal(r["ages"], expect), f
    # everything decays to 0 on still frames
    for f in range(5, 8):
        r = p.step(frame, threshold=15, duration=3, tag=f"still {f}")
    assert (r["ages"] == 0).all()
    assert r["still_frames"] == 3


def test_gpu_damage_threshold_zero():
    rng = np.random.default_rng(15)
    p = Pair(W, H)
    frame = rng.integers(1, 255, (H, W, 4), dtype=np.uint8)
    p.step(frame, threshold=0, duration=1)
    for f, (x, y, ch, d) in enumerate([(0, 0, 0, 1), (249, 89, 3, -1),
                                       (128, 40, 2, 1)]):
        frame = frame.copy()
        frame[y, x, ch] = int(frame[y, x, ch]) + d
        r = p.step(frame, threshold=0, duration=1, tag=f"frame {f + 1}")
        exp = np.zeros(16 * 6, np.uint16)
        exp[(y // 16) * 16 + x // 16] = 1
        assert np.array_equal(r["ages"], exp)
    r = p.step(frame, threshold=0, duration=1, tag="still")
    assert (r["ages"] == 0).all() and r["still_frames"] == 1


def test_gpu_composed_moving_cursor():
    """Watermark, moving cursor, 0.5x bilinear, then damage: four frames."""
    rng = np.random.default_rng(16)
    p = Pair(W, H, scale=0.5)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    wm = fm.make_watermark(rng, 40, 20)
    p.set_watermark(wm, 6)
    argb = fm.make_cursor(rng)
    for f in range(4):
        r = p.step(frame, cursor=(argb, 30 + 37 * f, 10 + 21 * f),
                   frame_idx=f, threshold=15, duration=2, tag=f"frame {f}")
        assert (r["w"], r["h"]) == (125, 45)
    assert 0 < np.count_nonzero(r["ages"]) < r["ages"].size


def test_gpu_resolution_change():
    """The same objects at 250x90, then 64x48 (everything reallocates and
    the first frame at the new size is all dirty), then 64x48 again."""
    rng = np.random.default_rng(17)
    p = Pair(W, H, scale=0.5)
    big = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    p.step(big, tag="250x90 a")
    p.step(big, tag="250x90 b")
    small = rng.integers(0, 256, (48, 64, 4), dtype=np.uint8)
    r = p.step(small, tag="64x48 a")
    assert (r["w"], r["h"]) == (32, 24)
    assert r["ages"].size == 2 * 2 and (r["ages"] == 30).all()
    small = small.copy()
    small[47, 63] ^= 0xFF
    r = p.step(small, tag="64x48 b")
    assert list(r["ages"]) == [29, 29, 29, 30]
