"""GPU (HIP/gfx950) JPEG pipeline vs the CPU reference + PIL decode.

Runs only on a box with an MI355X. Verifies:
  * the HIP pipeline actually engages (no silent CPU fallback)
  * GPU-encoded stripes decode with PIL and match the source (PSNR)
  * GPU output is coefficient-compatible with the CPU reference encoder
  * every coefficient of every emitted stripe, pad blocks included, is a
    rounding of a float64 DCT of the stripe's pixels (jpeg_ref.py), at odd
    sizes, four qualities, under a damage mask and across read-back growth
"""

import io
import math
import re
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from PIL import Image


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu-marked test ran on a host with no HIP device")


class Collector:
    def __init__(self):
        self.stripes = []
        self.lock = threading.Lock()

    def __call__(self, data, frame_id, y, width, height, is_keyframe,
                 capture_ts_ms, encode_done_ms, stripe_type):
        with self.lock:
            self.stripes.append(dict(data=data, frame_id=frame_id, y=y,
                                     width=width, height=height))


def psnr(a, b):
    mse = ((a.astype(np.int32) - b.astype(np.int32)) ** 2).mean()
    return 10 * math.log10(255 * 255 / max(mse, 1e-9))


def gpu_settings(**kw):
    s = hipflux.CaptureSettings()
    s.capture_width = 640
    s.capture_height = 352
    s.target_fps = 30
    s.output_mode = 0
    s.use_cpu = False
    s.gpu_id = 0
    s.capture_backend = "synthetic:desktop"
    s.stripe_height = 64
    s.damage_block_duration = 1
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_hip_pipeline_engages_and_decodes():
    require_gpu()
    col = Collector()
    cap = hipflux.ScreenCapture()
    cap.start_capture(col, gpu_settings())
    time.sleep(1.0)
    name = cap.pipeline
    cap.stop_capture()
    assert name == "hip-jpeg", f"HIP pipeline did not engage: {name}"
    assert col.stripes, "no stripes emitted"
    # frame 0 covers the full height; all stripes decode
    f0 = [s for s in col.stripes if s["frame_id"] == 0]
    assert sorted(s["y"] for s in f0) == [0, 64, 128, 192, 256, 320]
    for s in f0:
        img = Image.open(io.BytesIO(bytes(s["data"])[6:]))
        assert img.size == (640, s["height"])


@pytest.mark.parametrize("fullcolor", [False, True])
def test_gpu_matches_cpu_reference(fullcolor):
    """Same synthetic frame through GPU and CPU paths -> near-identical
    decoded images (float DCT rounding may differ by ±1 in few coeffs)."""
    require_gpu()

    results = {}
    for use_cpu in (False, True):
        col = Collector()
        cap = hipflux.ScreenCapture()
        s = gpu_settings(use_cpu=use_cpu, video_fullcolor=fullcolor,
                         capture_backend="synthetic:static")
        cap.start_capture(col, s)
        time.sleep(0.8)
        cap.stop_capture()
        f0 = sorted((st for st in col.stripes if st["frame_id"] == 0),
                    key=lambda st: st["y"])
        assert f0
        rows = [np.asarray(Image.open(io.BytesIO(bytes(st["data"])[6:]))
                           .convert("RGB")) for st in f0]
        results[use_cpu] = np.concatenate(rows, axis=0)

    gpu_img, cpu_img = results[False], results[True]
    assert gpu_img.shape == cpu_img.shape
    p = psnr(gpu_img, cpu_img)
    assert p > 40, f"GPU vs CPU decoded mismatch: {p:.1f} dB"


def test_gpu_1080p_throughput_sane():
    """1080p noise (100% damage): the GPU path must sustain well above the
    60 fps target on encode."""
    require_gpu()
    col = Collector()
    cap = hipflux.ScreenCapture()
    s = gpu_settings(capture_width=1920, capture_height=1080,
                     capture_backend="synthetic:noise", target_fps=240,
                     video_fullframe=True)
    cap.start_capture(col, s)
    time.sleep(2.0)
    frames = cap.frames_encoded
    enc_ms = cap.last_encode_ms
    cap.stop_capture()
    assert frames > 60, f"only {frames} frames encoded in 2 s"
    assert enc_ms < 16.0, f"per-frame encode {enc_ms:.1f} ms too slow"


def test_gpu_jpeg_entropy_matches_cpu_packer():
    """The GPU Huffman kernel must emit byte-identical JFIF streams to
    the CPU restart-row packer for the same quantized blocks, and the
    streams must decode in PIL."""
    require_gpu()
    import os
    from hipflux import _native
    w, h, n = 320, 192, 3
    rng = np.random.default_rng(29)
    frames = [np.ascontiguousarray(rng.integers(0, 256, (h, w, 4),
                                                dtype=np.uint8))
              for _ in range(n)]
    os.environ["HIPFLUX_CPU_JPEG_ENTROPY"] = "1"
    cpu_out = _native._pipeline_encode("gpu", frames, w, h, 80, 64, 0)
    del os.environ["HIPFLUX_CPU_JPEG_ENTROPY"]
    gpu_out = _native._pipeline_encode("gpu", frames, w, h, 80, 64, 0)
    for fi, (fa, fb) in enumerate(zip(cpu_out, gpu_out)):
        sa = sorted(fa, key=lambda t: t[1])
        sb = sorted(fb, key=lambda t: t[1])
        assert len(sa) == len(sb) == 3
        for (da, ya, _, _), (db, yb, _, _) in zip(sa, sb):
            assert ya == yb
            assert bytes(da) == bytes(db), \
                f"frame {fi} stripe {ya}: GPU JPEG entropy differs"
    # decodes in a real decoder
    img = Image.open(io.BytesIO(bytes(sorted(gpu_out[0],
                                             key=lambda t: t[1])[0][0])))
    assert img.size == (w, 64)
    arr = np.asarray(img.convert("L"))
    assert arr.std() > 10
    # 4:4:4 (fullcolor) path: same byte-equality contract
    os.environ["HIPFLUX_CPU_JPEG_ENTROPY"] = "1"
    c444 = _native._pipeline_encode("gpu", frames[:2], w, h, 80, 64, 0,
                                    False, True)
    del os.environ["HIPFLUX_CPU_JPEG_ENTROPY"]
    g444 = _native._pipeline_encode("gpu", frames[:2], w, h, 80, 64, 0,
                                    False, True)
    for fa, fb in zip(c444, g444):
        for (da, ya, _, _), (db, yb, _, _) in zip(
                sorted(fa, key=lambda t: t[1]),
                sorted(fb, key=lambda t: t[1])):
            assert bytes(da) == bytes(db), "fullcolor GPU entropy differs"
    img = Image.open(io.BytesIO(bytes(sorted(g444[0],
                                             key=lambda t: t[1])[0][0])))
    assert img.size == (w, 64)


# ---- every coefficient against a float64 DCT ----------------------------------
#
# The tests above compare the GPU with itself or by PSNR. These decode every
# emitted stripe with the from-spec decoder of jpeg_ref.py and hold 100 % of
# its coefficients, pad blocks included, to the float64 reference of the
# stripe's own pixels (established on the CPU encoder and on PIL in
# test_jpeg.py).

import jpeg_ref
from hipflux import _native

# (fullcolor, w, h, stripe_h): sizes at which the kernels take another path
COEFF_CASES = [
    (False, 16, 16, 16),     # one MCU: 6 items in a 256-thread scan
    (False, 17, 17, 16),     # both pads 1 pixel wide, second stripe 1 row high
    (False, 328, 72, 32),    # w%16 = h%16 = 8: luma pad blocks past ceil(w/8)
    (False, 322, 150, 64),   # the size the HEVC test uses
    (False, 333, 47, 32),    # pad > 8; chroma clamp on an odd width
    (False, 712, 24, 16),    # 45 MCUs x 6 = 270 items > 256 threads
    (True, 9, 9, 16),        # 3-item rows at the top, 6 items at most
    (True, 324, 36, 16),     # odd block counts; stripes cover two MCU rows
    (True, 700, 24, 16),     # 88 x 3 = 264 items > 256 threads
]
# all of them at quality 80; the two with every pad also at the extremes
COEFF_RUNS = [c + (80,) for c in COEFF_CASES] + [
    c + (q,) for c in (COEFF_CASES[2], COEFF_CASES[7]) for q in (1, 35, 100)]


def check_stripes(emitted, frame, w, h, stripe_h, quality, fullcolor,
                  expect_y=None):
    """Hold every stripe emitted for one frame to the reference; returns
    (coefficients checked, worst |c-r|-0.5, allowance there, coefficients
    that differ from the CPU encoder's)."""
    mcu = 8 if fullcolor else 16
    if expect_y is None:
        expect_y = list(range(0, h, stripe_h))
    assert sorted(y for _, y, _, _ in emitted) == expect_y
    checked = cpu_diff = 0
    worst = (-1.0, 0.0)
    for data, y0, sh, _ in emitted:
        assert sh == min(stripe_h, h - y0)
        d = jpeg_ref.decode_coeffs(bytes(data))
        assert (d["width"], d["height"], d["fullcolor"]) == (w, sh, fullcolor)
        assert d["dri"] == -(-w // mcu)
        px = frame[y0:y0 + sh]
        cpu = jpeg_ref.decode_coeffs(_native._jpeg_encode_restart(
            px.tobytes(), w, sh, quality, fullcolor))
        assert np.array_equal(cpu["qy"], d["qy"])
        assert np.array_equal(cpu["qc"], d["qc"])
        n = int((cpu["blocks"] != d["blocks"]).sum())
        cpu_diff += n
        ref = jpeg_ref.reference_coeff_real(px, w, sh, d["qy"], d["qc"],
                                            fullcolor)
        try:
            st = jpeg_ref.check_coeffs(d, ref, stripe=y0)
        except AssertionError as e:
            raise AssertionError(
                f"{e} [{n} coefficients of this stripe differ from the CPU "
                f"encoder's]") from None
        checked += st["checked"]
        worst = max(worst, (st["worst_excess"], st["worst_allow"]))
    return checked, worst[0], worst[1], cpu_diff


def report(tag, results):
    checked = sum(r[0] for r in results)
    excess, allow = max((r[1], r[2]) for r in results)
    print(f"\n{tag}: {checked} coefficients, worst |c-r|-0.5 = {excess:.3e} "
          f"(allowance there {allow:.3e}), {sum(r[3] for r in results)} "
          f"differ from the CPU encoder")


@pytest.mark.parametrize(
    "fullcolor,w,h,stripe_h,quality", COEFF_RUNS,
    ids=[f"{'444' if f else '420'}-{w}x{h}-q{q}"
         for f, w, h, _, q in COEFF_RUNS])
def test_gpu_coefficients_round_the_float64_reference(fullcolor, w, h,
                                                      stripe_h, quality):
    """Noise and structures through the HIP pipeline: every stripe decodes
    strictly, carries the right size and restart interval, and every one
    of its coefficients is a rounding of the float64 reference."""
    require_gpu()
    frames = [jpeg_ref.content_noise(w, h, 4000 + w),
              jpeg_ref.content_structures(w, h)]
    out = _native._pipeline_encode("gpu", frames, w, h, quality, stripe_h, 0,
                                   False, fullcolor)
    assert len(out) == len(frames)
    results = [check_stripes(out[i], frames[i], w, h, stripe_h, quality,
                             fullcolor) for i in range(len(frames))]
    report(f"{'444' if fullcolor else '420'} {w}x{h} q{quality}", results)


def test_gpu_damage_mask_emits_exactly_the_masked_stripes():
    """encode_mask with JPEG: only the masked-in stripes come out, each is
    right by itself and byte-equal to the same stripe of an unmasked run."""
    require_gpu()
    w, h, stripe_h, quality = 328, 136, 32, 80
    T, F = True, False
    masks = [[T, T, T, T, T], [F, T, F, T, T], [F, F, F, F, T]]
    frames = [jpeg_ref.content_noise(w, h, 4500 + i) for i in range(3)]
    full = _native._pipeline_encode("gpu", frames, w, h, quality, stripe_h,
                                    0, False, False)
    part = _native._pipeline_encode("gpu", frames, w, h, quality, stripe_h,
                                    0, False, False, encode_mask=masks)
    results = []
    for fi, mask in enumerate(masks):
        want_y = [i * stripe_h for i, m in enumerate(mask) if m]
        results.append(check_stripes(part[fi], frames[fi], w, h, stripe_h,
                                     quality, False, expect_y=want_y))
        whole = {y: bytes(d) for d, y, _, _ in full[fi]}
        assert sorted(whole) == list(range(0, h, stripe_h))
        for d, y, _, _ in part[fi]:
            assert bytes(d) == whole[y], \
                f"frame {fi} stripe {y}: differs from the unmasked run"
    report("masked 420 328x136 q80", results)


def test_gpu_readback_growth_refetches_whole_rows():
    """Flat, flat, noise, flat, noise at quality 95 with one frame in
    flight: a noise frame's rows outgrow the compacted read-back sized by
    the flat frame before it (2 * max + 64 words), so the rows are
    fetched again in full. Every frame is right by itself and byte-equal
    to the synchronous run."""
    require_gpu()
    w, h, stripe_h, quality = 328, 72, 32, 95
    flat = np.full((h, w, 4), 255, np.uint8)
    flat[:, :, :3] = 91
    frames = [flat, flat.copy(), jpeg_ref.content_noise(w, h, 4600),
              flat.copy(), jpeg_ref.content_noise(w, h, 4601)]
    runs = [_native._pipeline_encode("gpu", frames, w, h, quality, stripe_h,
                                     0, False, False, pipeline_depth=depth)
            for depth in (2, 1)]
    # the premise, in 32-bit words per MCU row (stuffing aside): every
    # noise row is longer than the cap a flat frame leaves behind
    def row_words(frame_out):
        rows = []
        for d, _, _, _ in frame_out:
            d = bytes(d)
            scan = d[d.index(b"\xff\xda") + 14:-2]
            rows += [(len(r) + 3) // 4 + 1
                     for r in re.split(rb"\xff[\xd0-\xd7]", scan)]
        assert len(rows) == 5
        return rows
    words = [row_words(fr) for fr in runs[0]]
    for noise, before in ((2, 0), (2, 1), (4, 3)):
        assert min(words[noise]) > 2 * max(words[before]) + 64
    results = [check_stripes(runs[0][i], frames[i], w, h, stripe_h, quality,
                             False) for i in range(len(frames))]
    for i in range(len(frames)):
        assert sorted((y, bytes(d)) for d, y, _, _ in runs[0][i]) == \
            sorted((y, bytes(d)) for d, y, _, _ in runs[1][i]), \
            f"frame {i}: depth 2 differs from depth 1"
    report("growth 420 328x72 q95", results)
