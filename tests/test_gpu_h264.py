"""HIP H.264 pipeline (gfx950) correctness on a real MI355X.

Strongest check: the GPU pipeline uses the same integer transform/quant
semantics and the same deterministic mode-decision rules as the CPU
reference pipeline, so on identical input frames both must produce streams
that DECODE IDENTICALLY under the from-spec Python decoder (stream bytes
may differ only if float CSC rounding diverges — also checked)."""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
from h264_ref_decoder import Decoder


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


def psnr(a, b):
    mse = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).mean()
    return 10 * math.log10(255 * 255 / max(mse, 1e-12))


def make_frames(w, h, n):
    """Gradient background + moving box + a noise band (mixed content)."""
    rng = np.random.default_rng(42)
    base = np.zeros((h, w, 4), np.uint8)
    base[:, :, 0] = np.linspace(0, 255, w, dtype=np.uint8)[None, :]
    base[:, :, 1] = np.linspace(0, 255, h, dtype=np.uint8)[:, None]
    base[:, :, 2] = 80
    base[:, :, 3] = 255
    base[h // 2:h // 2 + 16, :] = rng.integers(0, 256, (16, w, 4),
                                               dtype=np.uint8)
    frames = []
    for i in range(n):
        f = base.copy()
        x = (16 + i * 24) % max(1, w - 48)
        f[16:48, x:x + 48, 0] = 255
        f[16:48, x:x + 48, 2] = 0
        frames.append(np.ascontiguousarray(f))
    return frames


def reassemble(stripe_lists):
    """frames -> dict y -> concatenated stream bytes"""
    rows = {}
    for frame in stripe_lists:
        for data, y, hgt, key in frame:
            rows.setdefault(y, b"")
            rows[y] += bytes(data)
    return rows


def decode_rows(rows, w, stripe_h):
    out = {}
    for y, stream in rows.items():
        frames = Decoder().decode(stream)
        assert frames, f"stripe y={y}: no frames decoded"
        out[y] = frames
    return out


def test_gpu_stream_decodes_and_matches_cpu():
    require_gpu()
    w, h, n = 320, 192, 6
    frames = make_frames(w, h, n)
    gpu = _native._pipeline_encode("gpu", frames, w, h, 26, 64, 1)
    cpu = _native._pipeline_encode("cpu", frames, w, h, 26, 64, 1)
    rows_g, rows_c = reassemble(gpu), reassemble(cpu)
    assert set(rows_g) == set(rows_c) == {0, 64, 128}

    dec_g = decode_rows(rows_g, w, 64)
    dec_c = decode_rows(rows_c, w, 64)
    for y in dec_g:
        assert len(dec_g[y]) == len(dec_c[y]) == n
        for fi in range(n):
            gy = dec_g[y][fi][0]
            cy = dec_c[y][fi][0]
            p = psnr(gy, cy)
            assert p > 45, f"stripe {y} frame {fi}: GPU vs CPU decode {p:.1f} dB"

    # source fidelity on the final frame (smooth region should be high)
    src_y, _, _ = hipflux.bgrx_to_yuv420(frames[-1].tobytes(), w, h)
    sy = np.frombuffer(src_y, np.uint8).reshape(h, w)
    full_g = np.concatenate([dec_g[y][n - 1][0] for y in sorted(dec_g)], 0)
    assert psnr(full_g[:64], sy[:64]) > 32


def test_gpu_idr_bitstream_matches_cpu_exactly():
    """IDR mode decisions and integer paths are deterministic and identical
    on both pipelines; if float CSC agrees, the streams are byte-equal."""
    require_gpu()
    w, h = 256, 128
    frames = make_frames(w, h, 1)
    gpu = _native._pipeline_encode("gpu", frames, w, h, 28, 64, 1)
    cpu = _native._pipeline_encode("cpu", frames, w, h, 28, 64, 1)
    for (gd, gy, _, _), (cd, cy, _, _) in zip(
            sorted(gpu[0], key=lambda t: t[1]),
            sorted(cpu[0], key=lambda t: t[1])):
        assert gy == cy
        if bytes(gd) != bytes(cd):
            # allow CSC float rounding divergence but require near-identity
            dg = Decoder().decode(bytes(gd))[0][0]
            dc = Decoder().decode(bytes(cd))[0][0]
            p = psnr(dg, dc)
            assert p > 50, f"stripe {gy}: IDR streams differ badly ({p:.1f})"


def test_gpu_p_chain_no_drift():
    """Long P chain on slowly-changing content: decoded output must track
    the encoder (parse success + stable PSNR, no accumulating drift)."""
    require_gpu()
    w, h, n = 256, 128, 30
    frames = make_frames(w, h, n)
    gpu = _native._pipeline_encode("gpu", frames, w, h, 24, 64, 1)
    rows = reassemble(gpu)
    for y, stream in rows.items():
        decoded = Decoder().decode(stream)
        assert len(decoded) == n
    # PSNR of first vs last decoded frame against their sources ~ similar
    dec = decode_rows(rows, w, 64)
    ys = sorted(dec)
    for fi in (1, n - 1):
        full = np.concatenate([dec[y][fi][0] for y in ys], 0)
        src_y, _, _ = hipflux.bgrx_to_yuv420(frames[fi].tobytes(), w, h)
        sy = np.frombuffer(src_y, np.uint8).reshape(h, w)
        # exclude the noise band (poorly coded at qp24 by design)
        m = np.ones(h, bool)
        m[h // 2:h // 2 + 16] = False
        p = psnr(full[m], sy[m])
        assert p > 30, f"frame {fi}: PSNR {p:.1f} too low (drift?)"


def test_gpu_mfma_motion_search_exact():
    """Frame 1 = frame 0 rolled by (dx=4, dy=-2). The MFMA full-search ME
    must find mv=(-4,+2) for interior MBs — verified by parsing the coded
    MVs straight out of the bitstream. (Since inter MBs code residuals,
    the decoded P frame is no longer byte-equal to the rolled IDR; the MV
    check is the direct probe of the MFMA scoring/layout.)"""
    require_gpu()
    from scipy.ndimage import uniform_filter
    w, h = 256, 128
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (h, w), dtype=np.uint8).astype(np.float32)
    smooth = uniform_filter(base, 3).astype(np.uint8)
    f0 = np.zeros((h, w, 4), np.uint8)
    for c in range(3):
        f0[:, :, c] = smooth
    f0[:, :, 3] = 255
    dx, dy = 4, -2
    f1 = np.roll(np.roll(f0, dy, axis=0), dx, axis=1)
    out = _native._pipeline_encode(
        "gpu", [np.ascontiguousarray(f0), np.ascontiguousarray(f1)],
        w, h, 30, 64, 1)
    rows = reassemble(out)

    class MvDecoder(Decoder):
        def __init__(self):
            super().__init__()
            self.mvs = {}

        def decode_p16(self, br, mbx, mby, ctx, qp):
            info = super().decode_p16(br, mbx, mby, ctx, qp)
            self.mvs[(mbx, mby)] = tuple(ctx["left_mv"])
            return info

        def decode_skip(self, mbx, mby):
            super().decode_skip(mbx, mby)
            self.mvs[(mbx, mby)] = (0, 0)

    want = (dx * -4, dy * -4)  # quarter-pel units: (-16, +8)
    match = total = 0
    psnrs = []
    for y0, stream in rows.items():
        d = MvDecoder()
        frames = d.decode(bytes(stream))
        assert len(frames) == 2
        # interior MBs of this stripe: skip first column (mv x leaves the
        # frame) and the last MB row (mv y leaves the stripe)
        stripe_mbh = frames[0][0].shape[0] // 16
        for (mbx, mby), mv in d.mvs.items():
            if mbx == 0 or mby == stripe_mbh - 1:
                continue
            total += 1
            match += int(mv == want)
        # decoded P must track the rolled source closely (MC + residual)
        sy = np.roll(np.roll(smooth, dy, axis=0), dx, axis=1)
        psnrs.append(psnr(frames[1][0],
                          sy[y0:y0 + frames[1][0].shape[0]]))
    assert total > 0
    frac = match / total
    assert frac > 0.9, f"only {match}/{total} interior MBs found {want}"
    assert min(psnrs) > 30, f"P-frame quality too low: {psnrs}"
    # and the P frame must be far smaller than the IDR
    sizes = [sum(len(t[0]) for t in fr) for fr in out]
    assert sizes[1] < sizes[0] * 0.6, f"P frame too large: {sizes}"


def test_gpu_cavlc_matches_cpu_entropy():
    """The GPU CAVLC kernel must emit byte-identical streams to the CPU
    packer for the same levels/meta (IDR + P frames, mixed modes)."""
    require_gpu()
    import os
    w, h, n = 320, 192, 5
    frames = make_frames(w, h, n)
    os.environ["HIPFLUX_CPU_ENTROPY"] = "1"
    cpu_out = _native._pipeline_encode("gpu", frames, w, h, 26, 64, 1)
    del os.environ["HIPFLUX_CPU_ENTROPY"]
    gpu_out = _native._pipeline_encode("gpu", frames, w, h, 26, 64, 1)
    for fi, (fa, fb) in enumerate(zip(cpu_out, gpu_out)):
        sa = sorted(fa, key=lambda t: t[1])
        sb = sorted(fb, key=lambda t: t[1])
        assert len(sa) == len(sb)
        for (da, ya, _, _), (db, yb, _, _) in zip(sa, sb):
            assert ya == yb
            assert bytes(da) == bytes(db), \
                f"frame {fi} stripe {ya}: GPU CAVLC differs from CPU"


def test_gpu_h264_1080p_throughput():
    require_gpu()
    import time
    w, h = 1920, 1080
    rng = np.random.default_rng(0)
    frames = [np.ascontiguousarray(rng.integers(0, 256, (h, w, 4),
                                                dtype=np.uint8))
              for _ in range(20)]
    _native._pipeline_encode("gpu", frames[:2], w, h, 30, 64, 1)  # warmup
    t0 = time.monotonic()
    _native._pipeline_encode("gpu", frames, w, h, 30, 64, 1)
    dt = (time.monotonic() - t0) / len(frames)
    print(f"1080p noise encode: {dt*1000:.2f} ms/frame")
    assert dt < 0.05, f"1080p encode too slow: {dt*1000:.1f} ms"


def test_gpu_halfpel_and_odd_mvs():
    """GPU pipeline codes odd-integer and half-pel MVs and the streams
    stay decodable bit-exactly (the decoder asserts the half-pel grid and
    interpolates per 8.4.2.2.1 — any GPU/decoder interp mismatch breaks
    the P-chain PSNR)."""
    require_gpu()
    w, h = 192, 96
    rng = np.random.default_rng(31)
    base = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    f = base.astype(np.float32)
    for _ in range(2):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) +
             np.roll(f, 1, 0) + np.roll(f, -1, 0)) / 5
    f0 = f.astype(np.uint8)
    f0[:, :, 3] = 255
    f1 = np.roll(f0, 1, axis=1)
    fh = ((f0.astype(np.uint16) + np.roll(f0, 1, 1)) // 2).astype(np.uint8)
    fh[:, :, 3] = 255
    frames = [np.ascontiguousarray(x) for x in (f0, f1, fh)]
    out = _native._pipeline_encode("gpu", frames, w, h, 22, 96, 1)
    rows = reassemble(out)

    class MvDecoder(Decoder):
        def __init__(self):
            super().__init__()
            self.mvs = []

        def decode_p16(self, br, mbx, mby, ctx, qp):
            info = super().decode_p16(br, mbx, mby, ctx, qp)
            self.mvs.append(tuple(ctx["left_mv"]))
            return info

    all_mvs = []
    for y0, stream in rows.items():
        d = MvDecoder()
        decoded = d.decode(bytes(stream))
        assert len(decoded) == 3
        all_mvs += d.mvs
        # quality must track the source for the half-shifted frame
        sy, _, _ = hipflux.bgrx_to_yuv420(fh.tobytes(), w, h)
        syn = np.frombuffer(sy, np.uint8).reshape(h, w)
        p = psnr(decoded[2][0], syn[y0:y0 + decoded[2][0].shape[0]])
        assert p > 34, f"half-shift frame quality {p:.1f}"
    odd = [mv for mv in all_mvs if (mv[0] // 4) % 2 == 1 and mv[0] % 4 == 0]
    half = [mv for mv in all_mvs if mv[0] % 4 == 2 or mv[1] % 4 == 2]
    assert odd, "no odd-integer MVs coded by the GPU pipeline"
    assert half, "no half-pel MVs coded by the GPU pipeline"


def test_gpu_quarterpel_mvs():
    """Quarter-shifted content (3:1 column blend) produces quarter-pel
    MVs from the GPU pipeline and the stream decodes bit-exactly."""
    require_gpu()
    w, h = 192, 96
    rng = np.random.default_rng(41)
    base = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    f = base.astype(np.float32)
    for _ in range(2):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) +
             np.roll(f, 1, 0) + np.roll(f, -1, 0)) / 5
    f0 = f.astype(np.uint8)
    f0[:, :, 3] = 255
    fq = ((3 * f0.astype(np.uint16) + np.roll(f0, 1, 1)) // 4).astype(
        np.uint8)
    fq[:, :, 3] = 255
    out = _native._pipeline_encode(
        "gpu", [np.ascontiguousarray(f0), np.ascontiguousarray(fq)],
        w, h, 22, 96, 1)
    rows = reassemble(out)

    class MvDecoder(Decoder):
        def __init__(self):
            super().__init__()
            self.mvs = []

        def decode_p16(self, br, mbx, mby, ctx, qp):
            info = super().decode_p16(br, mbx, mby, ctx, qp)
            self.mvs.append(tuple(ctx["left_mv"]))
            return info

    all_mvs = []
    for y0, stream in rows.items():
        d = MvDecoder()
        decoded = d.decode(bytes(stream))
        assert len(decoded) == 2
        all_mvs += d.mvs
    quarter = [mv for mv in all_mvs if (mv[0] & 3) in (1, 3)
               or (mv[1] & 3) in (1, 3)]
    assert quarter, "no quarter-pel MVs coded by the GPU pipeline"


def test_gpu_wide_frame_segmented_slices():
    """Rows wider than 128 MBs split into multiple slices per row
    (segments): the stream must parse (mid-row first_mb), decode to high
    PSNR on smooth content, and the GPU CAVLC must stay byte-identical
    to the CPU packer over the segmented job list."""
    require_gpu()
    import os
    w, h, n = 2176, 32, 3   # 136 MBs wide -> 2 segments per row
    rng = np.random.default_rng(51)
    base = rng.integers(0, 256, (h, w, 4), dtype=np.uint8).astype(
        np.float32)
    for _ in range(2):
        base = (base + np.roll(base, 1, 1) + np.roll(base, -1, 1) +
                np.roll(base, 1, 0) + np.roll(base, -1, 0)) / 5
    frames = []
    for i in range(n):
        f = np.roll(base.astype(np.uint8), 4 * i, axis=1)
        f[:, :, 3] = 255
        frames.append(np.ascontiguousarray(f))

    os.environ["HIPFLUX_CPU_ENTROPY"] = "1"
    cpu_ent = _native._pipeline_encode("gpu", frames, w, h, 26, 32, 1)
    del os.environ["HIPFLUX_CPU_ENTROPY"]
    gpu_ent = _native._pipeline_encode("gpu", frames, w, h, 26, 32, 1)
    for fi, (fa, fb) in enumerate(zip(cpu_ent, gpu_ent)):
        for (da, ya, _, _), (db, yb, _, _) in zip(
                sorted(fa, key=lambda t: t[1]),
                sorted(fb, key=lambda t: t[1])):
            assert bytes(da) == bytes(db), \
                f"frame {fi} stripe {ya}: segmented GPU CAVLC differs"

    stream = bytearray()
    for fr in gpu_ent:
        for data, y, _, _ in fr:
            stream.extend(bytes(data))
    decoded = Decoder().decode(bytes(stream))
    assert len(decoded) == n
    src_y, _, _ = hipflux.bgrx_to_yuv420(frames[0].tobytes(), w, h)
    sy = np.frombuffer(src_y, np.uint8).reshape(h, w)
    p = psnr(decoded[0][0], sy)
    assert p > 34, f"segmented wide-frame IDR PSNR {p:.1f}"


def test_gpu_fast_scroll_motion_lock():
    """20 px/frame scroll through the GPU pipeline: quarter-res pyramid
    acquisition (±48 range) + the meta hint channel must lock most MBs
    onto mv x = -80 quarter-pel within a couple of P frames."""
    require_gpu()
    w, h, n = 320, 96, 5
    rng = np.random.default_rng(61)
    base = rng.integers(0, 256, (h, w, 4), dtype=np.uint8).astype(
        np.float32)
    for _ in range(2):
        base = (base + np.roll(base, 1, 1) + np.roll(base, -1, 1) +
                np.roll(base, 1, 0) + np.roll(base, -1, 0)) / 5
    f0 = base.astype(np.uint8)
    f0[:, :, 3] = 255
    frames = [np.ascontiguousarray(np.roll(f0, 20 * i, axis=1))
              for i in range(n)]
    out = _native._pipeline_encode("gpu", frames, w, h, 24, 96, 1)
    rows = reassemble(out)

    class MvDecoder(Decoder):
        def __init__(self):
            super().__init__()
            self.mvs = []

        def decode_p16(self, br, mbx, mby, ctx, qp):
            info = super().decode_p16(br, mbx, mby, ctx, qp)
            self.mvs.append(tuple(ctx["left_mv"]))
            return info

    late_mvs = []
    for y0, stream in rows.items():
        d = MvDecoder()
        decoded = d.decode(bytes(stream))
        assert len(decoded) == n
        # frames 3..n: acquisition done, tracking should hold
        per_frame = len(d.mvs) // (n - 1) if d.mvs else 0
        late_mvs += d.mvs[2 * per_frame:]
    locked = [mv for mv in late_mvs if mv[0] == -80]
    assert late_mvs and len(locked) > len(late_mvs) * 0.4, \
        f"GPU scroll not locked: {len(locked)}/{len(late_mvs)}"


def test_gpu_engine_soak_short():
    """Full engine path on GPU (capture thread -> damage -> HIP pipeline
    -> wire) for ~3 seconds of 1080p60 desktop-pattern content: stripes
    keep flowing, no stalls, recording tap works, IDR request honored."""
    require_gpu()
    import tempfile
    import threading
    import time

    with tempfile.TemporaryDirectory() as td:
        s = _native.CaptureSettings()
        s.capture_width = 1920
        s.capture_height = 1080
        s.target_fps = 60
        s.output_mode = 1
        s.use_cpu = False
        s.gpu_id = 0
        s.capture_backend = "synthetic:desktop"
        s.stripe_height = 64
        s.recording_path = td + "/rec"
        got = {"n": 0, "key": 0, "bytes": 0}
        done = threading.Event()

        def cb(data, frame_id, y, width, height, key, *a):
            got["n"] += 1
            got["bytes"] += len(data)
            if key:
                got["key"] += 1
            if got["n"] > 2000:
                done.set()

        cap = _native.ScreenCapture()
        cap.start_capture(cb, s)
        time.sleep(1.0)
        cap.request_idr_frame()
        done.wait(8)
        n_mid = got["n"]
        assert cap.is_capturing
        assert cap.pipeline.startswith("hip"), cap.pipeline
        time.sleep(1.0)
        cap.stop_capture()
        assert got["n"] > n_mid, "stream stalled"
        assert got["key"] >= 2           # initial IDR + requested IDR
        assert got["n"] >= 1000
        import glob
        recs = glob.glob(td + "/rec.s*.h264")
        assert recs and sum(len(open(f, "rb").read()) for f in recs) > 10000


def test_pipelined_depth2_byte_identical():
    """Depth-2 frame pipelining (submit N, emit N-1: host assembly
    overlaps the next frame's GPU work) must produce byte-identical
    per-frame streams to the synchronous path — including an IDR
    mid-sequence and a no-damage frame in the middle of the pipe."""
    require_gpu()
    w, h, n = 320, 192, 10
    frames = make_frames(w, h, n)
    sync = _native._pipeline_encode("gpu", frames, w, h, 26, 64, 1)
    piped = _native._pipeline_encode("gpu", frames, w, h, 26, 64, 1,
                                     pipeline_depth=2)
    assert len(sync) == len(piped) == n
    for fi in range(n):
        s = sorted((y, bytes(d)) for d, y, hh, k in sync[fi])
        q = sorted((y, bytes(d)) for d, y, hh, k in piped[fi])
        assert s == q, f"frame {fi}: pipelined stream differs"
    # decoder sanity on the pipelined stream
    rows = reassemble(piped)
    for y, stream in rows.items():
        assert len(Decoder().decode(stream)) == n


def test_pipelined_bench_pipeline_contract():
    """BenchPipeline with pipeline_depth=2: emissions lag by exactly one
    frame (last_frame_id), flush drains the pipe, per-frame byte counts
    match the synchronous run."""
    require_gpu()
    w, h, n = 320, 192, 8
    frames = make_frames(w, h, n)
    p1 = _native.BenchPipeline("gpu", w, h, qp=26, stripe_height=64,
                               output_mode=1, gpu_id=0)
    sizes1 = []
    for i, f in enumerate(frames):
        b, _ = p1.encode(f, i == 0)
        assert p1.last_frame_id == i
        sizes1.append(b)
    p2 = _native.BenchPipeline("gpu", w, h, qp=26, stripe_height=64,
                               output_mode=1, gpu_id=0, pipeline_depth=2)
    sizes2 = []
    for i, f in enumerate(frames):
        b, _ = p2.encode(f, i == 0)
        if i == 0:
            assert p2.last_frame_id == -1 and b == 0
        else:
            assert p2.last_frame_id == i - 1
            sizes2.append(b)
    b, _ = p2.flush()
    assert p2.last_frame_id == n - 1
    sizes2.append(b)
    assert sizes1 == sizes2


def test_gpu_engine_pipelined_depth2():
    """Engine path with pipeline_depth=2 (throughput mode): stripes keep
    flowing with per-stripe capture timestamps stamped by the pipeline
    (emission lags one frame), and the stream still decodes."""
    require_gpu()
    import threading
    import time

    s = _native.CaptureSettings()
    s.capture_width = 640
    s.capture_height = 384
    s.target_fps = 120
    s.output_mode = 1
    s.use_cpu = False
    s.gpu_id = 0
    s.capture_backend = "synthetic:desktop"
    s.stripe_height = 64
    s.pipeline_depth = 2
    s.video_fullframe = True          # exercise the steady pipelined path
    got = {"n": 0, "key": 0}
    done = threading.Event()

    def cb(data, frame_id, y, width, height, key, *a):
        got["n"] += 1
        if key:
            got["key"] += 1
        if got["n"] > 600:
            done.set()

    cap = _native.ScreenCapture()
    cap.start_capture(cb, s)
    done.wait(10)
    assert cap.is_capturing
    assert cap.pipeline.startswith("hip")
    cap.stop_capture()
    assert got["n"] > 600 and got["key"] >= 1


def test_gpu_pipelined_static_content_flushes():
    """Depth-2 + damage gating on STATIC content: after the initial
    frames the screen stops changing, so encode skips — the engine's
    idle-frame flush must still drain the last in-flight frame (bounded
    emission lag, no stuck stripes)."""
    require_gpu()
    import threading
    import time

    s = _native.CaptureSettings()
    s.capture_width = 640
    s.capture_height = 384
    s.target_fps = 120
    s.output_mode = 1
    s.use_cpu = False
    s.gpu_id = 0
    s.capture_backend = "synthetic:static"
    s.stripe_height = 64
    s.pipeline_depth = 2
    s.use_paint_over_quality = False   # no paint-over refresh traffic
    got = {"n": 0}
    cap = _native.ScreenCapture()
    cap.start_capture(lambda *a: got.__setitem__("n", got["n"] + 1), s)
    time.sleep(2.0)
    n_settled = got["n"]
    # static content: stream settles; every captured stripe must have
    # been emitted (nothing stuck in the pipe). The first frame is
    # 6 stripes; damage-gated follow-ups add a bounded few.
    assert n_settled >= 6
    time.sleep(1.0)
    assert got["n"] == n_settled, "static screen kept emitting"
    cap.request_idr_frame()
    time.sleep(1.0)
    assert got["n"] > n_settled, "IDR refresh did not flow"
    cap.stop_capture()


def test_gpu_pipelined_resolution_change():
    """Depth-2 with a mid-stream resolution change: the in-flight frame
    referencing the old buffers is dropped, streams restart with an IDR
    and keep flowing (no crash, no stale emission)."""
    require_gpu()
    w, h = 320, 192
    frames_a = make_frames(w, h, 4)
    frames_b = make_frames(512, 256, 4)
    p = _native.BenchPipeline("gpu", w, h, qp=26, stripe_height=64,
                              output_mode=1, gpu_id=0, pipeline_depth=2)
    for i, f in enumerate(frames_a):
        p.encode(f, i == 0)
    # frames_a's last frame is still in flight here; the resize drops it
    p.resize(512, 256)
    sizes = []
    for i, f in enumerate(frames_b):
        b, _ = p.encode(f, i == 0)
        sizes.append(b)
    b, _ = p.flush()
    sizes.append(b)
    # the dropped in-flight frame emits nothing; every new-size frame does
    assert sum(1 for b in sizes if b > 0) == len(frames_b)
    # and the new-size stream decodes end to end
    out = _native._pipeline_encode("gpu", frames_b, 512, 256, 26, 64, 1,
                                   pipeline_depth=2)
    rows = reassemble(out)
    for y, stream in rows.items():
        assert len(Decoder().decode(stream)) == len(frames_b)


def test_gpu_deblock_recon_matches_decoder():
    """The GPU deblock kernel's reconstruction must equal the from-spec
    decoder's (which filters per §8.7 from the idc=2 slice headers) —
    the strongest deblock check: any bS/table/order divergence breaks
    byte equality, and the P-frame chain amplifies drift."""
    require_gpu()
    w, h, n = 320, 192, 5
    frames = make_frames(w, h, n)
    out, dump = _native._pipeline_encode("gpu", frames, w, h, 30, 64, 1,
                                         True)
    stream = b""
    for fr in out:
        for data, y, hgt, key in fr:
            stream += bytes(data)
    # reassemble rows separately (independent bitstreams)
    rows = reassemble(out)
    ypitch = dump["ypitch"]
    cpitch = dump["cpitch"]
    ry = np.frombuffer(dump["y"], np.uint8).reshape(-1, ypitch)
    rcb = np.frombuffer(dump["cb"], np.uint8).reshape(-1, cpitch)
    rcr = np.frombuffer(dump["cr"], np.uint8).reshape(-1, cpitch)
    for y0, s in rows.items():
        decoded = Decoder().decode(s)
        assert len(decoded) == n
        dy = decoded[-1][0]
        gy = ry[y0:y0 + dy.shape[0], :w]
        assert np.array_equal(dy, gy), (
            f"stripe y={y0}: decoder recon != GPU deblocked recon")
        for name, dc, rc in (("cb", decoded[-1][1], rcb),
                             ("cr", decoded[-1][2], rcr)):
            assert dc.shape == (dy.shape[0] // 2, w // 2)
            gc = rc[y0 // 2:y0 // 2 + dc.shape[0], :w // 2]
            assert np.array_equal(dc, gc), (
                f"stripe y={y0}: decoder {name} != GPU deblocked {name}")


def test_gpu_fractional_scale_stream():
    """capture_scale on the HIP pipeline: the engine's fixed-point
    bilinear feeds the GPU encoder; the 0.5x stream decodes identically
    to a direct encode of the scaled frame (same QP, same kernels)."""
    require_gpu()
    import threading
    import time

    w, h = 256, 128
    shot, _, _ = _native.screenshot("synthetic:static", "", w, h)
    small, ow, oh = _native._bilinear_downscale(shot, w, h, 0.5)
    assert (ow, oh) == (128, 64)

    s = _native.CaptureSettings()
    s.capture_width = w
    s.capture_height = h
    s.capture_scale = 0.5
    s.target_fps = 30
    s.output_mode = 1
    s.use_cpu = False
    s.gpu_id = 0
    s.capture_backend = "synthetic:static"
    s.video_fullframe = True
    s.video_crf = 12
    s.video_cbr_mode = False
    s.stripe_height = 64
    got = []
    done = threading.Event()

    def cb(data, frame_id, y, width, height, key, *a):
        got.append((bytes(data), width, height))
        if len(got) >= 3:
            done.set()

    cap = _native.ScreenCapture()
    cap.start_capture(cb, s)
    assert done.wait(10)
    pipeline = cap.pipeline
    cap.stop_capture()
    assert pipeline.startswith("hip"), pipeline
    data, width, height = got[0]
    assert (width, height) == (128, 64)
    y_dec = Decoder().decode(data[10:])[0][0]
    # the GPU pipeline must encode the engine's scaled frame exactly as
    # a direct CPU encode of the same scaled pixels decodes (shared
    # mode-decision + transform semantics; crf 12 -> qp 12)
    import numpy as np
    exp = np.frombuffer(small, np.uint8).reshape(oh, ow, 4)
    enc = hipflux.H264Encoder(128, 64)
    r = enc.encode(np.ascontiguousarray(exp).tobytes(), qp=12, idr=True)
    y_direct = Decoder().decode(r["data"])[0][0]
    assert np.array_equal(y_dec, y_direct), \
        "GPU fractional-scale path diverges from the scaled direct encode"


def test_gpu_two_captures_concurrent():
    """Two engine captures (primary + display2 pattern) encode
    concurrently on one GPU — the multi-display production shape."""
    require_gpu()
    import threading
    import time

    caps, counts, events = [], [], []
    try:
        for i in range(2):
            s = _native.CaptureSettings()
            s.capture_width = 1280
            s.capture_height = 720
            s.target_fps = 60
            s.output_mode = 1 if i == 0 else 2   # h264 + hevc mixed
            s.use_cpu = False
            s.gpu_id = 0
            s.capture_backend = "synthetic:desktop"
            s.video_fullframe = True
            s.stripe_height = 64
            n = {"v": 0}
            ev = threading.Event()

            def cb(data, fid, y, w, h, key, *a, _n=n, _ev=ev):
                _n["v"] += 1
                if _n["v"] >= 200:
                    _ev.set()
            cap = _native.ScreenCapture()
            cap.start_capture(cb, s)
            caps.append(cap)
            counts.append(n)
            events.append(ev)
        for ev in events:
            assert ev.wait(15)
        for cap in caps:
            assert cap.is_capturing
            assert cap.pipeline.startswith("hip"), cap.pipeline
    finally:
        for cap in caps:
            cap.stop_capture()
    assert all(n["v"] >= 200 for n in counts)
