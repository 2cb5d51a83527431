"""H.264 fullcolor on the HIP pipeline, on a real MI355X: Hi444 (profile
244) separate-colour-plane streams, each plane coded as a monochrome
picture by the mono row / deblock / CAVLC kernels.

Every comparison is exact (np.array_equal / == on bytes). The recon
checks compare all three full-size planes over the whole MB-aligned pitch
and height, padding included, against the from-spec decoder's uncropped
planes; the debug dump holds only the last frame's reference, so
per-frame equality comes from encoding every prefix frames[:k].

Sizes are two 48-row stripes unless stated: 256x96, and 249x91 (odd
width and height, legal only with CropUnit 1; clamped source reads)."""

import contextlib
import functools
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
from h264_content import CountingDecoder, count_slice_nals, mixed_frames
from h264_ref_decoder import BitReader, Decoder, split_nals

N = 4
STRIPE_H = 48
SIZES = [(256, 96), (249, 91)]


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


@contextlib.contextmanager
def env_vars(**kv):
    """Set environment knobs around a pipeline construction (they are
    read when the pipeline is built) and restore them afterwards."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class PlaneDecoder(CountingDecoder):
    """CountingDecoder for separate colour planes: the uncropped frame is
    the three full-size planes (the base class reads self.cb, which a
    separate-plane stream never allocates)."""

    def finish_frame(self):
        Decoder.finish_frame(self)
        self.uncropped.append(tuple(p.astype(np.uint8) for p in self.planes))


@functools.lru_cache(maxsize=None)
def frames_for(w, h, n):
    """mixed_frames, built once per size and never modified."""
    return tuple(mixed_frames(w, h, n))


def encode(kind, w, h, qp, k=N, n=N, dump=False, **kw):
    frames = list(frames_for(w, h, n)[:k])
    return _native._pipeline_encode(kind, frames, w, h, qp, STRIPE_H, 1,
                                    dump, fullcolor=True, **kw)


def stripe_chunks(out):
    """frames -> {stripe y0: [bytes of each frame it was encoded in]}"""
    rows = {}
    for frame in out:
        for data, y, hgt, key in frame:
            rows.setdefault(y, []).append(bytes(data))
    return rows


def per_frame_bytes(out):
    return [sorted((y, bytes(d)) for d, y, hgt, key in fr) for fr in out]


def stripe_mb_rows(y0, h):
    return (min(y0 + STRIPE_H, h) - y0 + 15) // 16


def dump_planes(dump, w):
    """The dump's three planes, each full size with the luma pitch."""
    mbw = (w + 15) // 16
    assert dump["ypitch"] == dump["cpitch"] == mbw * 16
    planes = tuple(np.frombuffer(dump[k], np.uint8).reshape(-1, mbw * 16)
                   for k in ("y", "cb", "cr"))
    assert planes[0].shape == planes[1].shape == planes[2].shape
    return planes


def assert_planes_equal(planes, dump, w, h, y0):
    mbw = (w + 15) // 16
    rows = stripe_mb_rows(y0, h)
    for name, dp, gp in zip(("y", "cb", "cr"), planes, dump_planes(dump, w)):
        assert dp.shape == (rows * 16, mbw * 16), \
            f"stripe y={y0} plane {name}: decoder shape {dp.shape}"
        region = gp[y0:y0 + rows * 16]
        assert region.shape == dp.shape, \
            f"stripe y={y0} plane {name}: dump region {region.shape}"
        if not np.array_equal(dp, region):
            diff = np.argwhere(dp != region)
            r, c = (int(v) for v in diff[0])
            pytest.fail(
                f"stripe y={y0} plane {name}: first difference at (row {r}, "
                f"col {c}): decoder {int(dp[r, c])} != GPU "
                f"{int(region[r, c])}; {len(diff)} samples differ")


def assert_recon_equals_decoder(out, dump, w, h, known=None):
    """Decode every stripe stream of `out`; the decoder's uncropped planes
    of its last frame must equal the dump region. `known` ({y0: (chunks,
    decoder)} of a longer run) only saves decode time: a stream that is
    byte-for-byte a prefix of a known one decodes to the known decoder's
    planes after that many frames."""
    decoded = {}
    chunks_by_y = stripe_chunks(out)
    assert chunks_by_y, "nothing was encoded"
    for y0, chunks in sorted(chunks_by_y.items()):
        dec = None
        if known and y0 in known and known[y0][0][:len(chunks)] == chunks:
            dec = known[y0][1]
        if dec is None:
            dec = PlaneDecoder()
            frames = dec.decode(b"".join(chunks))
            assert len(frames) == len(chunks), (
                f"stripe y={y0}: decoded {len(frames)} frames from "
                f"{len(chunks)} encoded")
            assert dec.sps["profile_idc"] == 244 and dec.sps["separate"]
        assert_planes_equal(dec.uncropped[len(chunks) - 1], dump, w, h, y0)
        decoded[y0] = (chunks, dec)
    return decoded


@functools.lru_cache(maxsize=None)
def all_prefixes(w, h, qp, segs=0):
    """Decoder equality of the dump after frames[:k], k = N..1 (longest
    first, so shorter runs reuse its decode when their bytes are a
    prefix). Returns the longest run's (out, dump, decoded)."""
    ctx = env_vars(HIPFLUX_SEGS=segs) if segs else contextlib.nullcontext()
    first = known = None
    with ctx:
        for k in range(N, 0, -1):
            out, dump = encode("gpu", w, h, qp, k=k, dump=True)
            assert len(out) == k
            decoded = assert_recon_equals_decoder(out, dump, w, h, known)
            if first is None:
                first = (out, dump, decoded)
                known = decoded
    return first


def coverage(decoded):
    skip = inter = intra_p = 0
    bs = {k: 0 for k in range(5)}
    for chunks, dec in decoded.values():
        skip += dec.skip
        inter += dec.inter
        intra_p += dec.intra_in_p
        for k in bs:
            bs[k] += dec.bs[k]
    return skip, inter, intra_p, bs


def first_nal_sps_profile(data):
    nal = next(iter(split_nals(bytes(data))))
    assert nal[0] & 0x1F == 7, f"first NAL is type {nal[0] & 0x1F}, not SPS"
    return BitReader(nal[1:]).u(8)


# ---- 1. runs on HIP at all ---------------------------------------------------

def test_fullcolor_runs_on_hip():
    require_gpu()
    frames = list(frames_for(256, 96, N)[:1])
    out = _native._pipeline_encode("gpu", frames, 256, 96, 24, 48, 1, True,
                                   fullcolor=True)[0]
    assert len(out) == 1 and sorted(y for _, y, _, _ in out[0]) == [0, 48]
    for data, y, hgt, key in out[0]:
        assert key and hgt == 48
        assert first_nal_sps_profile(data) == 244, f"stripe y={y}"


# ---- 2. IDR bytes equal the CPU pipeline's -----------------------------------

@pytest.mark.parametrize("qp", [24, 38])
@pytest.mark.parametrize("w,h", SIZES)
def test_fullcolor_idr_bytes_equal_cpu(w, h, qp):
    """Same CSC, same intra decisions, same headers and start codes: the
    IDR frame is byte-for-byte the CPU Hi444 pipeline's, per stripe."""
    require_gpu()
    gpu = per_frame_bytes(encode("gpu", w, h, qp, k=1))[0]
    cpu = per_frame_bytes(encode("cpu", w, h, qp, k=1))[0]
    assert [y for y, _ in gpu] == [y for y, _ in cpu] == [0, 48]
    for (y0, g), (_, c) in zip(gpu, cpu):
        assert g == c, (f"stripe y={y0}: GPU {len(g)} bytes, CPU {len(c)} "
                        f"bytes, streams differ")


# ---- 3. recon equals the decoder, every prefix -------------------------------

QPS = [14, 24, 34, 38, 45]


@pytest.mark.parametrize("qp", QPS)
def test_fullcolor_recon_qp_sweep(qp):
    """qp 14: alpha = beta = 0, the decoder's filter must alter nothing;
    qp >= 24: it must alter some sample."""
    require_gpu()
    w, h = 256, 96
    out, dump, decoded = all_prefixes(w, h, qp)
    assert sorted(decoded) == [0, 48]
    skip, inter, intra_p, bs = coverage(decoded)
    print(f"GPU fullcolor {w}x{h} qp {qp}: skip={skip} inter={inter} "
          f"intra_in_p={intra_p} bs={bs}")
    changed = sum(dec.db_changed for _, dec in decoded.values())
    if qp == 14:
        assert sum(bs[k] for k in (1, 2, 3, 4)) > 0
        assert changed == 0
    else:
        assert changed > 0


# ---- 4. unaligned size -------------------------------------------------------

@pytest.mark.parametrize("qp", [24, 38])
def test_fullcolor_recon_unaligned(qp):
    """249x91: crop 7 right; last stripe 43 rows with crop 5 bottom."""
    require_gpu()
    w, h = 249, 91
    out, dump, decoded = all_prefixes(w, h, qp)
    assert sorted(decoded) == [0, 48]
    want = {0: (48, 249), 48: (43, 249)}
    for y0, (chunks, dec) in decoded.items():
        assert len(dec.frames) == N
        for planes in dec.frames:
            assert [p.shape for p in planes] == [want[y0]] * 3


# ---- 5. mid-row slices -------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES)
def test_fullcolor_recon_midrow_slices(w, h):
    """HIPFLUX_SEGS=3: 16 MBs -> 6, 6, 4 (the narrower last segment)."""
    require_gpu()
    out, dump, decoded = all_prefixes(w, h, 24, segs=3)
    for y0, (chunks, dec) in decoded.items():
        rows = stripe_mb_rows(y0, h)
        assert rows == 3 and len(chunks) == N
        for fi, chunk in enumerate(chunks):
            assert count_slice_nals(chunk) == 3 * rows * 3, \
                f"stripe y={y0} frame {fi}"


# ---- 6. GPU CAVLC equals the host packer -------------------------------------

@pytest.mark.parametrize("segs", [0, 3])
def test_fullcolor_gpu_cavlc_equals_host_packer(segs):
    require_gpu()
    w, h, qp = 256, 96, 38
    ctx = env_vars(HIPFLUX_SEGS=segs) if segs else contextlib.nullcontext()
    with ctx:
        gpu = per_frame_bytes(encode("gpu", w, h, qp))
        with env_vars(HIPFLUX_CPU_ENTROPY=1):
            host = per_frame_bytes(encode("gpu", w, h, qp))
    assert len(gpu) == len(host) == N
    for fi in range(N):
        assert [y for y, _ in gpu[fi]] == [y for y, _ in host[fi]] == [0, 48]
        for (y0, g), (_, c) in zip(gpu[fi], host[fi]):
            assert g == c, f"frame {fi} stripe y={y0}: CAVLC kernel != packer"


# ---- 7. depth 2 equals depth 1 -----------------------------------------------

def test_fullcolor_depth2_equals_depth1():
    require_gpu()
    w, h, qp = 256, 96, 24
    d1 = per_frame_bytes(encode("gpu", w, h, qp))
    d2 = per_frame_bytes(encode("gpu", w, h, qp, pipeline_depth=2))
    assert len(d1) == N and all(len(fr) == 2 for fr in d1)
    assert d1 == d2


# ---- 8. damage gating --------------------------------------------------------

DAMAGE_MASKS = [[True, True, True], [True, False, True],
                [True, False, True], [True, True, True]]


def test_fullcolor_damage_gated():
    """256x144, three stripes; the middle one is skipped on frames 1 and 2
    and encoded again on frame 3. Its three reference planes must stay as
    frame 0 left them across the skipped frames."""
    require_gpu()
    w, h, qp = 256, 144, 24
    known = None
    middle = {}
    for k in range(N, 0, -1):
        out, dump = encode("gpu", w, h, qp, k=k, dump=True,
                           encode_mask=DAMAGE_MASKS[:k])
        assert len(out) == k
        for fi, fr in enumerate(out):
            assert sorted(y for _, y, _, _ in fr) == \
                [y for y, m in zip((0, 48, 96), DAMAGE_MASKS[fi]) if m]
        decoded = assert_recon_equals_decoder(out, dump, w, h, known)
        assert sorted(decoded) == [0, 48, 96]
        if known is None:
            known = decoded
            assert [len(decoded[y][0]) for y in (0, 48, 96)] == [4, 2, 4]
        middle[k] = [p[48:96].copy() for p in dump_planes(dump, w)]
    for k in (2, 3):
        for name, a, b in zip(("y", "cb", "cr"), middle[1], middle[k]):
            assert np.array_equal(a, b), \
                f"plane {name} of the skipped stripe changed by frame {k - 1}"
    assert any(not np.array_equal(a, b)
               for a, b in zip(middle[1], middle[4]))


# ---- 9. mode coverage --------------------------------------------------------

def test_fullcolor_mode_coverage():
    """The streams of the qp sweep reach every mode the mono kernels have,
    so the equalities above are not vacuous. bS 2 (coded residual in an
    inter MB) cannot occur: such MBs are re-coded as I16x16."""
    require_gpu()
    cov = {}
    for qp in QPS:
        cov[qp] = coverage(all_prefixes(256, 96, qp)[2])
        skip, inter, intra_p, bs = cov[qp]
        print(f"GPU fullcolor 256x96 qp {qp}: skip={skip} inter={inter} "
              f"intra_in_p={intra_p} bs={bs}")
    for qp in QPS:
        assert cov[qp][3][2] == 0, f"qp {qp}: bS 2 occurred: {cov[qp][3]}"
    assert cov[24][0] >= 1, "no P_Skip at qp 24"
    assert cov[24][2] >= 1, "no intra MB inside a P slice at qp 24"
    assert sum(cov[qp][1] for qp in (34, 38, 45)) >= 1, "no P_L0_16x16"
    assert sum(cov[qp][3][1] for qp in (34, 38, 45)) >= 1, "no bS 1 edge"


# ---- 9b. the I16x16 re-code keeps the motion-search hint ---------------------

def test_fullcolor_recode_keeps_me_hint():
    """Meta word 0 of an MB: mode(2) | luma_mode<<2 | hint x (7 bits at 8)
    | hint y (7 bits at 15) | hopeless (bit 22); the hints are the best
    integer MV found, clamped to +-48, plus 64. The motion search writes
    them for every MB of a P slice; the row kernel, rewriting the word as
    intra, must carry bits 8..22 over. An inter MB re-coded as I16x16
    keeps its quarter-pel MV in word 1, so there the surviving hint is
    known exactly: clamp(mv >> 2). qp 24: every inter candidate is
    re-coded (the inter count of the sweep is 0)."""
    require_gpu()
    w, h, qp = 256, 96, 24
    out, dump = encode("gpu", w, h, qp, k=2, dump=True)
    n_mb = ((w + 15) // 16) * ((h + 15) // 16)
    meta = np.frombuffer(dump["meta"], np.int32).reshape(3, n_mb, 2)
    m0, m1 = meta[..., 0], meta[..., 1]
    mode = m0 & 3
    hx = ((m0 >> 8) & 127) - 64
    hy = ((m0 >> 15) & 127) - 64
    # a dropped field reads as -64: outside what the search can write
    assert np.all(np.abs(hx) <= 48) and np.all(np.abs(hy) <= 48), \
        "hint bits lost in some MB of the P frame"
    assert not np.any(mode == 1), "an inter MB survived at qp 24"
    recoded = (mode == 2) & (m1 != 0)       # intra, but carrying an MV
    n = int(np.count_nonzero(recoded))
    print(f"GPU fullcolor {w}x{h} qp {qp}: {n} re-coded MBs with mv != 0")
    assert n >= 1, "no inter MB with a motion vector was re-coded"
    mvx = (m1 << 16) >> 16                  # int16, quarter-pel
    mvy = m1 >> 16
    assert np.array_equal(hx[recoded], np.clip(mvx >> 2, -48, 48)[recoded])
    assert np.array_equal(hy[recoded], np.clip(mvy >> 2, -48, 48)[recoded])
    assert not np.any((m0[recoded] >> 22) & 1), "hopeless bit on an inter MB"


# ---- 10. engine --------------------------------------------------------------

def test_fullcolor_engine_uses_hip_pipeline():
    require_gpu()
    w, h = 128, 64
    s = _native.CaptureSettings()
    s.capture_width = w
    s.capture_height = h
    s.target_fps = 30
    s.output_mode = 1
    s.video_fullcolor = True
    s.use_cpu = False
    s.gpu_id = 0
    s.capture_backend = "synthetic:noise"
    s.video_fullframe = True
    s.stripe_height = 64
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
    cap.stop_capture()
    assert arrived, "no keyframe stripe arrived"
    assert pipeline == "hip-h264", pipeline
    data, y, width, height = got[0]
    assert (y, width, height) == (0, w, h)
    dec = Decoder()
    frames = dec.decode(data[10:])
    assert dec.sps["profile_idc"] == 244
    assert [p.shape for p in frames[0]] == [(h, w)] * 3
