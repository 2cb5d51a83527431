"""Host side of the three HIP pipelines (JPEG, H.264, HEVC) on a real
MI355X: frame pipelining, re-allocation on a resolution change, frame
upload from buffers whose addresses get reused, the H.264 segment plan
override, and the H.264 compacted read-back outgrowing its cap. Every
comparison is byte equality of emitted stripes."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hipflux = pytest.importorskip("hipflux")
from hipflux import _native
from h264_ref_decoder import Decoder, split_nals
from pipeline_content import env_vars, flat_and_mix

STRIPE_H = 64
# (id, output_mode, qp / jpeg quality)
CODECS = [("jpeg", 0, 60), ("h264", 1, 26), ("hevc", 2, 26)]


def require_gpu():
    if hipflux.hip_device_count() == 0:
        pytest.fail("gpu test ran on a host with no HIP device")


def fresh_frame(w, h, seed):
    """A newly allocated BGRX frame: smooth gradients, a seeded box and a
    seeded noise band. Equal arguments give equal pixels in a new array."""
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w, 4), np.uint8)
    f[:, :, 0] = np.linspace(0, 255, w, dtype=np.uint8)[None, :]
    f[:, :, 1] = np.linspace(0, 255, h, dtype=np.uint8)[:, None]
    f[:, :, 2] = 80
    f[:, :, 3] = 255
    f[h // 2:h // 2 + 16] = rng.integers(0, 256, (16, w, 4), dtype=np.uint8)
    x = int(rng.integers(0, w - 48))
    f[16:48, x:x + 48, 0] = 255
    f[16:48, x:x + 48, 2] = 0
    return np.ascontiguousarray(f)


def per_frame_bytes(out):
    return [sorted((y, bytes(d)) for d, y, hgt, key in fr) for fr in out]


# ---- depth 2 against depth 1 ------------------------------------------------

@pytest.mark.parametrize("mode,qp,fullcolor", [
    (0, 60, False), (0, 60, True), (2, 26, False)],
    ids=["jpeg420", "jpeg444", "hevc"])
def test_depth2_byte_identical_to_depth1(mode, qp, fullcolor):
    """One frame in flight (submit N, emit N-1) must not change a byte
    of any frame's stripes. (H.264: test_pipelined_depth2_byte_identical
    in test_gpu_h264.py.)"""
    require_gpu()
    w, h, n = 160, 128, 4
    frames = [fresh_frame(w, h, 100 + i) for i in range(n)]
    runs = [per_frame_bytes(_native._pipeline_encode(
        "gpu", frames, w, h, qp, STRIPE_H, mode, False, fullcolor,
        pipeline_depth=d)) for d in (1, 2)]
    assert len(runs[0]) == len(runs[1]) == n
    for fi in range(n):
        assert len(runs[0][fi]) == h // STRIPE_H, f"frame {fi}: no stripes"
        assert runs[0][fi] == runs[1][fi], f"frame {fi}: depth 2 differs"


# ---- resolution change --------------------------------------------------------

def first_frame_of_fresh_pipeline(mode, qp, w, h, seed):
    p = _native.BenchPipeline("gpu", w, h, qp=qp, stripe_height=STRIPE_H,
                              output_mode=mode, gpu_id=0, pipeline_depth=2)
    p.keep_stripes = True
    p.encode(fresh_frame(w, h, seed), True)
    p.flush()
    fid, stripes = p.kept_stripes()
    assert fid == 0
    return sorted((y, bytes(d)) for y, d in stripes)


# JPEG once more at sizes whose width and height are 8 past a multiple of
# 16: the last MCU column and row then hold luma blocks wholly outside the
# picture, which only stay equal to a fresh pipeline's if every frame
# writes them (a re-allocation hands back memory with old contents)
RESIZES = [c + ([(160, 128), (256, 192), (160, 128)],) for c in CODECS] + [
    ("jpeg-pad8", 0, 60, [(168, 136), (264, 200), (168, 136)])]


@pytest.mark.parametrize("name,mode,qp,sizes", RESIZES,
                         ids=[c[0] for c in RESIZES])
def test_resolution_change_restarts_like_a_fresh_pipeline(name, mode, qp,
                                                          sizes):
    """Depth 2 across 160x128 -> 256x192 -> 160x128, three frames each.
    The frame in flight at a resize references the old buffers and is
    dropped; every other frame emits, in order, and the first frame
    after each resize is byte-equal to what a fresh pipeline makes of it
    (JPEG and HEVC are all-intra; H.264 restarts with an IDR and fresh
    stripe state). Every frame is a newly allocated array that is
    released after its call, so the allocator may hand a later, larger
    frame an address an earlier one was uploaded from."""
    require_gpu()
    p = _native.BenchPipeline("gpu", *sizes[0], qp=qp,
                              stripe_height=STRIPE_H, output_mode=mode,
                              gpu_id=0, pipeline_depth=2)
    p.keep_stripes = True
    emitted = []            # frame ids in emission order
    first_after = {}        # segment -> kept stripes of its first frame
    fid = 0
    for seg, (w, h) in enumerate(sizes):
        if seg:
            p.resize(w, h)
        for i in range(3):
            nbytes, nstripes = p.encode(fresh_frame(w, h, 10 * seg + i),
                                        i == 0)
            if i == 0:
                # nothing to emit: the pipe was empty or just dropped
                assert (nbytes, nstripes) == (0, 0)
                assert p.last_frame_id == -1
            else:
                assert nbytes > 0 and nstripes == -(-h // STRIPE_H)
                emitted.append(p.last_frame_id)
            if i == 1:
                kept_id, stripes = p.kept_stripes()
                assert kept_id == fid - 1
                first_after[seg] = sorted((y, bytes(d)) for y, d in stripes)
            fid += 1
    nbytes, nstripes = p.flush()
    assert nbytes > 0 and nstripes == -(-sizes[-1][1] // STRIPE_H)
    emitted.append(p.last_frame_id)
    assert emitted == [0, 1, 3, 4, 6, 7, 8]
    for seg, (w, h) in enumerate(sizes):
        want = first_frame_of_fresh_pipeline(mode, qp, w, h, 10 * seg)
        assert [y for y, _ in want] == list(range(0, h, STRIPE_H))
        assert first_after[seg] == want, \
            f"{name}: first frame at {w}x{h} (segment {seg}) differs " \
            f"from a fresh pipeline's"


# ---- H.264 segment plan override ----------------------------------------------

def test_h264_segs_override_without_exact_split_is_normalised():
    """16 MBs do not split into 5 slices of ceil(16/5) = 4: the plan
    normalises to 4 slices of 4, so HIPFLUX_SEGS=5 is HIPFLUX_SEGS=4."""
    require_gpu()
    w, h, n = 256, 96, 2
    frames = [fresh_frame(w, h, 200 + i) for i in range(n)]
    outs = {}
    for segs in (4, 5):
        with env_vars(HIPFLUX_SEGS=segs):
            outs[segs] = per_frame_bytes(_native._pipeline_encode(
                "gpu", frames, w, h, 26, STRIPE_H, 1))
    assert outs[5] == outs[4]
    for y0 in (0, 64):
        stream = b"".join(d for fr in outs[5] for y, d in fr if y == y0)
        decoded = Decoder().decode(stream)
        assert len(decoded) == n
        assert decoded[0][0].shape[1] == w


# ---- H.264 read-back growth ---------------------------------------------------

def test_h264_readback_growth_refetches_whole_slices():
    """Flat, flat, mix, flat, mix (mix: noise in the first 16 rows) with
    one frame in flight and without. A frame leaves the compacted
    read-back a cap of 2 * max + 64 words per slice; each noise frame's
    first slice outgrows the cap of the frame before it and is fetched
    again in full. (The JPEG and HEVC uses of the same helper:
    test_gpu_readback_growth_refetches_whole_rows in test_gpu_jpeg.py,
    test_readback_growth in test_gpu_hevc_recon.py.)"""
    require_gpu()
    w, h, stripe_h, qp = 256, 96, 48, 24
    flat, mix = flat_and_mix(w, h)
    frames = [flat, flat, mix, flat, mix]
    runs = [per_frame_bytes(_native._pipeline_encode(
        "gpu", frames, w, h, qp, stripe_h, 1, pipeline_depth=d))
        for d in (2, 1)]
    # the premise, in 32-bit words per emitted slice NAL
    words = [[(len(n) + 3) // 4 + 1 for y, d in fr for n in split_nals(d)
              if n[0] & 0x1F in (1, 5)] for fr in runs[0]]
    print("slice words per frame:", words)
    assert all(len(ws) == h // 16 for ws in words)
    for noise in (2, 4):
        assert max(words[noise]) > 2 * max(words[noise - 1]) + 64
    assert len(runs[0]) == len(runs[1]) == len(frames)
    for fi in range(len(frames)):
        assert [y for y, _ in runs[0][fi]] == [0, 48]
        assert runs[0][fi] == runs[1][fi], f"frame {fi}: depth 2 differs"
    for y0 in (0, 48):
        stream = b"".join(d for fr in runs[0] for y, d in fr if y == y0)
        decoded = Decoder().decode(stream)
        assert len(decoded) == len(frames)
        assert decoded[0][0].shape == (48, w)
